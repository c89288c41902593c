"""oracle/bf16_emu.py on the CPU: with every rounding site off it is ref_cpu.field in float64; every
site does something; and the mutation table that the GPU bounds of tests/test_gpu_bf16_emu.py
(bf16_emu_cases.BOUNDS) are judged against.

MUTATION_TABLE: norm-relative distance (golden_util.rel_err) of each mutated emulation to the clean
one on the two 33 x 32 training shapes of the GPU test (1 056 points: 16 full 64-point tiles and a
ragged one of 32), per output key (stem) and per parameter-tensor class — the largest over the
tensors of a class.  A mutation is DETECTABLE when some key or class moves by at least twice its GPU
bound on BOTH shapes; NOT_DETECTABLE lists the rest with the reason (DESIGN §5 has both numbers).
The table is recomputed and compared here, so it cannot drift from the emulation.
"""
import numpy as np
import pytest
import torch

import bf16_emu_cases as cases
import golden_util as gu
from oracle import bf16_emu as emu
from oracle import ref_cpu
from oracle.weights import make_weights

DIMS = {}
for _cid, _dims, _P in cases.POINT_CASES:
    DIMS.setdefault(repr(_dims), _dims)
DIMS = list(DIMS.values())
TABLE_CASES = ("w512_sem_33x32", "w64_sem_33x32")

MUTATION_TABLE = {
    "drop_k32_last_tile": {
        "w512_sem_33x32": {'depth': 0.0013, 'weights': 0.00224, 'transparency': 0.00134, 'sun': 0.000784, 'rgb': 0.00236, 'albedo': 0.0038, 'sem_logits': 0.0365, 'embedding': 0.0587, 'trunk_weight': 0.0865, 'bias': 0.0871, 'head_weight': 0.0815},
        "w64_sem_33x32": {'depth': 0.000803, 'weights': 0.00138, 'transparency': 0.000973, 'sun': 0.00206, 'rgb': 0.0029, 'albedo': 0.00573, 'sem_logits': 0.047, 'embedding': 0.0815, 'trunk_weight': 0.163, 'bias': 0.151, 'head_weight': 0.137},
    },
    "skip_pe_zero_tile": {
        "w512_sem_33x32": {'depth': 0.00274, 'weights': 0.00518, 'transparency': 0.00312, 'sun': 0.00161, 'rgb': 0.00494, 'albedo': 0.00864, 'sem_logits': 0.13, 'trunk_weight': 0.232, 'bias': 0.154, 'head_weight': 0.161},
        "w64_sem_33x32": {'depth': 0.000919, 'weights': 0.00282, 'transparency': 0.00109, 'sun': 0.0062, 'rgb': 0.00828, 'albedo': 0.0122, 'sem_logits': 0.143, 'trunk_weight': 0.278, 'bias': 0.3, 'head_weight': 0.283},
    },
    "l0_hi_only": {
        "w512_sem_33x32": {'depth': 4.35e-05, 'weights': 0.000105, 'transparency': 5.02e-05, 'sun': 0.000213, 'rgb': 0.000491, 'albedo': 0.000584, 'sem_logits': 0.0035, 'embedding': 0.0125, 'trunk_weight': 0.0148, 'bias': 0.015, 'head_weight': 0.0109},
        "w64_sem_33x32": {'depth': 2.68e-05, 'weights': 7.06e-05, 'transparency': 3.24e-05, 'sun': 0.000495, 'rgb': 0.000434, 'albedo': 0.000484, 'sem_logits': 0.00206, 'embedding': 0.012, 'trunk_weight': 0.0141, 'bias': 0.0155, 'head_weight': 0.011},
    },
    "pad_is_class0": {
        "w512_sem_33x32": {'depth': 0.00149, 'weights': 0.00435, 'transparency': 0.00188, 'sun': 0.00552, 'rgb': 0.0163, 'albedo': 0.0252, 'sem_logits': 0.234, 'embedding': 0.275, 'trunk_weight': 0.607, 'bias': 0.567, 'head_weight': 0.442},
        "w64_sem_33x32": {'depth': 0.00204, 'weights': 0.00411, 'transparency': 0.0023, 'sun': 0.00892, 'rgb': 0.0209, 'albedo': 0.0198, 'sem_logits': 0.212, 'embedding': 0.451, 'trunk_weight': 0.57, 'bias': 0.572, 'head_weight': 0.472},
    },
    "bias_tail16": {
        "w512_sem_33x32": {'depth': 5.31e-05, 'weights': 0.000114, 'transparency': 6.24e-05, 'sun': 0.000219, 'rgb': 0.00055, 'albedo': 0.000632, 'sem_logits': 0.00614, 'embedding': 0.0149, 'trunk_weight': 0.0155, 'bias': 0.232, 'head_weight': 0.0109},
        "w64_sem_33x32": {'depth': 0.000213, 'weights': 0.000443, 'transparency': 0.000239, 'sun': 0.00151, 'rgb': 0.00269, 'albedo': 0.0026, 'sem_logits': 0.0332, 'embedding': 0.0363, 'trunk_weight': 0.0795, 'bias': 0.507, 'head_weight': 0.0457},
    },
    "swap_rows_last_tile": {
        "w512_sem_33x32": {'depth': 4.92e-06, 'weights': 0.000381, 'transparency': 4.43e-05, 'sun': 0.000196, 'rgb': 0.00183, 'albedo': 0.000504, 'embedding': 0.113, 'trunk_weight': 0.0712, 'bias': 0.0691, 'head_weight': 0.0601},
        "w64_sem_33x32": {'depth': 4.75e-07, 'weights': 3.68e-05, 'transparency': 4.27e-06, 'sun': 0.00015, 'rgb': 0.00259, 'albedo': 0.00075, 'embedding': 0.0607, 'trunk_weight': 0.0837, 'bias': 0.0689, 'head_weight': 0.0396},
    },
    "wgrad_split_missing": {
        "w512_sem_33x32": {'trunk_weight': 0.504},
        "w64_sem_33x32": {'trunk_weight': 0.511},
    },
    "sigma_bias_last_tile": {
        "w512_sem_33x32": {'bias': 0.501},
        "w64_sem_33x32": {'bias': 0.293},
    },
}

# mutation -> why no key reaches twice its bound (both numbers: DESIGN §5)
NOT_DETECTABLE = {
    "l0_hi_only": "dropping the lo planes is one more bf16 rounding of fc_net.0's operands: it moves every key by "
                  "what the kernels' own rounding flips move it (largest ratio to a bound: see DESIGN)",
}


def _field_inputs(dims, P=40):
    xyz, sun, lab, t = cases.point_inputs(dims, P)
    return (torch.tensor(xyz), torch.tensor(sun), torch.tensor(lab) if dims.sem else None,
            torch.tensor(t) if dims.beta else None)


@pytest.mark.parametrize("dims", DIMS, ids=[f"w{d.width}{'_sem' if d.sem else ''}{'' if d.mapping else '_nomap'}" for d in DIMS])
def test_emulation_off_is_float64_field(dims):
    xyz, sun, lab, t = _field_inputs(dims)
    dbl = lambda v: None if v is None else v.double()
    w = make_weights(dims, cases.SEED_W)
    R = torch.tensor(np.random.default_rng(5).standard_normal((xyz.shape[0], dims.n_outputs)))
    runs = {}
    for tag in ("ref", "emu"):
        p = emu.params64(w)
        if tag == "ref":
            out = ref_cpu.field(p, dims, xyz.double(), sun.double(), lab, dbl(t))
        else:
            out = emu.emu_field(p, dims, xyz.double(), sun.double(), lab, dbl(t), emu.EmuSites.off())
        (out * R).sum().backward()
        runs[tag] = (out.detach().numpy(), {n: (q.grad if q.grad is not None else torch.zeros_like(q)).numpy() for n, q in p.items()})
    (ro, rg), (eo, eg) = runs["ref"], runs["emu"]
    assert gu.rel_err(eo, ro) < 1e-12
    for n in rg:
        assert gu.rel_err(eg[n], rg[n]) < 1e-12 if np.any(rg[n]) else not np.any(eg[n]), n
    # and float64 field is the fp32 field the goldens pin, to fp32 rounding
    with torch.no_grad():
        f32 = ref_cpu.field(ref_cpu.to_params(w), dims, xyz, sun, lab, t).numpy()
    assert gu.rel_err(f32, ro) < 1e-5


def _one_render(sites):
    name = "w64_sem_33x32"
    return cases.emulate_train(name, cases.stratified_z(cases.train_inputs(name)), sites)


@pytest.mark.parametrize("site", emu.SITES)
def test_each_site_matters(site):
    """One site off (the others on) moves some output — for the two backward sites, some parameter
    gradient — by more than 1e-5 norm-relative."""
    dims, P = cases.POINT_CASES[3][1], 129   # W = 512, sem + beta
    if site in emu.FORWARD_SITES:
        on, off = cases.point_emulation(dims, P), cases.point_emulation(dims, P, emu.EmuSites().without(site))
        moved = max(gu.rel_err(off[:, c], on[:, c]) for c in range(on.shape[1]) if c not in (5, 6, 7))
    else:
        (oo, go), (of, gf) = cases.clean_train_emulation("w64_sem_33x32"), _one_render(emu.EmuSites().without(site))
        assert all(np.array_equal(oo[k], of[k]) for k in oo)   # a backward site leaves the forward alone
        moved = max(gu.rel_err(gf[n], go[n]) for n in go if np.any(go[n]))
    print(site, f"{moved:.2e}")
    assert moved > 1e-5, (site, moved)


def _distances(name, mut):
    co, cg = cases.clean_train_emulation(name)
    mo, mg = cases.emulate_train(name, cases.stratified_z(cases.train_inputs(name)), mut=mut)
    d = {}
    for k in co:
        bk = cases.out_stem(k)
        d[bk] = max(d.get(bk, 0.0), gu.rel_err(mo[k], co[k]))
    for n in cg:
        if np.any(cg[n]):
            bk = cases.param_class(n)
            d[bk] = max(d.get(bk, 0.0), gu.rel_err(mg[n], cg[n]))
    return {k: v for k, v in d.items() if v > 0}


@pytest.fixture(scope="module")
def distances():
    return {m: {n: _distances(n, m) for n in TABLE_CASES} for m in emu.MUTATIONS}


def test_mutation_table_is_current(distances):
    assert sorted(MUTATION_TABLE) == sorted(emu.MUTATIONS)
    for m, per_case in distances.items():
        print(m, {n: {k: float(f"{v:.3g}") for k, v in d.items()} for n, d in per_case.items()})
        for n, d in per_case.items():
            rec = MUTATION_TABLE[m][n]
            assert sorted(rec) == sorted(d), (m, n)
            for k, v in d.items():
                assert abs(v - rec[k]) <= 0.02 * rec[k], (m, n, k, v, rec[k])


def test_bounds_against_mutations_and_loose_bounds():
    """The two conditions on the GPU bounds.  (1) Every mutation but those of NOT_DETECTABLE moves, on
    both table shapes, some key or class by at least twice its bound.  (2) Every bound is at most 1/8
    of its OUT_TOL_KEY entry / of GRAD_TOL, but for those of OVER_EIGHTH (reported, not relaxed)."""
    undetected = set()
    for m, per_case in MUTATION_TABLE.items():
        for n, d in per_case.items():
            if not any(v >= 2.0 * cases.BOUNDS[k][1] for k, v in d.items()):
                undetected.add(m)
    assert undetected == set(NOT_DETECTABLE), undetected
    over = {k for k, (_, b) in cases.BOUNDS.items() if k in cases.LOOSE and b > cases.LOOSE[k] / 8}
    assert over == set(cases.OVER_EIGHTH), over
    for k, (measured, b) in cases.BOUNDS.items():
        assert measured > 0 and 2.9 * measured <= b <= 3.3 * measured, (k, measured, b)   # 3x, rounded up to two digits
