"""The fused training loss for every form the trainer combines (csrc/train_loss.hip,
spnerf_amd.FusedTrainLoss) — needs an MI355X.

Pinned to the reference's own numbers (tests/golden/losses.npz, as tests/test_losses.py pins the
torch classes), against the sum of the torch classes on synthetic render-shaped inputs (sun_sc and
beta strided views of a wider MLP-output buffer, weights with a gradient, fine keys), flags, edge
cases, the overlap with FusedRenderLoss, determinism, graph capture and a real β render whose
weights and β column receive gradient from the loss."""
import types

import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
from spnerf_amd import losses as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NO = 11            # columns of the stand-in MLP output
SUN_COL, BETA_COL = 4, 8
GRAD_KEYS = ("rgb", "depth", "sem_logits", "weights", "sun_sc", "beta")


# ---------------------------------------------------------------------------------------------
# pinned to the reference
# ---------------------------------------------------------------------------------------------

def fixture():
    with np.load(f"{gu.GOLDEN}/losses.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


D = fixture()
# tag -> (fine keys too?, FusedTrainLoss arguments, call arguments)
PINNED = {
    "snerf_sc": (False, dict(lambda_sc=0.1), ""),
    "snerf_fine": (True, dict(lambda_sc=0.05), ""),
    "satnerf_sc": (False, dict(lambda_sc=0.1, beta=True), ""),
    "satnerf_fine": (True, dict(lambda_sc=0.0, beta=True), ""),
    "depth_subset": (False, dict(lambda_sc=0.0, lambda_ds=1.0), "depth"),
    "depth_subset_fine": (True, dict(lambda_sc=0.0, lambda_ds=0.7), "depth"),
    "depth_gnll": (False, dict(lambda_sc=0.0, lambda_ds=1.0, GNLL=True), "depth"),
    "depth_all": (True, dict(lambda_sc=0.0, lambda_ds=1.0, usealldepth=True), "depth"),
    "sem": (False, dict(lambda_sc=0.0, lambda_ss=0.04), "sem"),
    "sem_fine": (True, dict(lambda_sc=0.0, lambda_ss=1.0), "sem"),
}


def strided_column(col, values):
    """(wide leaf (B·S, NO) holding ``values`` (B, S, 1) in column ``col``, its (B, S, 1) view)."""
    B, S = values.shape[:2]
    wide = torch.zeros(B * S, NO)
    wide[:, col] = torch.as_tensor(values).reshape(-1)
    wide = wide.to(DEV).requires_grad_(True)
    return wide, wide.view(B, S, NO)[..., col:col + 1]


def fixture_inputs(fine):
    """The fixture's render dictionary on the device: every tensor a leaf with a gradient, sun_sc and
    beta views of wider buffers.  Returns (inputs, {fixture key: the leaf or (wide leaf, column)})."""
    x, leaves = {}, {}
    for typ in ("coarse", "fine") if fine else ("coarse",):
        for k in ("rgb", "depth", "weights", "z_vals", "transparency_sc", "weights_sc", "sem_logits"):
            x[f"{k}_{typ}"] = torch.tensor(D[f"in_{k}_{typ}"], device=DEV, requires_grad=True)
            leaves[f"{k}_{typ}"] = x[f"{k}_{typ}"]
        for k, col in (("sun_sc", SUN_COL), ("beta", BETA_COL)):
            wide, view = strided_column(col, D[f"in_{k}_{typ}"])
            x[f"{k}_{typ}"] = view
            leaves[f"{k}_{typ}"] = (wide, col)
    return x, leaves


def grad_of(leaf, shape):
    if isinstance(leaf, tuple):
        wide, col = leaf
        if wide.grad is None:
            return np.zeros(shape, np.float32)
        return wide.grad.view(shape[0], shape[1], NO)[..., col:col + 1].cpu().numpy()
    return leaf.grad.cpu().numpy() if leaf.grad is not None else np.zeros(shape, np.float32)


@pytest.mark.parametrize("tag", sorted(PINNED))
def test_fused_train_loss_matches_the_reference_numbers(tag):
    """FusedTrainLoss always forms the colour term, which the depth and semantic fixtures do not
    hold: for those tags the expected loss adds the plain colour the reference recorded on the same
    inputs (snerf_fine's ``{typ}_color``), and the expected rgb gradients are the ones it recorded
    there — every expected number is still the reference's own."""
    fine, ctor, extra = PINNED[tag]
    x, leaves = fixture_inputs(fine)
    T = lambda k: torch.tensor(D["in_" + k], device=DEV)   # noqa: E731
    call = {}
    if extra == "depth":
        call = dict(target_depths=torch.stack([T("depth_t"), T("depth_w")], 1), target_valid_depth=T("valid"),
                    target_std=T("dstd"))
    if extra == "sem":
        call = dict(semantics=T("labels"))
    loss, terms = L.FusedTrainLoss(**ctor)(x, T("targets"), **call)
    loss.backward()
    typs = ("coarse", "fine") if fine else ("coarse",)
    want_loss = float(D[f"{tag}|loss"])
    want_terms = {k.split("|")[2]: float(D[k]) for k in D if k.startswith(f"{tag}|term|")}
    if extra:
        for typ in typs:
            want_terms[f"{typ}_color"] = float(D[f"snerf_fine|term|{typ}_color"])
            want_loss += want_terms[f"{typ}_color"]
    extras = {f"{n}_{typ}" for n in ("mse", "psnr") for typ in typs}
    assert set(terms) == set(want_terms) | extras, (sorted(terms), sorted(want_terms))
    assert all(v.dim() == 0 and v.device.type == "cuda" and not v.requires_grad for v in terms.values())
    print(f"{tag}: loss {float(loss)!r} want {want_loss!r}")
    np.testing.assert_allclose(float(loss), want_loss, rtol=1e-5, atol=1e-8)
    for k, v in want_terms.items():
        print(f"{tag}: {k} {float(terms[k])!r} want {v!r}")
        np.testing.assert_allclose(float(terms[k]), v, rtol=1e-5, atol=1e-8, err_msg=k)
    for typ in typs:
        np.testing.assert_allclose(float(terms[f"mse_{typ}"]), float(D[f"snerf_fine|term|{typ}_color"]), rtol=1e-5)
    np.testing.assert_allclose(float(terms["psnr_coarse"]), float(D["psnr"]), rtol=1e-5)
    for k, leaf in leaves.items():
        if k.startswith("z_vals"):
            continue
        want = D[f"{tag}|grad|{k}"]
        if extra and k.startswith("rgb_"):
            want = want + D[f"snerf_fine|grad|{k}"]
        gu.assert_close(f"{tag} grad {k}", grad_of(leaf, want.shape), want, rtol=1e-4, atol_frac=1e-6)


# ---------------------------------------------------------------------------------------------
# the combined step on synthetic inputs
# ---------------------------------------------------------------------------------------------

def synth(B=300, S=128, C=3, fine=False, seed=0):
    """Render-shaped inputs in the style of test_gpu_loss.inputs(): weights with a gradient, a β
    column and the solar column in one wide buffer per pass, optionally the fine keys.  Half the
    rays get a wide target deviation (left out when the prediction is close), half a narrow one.
    Returns (inputs, leaves {name_typ: leaf or (wide, col)}, targets dict)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    x, leaves = {}, {}
    d = lambda t: t.to(DEV)   # noqa: E731
    for typ in ("coarse", "fine") if fine else ("coarse",):
        out = rnd(B * S, NO)
        w = rnd(B, S) ** 3
        w = w / w.sum(1, keepdim=True) * (0.6 + 0.4 * rnd(B, 1))
        z = torch.sort(rnd(B, S) * 0.2, 1)[0]
        wide = d(out).requires_grad_(True)
        vals = {"rgb": rnd(B, 3), "depth": (w * z).sum(1), "weights": w, "sem_logits": torch.randn(B, C, generator=g)}
        for k, v in vals.items():
            x[f"{k}_{typ}"] = leaves[f"{k}_{typ}"] = d(v).requires_grad_(True)
        x[f"z_vals_{typ}"] = d(z)
        x[f"transparency_sc_{typ}"] = d(torch.cumprod(0.8 + 0.2 * rnd(B, S), 1))
        x[f"weights_sc_{typ}"] = d(0.1 * rnd(B, S))
        x[f"sun_sc_{typ}"] = wide.view(B, S, NO)[..., SUN_COL:SUN_COL + 1]
        x[f"beta_{typ}"] = wide.view(B, S, NO)[..., BETA_COL:BETA_COL + 1]
        leaves[f"sun_sc_{typ}"], leaves[f"beta_{typ}"] = (wide, SUN_COL), (wide, BETA_COL)
    depth0 = x["depth_coarse"].detach().cpu()
    td = torch.stack([depth0 * (0.7 + 0.6 * rnd(B)), 0.2 + 0.8 * rnd(B)], 1)
    tstd = torch.where(rnd(B) < 0.5, 0.15 + 0.1 * rnd(B), 1e-3 + 0.02 * rnd(B))
    valid = (rnd(B) < 0.7).long()
    rng = np.random.default_rng(seed)
    labels = torch.tensor(rng.choice(list(range(C)) + [-100], size=B, p=[0.85 / C] * C + [0.15]))
    if B == 1:
        valid, labels = torch.ones(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    t = dict(targets=d(rnd(B, 3)), td=d(td), valid=d(valid), tstd=d(tstd), labels=d(labels))
    return x, leaves, t


def selection(x, t, typ):
    """fp64 on the CPU: (applied, smallest relative distance of a ray to a selection threshold)."""
    w, z = x[f"weights_{typ}"].detach().double().cpu(), x[f"z_vals_{typ}"].detach().double().cpu()
    dpt = x[f"depth_{typ}"].detach().double().cpu()
    sig = ((z - dpt[:, None]) ** 2 * w).sum(1).sqrt()
    diff = (dpt - t["td"][:, 0].double().cpu()).abs()
    ts = t["tstd"].double().cpu()
    rel = torch.minimum((diff - ts).abs() / ts, (sig - ts).abs() / ts).min()
    return (t["valid"].cpu() > 0) & ((diff > ts) | (sig > ts)), float(rel)


def check_selection(x, t, fine, categories):
    """The condition on the inputs: no ray within 1e-4 relative of a selection threshold, and (when
    the batch has room for them) rays that are valid and applied, valid but left out, and invalid."""
    for typ in ("coarse", "fine") if fine else ("coarse",):
        applied, rel = selection(x, t, typ)
        assert rel > 1e-4, (typ, rel)
        if categories:
            v = t["valid"].cpu() > 0
            assert (v & applied).any() and (v & ~applied).any() and (~v).any(), typ


def torch_sum(x, t, lsc, beta, lds, gnll, alld, lss):
    loss, terms = (L.SatNerfLoss(lambda_sc=lsc) if beta else L.SNerfLoss(lambda_sc=lsc))(x, t["targets"])
    if lds > 0:
        ld, t2 = L.DepthLoss(lds, GNLL=gnll, usealldepth=alld)(x, t["td"][:, 0], t["td"][:, 1], t["valid"], t["tstd"])
        loss, terms = loss + ld, {**terms, **t2}
    if lss > 0:
        ls, t3 = L.SemanticLoss(lss)(x, t["labels"])
        loss, terms = loss + ls, {**terms, **t3}
    return loss, terms


def all_grads(leaves):
    out = {}
    for k, leaf in leaves.items():
        wide = leaf[0] if isinstance(leaf, tuple) else leaf
        if isinstance(leaf, tuple):
            g = None if wide.grad is None else wide.grad[:, leaf[1]]
        else:
            g = wide.grad
        out[k] = None if g is None else g.detach().clone()
    return out


def run(kind, x, leaves, t, cfg, scale=2.5, **call):
    """(loss, terms, gradients) of the fused loss or of the sum of the torch classes."""
    for leaf in leaves.values():
        (leaf[0] if isinstance(leaf, tuple) else leaf).grad = None
    if kind == "fused":
        loss, terms = L.FusedTrainLoss(cfg["lsc"], cfg["beta"], cfg["lds"], cfg["gnll"], cfg["alld"], cfg["lss"])(
            x, t["targets"], t["td"], t["valid"], t["tstd"], t["labels"], **call)
    else:
        loss, terms = torch_sum(x, t, cfg["lsc"], cfg["beta"], cfg["lds"], cfg["gnll"], cfg["alld"], cfg["lss"])
    (scale * loss).backward()
    return loss.detach(), {k: v.detach() for k, v in terms.items()}, all_grads(leaves)


def compare(a, b, rtol=1e-5, atol_frac=1e-6, what=""):
    (la, ta, ga), (lb, tb, gb) = a, b
    np.testing.assert_allclose(float(la), float(lb), rtol=rtol, err_msg=what + " loss")
    for k, v in tb.items():
        np.testing.assert_allclose(float(ta[k]), float(v), rtol=rtol, atol=1e-7, err_msg=what + " " + k)
    for k, want in gb.items():
        got = ga[k]
        if want is None and got is None:
            continue
        ref = torch.zeros_like(got) if want is None else want
        got = torch.zeros_like(ref) if got is None else got
        gu.assert_close(what + " grad " + k, got.cpu().numpy(), ref.cpu().numpy(), rtol=rtol, atol_frac=atol_frac)


FULL = dict(lsc=0.1, beta=True, lds=1.0, gnll=True, alld=False, lss=1.0)
SHAPES = [(1, 1, 1, False), (5, 65, 5, False), (300, 128, 3, False), (300, 128, 3, True)]
# seeds chosen so the inputs satisfy check_selection (a condition on the inputs, not a tolerance)
SEEDS = {(1, 1, 1, False): 0, (5, 65, 5, False): 0, (300, 128, 3, False): 0, (300, 128, 3, True): 0}


@pytest.mark.parametrize("form", ["gnll", "mse", "all"])
@pytest.mark.parametrize("B,S,C,fine", SHAPES)
def test_combined_step_matches_the_torch_classes(B, S, C, fine, form):
    """β colour + solar + depth (each form) + semantics, against the sum of the torch classes.
    A batch of one ray cannot hold the three selection categories; its threshold distance is
    still asserted."""
    cfg = dict(FULL, gnll=form == "gnll", alld=form == "all")
    x, leaves, t = synth(B, S, C, fine, SEEDS[(B, S, C, fine)])
    check_selection(x, t, fine, categories=B >= 5)
    ref = run("torch", x, leaves, t, cfg)
    got = run("fused", x, leaves, t, cfg)
    assert set(got[1]) == set(ref[1]) | {f"{n}_{typ}" for n in ("mse", "psnr") for typ in (("coarse", "fine") if fine else ("coarse",))}
    compare(got, ref, what=f"B{B} S{S} C{C} fine={fine} {form}")
    if form != "all":
        assert got[2]["weights_coarse"] is not None and got[2]["beta_coarse"] is not None
    mse = float(((x["rgb_coarse"].detach() - t["targets"]) ** 2).mean())
    np.testing.assert_allclose(float(got[1]["mse_coarse"]), mse, rtol=1e-5)
    np.testing.assert_allclose(float(got[1]["psnr_coarse"]), -10 * np.log10(mse), rtol=1e-5)


# ---------------------------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------------------------

def test_use_beta_false_is_the_snerf_configuration():
    x, leaves, t = synth(64, 32, 3, True)
    a = run("fused", x, leaves, t, FULL, use_beta=False)
    b = run("fused", x, leaves, t, dict(FULL, beta=False))
    assert "coarse_logbeta" not in a[1] and set(a[1]) == set(b[1])
    assert torch.equal(a[0], b[0])
    for k in b[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k, g in b[2].items():
        assert (g is None and a[2][k] is None) or torch.equal(a[2][k], g), k
    assert float(a[2]["beta_coarse"].abs().sum()) == 0.0     # the wide buffer's β column hears nothing
    compare(a, run("torch", x, leaves, t, dict(FULL, beta=False)), what="use_beta=False")


@pytest.mark.parametrize("gnll", [True, False])
def test_term_only_flags_report_the_term_and_leave_it_out(gnll):
    cfg = dict(FULL, gnll=gnll)
    x, leaves, t = synth(64, 32, 3, True)
    full = run("fused", x, leaves, t, cfg, scale=1.0)
    nod = run("fused", x, leaves, t, cfg, scale=1.0, add_depth=False)
    nos = run("fused", x, leaves, t, cfg, scale=1.0, add_sem=False)
    for got, drop, key in ((nod, ("coarse_ds", "fine_ds"), "depth"), (nos, ("coarse_ss", "fine_ss"), "sem_logits")):
        for k, v in full[1].items():
            assert torch.equal(got[1][k], v), k               # every term reported as when added
        want = float(full[0]) - sum(float(full[1][k]) for k in drop)
        np.testing.assert_allclose(float(got[0]), want, rtol=1e-5)
        for typ in ("coarse", "fine"):
            g = got[2][f"{key}_{typ}"]
            assert g is None or float(g.abs().sum()) == 0.0   # exactly zero: not even materialised
            assert full[2][f"{key}_{typ}"].abs().sum() > 0
    # without the depth term the weights hear only the β colour; without β too, nothing
    ref = run("torch", x, leaves, t, dict(cfg, lds=0.0), scale=1.0)
    compare((nod[0], {}, nod[2]), (ref[0], {}, ref[2]), what="add_depth=False")
    ref = run("torch", x, leaves, t, dict(cfg, lss=0.0), scale=1.0)
    compare((nos[0], {}, nos[2]), (ref[0], {}, ref[2]), what="add_sem=False")
    plain = run("fused", x, leaves, t, dict(cfg, beta=False), scale=1.0, add_depth=False)
    assert plain[2]["weights_coarse"] is None and plain[2]["weights_fine"] is None


# ---------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------

def test_all_rays_invalid_gives_zero_depth_term_and_gradients():
    x, leaves, t = synth(64, 32, 3)
    t["valid"] = torch.zeros_like(t["valid"])
    for gnll in (True, False):
        loss, terms, g = run("fused", x, leaves, t, dict(FULL, beta=False, gnll=gnll))
        assert float(terms["coarse_ds"]) == 0.0 and torch.isfinite(loss)
        assert float(g["depth_coarse"].abs().sum()) == 0.0
        assert g["weights_coarse"] is None or float(g["weights_coarse"].abs().sum()) == 0.0


def test_zero_weights_under_beta_are_finite():
    x, leaves, t = synth(64, 32, 3)
    with torch.no_grad():
        x["weights_coarse"].zero_()
    cfg = dict(FULL, lds=0.0)
    got = run("fused", x, leaves, t, cfg)
    ref = run("torch", x, leaves, t, cfg)
    # b = 0.05 on every ray: (3 + log 0.05) / 2 = 0.0021, the difference of two numbers near 3, so the
    # bound is absolute: one fp32 ulp at 3 (2.4e-7) for the rounded log and the rounded sum, halved
    np.testing.assert_allclose(float(got[1]["coarse_logbeta"]), (3 + np.log(0.05)) / 2, rtol=0, atol=2.4e-7)
    assert all(torch.isfinite(v).all() for v in got[2].values() if v is not None) and torch.isfinite(got[0])
    compare(got, ref, what="zero weights")


def test_gnll_ray_left_out_with_zero_spread_keeps_gradient_finite_and_zero():
    """tests/test_losses.py's case on the GPU: one-hot weights (zero predicted spread) on a ray
    without a depth prior."""
    S = 8
    w = torch.zeros(2, S)
    w[0, 3] = 1.0                      # zero spread, invalid prior → left out
    w[1] = torch.full((S,), 1.0 / S)   # spread out, applied
    z = torch.linspace(0.1, 0.9, S).repeat(2, 1)
    x = {"rgb_coarse": torch.rand(2, 3).to(DEV).requires_grad_(True), "weights_coarse": w.to(DEV).requires_grad_(True),
         "z_vals_coarse": z.to(DEV), "depth_coarse": (w * z).sum(1).to(DEV).requires_grad_(True)}
    td = torch.tensor([[0.5, 1.0], [0.2, 1.0]], device=DEV)
    valid, tstd = torch.tensor([0, 1], device=DEV), torch.tensor([0.01, 0.01], device=DEV)
    tgt = torch.rand(2, 3).to(DEV)
    loss, terms = L.FusedTrainLoss(0.0, False, 1.0, GNLL=True)(x, tgt, td, valid, tstd)
    loss.backward()
    gw, gd = x["weights_coarse"].grad, x["depth_coarse"].grad
    assert torch.isfinite(loss) and torch.isfinite(gw).all() and torch.isfinite(gd).all()
    assert float(gw[0].abs().sum()) == 0.0 and float(gd[0]) == 0.0
    assert float(gw[1].abs().sum()) > 0.0
    xr = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in x.items()}
    lr = L.SNerfLoss(0.0)(xr, tgt)[0] + L.DepthLoss(1.0, GNLL=True, usealldepth=False)(xr, td[:, 0], td[:, 1], valid, tstd)[0]
    lr.backward()
    np.testing.assert_allclose(float(loss), float(lr), rtol=1e-5)
    gu.assert_close("weights", gw.cpu().numpy(), xr["weights_coarse"].grad.cpu().numpy(), rtol=1e-5, atol_frac=1e-6)
    gu.assert_close("depth", gd.cpu().numpy(), xr["depth_coarse"].grad.cpu().numpy(), rtol=1e-5, atol_frac=1e-6)


def test_label_errors_are_nan_not_silent():
    """The NaN rules of test_gpu_loss.test_fused_loss_label_errors_are_nan_not_silent, per pass."""
    x, leaves, t = synth(64, 32, 3, True)
    bad = t["labels"].clone()
    bad[5] = 3
    loss, terms, g = run("fused", x, leaves, dict(t, labels=bad), FULL)
    assert torch.isnan(loss) and torch.isnan(terms["coarse_ss"]) and torch.isnan(terms["fine_ss"])
    for typ in ("coarse", "fine"):
        gl = g[f"sem_logits_{typ}"]
        assert torch.isnan(gl[5]).all() and torch.isfinite(torch.cat([gl[:5], gl[6:]])).all()
    assert torch.isfinite(g["rgb_coarse"]).all()
    # reported but not added: the loss stays finite
    loss, terms, g = run("fused", x, leaves, dict(t, labels=bad), FULL, add_sem=False)
    assert torch.isfinite(loss) and torch.isnan(terms["coarse_ss"])
    none = torch.full_like(t["labels"], -100)
    loss, terms, g = run("fused", x, leaves, dict(t, labels=none), FULL)
    assert torch.isnan(terms["coarse_ss"]) and torch.isnan(L.SemanticLoss(1.0)(x, none)[0])
    assert float(g["sem_logits_coarse"].abs().sum()) == 0.0 and float(g["sem_logits_fine"].abs().sum()) == 0.0
    # target_valid_depth=None means every ray has a prior
    a = L.FusedTrainLoss(0.0, False, 1.0)(x, t["targets"], t["td"], None, t["tstd"])[0]
    b = L.FusedTrainLoss(0.0, False, 1.0)(x, t["targets"], t["td"], torch.ones_like(t["valid"]), t["tstd"])[0]
    assert float(a) == float(b)


def test_beta_with_unequal_sample_counts_is_a_value_error():
    x, leaves, t = synth(16, 32, 3, True)
    for k in ("weights_fine", "z_vals_fine", "transparency_sc_fine", "weights_sc_fine"):
        x[k] = torch.cat([x[k].detach(), x[k].detach()], 1)
    x["sun_sc_fine"] = torch.cat([x["sun_sc_fine"].detach()] * 2, 1)
    with pytest.raises(ValueError, match="beta_coarse"):
        L.FusedTrainLoss(0.1, True)(x, t["targets"])
    loss, _ = L.FusedTrainLoss(0.1, False)(x, t["targets"])      # the plain form takes them
    assert torch.isfinite(loss)


# ---------------------------------------------------------------------------------------------
# overlap with FusedRenderLoss, determinism, graph capture
# ---------------------------------------------------------------------------------------------

def test_agrees_with_fused_render_loss_where_they_overlap():
    x, leaves, t = synth(300, 128, 3)
    cfg = dict(FULL, beta=False, gnll=False)
    got = run("fused", x, leaves, t, cfg)
    for leaf in leaves.values():
        (leaf[0] if isinstance(leaf, tuple) else leaf).grad = None
    loss, terms = L.FusedRenderLoss(cfg["lsc"], cfg["lds"], cfg["lss"])(x, t["targets"], t["td"], t["valid"], t["tstd"], t["labels"])
    (2.5 * loss).backward()
    compare(got, (loss.detach(), {k: v.detach() for k, v in terms.items()}, all_grads(leaves)), what="FusedRenderLoss")


def test_two_calls_are_bitwise_equal():
    x, leaves, t = synth(1000, 64, 3, True)
    a = run("fused", x, leaves, t, FULL)
    b = run("fused", x, leaves, t, FULL)
    assert torch.equal(a[0], b[0])
    for k, g in a[2].items():
        assert torch.equal(g, b[2][k]), k


def test_graph_replay_equals_eager():
    """Forward + backward captured and replayed on ONE stream: the warm-up, the capture and the
    replay all run on ``s``, and the gradients are taken with respect to the loss's own inputs (the
    sun_sc / beta views, not the wide leaves behind them), so that autograd neither accumulates
    two gradients into one leaf nor hands a gradient to a stream other than the capturing one —
    either would fork the capture onto a second stream."""
    fn = L.FusedTrainLoss(lambda_sc=0.1, beta=True, lambda_ds=1.0, GNLL=True, lambda_ss=1.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x, leaves, t = synth(300, 128, 3, True)      # the views are taken on s too: their nodes belong to it
        wrt = [x[f"{k}_{typ}"] for typ in ("coarse", "fine") for k in ("rgb", "sun_sc", "depth", "sem_logits", "weights")]
        wrt.append(x["beta_coarse"])

        def step():
            loss, terms = fn(x, t["targets"], t["td"], t["valid"], t["tstd"], t["labels"])
            return (loss, terms["psnr_coarse"]) + torch.autograd.grad(loss, wrt)

        for _ in range(2):
            eager = step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            captured = step()
        graph.replay()
    torch.cuda.synchronize()
    assert len(eager) == len(captured) == 13
    for i, (e, c) in enumerate(zip(eager, captured)):
        assert torch.equal(e, c), i


# ---------------------------------------------------------------------------------------------
# through a real render
# ---------------------------------------------------------------------------------------------

def test_gradients_through_a_real_beta_render():
    """64 rays x 32 samples of a small β + semantic model: the loss sends gradient into weights_coarse
    (g_w of the composite backward) and into the β and solar columns of the MLP output."""
    from oracle.weights import ModelDims, make_weights
    B, S = 64, 32
    dims = ModelDims(width=64, sem=True, beta=True)
    args = types.SimpleNamespace(n_samples=S, n_importance=0, model="sp-nerf", beta=True, guidedsample=False,
                                 sc_lambda=0.05, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.5)
    m = spnerf_amd.SPNeRF(num_sem_classes=dims.num_sem_classes, layers=dims.layers, feat=dims.width, mapping=dims.mapping,
                          t_embedding_dims=dims.t_dim, beta=True, sem=True)
    m.load_state_dict({k: torch.tensor(v) for k, v in make_weights(dims, 5).items()})
    m = m.to(DEV)
    emb = torch.nn.Embedding(8, dims.t_dim).to(DEV)
    with torch.no_grad():
        emb.weight.copy_(torch.linspace(-1, 1, 8 * dims.t_dim).reshape(8, dims.t_dim))
    rng = np.random.default_rng(11)
    draws = [("rand", rng.random((B, S), np.float32)), ("randn", rng.standard_normal((B, S), np.float32)),
             ("randn", rng.standard_normal((B, S), np.float32))]
    rays = torch.tensor(gu.synthetic_rays(B, 3), device=DEV)
    labels = torch.tensor(rng.choice([0, 1, 2, -100], size=B, p=[0.3, 0.3, 0.25, 0.15]), device=DEV)
    ts = torch.arange(B, device=DEV) % 8
    params = [p for p in m.parameters()] + [emb.weight]
    names = [n for n, _ in m.named_parameters()] + ["t.weight"]

    def render():
        for p in params:
            p.grad = None
        with spnerf_amd.random_source(spnerf_amd.ReplayRandom(draws)) as src:
            res = spnerf_amd.render_rays({"coarse": m, "t": emb}, args, rays, ts, semantics=labels, mode="train")
        assert src.used == len(draws)
        return res

    # one render per arm (the MLP backward frees its activations): the same draws, the same values
    res = render()
    g = torch.Generator().manual_seed(2)
    depth = res["depth_coarse"].detach().cpu()
    td = torch.stack([depth * (0.7 + 0.6 * torch.rand(B, generator=g)), 0.2 + 0.8 * torch.rand(B, generator=g)], 1).to(DEV)
    tstd = (depth.mean() * torch.where(torch.rand(B, generator=g) < 0.5, torch.tensor(4.0), torch.tensor(0.02))
            * (0.5 + torch.rand(B, generator=g))).to(DEV)
    valid = (torch.rand(B, generator=g) < 0.7).long().to(DEV)
    tgt = torch.rand(B, 3, generator=g).to(DEV)
    t = dict(targets=tgt, td=td, valid=valid, tstd=tstd, labels=labels)
    check_selection(res, t, False, categories=True)
    cfg = dict(lsc=0.05, beta=True, lds=1.0, gnll=True, alld=False, lss=0.04)
    want_loss, _ = torch_sum(res, t, cfg["lsc"], True, cfg["lds"], True, False, cfg["lss"])
    want_loss.backward()
    want = [None if p.grad is None else p.grad.detach().clone() for p in params]
    res2 = render()
    for k in ("rgb_coarse", "depth_coarse", "weights_coarse", "beta_coarse", "sun_sc_coarse", "sem_logits_coarse"):
        assert torch.equal(res2[k], res[k]), k
    loss, _ = L.FusedTrainLoss(cfg["lsc"], True, cfg["lds"], GNLL=True, lambda_ss=cfg["lss"])(
        res2, tgt, td, valid, tstd, labels)
    loss.backward()
    got = [None if p.grad is None else p.grad.detach().clone() for p in params]
    np.testing.assert_allclose(float(loss), float(want_loss), rtol=1e-5)
    for n, a, b in zip(names, got, want):
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.isfinite(a).all(), n
            gu.assert_close(f"grad {n}", a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol_frac=1e-6)
    assert float(got[-1].abs().max()) > 0      # the t-embedding hears the loss only through the β column
