"""The device-scalar kernels of a captured training step (include/spnerf_amd_train.h) against the
host-scalar entry points they stand beside — needs an MI355X.

* ``spnerf_train_step_begin``: the plan's rows and index slices in order, and past the end nothing
  moves but the error word.
* ``spnerf_adam_step_dev``: bit-equal to ``spnerf_adam_step`` over steps 1..3 on tensors of 1, 4 095,
  4 096, 4 097 and 5 000 (one float off a 16-byte boundary: the unaligned path) elements, once with
  more than 48 tensors (two launches); and within ``tests/test_gpu_adam.py``'s 1e-6 of
  ``torch.optim.Adam`` on the CPU.
* ``spnerf_composite_*_dev``: every output and ``d_out`` bit-equal to the scalar entry points for
  S in {1, 64, 65} and noise_std in {0, 0.37} under one Philox key, 7 rays.  At noise_std = 0 the
  scalar path skips the draw and the device path draws and multiplies by 0: a draw is finite
  (Box-Muller of u1 >= 2^-24), so the product is a zero and sigma's relu sees the same value."""
import ctypes

import numpy as np
import pytest
import torch

from spnerf_amd import _lib, _train_lib, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows_dev(rows):
    return torch.from_numpy(rows.view(np.int64).copy()).to(DEV)


def _cur_row(cur):
    return np.frombuffer(cur.cpu().numpy().tobytes(), train.ROW_DTYPE)[0]


@pytest.mark.parametrize("B", [5, 1])
def test_step_begin_walks_the_plan_and_stops_at_its_end(B):
    L = _train_lib.lib()
    plan = train.make_plan(1, dataset_len=3 * B + (2 if B > 1 else 0), batch_size=B, lr0=5e-4, noise_std0=1.0, seed=3)
    assert plan.n_steps == 3
    rows, perm = _rows_dev(plan.rows), plan.perm.to(DEV)
    state = torch.tensor([0, 3, B, 0], dtype=torch.int64, device=DEV)
    cur = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    idx = torch.full((B + 2,), -7, dtype=torch.int64, device=DEV)    # two guard elements behind the buffer

    def begin(b=B):
        _lib.check(L.spnerf_train_step_begin(_lib.ptr(state), _lib.ptr(rows), _lib.ptr(perm), _lib.ptr(cur), _lib.ptr(idx),
                                             b, _lib.stream_of(cur)), "train_step_begin")
        torch.cuda.synchronize()

    for k in range(3):
        begin()
        assert _cur_row(cur).tobytes() == plan.rows[k].tobytes(), k
        assert torch.equal(idx[:B].cpu(), plan.batch(k)) and idx[B:].tolist() == [-7, -7]
        assert state.tolist() == [k + 1, 3, B, 0]
    before = (cur.clone(), idx.clone())
    begin()                                        # the fourth launch: past the end
    assert torch.equal(cur, before[0]) and torch.equal(idx, before[1])
    assert state.tolist() == [3, 3, B, _train_lib.ERR_PAST_END]
    state.copy_(torch.tensor([1, 3, B, 0]))        # a batch size that is not the plan's moves nothing either
    begin(B + 1)
    assert torch.equal(cur, before[0]) and torch.equal(idx, before[1])
    assert state.tolist() == [1, 3, B, _train_lib.ERR_BATCH]
    state.copy_(torch.tensor([-1, 3, B, 0]))       # nor does a negative cursor
    begin()
    assert torch.equal(cur, before[0]) and state.tolist() == [-1, 3, B, _train_lib.ERR_PAST_END]


def _adam_lists(ts):
    n = len(ts)
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])


def _adam_tensors(sizes, seed):
    """Parameter-like tensors of the given sizes; the 5 000-element one starts one float past a
    16-byte boundary (the kernels' unaligned path)."""
    g = torch.Generator().manual_seed(seed)

    def one(n, scale=1.0):
        if n == 5000:
            return (torch.randn(n + 1, generator=g) * scale).to(DEV)[1:]
        return (torch.randn(n, generator=g) * scale).to(DEV)

    return one


@pytest.mark.parametrize("sizes", [[1, 4095, 4096, 4097, 5000], [1, 4095, 4096, 4097, 5000] + [3, 17, 64, 129, 5] * 10],
                         ids=["5-tensors", "55-tensors-two-launches"])
def test_adam_step_dev_is_adam_step(sizes):
    L = _train_lib.lib()
    lr, b1, b2, eps = 5e-4, 0.9, 0.999, 1e-8
    one = _adam_tensors(sizes, 0)
    init = [one(n) for n in sizes]
    assert init[4].data_ptr() % 16 == 4
    P = {k: [t.clone() if t.numel() != 5000 else torch.cat([t.new_zeros(1), t])[1:] for t in init] for k in "ab"}
    M = {k: [torch.zeros_like(t) for t in P[k]] for k in "ab"}
    V = {k: [torch.zeros_like(t) for t in P[k]] for k in "ab"}
    # the CPU reference: torch's single-tensor Adam
    C = [torch.nn.Parameter(t.cpu().clone()) for t in init]
    opt = torch.optim.Adam(C, lr=lr, betas=(b1, b2), eps=eps, foreach=False, fused=False)
    numel = (ctypes.c_int64 * len(sizes))(*sizes)
    cur = torch.zeros(3, dtype=torch.int64, device=DEV)
    gone = _adam_tensors(sizes, 1)
    for t in (1, 2, 3):
        grads = [gone(n, 10.0 ** (t - 2)) for n in sizes]
        _lib.check(L.spnerf_adam_step(len(sizes), _adam_lists(P["a"]), _adam_lists(grads), _adam_lists(M["a"]),
                                      _adam_lists(V["a"]), numel, lr, b1, b2, eps, t, _lib.stream_of(cur)), "adam_step")
        row = np.zeros(1, train.ROW_DTYPE)
        ss, bc = train.adam_scalars(lr, b1, b2, t)
        row[0] = (0.0, lr, ss, bc, t)
        cur.copy_(torch.from_numpy(row.view(np.int64).copy()))
        _lib.check(L.spnerf_adam_step_dev(len(sizes), _adam_lists(P["b"]), _adam_lists(grads), _adam_lists(M["b"]),
                                          _adam_lists(V["b"]), numel, _lib.ptr(cur), b1, b2, eps, _lib.stream_of(cur)),
                   "adam_step_dev")
        for c, gr in zip(C, grads):
            c.grad = gr.cpu().clone()
        opt.step()
        torch.cuda.synchronize()
        for i in range(len(sizes)):
            for name, X in (("param", P), ("exp_avg", M), ("exp_avg_sq", V)):
                assert torch.equal(X["a"][i], X["b"][i]), (t, sizes[i], name)
    for i, c in enumerate(C):     # tests/test_gpu_adam.py's bound for the comparison with torch
        q = c.detach()
        err = (P["b"][i].cpu() - q).abs().max().item()
        assert err <= 1e-6 * max(1.0, q.abs().max().item()), (sizes[i], err)
        st = opt.state[c]
        for k, X in (("exp_avg", M), ("exp_avg_sq", V)):
            d = (X["b"][i].cpu() - st[k]).abs().max().item()
            assert d <= 1e-6 * st[k].abs().max().item(), (sizes[i], k, d)


@pytest.mark.parametrize("noise_std", [0.0, 0.37])
@pytest.mark.parametrize("S", [1, 64, 65])
def test_composite_dev_is_the_scalar_composite(S, noise_std):
    L = _train_lib.lib()
    B, NO, n_sem, sem_col = 7, 12, 3, 9
    g = torch.Generator().manual_seed(100 + S)
    out = torch.randn(B * S, NO, generator=g)
    out[:, 3] = out[:, 3] * 2.0 + 0.5                       # sigma on both sides of the relu
    out[:, 4:8] = torch.rand(B * S, 4, generator=g)
    out = out.to(DEV)
    z = (torch.sort(torch.rand(B, S, generator=g), -1)[0] * 0.2).to(DEV)
    up = [torch.randn(s, generator=g).to(DEV) for s in ((B, 3), (B,), (B, S), (B, S), (B, n_sem))]
    state = torch.tensor([5, 17], dtype=torch.int64, device=DEV)     # one Philox key {seed, step}
    rng = _lib.Rng(state.data_ptr(), 1000, 2, 0)
    ns_dev = torch.tensor([noise_std], dtype=torch.float32, device=DEV)
    stream = _lib.stream_of(out)

    def run(dev_path, flags):
        wo = bool(flags & _lib.SPNERF_COMP_WEIGHTS_ONLY)
        first = torch.full((B, S) if wo else (B, 3), 9.0, device=DEV)
        o = [first, torch.full((B,), 9.0, device=DEV), torch.full((B, S), 9.0, device=DEV), torch.full((B, S), 9.0, device=DEV),
             torch.full((B, n_sem), 9.0, device=DEV)]
        d_out = torch.full((B * S, NO), 9.0, device=DEV)
        if dev_path:
            _lib.check(L.spnerf_composite_forward_dev(B, S, _lib.ptr(z), _lib.ptr(out), NO, None, _lib.ptr(ns_dev), sem_col,
                                                      n_sem, flags, *[_lib.ptr(t) for t in o], _lib.rng_ref(rng), stream),
                       "composite_forward_dev")
            _lib.check(L.spnerf_composite_backward_dev(B, S, _lib.ptr(z), _lib.ptr(out), NO, None, _lib.ptr(ns_dev), sem_col,
                                                       n_sem, flags, _lib.ptr(first if wo else up[0]),
                                                       *[_lib.ptr(t) for t in up[1:]], _lib.ptr(d_out), _lib.rng_ref(rng),
                                                       stream), "composite_backward_dev")
        else:   # as spnerf.composite passes it: no key when the host knows noise_std is 0 (the draw is skipped)
            key = _lib.rng_ref(rng) if noise_std != 0 else None
            _lib.check(L.spnerf_composite_forward(B, S, _lib.ptr(z), _lib.ptr(out), NO, None, noise_std, sem_col, n_sem, flags,
                                                  *[_lib.ptr(t) for t in o], key, stream), "composite_forward")
            _lib.check(L.spnerf_composite_backward(B, S, _lib.ptr(z), _lib.ptr(out), NO, None, noise_std, sem_col, n_sem,
                                                   flags, _lib.ptr(first if wo else up[0]), *[_lib.ptr(t) for t in up[1:]],
                                                   _lib.ptr(d_out), key, stream), "composite_backward")
        torch.cuda.synchronize()
        return o + [d_out]

    names = ("rgb / sun", "depth", "weights", "transparency", "sem_logits", "d_out")
    for flags in (0, _lib.SPNERF_COMP_WEIGHTS_ONLY, _lib.SPNERF_COMP_WEIGHTS_ONLY | _lib.SPNERF_COMP_SUN_COLUMN):
        a, b = run(False, flags), run(True, flags)
        for nm, x, y in zip(names, a, b):
            assert torch.equal(x, y), (flags, nm)           # bit-equal, untouched outputs included
        assert torch.isfinite(b[2]).all() and torch.isfinite(b[5]).all()
    if noise_std:   # the draw does reach sigma: the noisy weights differ from the noise-free ones
        ns_dev.zero_()
        assert not torch.equal(run(True, 0)[2], b[2]) or S == 1
