"""The data-parallel training-step C ABI (include/spnerf_amd_dp.h, spnerf_amd._dp_lib): the header,
the ctypes table and the built library agree, the older ABIs are what they were, argument errors
come back as codes before any launch, and the Trainer refuses a global batch that does not divide
over the ranks before it touches the library or a device — no GPU needed."""
import ctypes
import re
import types

import pytest

import abi_util
from spnerf_amd import _dp_lib, _train_lib, train

HEADER = abi_util.header_path("spnerf_amd_dp.h")
ONE = 256   # a non-NULL pointer value that is never dereferenced: the arguments are refused first


def test_dp_exports_match_the_header():
    # the element counts of the scaled Adam are a host array
    names = abi_util.check_table(_dp_lib, HEADER, "spnerf_", {("spnerf_adam_step_dev_scaled", 5): ctypes.POINTER(ctypes.c_int64)})
    assert names == ["spnerf_adam_step_dev_scaled", "spnerf_dp_abi_version", "spnerf_dp_step_begin"]
    assert all(_dp_lib.SIGNATURES[n][0] is ctypes.c_int32 for n in names)
    txt = open(HEADER).read()
    # the scaled Adam takes spnerf_adam_step_dev's arguments with grad_scale before the stream
    a, b = _train_lib.SIGNATURES["spnerf_adam_step_dev"][1], _dp_lib.SIGNATURES["spnerf_adam_step_dev_scaled"][1]
    assert b[:-2] == a[:-1] and b[-2] is ctypes.c_float and b[-1] is a[-1]
    # the header states what the scale means for a world that is, and is not, a power of two
    flat = " ".join(re.sub(r"^\s*\*", " ", line) for line in txt.splitlines())
    flat = re.sub(r"\s+", " ", flat)
    assert "bit-equal to spnerf_adam_step_dev" in flat
    assert "power-of-two world" in flat and "bit-equal to dividing" in flat and "DEFINED as the product" in flat


def begin(L, *, state=ONE, rows=ONE, perm=ONE, cur=ONE, idx=ONE, gidx=None, B=48, rank=0, world=2, rays=None, ld=11,
          clamp=None, sems=None, labels=None):
    return L.spnerf_dp_step_begin(state, rows, perm, cur, idx, gidx, B, rank, world, rays, ld, clamp, sems, labels, None)


def test_step_begin_argument_errors_are_reported_before_any_launch():
    L = _dp_lib.lib()
    err = L.spnerf_last_error
    assert begin(L, B=49) == -1 and b"does not divide" in err()
    assert begin(L, B=48, world=5) == -1 and b"does not divide" in err()
    assert begin(L, rank=2) == -1 and b"rank 2 outside [0, 2)" in err()
    assert begin(L, rank=-1) == -1 and b"rank -1 outside" in err()
    assert begin(L, world=0) == -1 and b"bad world size 0" in err()
    assert begin(L, world=-3, rank=0) == -1 and b"bad world size" in err()
    assert begin(L, rays=ONE) == -1 and b"rays and clamp go together" in err()
    assert begin(L, clamp=ONE) == -1 and b"rays and clamp go together" in err()
    assert begin(L, rays=ONE, clamp=ONE, ld=7) == -1 and b"ld_rays = 7 < 8" in err()
    assert begin(L, sems=ONE) == -1 and b"sems and labels_global go together" in err()
    assert begin(L, labels=ONE) == -1 and b"sems and labels_global go together" in err()
    assert begin(L, B=0) == -1 and b"bad batch size" in err()
    assert begin(L, B=1 << 31) == -1 and b"bad batch size" in err()
    for name in ("state", "rows", "perm", "cur", "idx"):
        assert begin(L, **{name: None}) == -1 and b"dp_step_begin: NULL pointer" in err(), name


def test_scaled_adam_argument_errors_are_reported():
    L = _dp_lib.lib()
    one = (ctypes.c_void_p * 1)(ONE)
    numel = (ctypes.c_int64 * 1)(8)
    f = L.spnerf_adam_step_dev_scaled
    assert f(1, one, one, one, one, numel, None, 0.9, 0.999, 1e-8, 0.5, None) == -1
    assert b"adam_step_dev_scaled: NULL step scalars" in L.spnerf_last_error()
    assert f(1, one, one, one, one, numel, ONE, 1.0, 0.999, 1e-8, 0.5, None) == -1
    assert b"bad hyper-parameters" in L.spnerf_last_error()
    assert f(1, one, None, one, one, numel, ONE, 0.9, 0.999, 1e-8, 0.5, None) == -1 and b"bad lists" in L.spnerf_last_error()
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert f(1, one, one, one, one, numel, ONE, 0.9, 0.999, 1e-8, bad, None) == -1
        assert b"grad_scale" in L.spnerf_last_error()
    assert f(0, None, None, None, None, None, ONE, 0.9, 0.999, 1e-8, 0.5, None) == 0   # nothing to do


def test_trainer_refuses_a_batch_that_does_not_divide_before_anything_else(monkeypatch):
    """The check needs neither the library nor a device: both are made to raise."""
    def refuse(*a, **k):
        raise AssertionError("Trainer loaded the library before checking batch_size against world")

    monkeypatch.setattr(_train_lib, "lib", refuse)
    monkeypatch.setattr(_dp_lib, "lib", refuse)
    a = types.SimpleNamespace(batch_size=49, chunk=5120)
    with pytest.raises(ValueError, match="49 does not divide over 2"):
        train.Trainer({}, a, {}, world=2)
    with pytest.raises(ValueError, match="world"):
        train.Trainer({}, a, {}, world=0)
    a.batch_size = 48
    with pytest.raises(ValueError, match="collectives"):
        train.Trainer({}, a, {}, world=2, collectives="device")
    with pytest.raises(ValueError, match="rank"):
        train.Trainer({}, a, {}, world=1, rank=1)


def test_reductions_can_leave_the_sum():
    """dp.GradBuckets.finish(scale=False) / dp.allreduce_grads(scale=False) exist and default to the
    divide-by-world behaviour (signatures only here; the gloo and GPU tests run them)."""
    import inspect

    from spnerf_amd import dp
    assert inspect.signature(dp.GradBuckets.finish).parameters["scale"].default is True
    assert inspect.signature(dp.allreduce_grads).parameters["scale"].default is True
