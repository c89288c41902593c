"""The training-step C ABI (include/spnerf_amd_train.h, spnerf_amd._train_lib): the header, the
ctypes table, the plan's numpy row type and the built library agree, and argument errors come back
as codes — no GPU needed."""
import ctypes
import re

import abi_util
import spnerf_amd
from spnerf_amd import _lib, _train_lib, train

HEADER = abi_util.header_path("spnerf_amd_train.h")
ONE = 256   # a non-NULL pointer value that is never dereferenced: the arguments are refused first

C_TYPES = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


def header_struct(name):
    """[(member, C type)] of a struct as the header declares it."""
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(m.strip(), ctype) for m in names.split(",")]
    return out


def test_train_exports_match_the_header():
    # the element counts of spnerf_adam_step_dev are a host array
    assert abi_util.check_table(_train_lib, HEADER, "spnerf_", {("spnerf_adam_step_dev", 5): ctypes.POINTER(ctypes.c_int64)}) == [
        "spnerf_adam_step_dev", "spnerf_composite_backward_dev", "spnerf_composite_forward_dev", "spnerf_train_abi_version",
        "spnerf_train_step_begin"]
    consts = abi_util.defines(HEADER, "SPNERF_TRAIN_")
    assert consts["SPNERF_TRAIN_ERR_PAST_END"] == _train_lib.ERR_PAST_END
    assert consts["SPNERF_TRAIN_ERR_BATCH"] == _train_lib.ERR_BATCH
    # the dev composites take the scalar entries' arguments with noise_std as a pointer
    for name in ("spnerf_composite_forward", "spnerf_composite_backward"):
        a, b = _lib.SIGNATURES[name][1], _train_lib.SIGNATURES[name + "_dev"][1]
        assert len(a) == len(b) and [x for x, y in zip(a, b) if x is not y] == [ctypes.c_float]
        assert b[a.index(ctypes.c_float)] is ctypes.c_void_p


def test_train_struct_layouts_match_the_header():
    for cname, cls in (("spnerf_train_step_scalars", _train_lib.StepScalars), ("spnerf_train_state", _train_lib.TrainState)):
        members = header_struct(cname)
        assert [m for m, _ in members] == [f for f, _ in cls._fields_], cname
        assert [C_TYPES[t] for _, t in members] == [t for _, t in cls._fields_], cname
    S, T = _train_lib.StepScalars, _train_lib.TrainState
    assert ctypes.sizeof(S) == 24 and ctypes.sizeof(T) == 32
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16]
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 8, 16, 24]
    # the plan's numpy rows are that struct
    assert train.ROW_DTYPE.itemsize == ctypes.sizeof(S)
    assert list(train.ROW_DTYPE.names) == [f for f, _ in S._fields_]
    assert [train.ROW_DTYPE.fields[f][1] for f, _ in S._fields_] == [getattr(S, f).offset for f, _ in S._fields_]


def test_argument_errors_are_reported():
    L = _train_lib.lib()
    assert L.spnerf_train_step_begin(None, ONE, ONE, ONE, ONE, 4, None) == -1 and b"NULL pointer" in L.spnerf_last_error()
    assert L.spnerf_train_step_begin(ONE, ONE, ONE, None, ONE, 4, None) == -1 and b"NULL pointer" in L.spnerf_last_error()
    assert L.spnerf_train_step_begin(ONE, ONE, ONE, ONE, ONE, 0, None) == -1 and b"bad batch size" in L.spnerf_last_error()
    one = (ctypes.c_void_p * 1)(ONE)
    numel = (ctypes.c_int64 * 1)(8)
    assert L.spnerf_adam_step_dev(1, one, one, one, one, numel, None, 0.9, 0.999, 1e-8, None) == -1
    assert b"NULL step scalars" in L.spnerf_last_error()
    assert L.spnerf_adam_step_dev(1, one, one, one, one, numel, ONE, 1.0, 0.999, 1e-8, None) == -1
    assert b"bad hyper-parameters" in L.spnerf_last_error()
    assert L.spnerf_adam_step_dev(1, one, None, one, one, numel, ONE, 0.9, 0.999, 1e-8, None) == -1
    assert b"bad lists" in L.spnerf_last_error()
    assert L.spnerf_adam_step_dev(0, None, None, None, None, None, ONE, 0.9, 0.999, 1e-8, None) == 0   # nothing to do
    args = [4, 16, ONE, ONE, 11, None, None, 8, 3, 0, ONE, ONE, ONE, ONE, ONE, None, None]
    assert L.spnerf_composite_forward_dev(*args) == -1 and b"composite_forward_dev: NULL pointer" in L.spnerf_last_error()
    args = [4, 16, ONE, ONE, 11, None, None, 8, 3, 0, None, None, None, None, None, ONE, None, None]
    assert L.spnerf_composite_backward_dev(*args) == -1 and b"composite_backward_dev: NULL pointer" in L.spnerf_last_error()


def test_trainer_is_exported_and_refuses_what_it_cannot_do():
    import types

    import pytest
    import torch
    assert spnerf_amd.Trainer is train.Trainer and spnerf_amd.make_plan is train.make_plan
    assert spnerf_amd.EpochPlan is train.EpochPlan
    a = types.SimpleNamespace(batch_size=4, chunk=5120)
    with pytest.raises(NotImplementedError, match="world"):
        train.Trainer({}, a, {}, world=2)
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        train.Trainer({}, a, {"rays": torch.zeros(8, 11), "rgbs": torch.zeros(8, 3)})
