"""The training-loss C ABI (include/spnerf_amd_loss.h, spnerf_amd._loss_lib): the header, the ctypes
table and the built library agree, and argument errors come back as codes — no GPU needed."""
import ctypes
import re

import abi_util
from spnerf_amd import _lib, _loss_lib

HEADER = abi_util.header_path("spnerf_amd_loss.h")
ONE = 256   # a non-NULL pointer value that is never dereferenced: the arguments are refused first


def test_loss_exports_match_the_header():
    structs = {"const spnerf_train_loss_opts*": ctypes.POINTER(_loss_lib.TrainLossOpts),
               "const spnerf_train_loss_pass*": ctypes.POINTER(_loss_lib.TrainLossPass)}
    assert abi_util.check_table(_loss_lib, HEADER, "spnerf_", structs) == [
        "spnerf_loss_abi_version", "spnerf_train_loss_backward", "spnerf_train_loss_forward", "spnerf_train_loss_workspace_bytes"]
    consts = abi_util.defines(HEADER, "SPNERF_LOSS_")
    assert consts["SPNERF_LOSS_BETA"] == _loss_lib.LOSS_BETA
    assert consts["SPNERF_LOSS_DEPTH_TERM_ONLY"] == _loss_lib.LOSS_DEPTH_TERM_ONLY
    assert consts["SPNERF_LOSS_SEM_TERM_ONLY"] == _loss_lib.LOSS_SEM_TERM_ONLY
    assert [consts[f"SPNERF_LOSS_DEPTH_{n}"] for n in ("NONE", "SUBSET_MSE", "SUBSET_GNLL", "ALL")] == \
        [_loss_lib.DEPTH_NONE, _loss_lib.DEPTH_SUBSET_MSE, _loss_lib.DEPTH_SUBSET_GNLL, _loss_lib.DEPTH_ALL]
    assert consts["SPNERF_LOSS_RESULT_FLOATS"] == _loss_lib.RESULT_FLOATS
    assert consts["SPNERF_LOSS_PASS_BASE"] == _loss_lib.PASS_BASE
    assert consts["SPNERF_LOSS_PASS_TERMS"] == _loss_lib.PASS_TERMS
    assert _loss_lib.PASS_BASE + 2 * _loss_lib.PASS_TERMS == _loss_lib.RESULT_FLOATS
    header_slots = {k[len("SPNERF_LOSS_TERM_"):].lower(): v for k, v in consts.items() if k.startswith("SPNERF_LOSS_TERM_")}
    ours = {k.replace("sc_term", "sc"): v for k, v in _loss_lib.TERM_SLOTS.items()}
    assert header_slots == ours


def test_loss_struct_layouts_match_the_header():
    """Member order of the two structs as the header declares them, and their natural-alignment
    sizes on an LP64 host."""
    hdr = open(HEADER).read()
    for cname, cls in (("spnerf_train_loss_pass", _loss_lib.TrainLossPass), ("spnerf_train_loss_opts", _loss_lib.TrainLossOpts)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                members += [m.strip(" *") for m in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert members == [f for f, _ in cls._fields_], cname
    assert ctypes.sizeof(_loss_lib.TrainLossPass) == 8 + 13 * 8
    assert ctypes.sizeof(_loss_lib.TrainLossOpts) == 48 + 8 * 8 + 8 + 8


def make(beta=False, form=0, lambda_sc=0.0, lambda_ss=0.0, fine=False, **over):
    """(opts, coarse, fine or None) with every pointer that configuration needs set to ONE."""
    o = _loss_lib.TrainLossOpts()
    o.n_rays, o.n_classes, o.world, o.n_global = 8, 3, 1, 8
    o.flags = _loss_lib.LOSS_BETA if beta else 0
    o.depth_form, o.lambda_sc, o.lambda_ds, o.lambda_ss = form, lambda_sc, 1.0 if form else 0.0, lambda_ss
    o.ld_beta, o.ld_td = 1, 2
    for f in ("target", "beta", "target_depth", "target_weight", "valid", "target_std", "labels", "labels_global", "d_beta"):
        setattr(o, f, ONE)
    passes = []
    for _ in range(2 if fine else 1):
        p = _loss_lib.TrainLossPass()
        p.n_samples, p.ld_sun = 16, 1
        for f, _t in _loss_lib.TrainLossPass._fields_[2:]:
            setattr(p, f, ONE)
        passes.append(p)
    for k, v in over.items():
        obj, name = k.split("__")
        setattr({"o": o, "c": passes[0], "f": passes[-1]}[obj], name, v)
    return o, passes[0], (passes[1] if fine else None)


def forward(o, c, f, ws=ONE, res=ONE):
    L = _loss_lib.lib()
    return L.spnerf_train_loss_forward(ctypes.byref(o) if o is not None else None, ctypes.byref(c) if c is not None else None,
                                       ctypes.byref(f) if f is not None else None, ws, res, None)


def test_workspace_bytes():
    L = _loss_lib.lib()
    assert L.spnerf_train_loss_workspace_bytes(-1) < 0
    a, b = L.spnerf_train_loss_workspace_bytes(1), L.spnerf_train_loss_workspace_bytes(4096)
    assert 0 < a < b
    assert L.spnerf_train_loss_workspace_bytes(1 << 40) == L.spnerf_train_loss_workspace_bytes(1 << 20)   # capped grid


def test_forward_argument_errors_are_reported():
    L = _loss_lib.lib()
    o, c, _ = make()
    assert forward(None, c, None) == -1 and b"NULL opts" in L.spnerf_last_error()
    assert forward(o, None, None) == -1 and b"NULL opts" in L.spnerf_last_error()
    assert forward(o, c, None, ws=None) == -1 and b"NULL workspace" in L.spnerf_last_error()
    assert forward(o, c, None, res=None) == -1 and b"NULL workspace" in L.spnerf_last_error()
    cases = [
        (dict(o__n_rays=0), b"bad size B"),
        (dict(o__target=None), b"NULL target"),
        (dict(c__rgb=None), b"coarse pass: NULL rgb"),
        (dict(c__n_samples=0), b"bad size S"),
        (dict(o__flags=64), b"unknown flags"),
        (dict(form=7), b"unknown depth form"),
        (dict(beta=True, o__beta=None), b"NULL beta"),
        (dict(beta=True, o__ld_beta=0), b"NULL beta"),
        (dict(beta=True, c__weights=None), b"NULL weights"),
        (dict(beta=True, fine=True, f__n_samples=24), b"24 fine samples, 16 coarse"),
        (dict(fine=True, f__rgb=None), b"fine pass: NULL rgb"),
        (dict(lambda_sc=0.1, c__sun_sc=None), b"NULL solar inputs"),
        (dict(lambda_sc=0.1, c__ld_sun=0), b"NULL solar inputs"),
        (dict(form=_loss_lib.DEPTH_ALL, c__depth=None), b"NULL depth"),
        (dict(form=_loss_lib.DEPTH_ALL, o__target_depth=None), b"NULL depth targets"),
        (dict(form=_loss_lib.DEPTH_ALL, o__target_weight=None), b"NULL target_weight"),
        (dict(form=_loss_lib.DEPTH_SUBSET_MSE, o__valid=None), b"NULL valid"),
        (dict(form=_loss_lib.DEPTH_SUBSET_GNLL, c__z_vals=None), b"NULL z_vals"),
        (dict(form=_loss_lib.DEPTH_SUBSET_GNLL, c__weights=None), b"NULL weights"),
        (dict(lambda_ss=1.0, c__sem_logits=None), b"NULL sem_logits"),
        (dict(lambda_ss=1.0, o__labels=None), b"NULL labels"),
        (dict(lambda_ss=1.0, o__n_classes=65), b"classes outside"),
        (dict(lambda_ss=1.0, o__labels_global=None), b"NULL labels_global"),
        (dict(lambda_ss=1.0, o__world=0), b"bad world"),
    ]
    for kw, text in cases:
        assert forward(*make(**kw)) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())


def test_backward_argument_errors_are_reported():
    L = _loss_lib.lib()

    def backward(o, c, f, res=ONE, g=ONE):
        return L.spnerf_train_loss_backward(ctypes.byref(o), ctypes.byref(c), ctypes.byref(f) if f is not None else None,
                                            res, g, None)

    assert backward(*make(), g=None) == -1 and b"NULL result / g_loss" in L.spnerf_last_error()
    for kw, text in [(dict(c__d_rgb=None), b"coarse pass: NULL gradient pointer"),
                     (dict(beta=True, o__d_beta=None), b"NULL d_beta"),
                     (dict(beta=True, c__d_weights=None), b"NULL gradient pointer"),
                     (dict(form=_loss_lib.DEPTH_SUBSET_GNLL, fine=True, f__d_weights=None), b"fine pass: NULL gradient pointer"),
                     (dict(form=_loss_lib.DEPTH_SUBSET_MSE, c__d_depth=None), b"NULL gradient pointer"),
                     (dict(lambda_sc=0.1, c__d_sun=None), b"NULL gradient pointer"),
                     (dict(lambda_ss=1.0, c__d_logits=None), b"NULL gradient pointer")]:
        assert backward(*make(**kw)) == -1, kw
        assert text in L.spnerf_last_error(), (kw, L.spnerf_last_error())
    # a term-only depth or semantic term writes no gradient and needs no buffer: only then the
    # call would reach the launch, so these are checked as accepted on the GPU (test_gpu_train_loss)


def test_fused_train_loss_is_exported_and_refuses_cpu_tensors():
    import pytest
    import torch
    import spnerf_amd
    assert spnerf_amd.FusedTrainLoss is spnerf_amd.losses.FusedTrainLoss
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        spnerf_amd.FusedTrainLoss(lambda_sc=0.0)({"rgb_coarse": torch.zeros(4, 3)}, torch.zeros(4, 3))
