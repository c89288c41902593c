"""LPIPS on the GPU: ``lpips``, the fourth score of the reference's offline evaluation
(eval.py:20,128-135,399: ``lpips.LPIPS(net='alex')`` of the ``lpips`` package 0.1, ``spatial=False``,
one image pair), run by csrc/lpips.hip (include/spnerf_amd_lpips.h) in fp32 with fp64 final sums.
The network's weights are data the caller brings; ``LpipsWeights`` packs them for the kernels.

The ``lpips`` package is not a dependency and was not available when this was written: the key
names ``from_state_dict`` accepts are written from the package's published source
(``lpips/pretrained_networks.py`` ``alexnet``: slices of torchvision's ``features``;
``lpips/lpips.py`` ``NetLinLayer``: ``model = [Dropout, Conv2d(C, 1, 1, bias=False)]``).  The
definition itself is pinned to an independent fp64 restatement (tests/lpips_torch.py) with seeded
weights, not to the package.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, _lpips_lib
from .image import _as_chw

RESULT_BYTES = ctypes.sizeof(_lpips_lib.LpipsResult)
CHANNELS = (64, 192, 384, 256, 256)
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
# the index of each tap's convolution in torchvision's alexnet.features, and the slice of the lpips
# package's `net` that holds it (the slices keep the indices of `features`)
_FEATURE_INDEX = (0, 3, 6, 8, 10)
DEFAULT_MAX_WORKSPACE = 256 << 20
DEFAULT_BAND = 128 << 20


def tap_sizes(H: int, W: int):
    """(h, w) of the five taps of an H x W image (floor division throughout)."""
    def conv1(n):
        return (n + 4 - 11) // 4 + 1

    def pool(n):
        return (n - 3) // 2 + 1
    a = (conv1(H), conv1(W))
    b = (pool(a[0]), pool(a[1]))
    c = (pool(b[0]), pool(b[1]))
    return [a, b, c, c, c]


def state_dict_tensors(sd, lin_sd=None):
    """(convs, biases, lins) out of a state_dict in either naming: the ``lpips`` package's
    (``net.slice{1..5}.{0,3,6,8,10}.weight|bias`` and ``lin{0..4}.model.1.weight``), or the split
    form — torchvision's ``features.{0,3,6,8,10}.weight|bias`` with the package's lin file
    (``lin{0..4}.model.1.weight``) in ``lin_sd`` or merged into ``sd``.  A missing entry raises
    ``ValueError`` naming the key; shapes are checked by ``LpipsWeights.from_tensors``."""
    merged = dict(sd)
    if lin_sd is not None:
        merged.update(lin_sd)
    convs, biases, lins = [], [], []
    for l, idx in enumerate(_FEATURE_INDEX):
        names = (f"net.slice{l + 1}.{idx}", f"features.{idx}")
        stem = next((n for n in names if n + ".weight" in merged), None)
        if stem is None:
            raise ValueError(f"lpips weights: neither {names[0]}.weight nor {names[1]}.weight in the state_dict")
        if stem + ".bias" not in merged:
            raise ValueError(f"lpips weights: {stem}.bias missing from the state_dict")
        key = f"lin{l}.model.1.weight"
        if key not in merged:
            raise ValueError(f"lpips weights: {key} missing from the state_dict")
        convs.append(merged[stem + ".weight"])
        biases.append(merged[stem + ".bias"])
        lins.append(merged[key])
    return convs, biases, lins


def _checked(convs, biases, lins):
    """The three lists as contiguous fp32 tensors of the right shapes (lins flattened to (C,))."""
    for name, seq in (("convs", convs), ("biases", biases), ("lins", lins)):
        if len(seq) != 5:
            raise ValueError(f"lpips weights: {name} has {len(seq)} entries, not 5")
    out = ([], [], [])
    for l in range(5):
        w, b, n = torch.as_tensor(convs[l]), torch.as_tensor(biases[l]), torch.as_tensor(lins[l])
        if tuple(w.shape) != CONV_SHAPES[l]:
            raise ValueError(f"lpips weights: convs[{l}] is {tuple(w.shape)}, not {CONV_SHAPES[l]}")
        if tuple(b.shape) != (CHANNELS[l],):
            raise ValueError(f"lpips weights: biases[{l}] is {tuple(b.shape)}, not {(CHANNELS[l],)}")
        if n.numel() != CHANNELS[l] or tuple(n.shape) not in ((CHANNELS[l],), (1, CHANNELS[l], 1, 1)):
            raise ValueError(f"lpips weights: lins[{l}] is {tuple(n.shape)}, not {(1, CHANNELS[l], 1, 1)} or {(CHANNELS[l],)}")
        for dst, t in zip(out, (w, b, n.reshape(-1))):
            dst.append(t.detach().float().contiguous())
    return out


class LpipsWeights:
    """The AlexNet and lin weights of LPIPS, packed on the device in the layout the kernels read
    (``packed``: one fp32 buffer of ``spnerf_lpips_weights_floats()`` values)."""

    def __init__(self, packed):
        self.packed = packed

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_tensors(cls, convs, biases, lins, device=None):
        """``convs[l]``: (C_out, C_in, k, k) as torch holds a convolution; ``biases[l]``: (C_out,);
        ``lins[l]``: (C_out,) or (1, C_out, 1, 1).  Mis-shaped entries raise ``ValueError`` naming
        them; the tensors are moved to ``device`` (default: where ``convs[0]`` is), which must be
        the GPU."""
        convs, biases, lins = _checked(convs, biases, lins)
        dev = torch.device(device) if device is not None else convs[0].device
        moved = [[t.to(dev) for t in seq] for seq in (convs, biases, lins)]
        _lib.require_device(*moved[0])
        L = _lpips_lib.lib()
        packed = torch.empty(int(L.spnerf_lpips_weights_floats()), dtype=torch.float32, device=dev)
        arrays = [(ctypes.c_void_p * 5)(*[t.data_ptr() for t in seq]) for seq in moved]
        with torch.cuda.device(dev):
            _lib.check(L.spnerf_lpips_pack_weights(arrays[0], arrays[1], arrays[2], _lib.ptr(packed), _lib.stream_of(packed)),
                       "lpips_pack_weights")
        for seq in moved:                       # the pack is stream-ordered: its sources live until it ran
            for t in seq:
                t.record_stream(torch.cuda.current_stream(dev))
        return cls(packed)

    @classmethod
    def from_state_dict(cls, sd, device, lin_sd=None):
        """From ``lpips.LPIPS(net='alex').state_dict()``, or from torchvision's
        ``alexnet().state_dict()`` with the package's lin file as ``lin_sd`` (see
        ``state_dict_tensors``; the key names are written from the package's published source)."""
        return cls.from_tensors(*state_dict_tensors(sd, lin_sd), device=device)


def workspace_bytes(H, W, max_bytes=None) -> int:
    """Bytes ``spnerf_lpips`` is given for an H x W pair when the caller allows ``max_bytes`` (0: what
    runs every convolution whole; None: 256 MiB, or the activations plus a 128 MiB band where those
    alone are larger)."""
    size = _lpips_lib.lib().spnerf_lpips_workspace_bytes
    n = size(int(H), int(W), int(DEFAULT_MAX_WORKSPACE if max_bytes is None else max_bytes))
    if n < 0:
        _lib.check(int(n), "lpips_workspace_bytes")
    if max_bytes is None and n > DEFAULT_MAX_WORKSPACE:     # the activations alone exceed the default cap:
        n = size(int(H), int(W), int(n) + DEFAULT_BAND)     # a band of 32 rows would mean thousands of launches
    return int(n)


def bands(H, W, nbytes):
    """How many row bands each of the five convolutions runs in with a workspace of ``nbytes``."""
    out = (ctypes.c_int32 * 5)()
    _lib.check(_lpips_lib.lib().spnerf_lpips_bands(int(H), int(W), int(nbytes), out), "lpips_bands")
    return list(out)


def launch_lpips(x, y, H, W, strides, normalize, weights, result_ptr, max_bytes=None, features=None) -> None:
    """``spnerf_lpips`` on the current stream of ``x``'s device: images ``x`` and ``y`` (fp32 device
    tensors sharing the element strides ``(channel, row, pixel)``) into the ``spnerf_lpips_result``
    at device address ``result_ptr``."""
    if not isinstance(weights, LpipsWeights):
        raise TypeError(f"lpips: weights must be an LpipsWeights, got {type(weights).__name__}")
    if weights.device != x.device:
        raise ValueError(f"lpips: weights on {weights.device}, images on {x.device}")
    L = _lpips_lib.lib()
    nbytes = workspace_bytes(H, W, max_bytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.check(L.spnerf_lpips(_lib.ptr(x), _lib.ptr(y), H, W, int(strides[0]), int(strides[1]), int(strides[2]),
                              1 if normalize else 0, _lib.ptr(weights.packed), _lib.ptr(ws), nbytes, _lib.ptr(features),
                              ctypes.c_void_p(result_ptr), _lib.stream_of(x)), "lpips")


def lpips(pred, gt, weights, layout="hwc", hw=None, normalize=True, return_layers=False, return_features=False,
          max_workspace_bytes=None):
    """``lpips.LPIPS(net='alex')(pred, gt)`` for one pair of 3-channel images, as a 0-dim float64
    device tensor, without a host synchronisation.  ``normalize=True`` (the default, what
    eval.py:131-132 does by hand) takes images in [0, 1]; ``False`` takes them in [−1, 1].

    ``layout="hwc"``: (H, W, 3) images, or with ``hw=(H, W)`` the (H·W, 3) planes ``render_image``
    returns; ``layout="chw"``: (1, 3, H, W) or (3, H, W).  Strided views are read in place when both
    images share their strides; otherwise both are made contiguous first.  Images smaller than
    31 x 31 are refused (the second pool has no window).

    ``return_layers=True`` gives ``(score, layers)``, the (5,) float64 per-tap terms whose sum the
    score is.  ``return_features=True`` appends the five taps after their ReLU, each a
    (2, h, w, C) fp32 tensor: ``pred``'s map, then ``gt``'s.  ``max_workspace_bytes`` caps the
    workspace (default 256 MiB, ``workspace_bytes``): convolutions whose im2col rows do not fit run in row bands, with
    the same bits."""
    _lib.require_device(pred, gt)
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"lpips: images of different shapes {tuple(pred.shape)} and {tuple(gt.shape)}")
    x = _as_chw(pred.float(), layout, hw)
    y = _as_chw(gt.to(pred.device).float(), layout, hw)
    if x.shape[0] != 3:
        raise ValueError(f"lpips: images have {x.shape[0]} channels, not 3")
    if x.stride() != y.stride():
        x, y = x.contiguous(), y.contiguous()
    _, H, W = x.shape
    res = torch.empty(RESULT_BYTES // 8, dtype=torch.float64, device=x.device)
    feats = flat = None
    if return_features:
        sizes = tap_sizes(H, W)
        counts = [2 * h * w * c for (h, w), c in zip(sizes, CHANNELS)]
        flat = torch.empty(sum(counts), dtype=torch.float32, device=x.device)
        feats = [t.view(2, h, w, c) for t, (h, w), c in zip(flat.split(counts), sizes, CHANNELS)]
    launch_lpips(x, y, H, W, x.stride(), normalize, weights, res.data_ptr(), max_workspace_bytes, flat)
    out = (res[0],) + ((res[1:6],) if return_layers or return_features else ()) + ((feats,) if return_features else ())
    return out[0] if len(out) == 1 else out
