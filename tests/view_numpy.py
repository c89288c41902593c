"""numpy restatement of the image metrics the validation step logs (the reference's
modules/metrics.py: mse :197, psnr :206, miou :218, overall_accuracy :239) and the loader of the
whole-view fixture (tests/golden/view_w64.npz, made by tests/golden/gen_view_golden.py).

The squared error is summed in float64 (as spnerf_view_metrics does; the fixture's psnr is the
reference's function on float64 tensors).  miou and overall accuracy follow the reference's
float32 arithmetic: ``.float().sum()`` counts, a float32 division per class, ``torch.mean`` of the
float32 stack, and correct / numel(gt) as float32 — ignored labels stay in that count."""
from __future__ import annotations

import ast
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_w64.npz")
CASES = ("a", "b", "c")


def mse(rgb, target) -> float:
    d = np.asarray(rgb, np.float64).ravel() - np.asarray(target, np.float64).ravel()
    return float(np.sum(d * d) / d.size)


def psnr(rgb, target) -> float:
    with np.errstate(divide="ignore"):
        return float(-10.0 * np.log10(np.float64(mse(rgb, target))))


def confusion(pred, gt, num_classes: int) -> np.ndarray:
    """(C + 1, C) int64 counts of (label, prediction); labels outside [0, C) in the last row."""
    pred = np.asarray(pred).ravel().astype(np.int64)
    gt = np.asarray(gt).ravel().astype(np.int64)
    C = num_classes
    t = np.zeros((C + 1, C), np.int64)
    row = np.where((gt >= 0) & (gt < C), gt, C)
    ok = (pred >= 0) & (pred < C)
    np.add.at(t, (row[ok], pred[ok]), 1)
    return t


def miou(pred, gt, num_classes: int) -> float:
    pred, gt = np.asarray(pred).ravel(), np.asarray(gt).ravel()
    ious = []
    for c in range(num_classes):
        p, g = pred == c, gt == c
        inter, union = np.float32((p & g).sum()), np.float32((p | g).sum())
        ious.append(np.float32(0.0) if union == 0 else inter / union)
    total = np.float32(0.0)
    for v in ious:
        total = np.float32(total + v)
    return float(total / np.float32(num_classes))


def overall_accuracy(pred, gt) -> float:
    pred, gt = np.asarray(pred).ravel(), np.asarray(gt).ravel()
    return float(np.float32((pred == gt).sum()) / np.float32(gt.size))


def view_metrics(rgb, target, pred=None, gt=None, num_classes: int = 0) -> dict:
    out = {"mse": mse(rgb, target), "psnr": psnr(rgb, target), "n": int(np.asarray(rgb).size // 3), "miou": None, "oa": None,
           "correct": None, "confusion": None}
    if gt is not None and num_classes > 0:
        t = confusion(pred, gt, num_classes)
        out.update(confusion=t, correct=int(np.trace(t[:num_classes])), miou=miou(pred, gt, num_classes),
                   oa=overall_accuracy(pred, gt))
    return out


def load_case(case: str) -> dict:
    """One case of the fixture in golden_util.load's form: its arrays without the ``<case>|``
    prefix, the view's ``h``, ``w``, ``target`` and ``labels``, and ``meta`` as a dictionary."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        data = {k.split("|", 1)[1]: z[k] for k in z.files if k.startswith(case + "|")}
        data.update(h=int(z["h"]), w=int(z["w"]))
    data["meta"] = ast.literal_eval(str(data.pop("meta")))
    return data
