"""scoring.py's primary and secondary tiers and its calibration residual, computed by the gfx950 kernels of
csrc/rm_score.hip (rm_score_captures, include/rm_hip.h): N captures against one reference in one call.

The device returns integer counts and the floating-point statistics (csrc/rm_score.h states each definition); the rates
are formed here from the counts with the very divisions scoring.py uses, so IoU, the false-hit / false-miss rates and the
percentiles equal the host's bit for bit, and the means differ from NumPy's pairwise sums by rounding only.  The same
inputs give the same bits on every run, and a capture scores the same alone or in a batch.

scoring.py stays the default everywhere; DESIGN.md, "Scoring on the device", records what has been measured of the two
paths.  Captures are the dicts scoring.py takes: "hit", "depth" and optionally
"normal"; float32 maps are passed as they are, anything else as float64.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from . import _native, scoring

def _check_shapes(methods: Sequence[Dict], reference: Dict):
    shape = np.shape(reference["hit"])
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"scoring needs (H, W) maps, not {shape}")
    for m in methods:
        if np.shape(m["hit"]) != shape:
            raise ValueError(f"shape mismatch: method {np.shape(m['hit'])} vs reference {shape}")
    return shape


def _score(methods: Sequence[Dict], reference: Dict, keys: Sequence[str], band_k: int) -> List[Dict]:
    shape = _check_shapes(methods, reference)
    pick = lambda c: {k: c[k] for k in keys}      # noqa: E731
    return _native.score_captures(shape[1], shape[0], pick(reference), [pick(m) for m in methods], band_k=band_k)


def _hit_metrics(r: Dict, pixels: int) -> Dict[str, float]:
    """scoring._hit_metrics from the device's counts"""
    both = r["n_co_hit"]
    only_mine, only_truth = r["n_method_hit"] - both, r["n_reference_hit"] - both
    covered = r["n_union"]
    return {
        "false_hit_rate": only_mine / pixels,
        "false_miss_rate": only_truth / pixels,
        "iou": both / covered if covered else 1.0,
        "agreement": (pixels - only_mine - only_truth) / pixels,
    }


def score_capture_batch(methods: Sequence[Dict], reference: Dict, ssim: bool = False) -> List[Dict[str, Dict]]:
    """scoring.score_capture(m, reference) of every m of `methods`, with its keys and grouping, from one device call.  The
    normal angles are NaN when the reference or a method carries no normals.  ssim=True also fills the tertiary keys
    (ssim.ssim_scores_batch, a second device call); otherwise they hold None, as score_capture leaves them."""
    methods = list(methods)
    if not methods:
        return []
    shape = _check_shapes(methods, reference)
    normals = reference.get("normal") is not None and all(m.get("normal") is not None for m in methods)
    results = _score(methods, reference, ("depth", "hit") + (("normal",) if normals else ()), band_k=-1)
    tertiary = [dict.fromkeys(scoring.SSIM_KEYS) for _ in methods]
    if ssim:
        from . import ssim as ssim_module
        tertiary = ssim_module.ssim_scores_batch(methods, reference)
    reports = []
    for r, third in zip(results, tertiary):
        report = {
            "hit": _hit_metrics(r, shape[0] * shape[1]),
            "depth": {"rmse": r["depth_rmse"], "mae": r["depth_mae"], "p95": r["depth_p95"], "n_pixels": r["n_co_hit"]},
            "normal": {"mean_deg": r["normal_mean_deg"], "p95_deg": r["normal_p95_deg"]},
            "ssim": third,
        }
        report["primary"] = report["hit"]
        report["secondary"] = {"depth": report["depth"], "normal": report["normal"]}
        report["tertiary"] = report["ssim"]
        reports.append(report)
    return reports


def residual_batch(methods: Sequence[Dict], truth: Dict, k: int = 2) -> List[Dict[str, float]]:
    """scoring.residual(m["hit"], m["depth"], truth["hit"], truth["depth"], scoring.silhouette_band(truth["hit"], k)) of
    every m of `methods`, with its keys, from one device call; the band is made once, on the device."""
    methods = list(methods)
    if not methods:
        return []
    out = []
    for r in _score(methods, truth, ("depth", "hit"), band_k=int(k)):
        n_mine, n_truth, n_both = r["n_method_hit"], r["n_reference_hit"], r["n_co_hit"]
        out.append({
            "iou": n_both / max(r["n_union"], 1),
            "core_iou": r["n_co_hit_core"] / max(r["n_union_core"], 1),
            "false_hit": (n_mine - n_both) / max(n_mine, 1),
            "false_miss": (n_truth - n_both) / max(n_truth, 1),
            "depth_rmse": r["depth_rmse"], "depth_med": r["depth_med"], "depth_p95": r["depth_p95"],
            "depth_signed": r["depth_signed"],
            "n_analytic_hit": n_truth, "n_method_hit": n_mine, "n_co_hit": n_both,
        })
    return out
