"""Accuracy of a capture against a ground-truth capture, with the metric names and result keys of the reference's
metrics/scoring.py.

Metrics, in the reference's order of importance:
  * primary -- the hit masks: intersection over union (the ranking metric, PRIMARY_METRIC), and the fractions of all
    pixels that the method hits and the truth misses (false hits) or the other way round (false misses);
  * secondary -- where both captures hit: the absolute depth error (rmse, mae, 95th percentile) and the angle between
    the normals (mean, 95th percentile, degrees);
  * tertiary -- SSIM of depth, normal and colour images.  The reference computes them with skimage, which this project
    does not use: compute_ssim=True raises NotImplementedError and the tertiary keys hold None.

Captures are dicts of equally shaped maps: "hit" (bool), "depth", "normal" (..., 3) -- GPURunner.capture,
interval_oracle.interval_capture and analytic maps all qualify.  score_capture returns the grouped view (primary /
secondary / tertiary) and the flat keys older callers read (hit / depth / normal / ssim).
"""
from __future__ import annotations

from typing import Dict

import numpy as np

PRIMARY_METRIC = "iou"
SSIM_KEYS = ("depth_ssim", "normal_ssim", "color_ssim", "color_rmse")
NAN = float("nan")


def _mask(a) -> np.ndarray:
    return np.asarray(a, dtype=bool)


def _cohit(method: Dict, reference: Dict) -> np.ndarray:
    """pixels both captures hit"""
    return _mask(method["hit"]) & _mask(reference["hit"])


def _hit_metrics(m_hit, r_hit) -> Dict[str, float]:
    """IoU of the two hit masks (1.0 when neither hits anything), false-hit and false-miss fractions of all pixels, and
    the fraction of pixels on which the masks agree."""
    mine, truth = _mask(m_hit), _mask(r_hit)
    pixels = mine.size
    both = np.count_nonzero(mine & truth)
    only_mine = np.count_nonzero(mine & ~truth)
    only_truth = np.count_nonzero(truth & ~mine)
    covered = both + only_mine + only_truth
    return {
        "false_hit_rate": only_mine / pixels,
        "false_miss_rate": only_truth / pixels,
        "iou": both / covered if covered else 1.0,
        "agreement": (pixels - only_mine - only_truth) / pixels,
    }


def _spread(values: np.ndarray) -> Dict[str, float]:
    """mean and 95th percentile (numpy's linear interpolation) of a non-empty sample"""
    return {"mean": float(values.mean()), "p95": float(np.percentile(values, 95))}


def _depth_metrics(method: Dict, reference: Dict) -> Dict[str, float]:
    """|depth - reference depth| over the co-hit pixels (NaN statistics and n_pixels = 0 without any)."""
    sel = _cohit(method, reference)
    count = int(np.count_nonzero(sel))
    if count == 0:
        return {"rmse": NAN, "mae": NAN, "p95": NAN, "n_pixels": 0}
    gap = np.abs(np.asarray(method["depth"], dtype=np.float64)[sel] - np.asarray(reference["depth"], dtype=np.float64)[sel])
    s = _spread(gap)
    return {"rmse": float(np.sqrt(np.square(gap).mean())), "mae": s["mean"], "p95": s["p95"], "n_pixels": count}


def _normal_angle_error(method: Dict, reference: Dict) -> Dict[str, float]:
    """angle in degrees between the (unit) normals over the co-hit pixels; the cosine is clamped to [-1, 1]."""
    sel = _cohit(method, reference)
    if not sel.any():
        return {"mean_deg": NAN, "p95_deg": NAN}
    n_m = np.asarray(method["normal"], dtype=np.float64)[sel]
    n_r = np.asarray(reference["normal"], dtype=np.float64)[sel]
    cosine = np.minimum(np.maximum(np.einsum("ij,ij->i", n_m, n_r), -1.0), 1.0)
    s = _spread(np.rad2deg(np.arccos(cosine)))
    return {"mean_deg": s["mean"], "p95_deg": s["p95"]}


def score_capture(method: Dict, reference: Dict, *, compute_ssim: bool = False) -> Dict[str, Dict]:
    """The accuracy report of `method` against `reference` (same resolution and camera)."""
    if compute_ssim:
        raise NotImplementedError("SSIM needs skimage, which this project does not use: pass compute_ssim=False")
    shape_m, shape_r = np.shape(method["hit"]), np.shape(reference["hit"])
    if shape_m != shape_r:
        raise ValueError(f"shape mismatch: method {shape_m} vs reference {shape_r}")
    report = {
        "hit": _hit_metrics(method["hit"], reference["hit"]),
        "depth": _depth_metrics(method, reference),
        "normal": _normal_angle_error(method, reference),
        "ssim": dict.fromkeys(SSIM_KEYS),
    }
    report["primary"] = report["hit"]
    report["secondary"] = {"depth": report["depth"], "normal": report["normal"]}
    report["tertiary"] = report["ssim"]
    return report


# ---- the calibration residual (the reference's gpu/oracle_calibration.py: silhouette_band, residual) ---------------------

def _grow(mask: np.ndarray, k: int) -> np.ndarray:
    """the mask grown k times by its 4-neighbourhood"""
    m = _mask(mask).copy()
    for _ in range(int(k)):
        g = m.copy()
        g[1:, :] |= m[:-1, :]
        g[:-1, :] |= m[1:, :]
        g[:, 1:] |= m[:, :-1]
        g[:, :-1] |= m[:, 1:]
        m = g
    return m


def silhouette_band(hit, k: int = 2) -> np.ndarray:
    """Pixels within k (4-connected steps) of the boundary of a hit mask: hit pixels next to a miss and misses next to a
    hit, grown k times."""
    h = _mask(hit)
    edge = (_grow(~h, 1) & h) | (_grow(h, 1) & ~h)
    return _grow(edge, k)


def residual(method_hit, method_depth, truth_hit, truth_depth, band) -> Dict[str, float]:
    """A method's frame against the truth's, with the reference's keys: iou (0 over an empty union, as the reference
    divides by max(union, 1)), core_iou (outside `band`), false_hit (of the method's hits), false_miss (of the truth's),
    depth_rmse / depth_med / depth_p95 / depth_signed over the co-hit pixels (NaN without any) and the three counts."""
    mine, truth, core = _mask(method_hit), _mask(truth_hit), ~_mask(band)
    both, either = mine & truth, mine | truth
    n_mine, n_truth, n_both = int(mine.sum()), int(truth.sum()), int(both.sum())
    out = {
        "iou": n_both / max(int(either.sum()), 1),
        "core_iou": int((both & core).sum()) / max(int((either & core).sum()), 1),
        "false_hit": int((mine & ~truth).sum()) / max(n_mine, 1),
        "false_miss": int((truth & ~mine).sum()) / max(n_truth, 1),
    }
    if n_both:
        gap = np.asarray(method_depth, dtype=np.float64)[both] - np.asarray(truth_depth, dtype=np.float64)[both]
        mag = np.abs(gap)
        out.update(depth_rmse=float(np.sqrt(np.mean(gap * gap))), depth_med=float(np.median(mag)),
                   depth_p95=float(np.percentile(mag, 95)), depth_signed=float(np.mean(gap)))
    else:
        out.update(depth_rmse=NAN, depth_med=NAN, depth_p95=NAN, depth_signed=NAN)
    out.update(n_analytic_hit=n_truth, n_method_hit=n_mine, n_co_hit=n_both)
    return out
