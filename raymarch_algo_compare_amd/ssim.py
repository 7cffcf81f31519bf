"""The tertiary tier of capture scoring: SSIM of the depth, normal and colour images of a capture against a reference
capture, and the RMSE of the two colour images -- the four numbers the reference's metrics/scoring.py takes from skimage
(scoring.SSIM_KEYS), computed by the gfx950 kernels of csrc/rm_ssim.hip (rm_ssim_scores, include/rm_hip.h).

The definition (csrc/rm_ssim.h states it in full): Wang et al. 2004 with the defaults of
skimage.metrics.structural_similarity on 8-bit images -- 7 x 7 uniform window, sample covariances, C1 = (0.01 * 255)^2,
C2 = (0.03 * 255)^2, the mean over the windows that lie inside the image -- and a three-channel image scores the mean of
its channels.  The 8-bit images are made from a capture's float32 maps as the reference's data/capture_io.py makes them
(to_images below is that in NumPy, for tests and PNG writers; the kernels quantise on the fly); both depth images use
the REFERENCE capture's depth range over its hits.

Captures are dicts of (H, W) maps as everywhere in scoring.py: "hit", "depth", and optionally "normal" and "color"
(H, W, 3).  Maps are read as float32, the type the reference's captures have.  A map that either capture lacks gives
None in the scores that need it (the interval oracle's captures carry no colour), which is the reference's own key set
with compute_ssim=False for those keys.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, scoring

MIN_SIDE = 7      # the window


def _to_u8(x: np.ndarray) -> np.ndarray:
    x = np.nan_to_num(x, nan=0.0, posinf=1.0, neginf=0.0)
    return np.clip(x * np.float32(255.0), 0, 255).astype(np.uint8)


def depth_range(reference: Dict) -> Tuple[float, float]:
    """(min, max) of a capture's depth over its hits; (0, 1) without a hit."""
    hit = np.asarray(reference["hit"]) != 0
    if not hit.any():
        return 0.0, 1.0
    d = np.asarray(reference["depth"], dtype=np.float32)[hit]
    return float(d.min()), float(d.max())


def to_images(capture: Dict, drange: Tuple[float, float]) -> Dict[str, Optional[np.ndarray]]:
    """The uint8 images {"depth" (H, W), "normal" (H, W, 3), "color" (H, W, 3)} of a capture; None for a map it lacks.
    drange: the depth range both captures of a comparison share (depth_range of the reference capture)."""
    hit = np.asarray(capture["hit"]) != 0
    depth = np.asarray(capture["depth"], dtype=np.float32)
    lo, hi = float(drange[0]), float(drange[1])
    rng = np.float32(max(hi - lo, 1e-6))
    norm = np.clip((depth - np.float32(lo)) / rng, np.float32(0.0), np.float32(1.0))
    out = {"depth": _to_u8(np.where(hit, np.float32(1.0) - norm, np.float32(0.0))), "normal": None, "color": None}
    if capture.get("normal") is not None:
        n = np.asarray(capture["normal"], dtype=np.float32)
        out["normal"] = _to_u8(np.where(hit[..., None], n * np.float32(0.5) + np.float32(0.5), np.float32(0.0)))
    if capture.get("color") is not None:
        out["color"] = _to_u8(np.asarray(capture["color"], dtype=np.float32))
    return out


def _shared(methods: Sequence[Dict], reference: Dict, key: str) -> bool:
    """True when the reference and every method carry map `key`"""
    return reference.get(key) is not None and all(m.get(key) is not None for m in methods)


def ssim_scores_batch(methods: Sequence[Dict], reference: Dict) -> List[Dict[str, Optional[float]]]:
    """One {"depth_ssim", "normal_ssim", "color_ssim", "color_rmse"} per method, all scored against `reference` in one
    call (its images are made once).  A method's scores do not depend on the others in the batch."""
    methods = list(methods)
    if not methods:
        return []
    shape = np.shape(reference["hit"])
    for m in methods:
        if np.shape(m["hit"]) != shape:
            raise ValueError(f"shape mismatch: method {np.shape(m['hit'])} vs reference {shape}")
    if len(shape) != 2 or min(shape) < MIN_SIDE:
        raise ValueError(f"SSIM needs (H, W) maps with both sides >= {MIN_SIDE}, not {shape}")
    keys = ["depth", "hit"] + [k for k in ("normal", "color") if _shared(methods, reference, k)]
    pick = lambda c: {k: c[k] for k in keys}      # noqa: E731  (a map one side lacks is dropped on both)
    out = _native.ssim_scores(shape[1], shape[0], pick(reference), [pick(m) for m in methods])
    return [{k: (None if math.isnan(v) else float(v)) for k, v in zip(scoring.SSIM_KEYS, row)} for row in out]


def ssim_scores(method: Dict, reference: Dict) -> Dict[str, Optional[float]]:
    """{"depth_ssim", "normal_ssim", "color_ssim", "color_rmse"} of `method` against `reference`."""
    return ssim_scores_batch([method], reference)[0]


def score_capture_full(method: Dict, reference: Dict) -> Dict[str, Dict]:
    """scoring.score_capture(method, reference) with the tertiary tier (report["ssim"] is report["tertiary"]) filled in."""
    report = scoring.score_capture(method, reference, compute_ssim=False)
    report["ssim"].update(ssim_scores(method, reference))
    return report
