"""The sound segment tracer -- the reference's gpu/faithful_offline.py and gpu/interval_autodiff.py, on the GPU.

The accuracy / cost ceiling of the comparison: a Galin-style segment tracer whose directional Lipschitz bound K over the
probe [t, t + h] is not sampled (the `Segment` strategy's three samples tunnel) but proven, by a dual interval -- the
enclosure of the SDF's value and of its derivative along the ray (csrc/rm_segment.h).  The step |f| / K cannot pass the
surface, so the tracer reaches the interval oracle's hit mask with a handful of steps.  Scenes: as the interval oracle
(has_segment); Sphere, Grazing Plane, Cube and Thin Torus are the reference's COMPONENT_SCENES bit for bit.

    cap = faithful_capture("Thin Torus", RenderConfig(width=384, height=384))
    python -m raymarch_algo_compare_amd.faithful_segment --scenes "Sphere,Thin Torus" --res 384 --out report.json

The rays are the library's camera rays, so the maps line up pixel for pixel with interval_capture and GPURunner.capture.
`l_global` bounds |grad f| times the length of the direction: the default 1 holds for exact SDFs and unit directions.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, registry, scoring
from .config import RenderConfig
from .interval_oracle import DEFAULT_T_MAX, _camera, _scene_id, interval_capture

DEFAULT_TOL = 1e-4


def has_segment(scene) -> bool:
    """True when the scene has a dual-interval extension (needs no GPU)."""
    try:
        return _native.segment_supported(_scene_id(scene))
    except KeyError:
        return False


def segment_sdf(scene, ro, rd, t0, t1) -> Dict[str, np.ndarray]:
    """{val_lo, val_hi, der_lo, der_hi} of the scene's SDF over the segments ro + rd * [t0, t1] (rd (M, 3) as given, ro (3,)
    or (M, 3), t0 / t1 (M,)): the value enclosure and the enclosure of d/dt along the ray."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    t0 = np.broadcast_to(np.asarray(t0, dtype=np.float64), (len(rd),))
    t1 = np.broadcast_to(np.asarray(t1, dtype=np.float64), (len(rd),))
    out = _native.segment_sdf_eval(_scene_id(scene), np.concatenate([ro, rd, t0[:, None], t1[:, None]], axis=1))
    return {"val_lo": out[:, 0], "val_hi": out[:, 1], "der_lo": out[:, 2], "der_hi": out[:, 3]}


def segment_trace(ro, rd, scene, t_max: float = DEFAULT_T_MAX, tol: float = DEFAULT_TOL,
                  l_global: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """(t_hit (inf on a miss), iters) per ray.  ro: (3,) or (M, 3); rd: (M, 3), used as given."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    if len(rd) == 0:
        return np.empty(0), np.empty(0, np.int32)
    t, iters, _ = _native.segment_march_rays(_scene_id(scene), ro, rd, _native.segment_config(t_max=t_max, tol=tol, l_global=l_global))
    return t, iters


def faithful_capture(scene, render_cfg_or_camera, tol: float = DEFAULT_TOL, bound_radius: float = 0.0,
                     cfg: Optional["_native.RmSegmentConfig"] = None) -> Optional[Dict[str, np.ndarray]]:
    """{depth (H, W) float64, hit (H, W) bool, iters (H, W) int32 (0: pruned), cursor (H, W) float64 (the final t)} on the
    library's camera rays; None for a scene without an extension.  `cfg` replaces tol / bound_radius when given."""
    sid = _scene_id(scene)
    if not _native.segment_supported(sid):
        return None
    cam = _camera(render_cfg_or_camera)
    if cfg is None:
        cfg = _native.segment_config(tol=tol, bound_radius=bound_radius)
    out = _native.segment_render(sid, cam.params14(), cam.width, cam.height, cfg)
    return {"depth": out["depth"], "hit": out["hit"] > 0, "iters": out["iters"], "cursor": out["cursor"]}


def cost(cap: Dict[str, np.ndarray]) -> Dict[str, float]:
    """iters median / p95 / max over the hit rays of a faithful_capture (0 without a hit): the reference's `cost`."""
    it = cap["iters"][cap["hit"]]
    if it.size == 0:
        return {"iters_median": 0.0, "iters_p95": 0.0, "iters_max": 0}
    return {"iters_median": float(np.median(it)), "iters_p95": float(np.percentile(it, 95)), "iters_max": int(it.max())}


def evaluate(scene_names: Sequence[str], width: int = 384, height: int = 384, verbose: bool = False) -> Dict:
    """The reference's report: per scene `accuracy_vs_oracle` (scoring.residual against interval_capture, silhouette band
    k = 2) and `cost`.  Scenes without an extension are left out."""
    report: Dict = {"resolution": [width, height], "scenes": {}}
    for name in scene_names:
        scene = registry.find_scene_exact(name) or registry.get_scene_by_name(name)
        if scene is None or not has_segment(scene):
            if verbose:
                print(f"  [skip] {name}: no interval extension")
            continue
        rc = RenderConfig(width=width, height=height)
        if scene.camera_position is not None:
            rc.camera_position = scene.camera_position
        if scene.camera_target is not None:
            rc.camera_target = scene.camera_target
        gold = interval_capture(scene, rc)
        fc = faithful_capture(scene, rc)
        res = scoring.residual(fc["hit"], fc["depth"], gold["hit"], gold["depth"], scoring.silhouette_band(gold["hit"], k=2))
        report["scenes"][scene.name] = {"accuracy_vs_oracle": res, "cost": cost(fc)}
        if verbose:
            c = report["scenes"][scene.name]["cost"]
            print(f"{scene.name:24s} IoU {res['iou']:.4f} (core {res['core_iou']:.4f}) depth med {res['depth_med']:.2e}  "
                  f"steps to hit: median {c['iters_median']:.0f} p95 {c['iters_p95']:.0f} max {c['iters_max']}")
    return report


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(description="Sound segment tracer: the accuracy / cost ceiling against the interval oracle.")
    p.add_argument("--scenes", default="Sphere,Grazing Plane,Cube,Thin Torus")
    p.add_argument("--res", type=int, default=384)
    p.add_argument("--out", default="faithful_segment.json")
    a = p.parse_args(argv)
    report = evaluate([s.strip() for s in a.scenes.split(",") if s.strip()], a.res, a.res, verbose=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(report, f, indent=2)
    print(f"saved -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
