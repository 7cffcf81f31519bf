"""Revised affine arithmetic as a sound range -- the reference's gpu/affine.py, on the GPU.

The third sound evaluation of a scene over a ray segment, next to the interval oracle's box and the segment tracer's dual
interval: a quantity is tracked as x0 + x1 * eps + e * [-1, 1] with one noise symbol eps for the march parameter
(csrc/rm_affine.h).  The interval oracle's march runs with that range plugged in; what is measured is tightness -- the SDF
segment evaluations each range needs to reach the same hit map.  Two modes:

    "affine"  the reference's range: tighter than the interval on the smooth chain (square, sqrt: Sphere), looser wherever
              a non-smooth op drops to a hull (Cube, Thin Torus);
    "meet"    the intersection of the affine and the interval range of each probe: sound because both are, per probe at
              least as tight as either, at the price of one more walk over the scene's program.

    cap = capture("Sphere", RenderConfig(width=384, height=384), "meet")
    python -m raymarch_algo_compare_amd.affine_range --scenes "Sphere,Cube" --res 384 --out affine_revaa.json

Scenes: as the interval oracle (has_affine), registered scene programs included; Sphere, Grazing Plane, Cube and Thin
Torus are the reference's COMPONENT_SCENES over its AAForm bit for bit.  The rays are the library's camera rays, so the
maps line up pixel for pixel with interval_capture.  Eval totals are counts, not times: tools/affine_cost.py times the
kernels.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, registry, scoring
from .config import RenderConfig
from .interval_oracle import DEFAULT_T_MAX, DEFAULT_TOL, _camera, _config, _scene_id, interval_capture

MODES = {"affine": _native.RM_RANGE_AFFINE, "meet": _native.RM_RANGE_MEET}


def _mode(mode) -> int:
    if mode in MODES:
        return MODES[mode]
    if mode in MODES.values():
        return int(mode)
    raise ValueError(f"unknown range mode {mode!r}: one of {sorted(MODES)}")


def has_affine(scene) -> bool:
    """True when the scene has an affine extension (needs no GPU)."""
    try:
        return _native.affine_supported(_scene_id(scene))
    except KeyError:
        return False


def affine_range(scene, ro, rd, t0, t1, mode="affine") -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of the scene's SDF over the segments ro + rd * [t0, t1] (rd (M, 3) as given, ro (3,) or (M, 3), t0 / t1 (M,))."""
    return _range(scene, ro, rd, t0, t1, mode, False)[0].T


def affine_form(scene, ro, rd, t0, t1) -> Dict[str, np.ndarray]:
    """{x0, x1, e, lo, hi} of the affine form of the scene's SDF over the same segments."""
    rng, form = _range(scene, ro, rd, t0, t1, "affine", True)
    return {"x0": form[:, 0], "x1": form[:, 1], "e": form[:, 2], "lo": rng[:, 0], "hi": rng[:, 1]}


def _range(scene, ro, rd, t0, t1, mode, want_form):
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    t0 = np.broadcast_to(np.asarray(t0, dtype=np.float64), (len(rd),))
    t1 = np.broadcast_to(np.asarray(t1, dtype=np.float64), (len(rd),))
    segs = np.concatenate([ro, rd, t0[:, None], t1[:, None]], axis=1)
    return _native.affine_range_eval(_scene_id(scene), segs, _mode(mode), want_form)


def march_count(ro, rd, scene, mode="affine", t_max: float = DEFAULT_T_MAX, tol: float = DEFAULT_TOL) -> Tuple[np.ndarray, int]:
    """(t_hit (inf on a miss), total range evaluations) of the rays.  ro: (3,) or (M, 3); rd: (M, 3), used as given."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    if len(rd) == 0:
        return np.empty(0), 0
    t, steps = _native.affine_march_rays(_scene_id(scene), ro, rd, _mode(mode), _config(t_max, tol))
    return t, int(steps.sum())


def capture(scene, width_or_view, height: Optional[int] = None, mode="affine", t_max: float = DEFAULT_T_MAX,
            tol: float = DEFAULT_TOL, bound_radius: float = 0.0) -> Optional[Dict]:
    """{depth (H, W) float64, hit (H, W) bool, steps (H, W) int32 (0: pruned), evals: the sum of steps} of the march with
    the range of `mode`; None for a scene without an extension.  The view is a RenderConfig or a Camera, or a width and a
    height with the scene's own camera."""
    sid = _scene_id(scene)
    if not _native.affine_supported(sid):
        return None
    view = width_or_view if height is None else _render_config(registry.get_scene_by_id(sid), int(width_or_view), int(height))
    cam = _camera(view)
    out = _native.affine_render(sid, cam.params14(), cam.width, cam.height, _mode(mode), _config(t_max, tol, bound_radius=bound_radius))
    return {"depth": out["depth"], "hit": out["hit"] > 0, "steps": out["steps"], "evals": int(out["steps"].sum(dtype=np.int64))}


def _render_config(scene, width: int, height: int) -> RenderConfig:
    rc = RenderConfig(width=width, height=height)
    if scene is not None and scene.camera_position is not None:
        rc.camera_position = scene.camera_position
    if scene is not None and scene.camera_target is not None:
        rc.camera_target = scene.camera_target
    return rc


def evaluate(scene_names: Sequence[str], width: int = 384, height: int = 384, verbose: bool = False) -> Dict:
    """The reference's report: per scene `affine` and `interval` ({iou, core_iou, evals}; scoring.residual against
    interval_capture, silhouette band k = 2) and eval_speedup_aa_over_ia, plus `meet` and eval_speedup_meet_over_ia.  The
    interval side is interval_capture itself and its step sum.  Scenes without an extension are left out."""
    report: Dict = {"resolution": [width, height], "scenes": {}}
    for name in scene_names:
        scene = registry.find_scene_exact(name) or registry.get_scene_by_name(name)
        if scene is None or not has_affine(scene):
            if verbose:
                print(f"  [skip] {name}: no interval extension")
            continue
        rc = _render_config(scene, width, height)
        gold = interval_capture(scene, rc)
        band = scoring.silhouette_band(gold["hit"], k=2)
        entry: Dict = {}
        for key, cap in (("affine", capture(scene, rc, mode="affine")), ("interval", gold), ("meet", capture(scene, rc, mode="meet"))):
            res = scoring.residual(cap["hit"], cap["depth"], gold["hit"], gold["depth"], band)
            entry[key] = {"iou": res["iou"], "core_iou": res["core_iou"], "evals": int(cap["steps"].sum(dtype=np.int64))}
        entry["eval_speedup_aa_over_ia"] = entry["interval"]["evals"] / max(entry["affine"]["evals"], 1)
        entry["eval_speedup_meet_over_ia"] = entry["interval"]["evals"] / max(entry["meet"]["evals"], 1)
        report["scenes"][scene.name] = entry
        if verbose:
            print(f"=== {scene.name} ===")
            for key in ("affine", "interval", "meet"):
                e = entry[key]
                print(f"  {key:8s}: IoU {e['iou']:.4f} (core {e['core_iou']:.4f})  evals {e['evals']:,}")
            print(f"  interval / affine {entry['eval_speedup_aa_over_ia']:.2f}   interval / meet {entry['eval_speedup_meet_over_ia']:.2f}")
    return report


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(description="Revised affine arithmetic against interval arithmetic: SDF segment evaluations.")
    p.add_argument("--scenes", default="Sphere,Grazing Plane,Cube,Thin Torus")
    p.add_argument("--res", type=int, default=384)
    p.add_argument("--out", default="affine_revaa.json")
    a = p.parse_args(argv)
    report = evaluate([s.strip() for s in a.scenes.split(",") if s.strip()], a.res, a.res, verbose=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(report, f, indent=2)
    print(f"saved -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
