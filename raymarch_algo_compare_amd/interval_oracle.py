"""Sound first-hit ground truth by interval root isolation -- the reference's gpu/interval_oracle.py, on the GPU.

Each ray marches segments [t, t + h]: the interval extension of the scene's SDF over the segment's box (csrc/
rm_interval.h) proves a segment empty when its lower bound is > 0, so the march cannot tunnel through thin features the
way a sampling marcher can; a non-empty segment is halved until h <= tol, and the ray hits at t.  Scenes with an
extension: the 14 catalogue scenes that are compositions of primitives.py (has_interval) and every registered scene
program.  Sphere, Grazing Plane, Cube and Thin Torus are the reference's INTERVAL_SCENES bit for bit.

    cap = interval_capture("Thin Torus", RenderConfig(width=384, height=384))
    scoring.score_capture(GPURunner().capture(...), cap, compute_ssim=False)

The rays are the library's camera rays (the ones rm_render marches), so the maps line up pixel for pixel with
GPURunner.capture and HipCollector frames.  Scenes may be given by name, id or SceneInfo (a registered program too).
Rounding is to nearest, as in the reference: the enclosure is exact in real arithmetic only.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from . import _native, registry
from .camera import Camera
from .config import RenderConfig

# Bounding-sphere radius per scene (origin-centred) of the reference's pre-prune; None: no prune.  The library applies
# these itself (RmIntervalConfig.bound_radius = 0).
SCENE_BOUND: Dict[str, Optional[float]] = {
    "Sphere": 1.05,
    "Cube": 1.7421,        # sqrt(3) + slack
    "Thin Torus": 1.65,    # R + r + slack
    "Grazing Plane": None,
}

DEFAULT_T_MAX = 100.0
DEFAULT_TOL = 1e-5


def _scene_id(scene) -> int:
    if isinstance(scene, registry.SceneInfo):
        return int(scene.id)
    if isinstance(scene, (int, np.integer)):
        return int(scene)
    info = registry.find_scene_exact(scene) or registry.get_scene_by_name(scene)
    if info is None:
        raise KeyError(f"unknown scene {scene!r}")
    return int(info.id)


def has_interval(scene) -> bool:
    """True when the scene has an interval extension (needs no GPU)."""
    try:
        return _native.interval_supported(_scene_id(scene))
    except KeyError:
        return False


def interval_sdf(scene, lo, hi) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) enclosure of the scene's SDF over each box [lo, hi] (corners (..., 3)); result shape (...)."""
    lo = np.asarray(lo, dtype=np.float64)
    out_lo, out_hi = _native.interval_sdf_eval(_scene_id(scene), lo, hi)
    return out_lo.reshape(lo.shape[:-1]), out_hi.reshape(lo.shape[:-1])


def _config(t_max, tol, **kw) -> "_native.RmIntervalConfig":
    return _native.interval_config(t_max=t_max, tol=tol, **kw)


def first_hit(ro, rd, scene, t_max: float = DEFAULT_T_MAX, tol: float = DEFAULT_TOL) -> np.ndarray:
    """Nearest provable intersection t per ray (inf if none).  ro: (3,) or (M, 3); rd: (M, 3), used as given (not
    normalised, as the reference)."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    if len(rd) == 0:
        return np.empty(0)
    t, _, _ = _native.interval_march_rays(_scene_id(scene), ro, rd, _config(t_max, tol), want_normals=False)
    return t


def _camera(view) -> Camera:
    if isinstance(view, Camera):
        return view
    if isinstance(view, RenderConfig):
        return Camera(view.camera_position, view.camera_target, view.camera_up, view.fov_degrees, view.width, view.height)
    raise TypeError("interval_capture takes a RenderConfig or a Camera")


def interval_capture(scene, render_cfg_or_camera, t_max: float = DEFAULT_T_MAX, tol: float = DEFAULT_TOL,
                     bound_radius: float = 0.0) -> Optional[Dict[str, np.ndarray]]:
    """Sound first-hit {depth (H, W) float64, hit (H, W) bool, normal (H, W, 3) float64, steps (H, W) int32} on the
    library's camera rays; None for a scene without an interval extension.  bound_radius: 0 = the library's prune
    (SCENE_BOUND), > 0 = this origin-centred sphere, < 0 = no prune."""
    sid = _scene_id(scene)
    if not _native.interval_supported(sid):
        return None
    cam = _camera(render_cfg_or_camera)
    out = _native.interval_render(sid, cam.params14(), cam.width, cam.height, _config(t_max, tol, bound_radius=bound_radius))
    return {"depth": out["depth"], "hit": out["hit"] > 0, "normal": out["normal"], "steps": out["steps"]}
