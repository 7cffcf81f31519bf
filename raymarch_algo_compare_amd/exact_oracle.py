"""Exact first-hit ground truth by closed-form ray / surface intersection -- the independent anchor of the oracle-trust
chain, on the GPU.

Every other ground truth here is a march (the interval oracle, the segment tracer, the affine range).  This one shares no
algorithm with them: each leaf of a hard-CSG scene program cuts the ray in a few closed intervals with closed-form end
points, union / intersection / subtraction are set algebra on those intervals, round / onion / scale over a sphere,
plane, torus or capsule only move the level at which the leaf is cut (csrc/rm_exact.h).  The first hit is the smallest
end point t > t_min of a maximal interval of { t : f(o + t d) <= 0 }: an entry, the exit when the eye is inside the
solid, or a contact of measure zero.

Scenes with an exact form (has_exact): catalogue ids 0-6, 8 and 14, the program twins of Bad Lipschitz Sphere and Bumpy
Sphere, and every registered scene program made of sphere, box, plane, cylinder, torus, capsule, union, subtract,
intersect and translate, with round / onion / scale directly over a sphere, plane, torus or capsule (not over a
combinator's result; at most three onions over one leaf; no torus cut where its tube closes the hole).  why_not gives the
reason for any other.

    cap = exact_capture("Hollow Cube (CSG)", RenderConfig(width=384, height=384))
    scoring.residual(interval_capture(...), cap)

The rays are the library's camera rays, so the maps line up pixel for pixel with interval_capture, GPURunner.capture and
HipCollector frames.  analytic.py (host NumPy, four scenes) stays as the host checker the tests compare this against.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import _native
from .interval_oracle import _camera, _scene_id

DEFAULT_T_MAX = 100.0
T_MIN = 1e-6     # analytic.py's: roots closer than this are behind / at the eye


def has_exact(scene) -> bool:
    """True when the scene has an exact form (needs no GPU)."""
    try:
        return _native.exact_supported(_scene_id(scene))
    except KeyError:
        return False


def why_not(scene) -> Optional[str]:
    """The reason the scene has no exact form; None when it has one (needs no GPU)."""
    try:
        sid = _scene_id(scene)
    except KeyError as e:
        return str(e.args[0])
    return _native.exact_refusal(sid)


def first_hit(ro, rd, scene, t_max: float = float("inf")) -> np.ndarray:
    """Exact first intersection t per ray (inf if none).  ro: (3,) or (M, 3); rd: (M, 3), used as given (not normalised:
    t scales by 1 / |rd|)."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    if len(rd) == 0:
        return np.empty(0)
    t, _, _ = _native.exact_march_rays(_scene_id(scene), ro, rd, _native.exact_config(t_max=t_max), want_normals=False)
    return t


def exact_capture(scene, render_cfg_or_camera, t_max: float = DEFAULT_T_MAX) -> Optional[Dict[str, np.ndarray]]:
    """Exact first-hit {depth (H, W) float64, hit (H, W) bool, normal (H, W, 3) float64, leaf (H, W) int32: the index in
    the scene's program of the primitive whose boundary was hit, -1 on a miss} on the library's camera rays; None for a
    scene without an exact form."""
    sid = _scene_id(scene)
    if not _native.exact_supported(sid):
        return None
    cam = _camera(render_cfg_or_camera)
    out = _native.exact_render(sid, cam.params14(), cam.width, cam.height, _native.exact_config(t_max=t_max))
    return {"depth": out["depth"], "hit": out["hit"] > 0, "normal": out["normal"], "leaf": out["leaf"]}
