"""An error bar on the interval oracle, per ray: the certified first-hit bracket (csrc/rm_certify.h), on the GPU.

The interval oracle's depth is early by up to its tolerance, and where its enclosure never clears -- a probe across a
repeat cell's boundary, a tangent CSG cut -- it reports a hit the pointwise SDF does not have.  The certified march returns,
per ray, a bracket [t_lo, t_hi] and a status:

    MISS (0)  all of [0, t_max] is proven free of the solid                          t_lo = t_hi = inf
    HIT  (1)  [0, t_lo) is proven free, g(t_hi) < 0 was computed, t_hi - t_lo <= width
    OPEN (2)  anything else (no witness, a probe shrunk to rounding, the step budget): the bracket reached, still sound

Every part of [0, t_lo) was discharged by a proof: the interval enclosure's lo > 0, or g(a) > K h with K the dual-interval
bound of |g'| over the probe (the segment tracer's rule).  The second proof rests on g being continuous and on `l_global`
bounding |grad f| times the direction's length: certified_capture and oracle_error_bar take it from the scene's Lipschitz
bound (2 for Bad Lipschitz Sphere's twin), certified_first_hit from its argument.  Rounding is to nearest.

    bar = oracle_error_bar("Pillar Forest", RenderConfig(width=384, height=384))
    python -m raymarch_algo_compare_amd.sweep --oracle interval --certify ...

Scenes: as the interval oracle (has_certify): catalogue ids, registered programs and twins.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from . import _native, registry
from .interval_oracle import DEFAULT_T_MAX, DEFAULT_TOL, _camera, _scene_id, interval_capture

MISS, HIT, OPEN = _native.RM_CERTIFY_MISS, _native.RM_CERTIFY_HIT, _native.RM_CERTIFY_OPEN
STATUS_NAMES = {MISS: "miss", HIT: "hit", OPEN: "open"}
FALSE_HIT_GAP = 1e-3      # a proven-free stretch this far past the oracle's depth is no matter of its tolerance


def has_certify(scene) -> bool:
    """True when the scene can be certified (needs no GPU): the scenes of the interval oracle."""
    try:
        return _native.certify_supported(_scene_id(scene))
    except KeyError:
        return False


def _lipschitz(scene, sid: int) -> float:
    """the scene's own Lipschitz bound where the registry knows one (a registered program carries its own), at least 1"""
    info = scene if isinstance(scene, registry.SceneInfo) else None
    if info is None and 0 <= sid < len(registry.SCENES):
        info = registry.SCENES[sid]
    if info is None:
        info = next((s for s in registry.get_all_scenes() if int(s.id) == sid), None)
    bound = info.known_lipschitz_bound() if info is not None else None
    return max(1.0, float(bound or 1.0))


def certified_first_hit(ro, rd, scene, t_max: float = DEFAULT_T_MAX, width: float = 0.0, l_global: float = 0.0,
                        max_steps: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(t_lo, t_hi, status, steps) per ray.  ro: (3,) or (M, 3); rd: (M, 3), used as given (not normalised: pass
    l_global = the scene's Lipschitz bound times |rd|; 0 = 1).  width 0: 1e-10 (1 + t_lo)."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    ro = np.broadcast_to(np.asarray(ro, dtype=np.float64), rd.shape)
    if len(rd) == 0:
        return np.empty(0), np.empty(0), np.empty(0, np.uint8), np.empty(0, np.int32)
    cfg = _native.certify_config(t_max=t_max, width=width, l_global=l_global, max_steps=max_steps)
    return _native.certify_march_rays(_scene_id(scene), ro, rd, cfg)


def certified_capture(scene, render_cfg_or_camera, t_max: float = DEFAULT_T_MAX, width: float = 0.0, bound_radius: float = 0.0,
                      l_global: float = 0.0, cfg: Optional["_native.RmCertifyConfig"] = None) -> Optional[Dict]:
    """{t_lo, t_hi (H, W) float64, status (H, W) uint8, steps (H, W) int32, capture: {depth = t_hi (0 off HIT pixels), hit =
    (status == HIT)}} on the library's camera rays; None for a scene without an interval extension.  `capture` is what
    scoring.py consumes.  l_global 0: the scene's Lipschitz bound (at least 1).  `cfg` replaces the other arguments."""
    sid = _scene_id(scene)
    if not _native.certify_supported(sid):
        return None
    cam = _camera(render_cfg_or_camera)
    if cfg is None:
        cfg = _native.certify_config(t_max=t_max, width=width, bound_radius=bound_radius,
                                     l_global=l_global if l_global else _lipschitz(scene, sid))
    out = _native.certify_render(sid, cam.params14(), cam.width, cam.height, cfg)
    hit = out["status"] == HIT
    return {"t_lo": out["t_lo"], "t_hi": out["t_hi"], "status": out["status"], "steps": out["steps"],
            "capture": {"depth": np.where(hit, out["t_hi"], 0.0), "hit": hit}}


def error_bar(cert: Dict, oracle: Dict) -> Dict:
    """The error bar of one interval-oracle capture from the certified capture of the same rays (host arithmetic; no GPU):
    the counts per status, the oracle's hits that are proven free (`false_hits`: the ray is a MISS, or its t_lo lies more
    than `FALSE_HIT_GAP` past the oracle's depth), and t_hi - t_interval (median, p95, max) over the HIT pixels the oracle hits
    too (NaN without any): where the oracle's hit is a false one on a ray that hits further on, the lag is that distance."""
    st = cert["status"]
    o_hit = np.asarray(oracle["hit"], dtype=bool)
    false = o_hit & ((st == MISS) | (cert["t_lo"] - oracle["depth"] > FALSE_HIT_GAP))
    sel = o_hit & (st == HIT)
    lag = (cert["t_hi"] - oracle["depth"])[sel]
    stat = (lambda f: float(f(lag))) if lag.size else (lambda f: float("nan"))
    return {"n_pixels": int(st.size), "n_miss": int((st == MISS).sum()), "n_hit": int((st == HIT).sum()),
            "n_open": int((st == OPEN).sum()), "n_oracle_hit": int(o_hit.sum()), "false_hits": int(false.sum()),
            "oracle_hit_open": int((o_hit & (st == OPEN)).sum()), "oracle_miss_hit": int((~o_hit & (st == HIT)).sum()),
            "lag_median": stat(np.median), "lag_p95": stat(lambda v: np.percentile(v, 95)), "lag_max": stat(np.max),
            "steps_median": float(np.median(cert["steps"])), "steps_max": int(cert["steps"].max())}


def oracle_error_bar(scene, render_cfg_or_camera, t_max: float = DEFAULT_T_MAX, tol: float = DEFAULT_TOL,
                     bound_radius: float = 0.0) -> Optional[Dict]:
    """error_bar of the interval oracle's frame of `scene` at tolerance `tol` (both frames with the same prune); None for a
    scene without an interval extension."""
    cert = certified_capture(scene, render_cfg_or_camera, t_max=t_max, bound_radius=bound_radius)
    if cert is None:
        return None
    return error_bar(cert, interval_capture(scene, render_cfg_or_camera, t_max=t_max, tol=tol, bound_radius=bound_radius))
