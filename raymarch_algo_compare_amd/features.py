"""Strategy-independent discovery features of a (scene, viewpoint), computed on the device.

The reference's research layer (report/features.py, "Phase 6.1") describes each (scene, viewpoint) by seven numbers that a
sweep's rows are joined against, so that one can ask what about a scene predicts which method wins there:

  view features, from one dense-march capture (rm_view_features, csrc/rm_features.hip)
    hit_rate           hit pixels / pixels
    grazing_frac       hits with |ray . normal| < GRAZING_COS, over the hits
    silhouette_cplx    hit pixels with a non-hit 4-neighbour (the image edge counts as one) / sqrt(hits)
    hardness_mean      mean SDF evaluations of the dense march over the hit rays
    hardness_cv        their population standard deviation / mean
  intrinsic features, from samples of the scene's SDF inside the padded box of the visible hit points
  (rm_intrinsic_features: the samples are generated, evaluated and reduced on the device, nothing but the random draws
  goes up and nothing but the results comes down)
    lipschitz_p99      99th percentile of |grad f| by central differences at uniform points
    thin_slab          median length of the solid (f < 0) runs along random chords, in box diagonals

The random draws (sample_sets) are NumPy's, in the reference's order, so a seed gives the reference's samples.  The
`*_numpy` functions state the same definitions over _native.sdf_eval in NumPy, as scoring.py does for rm_score_captures:
they are what the device is tested against and are never called in its place.

    python -m raymarch_algo_compare_amd.features --scenes Sphere,Mandelbulb --res 256 --out features.jsonl
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

GRAZING_COS = 0.20          # |cos(ray, n)| below this is grazing
_LIP_SAMPLES = 1500         # points of the Lipschitz estimate
_LIP_EPS = 1e-4             # central-difference step
_CHORDS = 240               # random chords of the thin-slab measurement
_CHORD_STEPS = 160          # samples per chord
MIN_HITS = 8                # fewer hit pixels: no box, NaN intrinsic features

VIEW_KEYS = ("hit_rate", "grazing_frac", "silhouette_cplx", "hardness_mean", "hardness_cv")
INTRINSIC_KEYS = ("lipschitz_p99", "thin_slab")
FEATURE_KEYS = VIEW_KEYS + INTRINSIC_KEYS

# the dense-march capture the view features are taken from (the reference's groundtruth.dense_march_config / _params)
DENSE_STRATEGY_KEY = "Dense-March"
DENSE_MAX_ITERATIONS = 40000
DENSE_HIT_THRESHOLD = 1e-6
DENSE_PARAMS = {"stepScale": 0.5, "minStep": 0.002}


# ---- samples ----------------------------------------------------------------------------------------------------------

def padded_box(hit_lo, hit_hi) -> Tuple[np.ndarray, np.ndarray, float]:
    """(lo, hi, diag) of the sampling box of hit points spanning [hit_lo, hit_hi]: each side padded by 0.05 * span + 1e-3;
    diag = |span| of the unpadded box, 1.0 when that is 0."""
    lo, hi = np.asarray(hit_lo, np.float64), np.asarray(hit_hi, np.float64)
    span = hi - lo
    diag = float(np.linalg.norm(span)) or 1.0
    pad = 0.05 * span + 1e-3
    return lo - pad, hi + pad, diag


def sample_sets(lo, hi, rng: np.random.Generator, n_lip: Optional[int] = None, n_chords: Optional[int] = None,
                chord_steps: Optional[int] = None) -> Dict[str, np.ndarray]:
    """One sample set in the box [lo, hi], drawn in the reference's order: rng.random((n_lip, 3)) once, then rng.random(3)
    twice per chord.  pts (n_lip, 3), chords (n_chords, 6: a, b), seglen (n_chords: |b - a| as np.linalg.norm gives it),
    ts (chord_steps: np.linspace(0, 1))."""
    n_lip = _LIP_SAMPLES if n_lip is None else int(n_lip)
    n_chords = _CHORDS if n_chords is None else int(n_chords)
    chord_steps = _CHORD_STEPS if chord_steps is None else int(chord_steps)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pts = lo + rng.random((n_lip, 3)) * (hi - lo)
    ts = np.linspace(0.0, 1.0, chord_steps)
    chords, seglen = np.empty((n_chords, 6)), np.empty(n_chords)
    for c in range(n_chords):
        a = lo + rng.random(3) * (hi - lo)
        b = lo + rng.random(3) * (hi - lo)
        chords[c, :3], chords[c, 3:] = a, b
        seglen[c] = float(np.linalg.norm(b - a))
    return {"pts": pts, "chords": chords, "seglen": seglen, "ts": ts}


def _stack(sets: Sequence[Dict[str, np.ndarray]]):
    """the arrays of `sets` as rm_intrinsic_features takes them; every set must have the shape of the first"""
    if not sets:
        raise ValueError("no sample set")
    pts = np.ascontiguousarray(np.stack([np.asarray(s["pts"], np.float64).reshape(-1, 3) for s in sets]))
    chords = np.ascontiguousarray(np.stack([np.asarray(s["chords"], np.float64).reshape(-1, 6) for s in sets]))
    seglen = np.ascontiguousarray(np.stack([np.asarray(s["seglen"], np.float64).reshape(-1) for s in sets]))
    ts = np.ascontiguousarray(sets[0]["ts"], np.float64).reshape(-1)
    if seglen.shape != chords.shape[:2]:
        raise ValueError("one seglen per chord")
    for s in sets[1:]:
        if not np.array_equal(np.asarray(s["ts"], np.float64).reshape(-1), ts):
            raise ValueError("the sets of one call share ts")
    return pts, chords, seglen, ts


# ---- the device ---------------------------------------------------------------------------------------------------------

def intrinsic_features_device(scene_id: int, sets: Sequence[Dict[str, np.ndarray]], eps: float = _LIP_EPS, details: bool = False,
                              warmup: int = 0, repeats: int = 0):
    """rm_intrinsic_features over `sets` (sample_sets dicts of one shape) in one call: one dict per set with lipschitz_p99,
    slab_median (a length: not divided by the diagonal), n_finite, n_slabs and, with `details`, gmag (n_lip; NaN = left out)
    and slab_counts (n_chords)."""
    from . import _native
    pts, chords, seglen, ts = _stack(sets)
    return _native.intrinsic_features(scene_id, pts, eps, chords, seglen, ts, details=details, warmup=warmup, repeats=repeats)


def intrinsic_features(scene, boxes: Sequence[Optional[Tuple]], rng: np.random.Generator) -> List[Dict[str, float]]:
    """{lipschitz_p99, thin_slab} of `scene` (a registry scene or an id) in every box of `boxes` -- (hit_lo, hit_hi) corner
    pairs of the visible hit points, or None for a view with fewer than MIN_HITS hits (NaN features, no draw: the
    reference returns before it draws) -- from ONE rm_intrinsic_features call.  Draws from `rng` box after box."""
    scene_id = int(getattr(scene, "id", scene))
    nan = float("nan")
    out: List[Dict[str, float]] = [{"lipschitz_p99": nan, "thin_slab": nan} for _ in boxes]
    live, sets, diags = [], [], []
    for i, box in enumerate(boxes):
        if box is None:
            continue
        lo, hi, diag = padded_box(*box)
        live.append(i)
        sets.append(sample_sets(lo, hi, rng))
        diags.append(diag)
    if sets:
        for i, diag, r in zip(live, diags, intrinsic_features_device(scene_id, sets)):
            out[i] = {"lipschitz_p99": float(r["lipschitz_p99"]), "thin_slab": float(np.float64(r["slab_median"]) / diag)}
    return out


def view_features(captures: Sequence[Dict], cameras: Sequence) -> List[Dict]:
    """rm_view_features over the captures (dicts with hit, depth, normal, evals of one frame size; float32 maps) seen by
    `cameras` (Camera objects or 14-double arrays), in one call: per capture the five VIEW_KEYS, the integer counts n_hit,
    n_grazing, n_perimeter, sum_evals and `box` -- (lo, hi) of the hit points, None with fewer than MIN_HITS hits."""
    from . import _native
    cams = np.stack([np.asarray(c.params14() if hasattr(c, "params14") else c, np.float64).reshape(14) for c in cameras])
    out = []
    for r in _native.view_features(cams, captures):
        r = dict(r)
        lo, hi = r.pop("box_lo"), r.pop("box_hi")
        r["box"] = (lo, hi) if r["n_hit"] >= MIN_HITS else None
        out.append(r)
    return out


def dense_capture(scene, viewpoint, width: int, height: int, runner=None):
    """(camera, the device capture of the dense march) of `scene` from `viewpoint`"""
    from .camera import Camera
    from .config import MarchConfig
    from .runner import GPURunner
    runner = runner or GPURunner()
    rc = viewpoint.render_config(width, height)
    cap = runner.capture(scene.id, 9, rc, MarchConfig(max_iterations=DENSE_MAX_ITERATIONS, hit_threshold=DENSE_HIT_THRESHOLD),
                         lipschitz=scene.known_lipschitz_bound(), params=dict(DENSE_PARAMS), strategy_key=DENSE_STRATEGY_KEY,
                         device=True)
    cam = Camera(rc.camera_position, rc.camera_target, rc.camera_up, rc.fov_degrees, rc.width, rc.height)
    return cam, cap


def scene_features(scene, width: int, height: int, rng: np.random.Generator, runner=None) -> List[Dict[str, float]]:
    """The seven features of every curated viewpoint of `scene`: one dense-march capture per viewpoint, one
    rm_view_features call over all of them, one rm_intrinsic_features call with one sample set per viewpoint."""
    from .viewpoints import viewpoints_for
    pairs = [dense_capture(scene, vp, width, height, runner) for vp in viewpoints_for(scene)]
    views = view_features([cap for _, cap in pairs], [cam for cam, _ in pairs])
    intr = intrinsic_features(scene, [v["box"] for v in views], rng)
    return [{**{k: float(v[k]) for k in VIEW_KEYS}, **i} for v, i in zip(views, intr)]


def scene_view_features(scene, viewpoint, res: int, rng: np.random.Generator, runner=None) -> Dict[str, float]:
    """The seven features of one (scene, viewpoint) at res x res, as the reference's scene_view_features."""
    cam, cap = dense_capture(scene, viewpoint, res, res, runner)
    view = view_features([cap], [cam])[0]
    intr = intrinsic_features(scene, [view["box"]], rng)[0]
    return {**{k: float(view[k]) for k in VIEW_KEYS}, **intr}


# ---- the NumPy statement ------------------------------------------------------------------------------------------------

def intrinsic_features_numpy(scene_id: int, sets: Sequence[Dict[str, np.ndarray]], eps: float = _LIP_EPS, sdf=None) -> List[Dict]:
    """What rm_intrinsic_features computes, by the reference's NumPy expressions over `sdf(points (n, 3)) -> (n,)` (default:
    _native.sdf_eval of the scene): per set lipschitz_p99, slab_median, n_finite, n_slabs, gmag (NaN = left out) and
    slab_counts."""
    if sdf is None:
        from . import _native
        sdf = lambda p: _native.sdf_eval(scene_id, p)      # noqa: E731
    out = []
    for s in sets:
        pts, chords, seglen, ts = (np.asarray(s[k], np.float64) for k in ("pts", "chords", "seglen", "ts"))
        steps = len(ts)
        grad = np.empty((len(pts), 3))
        with np.errstate(all="ignore"):
            for ax in range(3):
                e = np.zeros(3)
                e[ax] = eps
                grad[:, ax] = (sdf(pts + e) - sdf(pts - e)) / (2 * eps)
            gmag = np.linalg.norm(grad, axis=1) if len(pts) else np.empty(0)
        keep = np.isfinite(gmag)
        finite = gmag[keep]
        lengths: List[float] = []
        counts = np.zeros(len(chords), np.int32)
        for c in range(len(chords)):
            a, b = chords[c, :3], chords[c, 3:]
            seg = a[None, :] + ts[:, None] * (b - a)[None, :]
            inside = sdf(seg) < 0.0
            if not inside.any():
                continue
            d = np.diff(inside.astype(np.int8))
            starts, ends = np.where(d == 1)[0] + 1, np.where(d == -1)[0] + 1
            if inside[0]:
                starts = np.r_[0, starts]
            if inside[-1]:
                ends = np.r_[ends, steps]
            step_len = float(seglen[c]) / (steps - 1)
            for st, en in zip(starts, ends):
                lengths.append((en - st) * step_len)
            counts[c] = len(starts)
        out.append({"lipschitz_p99": float(np.percentile(finite, 99)) if finite.size else float("nan"),
                    "slab_median": float(np.median(lengths)) if lengths else float("nan"),
                    "n_finite": int(finite.size), "n_slabs": len(lengths),
                    "gmag": np.where(keep, gmag, np.nan), "slab_counts": counts})
    return out


def view_features_numpy(capture: Dict, camera) -> Dict:
    """What rm_view_features computes for one capture, by the reference's NumPy expressions (its _view_features with this
    library's camera rays): the five VIEW_KEYS, the counts and box_lo / box_hi of the hit points (+inf / -inf without a hit)."""
    from .camera import Camera
    from .runner import ray_directions
    hit = np.asarray(capture["hit"]) != 0
    h, w = hit.shape
    c14 = np.asarray(camera.params14() if hasattr(camera, "params14") else camera, np.float64).reshape(14)
    if not isinstance(camera, Camera):
        class _Cam:      # ray_directions reads these three
            width, height = w, h
            params14 = staticmethod(lambda: c14)
        camera = _Cam()
    rd = ray_directions(camera)
    n_hit = int(hit.sum())
    out = {"hit_rate": float(hit.mean()), "n_hit": n_hit, "n_grazing": 0, "n_perimeter": 0, "sum_evals": 0,
           "grazing_frac": 0.0, "silhouette_cplx": 0.0, "hardness_mean": 0.0, "hardness_cv": 0.0,
           "box_lo": np.full(3, np.inf), "box_hi": np.full(3, -np.inf)}
    if n_hit == 0:
        return out
    cosang = np.abs(np.sum(rd * np.asarray(capture["normal"]), axis=-1))
    out["n_grazing"] = int((hit & (cosang < GRAZING_COS)).sum())
    out["grazing_frac"] = float(out["n_grazing"]) / n_hit
    pad = np.pad(hit, 1, constant_values=False)
    interior = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    out["n_perimeter"] = int((hit & ~interior).sum())
    out["silhouette_cplx"] = out["n_perimeter"] / float(np.sqrt(n_hit))
    ev = np.asarray(capture["evals"])[hit].astype(np.float64)
    with np.errstate(invalid="ignore"):      # evals are counts (rm_features.h): NaN and negatives 0, above 2^24 2^24, truncated
        ev = np.trunc(np.clip(np.where(np.isnan(ev), 0.0, ev), 0.0, float(1 << 24)))
    m = float(ev.mean())
    out["sum_evals"] = int(ev.sum())
    out["hardness_mean"] = m
    out["hardness_cv"] = float(ev.std() / m) if m > 0 else 0.0
    pts = (c14[0:3][None, None, :] + np.asarray(capture["depth"])[..., None] * rd)[hit]
    out["box_lo"], out["box_hi"] = pts.min(axis=0), pts.max(axis=0)
    return out


# ---- the command line -----------------------------------------------------------------------------------------------------

def build(scene_names: Optional[Sequence[str]], res: int, seed: int = 0, verbose: bool = False) -> List[Dict]:
    """One row per (scene, viewpoint) with the reference's row keys; one generator runs through all of them in order."""
    from . import registry
    from .viewpoints import viewpoints_for
    scenes = registry.get_all_scenes() if not scene_names else [registry.get_scene_by_name(n) for n in scene_names]
    if any(s is None for s in scenes):
        raise KeyError(f"unknown scene among {list(scene_names)}")
    rng = np.random.default_rng(seed)
    rows = []
    for scene in scenes:
        if verbose:
            print(f"  features: {scene.name} ...", file=sys.stderr)
        for vp, f in zip(viewpoints_for(scene), scene_features(scene, res, res, rng)):
            rows.append({"scene": scene.name, "scene_category": scene.category, "viewpoint": vp.name,
                         "view_category": vp.category, "features": f})
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Per (scene, viewpoint) discovery features, computed on the device.")
    ap.add_argument("--scenes", default="", help="comma-separated scene names (default: all)")
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--out", default="features.jsonl")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    rows = build([s for s in a.scenes.split(",") if s], a.res, a.seed, verbose=True)
    with open(a.out, "w", encoding="utf-8") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(f"{len(rows)} scene-views -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
