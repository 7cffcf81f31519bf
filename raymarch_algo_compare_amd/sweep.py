"""Budget / residual sweeps over the curated viewpoints, one batched launch per (scene, strategy).

The reference's dataset builder (sweep.py:96-283) renders every (scene, strategy, viewpoint, level)
cell on its own: `budget` mode sweeps max_iterations at a fixed epsilon, `residual` mode sweeps the
hit threshold at a fixed iteration cap (sweep.py:96-127; default levels sweep.py:48-54).  Small frames
are bound by the latency of their longest ray, so here all viewpoints x all levels of one (scene,
strategy) go through ONE rm_render_batch launch (per-frame camera + march configuration, the tails of
the frames overlap) and the rows are cut from the returned maps on the host.

A row holds the identifiers, the level, the iteration and SDF-evaluation statistics the reference records
(mean / median / p95 / max, sweep.py:78-81, :239-245), its adjacent-pixel divergence proxy (sweep.py:84-93), the hit rate and
the error against the finest level of the same viewpoint (the finest level stands in for the
reference's separately rendered ground truth: mean |depth - depth_finest| over common hits and the
number of pixels whose hit flag differs).  Arithmetic is the CPU path's fp64, so rows are comparable
with the reference's CPU columns, not with its GLSL column.

    python -m raymarch_algo_compare_amd.sweep --scenes Sphere,Mandelbulb --strategies Standard,Enhanced \
           --mode budget --width 384 --height 384 --out sweep.csv
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import certified_oracle, exact_oracle, faithful_segment, interval_oracle, registry, scoring
from .camera import Camera
from .collector import HipCollector
from .config import MarchConfig
from .viewpoints import viewpoints_for

DEFAULT_BUDGETS = [32, 64, 128, 256, 512]                       # reference sweep.py:48
DEFAULT_EPSILONS = [1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5]   # reference sweep.py:54

# The reference's per-strategy parameter grid (param_grid.py:20-27: shader uniform -> values, first = default), by
# registry key, for the strategies whose CPU-path arithmetic reads that constant (its Segment `kappa` row belongs to the
# shader's own segment tracing; Safe-Relaxed is shader-only and parity unpinned -- registry.SHADER_ONLY_STRATEGIES).
# Uniform names are mapped by runner.SHADER_UNIFORMS.
STRATEGY_PARAM_GRID = {
    "Relaxed": {"omega": [1.2, 1.4, 1.6, 1.8]},
    "Heuristic-Auto-Relaxed": {"omega": [1.2, 1.4, 1.6, 1.8]},
    "Skipping-Spheres": {"margin": [0.02, 0.05, 0.1, 0.2]},
    "Safe-Relaxed": {"omega": [1.2, 1.5, 1.8, 2.0]},
}


def param_combos(strategy_key: str):
    """Each override dict of a strategy's grid (cartesian product); one empty dict without tunables (param_grid.py:30-40)."""
    import itertools
    grid = STRATEGY_PARAM_GRID.get(strategy_key)
    if not grid:
        return [{}]
    keys = list(grid)
    return [dict(zip(keys, vals)) for vals in itertools.product(*(grid[k] for k in keys))]


def param_label(params: Dict) -> str:
    """Stable short label of a combo (param_grid.py:43-48)."""
    return "default" if not params else ",".join(f"{k}={v:g}" for k, v in sorted(params.items()))


ROW_FIELDS = ["scene", "strategy", "params", "viewpoint", "category", "sweep_axis", "level", "max_iterations", "hit_threshold",
              "width", "height", "iters_mean", "iters_median", "iters_p95", "iters_max", "evals_mean", "evals_median", "evals_p95", "evals_max",
              "divergence_proxy", "hit_rate",
              "depth_mae_vs_finest", "hit_flips_vs_finest", "ms_per_frame"]
# with an oracle (run_sweep(oracle="interval")): each frame against the sound first hit of its viewpoint
# (interval_oracle.interval_capture, scoring.py); empty cells for a scene without an interval extension
ORACLE_FIELDS = ["oracle_iou", "oracle_false_hit", "oracle_false_miss", "oracle_depth_mae", "oracle_depth_rmse",
                 "oracle_depth_p95"]
# "exact": the closed-form first hit instead (exact_oracle.exact_capture): no tolerance, the same columns; empty cells for a
# scene without an exact form
ORACLES = ("interval", "exact")
# with a ceiling (run_sweep(ceiling="segment")): the sound segment tracer's frame of the viewpoint (faithful_segment.
# faithful_capture) against the interval oracle's (scoring.residual) and its steps over the hit rays -- what a tracer that
# cannot tunnel reaches there and pays for it; the same four values on every row of a scene and viewpoint, empty cells for a
# scene without an interval extension
CEILING_FIELDS = ["ceiling_iou", "ceiling_depth_med", "ceiling_iters_median", "ceiling_iters_p95"]
CEILINGS = ("segment",)
# with certify (run_sweep(oracle="interval", certify=True)): each frame against the certified first-hit bracket of its
# viewpoint (certified_oracle.certified_capture) -- the share of pixels the certificate leaves OPEN, the frame's IoU against
# the certified hit mask with every OPEN pixel counted against the frame and then for it, and |depth - t_hi| over the HIT
# pixels the frame hits; empty cells for a scene without an interval extension
CERTIFY_FIELDS = ["cert_open_frac", "cert_iou_lo", "cert_iou_hi", "cert_depth_mae", "cert_depth_p95"]
# with ssim (run_sweep(oracle=..., ssim=True)): the tertiary tier of scoring.py -- each frame's depth and normal images
# against the oracle capture's (ssim.py; the frame's normals as GPURunner.capture takes them, at its own hit points).  The
# oracle captures carry no colour, so the two colour columns are empty cells, as are all four without an oracle capture.
SSIM_FIELDS = list(scoring.SSIM_KEYS)
# with features (run_sweep(features=True)): the strategy-independent discovery features of the row's (scene, viewpoint)
# (features.py: five from a dense-march capture, two from samples of the scene's SDF in the box of the visible hit
# points), the same seven values on every row of a scene and viewpoint
FEATURE_FIELDS = ["feat_hit_rate", "feat_grazing_frac", "feat_silhouette_cplx", "feat_hardness_mean", "feat_hardness_cv",
                  "feat_lipschitz_p99", "feat_thin_slab"]


def build_levels(mode: str, *, budgets: Sequence[int] = DEFAULT_BUDGETS, epsilons: Sequence[float] = DEFAULT_EPSILONS,
                 cap: int = 512, hit_threshold: float = 1e-4) -> List[Tuple[float, MarchConfig, Dict]]:
    """(level value, MarchConfig, extra columns) per level -- the reference's two axes (sweep.py:96-127)."""
    if mode == "budget":
        return [(float(b), MarchConfig(max_iterations=int(b), hit_threshold=hit_threshold),
                 {"sweep_axis": "budget", "max_iterations": int(b), "hit_threshold": hit_threshold}) for b in budgets]
    if mode == "residual":
        return [(float(e), MarchConfig(max_iterations=int(cap), hit_threshold=float(e)),
                 {"sweep_axis": "residual", "max_iterations": int(cap), "hit_threshold": float(e)}) for e in epsilons]
    raise ValueError(f"unknown sweep mode {mode!r}")


def divergence_proxy(iters2d: np.ndarray) -> float:
    """Mean absolute iteration-count difference between adjacent pixels (reference sweep.py:84-93)."""
    a = np.asarray(iters2d, dtype=np.float64)
    dx = np.abs(a[:, 1:] - a[:, :-1])
    dy = np.abs(a[1:, :] - a[:-1, :])
    n = dx.size + dy.size
    return float((dx.sum() + dy.sum()) / n) if n else 0.0


def finest_index(mode: str, levels) -> int:
    """The most accurate level of an axis: the largest budget, the smallest epsilon."""
    vals = [lv[0] for lv in levels]
    return int(np.argmax(vals)) if mode == "budget" else int(np.argmin(vals))


def sweep_cell(collector: HipCollector, scene, strategy, mode: str, levels, width: int, height: int, grid: bool = False,
               oracle_frames: Optional[Dict[str, Optional[Dict]]] = None,
               ceiling_cols: Optional[Dict[str, Dict]] = None, keep: Optional[List] = None,
               defer_oracle: bool = False) -> List[Dict]:
    """All viewpoints x parameter combos x levels of one (scene, strategy) in one batched launch -> one row per
    frame.  `grid` brute-forces the strategy's tunable parameters (reference sweep.py:181,222-223).  `oracle_frames`
    (viewpoint name -> oracle capture, None without one) adds the ORACLE_FIELDS columns, `ceiling_cols` (viewpoint name ->
    CEILING_FIELDS values) those.  `keep` (a list) receives (row, viewpoint name, camera, hit map, depth map) of every row,
    for ssim_columns and device_oracle_columns.  `defer_oracle`: the ORACLE_FIELDS cells are left empty here, for
    device_oracle_columns to fill."""
    from .runner import GPURunner
    vps = viewpoints_for(scene)
    combos = param_combos(strategy.key) if grid else [{}]
    cams, cfgs, prms, tags = [], [], [], []
    for vp in vps:
        cam = Camera(vp.position, vp.target, vp.up, 60.0, width, height)
        for combo in combos:
            for li, (value, mc, extra) in enumerate(levels):
                cams.append(cam)
                cfgs.append(mc)
                prms.append(GPURunner.strategy_params(combo))
                tags.append((vp, li, value, extra, combo))
    frames = collector.benchmark_batch(strategy, scene, cams, cfgs, want_evals=True, params=prms)
    fin = finest_index(mode, levels)
    rows = []
    for i, ((vp, li, value, extra, combo), st) in enumerate(zip(tags, frames)):
        ref = frames[i - li + fin]                     # finest level of the same viewpoint and parameter combo
        both = st.hit_map & ref.hit_map
        it = st.iteration_heatmap
        rows.append({
            "scene": scene.name, "strategy": strategy.short_name, "params": param_label(combo), "viewpoint": vp.name,
            "category": vp.category,
            "sweep_axis": extra["sweep_axis"], "level": value, "max_iterations": extra["max_iterations"],
            "hit_threshold": extra["hit_threshold"], "width": width, "height": height,
            "iters_mean": float(it.mean()), "iters_median": float(np.median(it)), "iters_p95": float(np.percentile(it, 95)),
            "iters_max": float(it.max()),
            # SDF evaluations per ray -- the workload the iteration count under-reports for Segment / RevAA / Hybrid
            # (reference sweep.py:239-245 records the same distribution from its capture)
            "evals_mean": float(st.evals_map.mean()), "evals_median": float(np.median(st.evals_map)),
            "evals_p95": float(np.percentile(st.evals_map, 95)), "evals_max": float(st.evals_map.max()),
            "divergence_proxy": divergence_proxy(it), "hit_rate": float(st.hit_map.mean()),
            "depth_mae_vs_finest": float(np.abs(st.depth_map[both] - ref.depth_map[both]).mean()) if both.any() else 0.0,
            "hit_flips_vs_finest": int((st.hit_map != ref.hit_map).sum()),
            "ms_per_frame": float(st.kernel_ms),
        })
        if oracle_frames is not None:
            rows[-1].update(oracle_columns({"hit": st.hit_map, "depth": st.depth_map},
                                           None if defer_oracle else oracle_frames.get(vp.name)))
        if ceiling_cols is not None:
            rows[-1].update(ceiling_cols[vp.name])
        if keep is not None:
            keep.append((rows[-1], vp.name, cams[i], st.hit_map, st.depth_map))
    return rows


def oracle_columns(frame: Dict, oracle: Optional[Dict]) -> Dict:
    """ORACLE_FIELDS of one frame against its oracle capture (scoring.py); None (an empty cell) without one."""
    if oracle is None:
        return {k: None for k in ORACLE_FIELDS}
    h = scoring._hit_metrics(frame["hit"], oracle["hit"])
    d = scoring._depth_metrics(frame, oracle)
    return {"oracle_iou": h["iou"], "oracle_false_hit": h["false_hit_rate"], "oracle_false_miss": h["false_miss_rate"],
            "oracle_depth_mae": d["mae"], "oracle_depth_rmse": d["rmse"], "oracle_depth_p95": d["p95"]}


def device_oracle_columns(kept: List, oracle_frames: Dict[str, Optional[Dict]]) -> None:
    """Fills the ORACLE_FIELDS columns of the kept rows of one scene (sweep_cell's `keep`, with defer_oracle) on the device:
    all rows of a viewpoint -- every strategy, parameter combo and level -- against that viewpoint's oracle capture in ONE
    rm_score_captures call (score_device.py).  Rows of a viewpoint without an oracle capture keep their empty cells."""
    from . import score_device
    by_vp: Dict[str, List] = {}
    for item in kept:
        by_vp.setdefault(item[1], []).append(item)
    for name, items in by_vp.items():
        truth = oracle_frames.get(name)
        if truth is None:
            continue
        methods = [{"hit": hit, "depth": depth} for _, _, _, hit, depth in items]
        for (row, *_), rep in zip(items, score_device.score_capture_batch(methods, {"hit": truth["hit"], "depth": truth["depth"]})):
            h, d = rep["hit"], rep["depth"]
            row.update({"oracle_iou": h["iou"], "oracle_false_hit": h["false_hit_rate"], "oracle_false_miss": h["false_miss_rate"],
                        "oracle_depth_mae": d["mae"], "oracle_depth_rmse": d["rmse"], "oracle_depth_p95": d["p95"]})


def device_normal_maps(scene, items: List) -> List[np.ndarray]:
    """The (H, W, 3) float32 normal maps of the kept rows `items` of one viewpoint, all from ONE rm_shade_frames call (the
    capture kernel, csrc/rm_capture.h: the hit point on the very ray the frame marched, from the frame's fp32 depth)."""
    from . import _native
    cams = np.stack([cam.params14() for _, _, cam, _, _ in items])
    hit = np.stack([np.asarray(h, dtype=bool) for _, _, _, h, _ in items])
    depth = np.stack([np.asarray(d, dtype=np.float32) for _, _, _, _, d in items])
    return list(_native.shade_frames(scene.id, cams, hit, depth=depth)["normal"])


def ssim_columns(scene, kept: List, oracle_frames: Dict[str, Optional[Dict]], device_normals: bool = False) -> None:
    """Adds the SSIM_FIELDS columns to the kept rows of one scene (sweep_cell's `keep`): all rows of a viewpoint -- every
    strategy, parameter combo and level -- against that viewpoint's oracle capture in ONE rm_ssim_scores call.
    `device_normals`: the rows' normals come from one rm_shade_frames call per viewpoint (device_normal_maps) instead of one
    hit_normals round trip per row."""
    from . import ssim
    from .runner import hit_normals, ray_directions
    by_vp: Dict[str, List] = {}
    for item in kept:
        by_vp.setdefault(item[1], []).append(item)
    for name, items in by_vp.items():
        truth = oracle_frames.get(name)
        if truth is None:
            for row, *_ in items:
                row.update(dict.fromkeys(SSIM_FIELDS))
            continue
        if device_normals:
            methods = [{"hit": np.asarray(hit, dtype=bool), "depth": depth, "normal": normal}
                       for (_, _, _, hit, depth), normal in zip(items, device_normal_maps(scene, items))]
            for (row, *_), cols in zip(items, ssim.ssim_scores_batch(methods, truth)):
                row.update(cols)
            continue
        rd = ray_directions(items[0][2])
        methods = []
        for _, _, cam, hit, depth in items:
            hit = np.asarray(hit, dtype=bool)
            normal = np.zeros(hit.shape + (3,), np.float32)
            if hit.any():
                normal[hit] = hit_normals(scene.id, cam, rd, depth, hit)
            methods.append({"hit": hit, "depth": depth, "normal": normal})
        for (row, *_), cols in zip(items, ssim.ssim_scores_batch(methods, truth)):
            row.update(cols)


def feature_columns_for(scene, width: int, height: int, rng: np.random.Generator) -> Dict[str, Dict]:
    """FEATURE_FIELDS of every curated viewpoint of `scene`: one dense-march capture per viewpoint, one rm_view_features
    call over all of them and one rm_intrinsic_features call with one sample set per viewpoint (features.scene_features)."""
    from . import features
    feats = features.scene_features(scene, width, height, rng)
    return {vp.name: {"feat_" + k: f[k] for k in features.FEATURE_KEYS} for vp, f in zip(viewpoints_for(scene), feats)}


def sound_scene(scene, twins: bool = False):
    """The scene the sound side evaluates for `scene`: the scene itself when it has an interval extension; with `twins`,
    the registered program twin (scene_program.register_twin) of a catalogue scene that has none but has a twin; else
    None."""
    if interval_oracle.has_interval(scene):
        return scene
    if twins:
        from . import scene_program
        if scene.id in scene_program.catalogue_twins():
            return scene_program.register_twin(scene)
    return None


def exact_scene(scene, twins: bool = False):
    """sound_scene for the exact first hit: the scene itself when it has an exact form; with `twins`, its registered
    program twin when that has one (Bad Lipschitz Sphere, Bumpy Sphere); else None."""
    if exact_oracle.has_exact(scene):
        return scene
    if twins:
        from . import scene_program
        if scene.id in scene_program.catalogue_twins():
            twin = scene_program.register_twin(scene)
            if exact_oracle.has_exact(twin):
                return twin
    return None


def oracle_frames_for(scene, width: int, height: int, oracle: str, tol: float, twins: bool = False) -> Dict[str, Optional[Dict]]:
    """The oracle capture of every curated viewpoint of `scene` (None for each when it has no interval extension -- for
    "exact": no exact form -- and, with `twins`, no program twin that has one either); `oracle` is one of ORACLES (run_sweep
    has checked it).  `tol` is the interval oracle's; the exact first hit has none."""
    vps = viewpoints_for(scene)
    if oracle == "exact":
        sound = exact_scene(scene, twins)
        if sound is None:
            return {vp.name: None for vp in vps}
        return {vp.name: exact_oracle.exact_capture(sound, Camera(vp.position, vp.target, vp.up, 60.0, width, height)) for vp in vps}
    sound = sound_scene(scene, twins)
    if sound is None:
        return {vp.name: None for vp in vps}
    return {vp.name: interval_oracle.interval_capture(sound, Camera(vp.position, vp.target, vp.up, 60.0, width, height), tol=tol)
            for vp in vps}


def certify_columns(frame: Dict, cert: Optional[Dict]) -> Dict:
    """CERTIFY_FIELDS of one frame against the certified capture of its viewpoint; None (empty cells) without one.  An OPEN
    pixel's truth is unknown: cert_iou_lo takes it to be the opposite of the frame's answer, cert_iou_hi the frame's own, so
    the IoU against the true mask lies between the two whatever the OPEN pixels are."""
    if cert is None:
        return {k: None for k in CERTIFY_FIELDS}
    mine = np.asarray(frame["hit"], dtype=bool)
    hit, open_ = cert["status"] == certified_oracle.HIT, cert["status"] == certified_oracle.OPEN
    d = scoring._depth_metrics(frame, cert["capture"])
    return {"cert_open_frac": float(open_.mean()),
            "cert_iou_lo": scoring._hit_metrics(mine, hit | (open_ & ~mine))["iou"],
            "cert_iou_hi": scoring._hit_metrics(mine, hit | (open_ & mine))["iou"],
            "cert_depth_mae": d["mae"], "cert_depth_p95": d["p95"]}


def certify_frames_for(scene, width: int, height: int, twins: bool = False) -> Dict[str, Optional[Dict]]:
    """The certified capture of every curated viewpoint of `scene` (None for each without an interval extension and, with
    `twins`, without a twin that has one); l_global is the scene's own Lipschitz bound, for a twin too."""
    vps = viewpoints_for(scene)
    sound = sound_scene(scene, twins)
    if sound is None:
        return {vp.name: None for vp in vps}
    l_global = max(1.0, float(scene.known_lipschitz_bound() or 1.0))
    return {vp.name: certified_oracle.certified_capture(sound, Camera(vp.position, vp.target, vp.up, 60.0, width, height),
                                                        l_global=l_global) for vp in vps}


def ceiling_columns(frame: Optional[Dict], oracle: Optional[Dict], device_score: bool = False) -> Dict:
    """CEILING_FIELDS of one faithful_capture frame against the oracle capture of its viewpoint; None (empty cells) without
    them.  `device_score`: the residual comes from the device (score_device.residual_batch)."""
    if frame is None or oracle is None:
        return {k: None for k in CEILING_FIELDS}
    if device_score:
        from . import score_device
        res = score_device.residual_batch([{"hit": frame["hit"], "depth": frame["depth"]}], oracle, k=2)[0]
    else:
        res = scoring.residual(frame["hit"], frame["depth"], oracle["hit"], oracle["depth"], scoring.silhouette_band(oracle["hit"], k=2))
    c = faithful_segment.cost(frame)
    return {"ceiling_iou": res["iou"], "ceiling_depth_med": res["depth_med"], "ceiling_iters_median": c["iters_median"],
            "ceiling_iters_p95": c["iters_p95"]}


def ceiling_columns_for(scene, width: int, height: int, oracle_frames: Dict[str, Optional[Dict]], tol: float,
                        twins: bool = False, device_score: bool = False) -> Dict[str, Dict]:
    """ceiling_columns of every curated viewpoint of `scene` (oracle_frames: oracle_frames_for of the same scene, size and
    `twins`)."""
    out = {}
    sound = sound_scene(scene, twins)
    cfg = None
    if sound is not None and sound is not scene:       # a twin: the tracer's clamp on K must admit the scene's own bound
        from . import _native
        cfg = _native.segment_config(tol=tol, l_global=max(1.0, float(scene.known_lipschitz_bound() or 1.0)))
    for vp in viewpoints_for(scene):
        truth = oracle_frames.get(vp.name)
        frame = None if truth is None else faithful_segment.faithful_capture(
            sound, Camera(vp.position, vp.target, vp.up, 60.0, width, height), tol=tol, cfg=cfg)
        out[vp.name] = ceiling_columns(frame, truth, device_score)
    return out


def run_sweep(scene_names: Optional[Sequence[str]] = None, strategy_names: Optional[Sequence[str]] = None, mode: str = "budget",
              width: int = 384, height: int = 384, budgets: Sequence[int] = DEFAULT_BUDGETS,
              epsilons: Sequence[float] = DEFAULT_EPSILONS, cap: int = 512, hit_threshold: float = 1e-4,
              out_path: Optional[str] = None, device_id: int = 0, verbose: bool = False, grid: bool = False,
              oracle: Optional[str] = None, oracle_tol: float = interval_oracle.DEFAULT_TOL,
              ceiling: Optional[str] = None, ceiling_tol: float = faithful_segment.DEFAULT_TOL, ssim: bool = False,
              oracle_twins: bool = False, device_capture: bool = False, device_score: bool = False, features: bool = False,
              feature_seed: int = 0, certify: bool = False) -> List[Dict]:
    """Sweep `mode` over the curated viewpoints of the named scenes (default: all 20) for the named
    strategies (default: all 11).  Unknown names raise KeyError.  Returns the rows; writes CSV (or JSON
    for a .json path) when `out_path` is given.  oracle="interval": every row also scores its frame against the
    interval oracle's first hit of its viewpoint (ORACLE_FIELDS; one oracle frame per scene and viewpoint, tolerance
    `oracle_tol`).  oracle="exact": the same columns against the closed-form first hit (exact_oracle.exact_capture; empty
    cells for a scene without an exact form; with oracle_twins also Bad Lipschitz Sphere and Bumpy Sphere).  ceiling="segment": every row also carries the sound segment tracer's result at its viewpoint
    (CEILING_FIELDS; hit tolerance `ceiling_tol`, scored against the interval oracle at `oracle_tol`).  ssim=True (only
    with an oracle): every row also carries SSIM_FIELDS against the oracle capture of its viewpoint.  oracle_twins=True: a
    catalogue scene without an interval extension but with a program twin (scene_program.catalogue_twins: Menger, Bad
    Lipschitz Sphere, Bumpy Sphere, Gyroid, Box Lattice) is scored against its twin's oracle capture and ceiling frame; the
    twin, the same point function bit for bit, stays registered.  Off, those scenes keep their empty cells.  A twin's
    ceiling frame is traced with the tracer's clamp on K (RmSegmentConfig.l_global) raised to the scene's Lipschitz bound
    (2 for Bad Lipschitz Sphere), a scene with its own interval form with the default clamp of 1: where the bound is above
    1 the two kinds of ceiling row come from different tracer configs.  device_capture=True (with ssim): the frames' normals
    come from the capture kernel, one rm_shade_frames call per viewpoint (ssim_columns); off, the output is unchanged.
    device_score=True (only with an oracle): ORACLE_FIELDS, and the residual behind CEILING_FIELDS when a ceiling is asked
    for, come from the device -- one rm_score_captures call per viewpoint over all of its rows (device_oracle_columns); the
    count-derived and percentile columns equal the host's, the means differ by summation order only.  Off, the output is
    unchanged.  features=True: every row also carries FEATURE_FIELDS, the discovery features of its (scene, viewpoint),
    computed on the device once per scene (feature_columns_for); the samples are drawn from
    np.random.default_rng(feature_seed), scene after scene, viewpoint after viewpoint.  Off, the output is unchanged.
    certify=True (only with oracle="interval"): every row also carries CERTIFY_FIELDS, its frame against the certified
    first-hit bracket of its viewpoint (certify_columns; one certified frame per scene and viewpoint), after every other
    column.  Off, the output is unchanged."""
    if oracle is not None and oracle not in ORACLES:                       # before anything touches the GPU
        raise ValueError(f"unknown oracle {oracle!r}: one of {ORACLES}")
    if ceiling is not None and ceiling not in CEILINGS:
        raise ValueError(f"unknown ceiling {ceiling!r}: one of {CEILINGS}")
    if ssim and oracle is None:
        raise ValueError("ssim needs an oracle to score against: pass oracle=")
    if device_capture and not ssim:
        raise ValueError("device_capture computes the normals of the ssim columns: pass ssim=True")
    if device_score and oracle is None:
        raise ValueError("device_score scores against an oracle: pass oracle=")
    if certify and oracle != "interval":
        raise ValueError("certify puts an error bar on the interval oracle: pass oracle=\"interval\"")
    scenes = registry.get_all_scenes() if not scene_names else [_need(registry.get_scene_by_name(n), "scene", n) for n in scene_names]
    strats = ([registry.get_strategy_by_name(k) for k in registry.list_strategies()] if not strategy_names
              else [_need(registry.get_shader_strategy(n) or registry.get_strategy_by_name(n), "strategy", n) for n in strategy_names])
    levels = build_levels(mode, budgets=budgets, epsilons=epsilons, cap=cap, hit_threshold=hit_threshold)
    collector = HipCollector(MarchConfig(), device_id=device_id)
    feature_rng = np.random.default_rng(feature_seed) if features else None
    rows: List[Dict] = []
    for scene in scenes:
        first = len(rows)
        truth = (oracle_frames_for(scene, width, height, "interval", oracle_tol, oracle_twins)
                 if oracle == "interval" or ceiling is not None else None)          # (the ceiling is scored against the interval oracle)
        ofr = None if oracle is None else (truth if oracle == "interval" else
                                           oracle_frames_for(scene, width, height, oracle, oracle_tol, oracle_twins))
        ccols = (ceiling_columns_for(scene, width, height, truth, ceiling_tol, oracle_twins, device_score)
                 if ceiling is not None else None)
        kept: Optional[List] = [] if ssim or device_score or certify else None
        for strat in strats:
            if strat.has_lipschitz:
                strat.lipschitz = scene.known_lipschitz_bound() or 1.0      # run_once wiring (reference main.py:58-61)
            cell = sweep_cell(collector, scene, strat, mode, levels, width, height, grid, ofr, ccols, kept, device_score)
            rows.extend(cell)
            if verbose:
                print(f"{scene.name:24s} {strat.short_name:24s} {len(cell):3d} frames  "
                      f"{sum(r['ms_per_frame'] for r in cell):8.2f} ms", file=sys.stderr)
        if kept and device_score:
            device_oracle_columns(kept, ofr)
        if kept and ssim:
            ssim_columns(scene, kept, ofr, device_normals=device_capture)
        if features:
            fcols = feature_columns_for(scene, width, height, feature_rng)
            for row in rows[first:]:
                row.update(fcols[row["viewpoint"]])
        if certify:
            cert = certify_frames_for(scene, width, height, oracle_twins)
            for row, name, _, hit_map, depth_map in kept:
                row.update(certify_columns({"hit": hit_map, "depth": depth_map}, cert.get(name)))
    if out_path:
        write_rows(rows, out_path)
    return rows


def write_rows(rows: List[Dict], path: str) -> None:
    if path.lower().endswith(".json"):
        with open(path, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1, ensure_ascii=False)
        return
    fields = ROW_FIELDS + (ORACLE_FIELDS if rows and "oracle_iou" in rows[0] else []) + \
        (CEILING_FIELDS if rows and "ceiling_iou" in rows[0] else []) + (SSIM_FIELDS if rows and "depth_ssim" in rows[0] else []) + \
        (FEATURE_FIELDS if rows and "feat_hit_rate" in rows[0] else []) + (CERTIFY_FIELDS if rows and "cert_open_frac" in rows[0] else [])
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=fields)
        w.writeheader()
        w.writerows(rows)


def _need(obj, kind, name):
    if obj is None:
        raise KeyError(f"unknown {kind} {name!r}")
    return obj


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="", help="comma-separated scene names (default: all)")
    ap.add_argument("--strategies", default="", help="comma-separated strategy names (default: all)")
    ap.add_argument("--mode", default="budget", choices=["budget", "residual"])
    ap.add_argument("--budgets", default=",".join(map(str, DEFAULT_BUDGETS)))
    ap.add_argument("--epsilons", default=",".join(map(str, DEFAULT_EPSILONS)))
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--hit-threshold", type=float, default=1e-4)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--out", default="sweep.csv")
    ap.add_argument("--grid", action="store_true", help="also sweep each strategy's tunable parameters (STRATEGY_PARAM_GRID)")
    ap.add_argument("--oracle", default=None, choices=list(ORACLES),
                    help="score every frame against a first-hit oracle (adds the oracle_* columns): the sound interval march or the "
                         "closed-form exact first hit")
    ap.add_argument("--oracle-tol", type=float, default=interval_oracle.DEFAULT_TOL, help="the oracle's hit tolerance")
    ap.add_argument("--ceiling", default=None, choices=list(CEILINGS),
                    help="add the sound segment tracer's result per scene and viewpoint (the ceiling_* columns)")
    ap.add_argument("--ceiling-tol", type=float, default=faithful_segment.DEFAULT_TOL, help="the ceiling tracer's hit tolerance")
    ap.add_argument("--ssim", action="store_true",
                    help="with --oracle: add the SSIM columns of every frame against the oracle capture (depth_ssim, normal_ssim, ...)")
    ap.add_argument("--device-capture", action="store_true",
                    help="with --ssim: the frames' normals from the capture kernel, one rm_shade_frames call per viewpoint, instead "
                         "of one host round trip per row")
    ap.add_argument("--device-score", action="store_true",
                    help="with --oracle: the oracle_* columns (and the residual behind the ceiling_* columns) from the device, one "
                         "rm_score_captures call per viewpoint, instead of NumPy per row")
    ap.add_argument("--oracle-twins", action="store_true",
                    help="with --oracle / --ceiling: score a catalogue scene that has no interval form against its program twin "
                         "(Menger, Bad Lipschitz Sphere, Bumpy Sphere, Gyroid, Box Lattice); a twin's ceiling is traced with l_global = the "
                         "scene's Lipschitz bound, not the default 1")
    ap.add_argument("--certify", action="store_true",
                    help="with --oracle interval: add the cert_* columns, every frame against the certified first-hit bracket of "
                         "its viewpoint (the interval oracle's per-ray error bar)")
    ap.add_argument("--features", action="store_true",
                    help="add the discovery features of every row's (scene, viewpoint), computed on the device (the feat_* columns)")
    ap.add_argument("--feature-seed", type=int, default=0, help="seed of the features' random samples")
    a = ap.parse_args(argv)
    if a.ssim and a.oracle is None:
        ap.error("--ssim needs --oracle")
    if a.device_capture and not a.ssim:
        ap.error("--device-capture needs --ssim")
    if a.device_score and a.oracle is None:
        ap.error("--device-score needs --oracle")
    if a.certify and a.oracle != "interval":
        ap.error("--certify needs --oracle interval")
    if a.oracle_twins and a.oracle is None and a.ceiling is None:
        ap.error("--oracle-twins needs --oracle or --ceiling")
    rows = run_sweep([s for s in a.scenes.split(",") if s], [s for s in a.strategies.split(",") if s], a.mode, a.width, a.height,
                     [int(v) for v in a.budgets.split(",")], [float(v) for v in a.epsilons.split(",")], a.cap, a.hit_threshold,
                     a.out, verbose=True, grid=a.grid, oracle=a.oracle, oracle_tol=a.oracle_tol,
                     ceiling=a.ceiling, ceiling_tol=a.ceiling_tol, ssim=a.ssim, oracle_twins=a.oracle_twins,
                     device_capture=a.device_capture, device_score=a.device_score, features=a.features, feature_seed=a.feature_seed,
                     certify=a.certify)
    print(f"{len(rows)} rows -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
