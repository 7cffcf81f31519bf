#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports /root/reference, which never travels
to the GPU box).  The outputs are data only -- inputs (camera, config, ids) and
expected outputs (iteration maps, hit masks, depths, stats scalars).

For every (scene, strategy) the scene/strategy/camera/Lipschitz wiring follows
run_once (reference main.py:39-74) with a FRESH RenderConfig, and the pixel loop
follows MetricsCollector.benchmark_strategy (metrics/collector.py:40-44); the
stats scalars come from the reference's own RayMarchStats.compute (core/types.py:77-137).

Layout of each frames_*.npz (keys prefixed "s{scene_id}_k{strategy_id}_"):
  iters   int16 (H,W)         exact iteration counts (max possible 521)
  hitbits uint8 packbits(H*W) exact hit mask
  t_hit   float64 (n_hits,)   raw t of the hit rays, row-major order
  sha_t / sha_fs              sha256 over the little-endian float64 bytes of t / final_sdf
                              of ALL rays (pins the oracle bit-for-bit without storing them)
  cam     float64 (14,)       position, forward, right, up, half_width, half_height
  meta    float64 (8,)        W, H, row0, rows, max_iterations, hit_threshold, max_distance, lipschitz

frames_config_<family>.npz and rays_config.npz (--only config, --only rays) are laid out differently: see the
comment above CONFIG_SEED.

Usage:  python oracle/gen_golden.py [--only frames64|frames160|rows1080|sdf|stats|leak|leakseq|params|schema|viewpoints|evals|analytic|config|rays|sdf_edges|ray_edges]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from raymarching_benchmark.config import MarchConfig, RenderConfig  # noqa: E402
from raymarching_benchmark.core.camera import Camera  # noqa: E402
from raymarching_benchmark.core.types import RayMarchStats  # noqa: E402
from raymarching_benchmark.core.vec3 import Vec3  # noqa: E402
from raymarching_benchmark.scenes.catalog import get_all_scenes  # noqa: E402
from raymarching_benchmark.strategies import STRATEGIES  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SCENES = get_all_scenes()
STRAT_KEYS = list(STRATEGIES.keys())


def wire(scene_id: int, strat_id: int, width: int, height: int, render: RenderConfig | None = None):
    """run_once's wiring (main.py:39-74) for registry ids."""
    scene = get_all_scenes()[scene_id]
    strategy = STRATEGIES[STRAT_KEYS[strat_id]]()
    render = render or RenderConfig(width=width, height=height)
    sug = scene.suggested_camera()
    if sug:
        render.camera_position = sug.camera_position
        render.camera_target = sug.camera_target
        render.camera_up = sug.camera_up
        render.fov_degrees = sug.fov_degrees
    lipschitz = 1.0
    if hasattr(strategy, "lipschitz"):
        bound = scene.known_lipschitz_bound()
        if bound is not None:
            strategy.lipschitz = bound
        lipschitz = float(strategy.lipschitz)
    cam = Camera(position=Vec3(*render.camera_position), target=Vec3(*render.camera_target),
                 up=Vec3(*render.camera_up), fov_degrees=render.fov_degrees,
                 width=render.width, height=render.height)
    return scene, strategy, cam, lipschitz, render


def cam14(cam: Camera) -> np.ndarray:
    return np.array([*cam.position.to_tuple(), *cam.forward.to_tuple(), *cam.right.to_tuple(),
                     *cam.up.to_tuple(), cam.half_width, cam.half_height], dtype=np.float64)


def march_rows(scene, strategy, cam, mc, row0, rows):
    results = []
    for py in range(row0, row0 + rows):
        for px in range(cam.width):
            results.append(strategy.march(cam.get_ray(px, py), scene.sdf, mc))
    return results


def pack(prefix, results, cam, mc, lipschitz, row0, rows, store):
    W = cam.width
    iters = np.array([r.iterations for r in results], dtype=np.int32).reshape(rows, W)
    hit = np.array([bool(r.hit) for r in results], dtype=bool)
    t = np.array([float(r.t) for r in results], dtype="<f8")
    fs = np.array([float(r.final_sdf) for r in results], dtype="<f8")
    assert iters.max() < 32767
    store[prefix + "iters"] = iters.astype(np.int16)
    store[prefix + "hitbits"] = np.packbits(hit)
    store[prefix + "t_hit"] = t[hit]
    store[prefix + "sha_t"] = np.frombuffer(hashlib.sha256(t.tobytes()).digest(), dtype=np.uint8)
    store[prefix + "sha_fs"] = np.frombuffer(hashlib.sha256(fs.tobytes()).digest(), dtype=np.uint8)
    store[prefix + "cam"] = cam14(cam)
    store[prefix + "meta"] = np.array([W, cam.height, row0, rows, mc.max_iterations, mc.hit_threshold,
                                       mc.max_distance, lipschitz], dtype=np.float64)


def stats_dict(scene, strategy, results, W, H):
    s = RayMarchStats(strategy_name=strategy.short_name, scene_name=scene.name)
    s.compute(results, W, H, 1.0)
    return {
        "strategy": s.strategy_name, "scene": s.scene_name, "total_rays": s.total_rays,
        "hit_count": s.hit_count, "miss_count": s.miss_count, "sample_count": s.sample_count,
        "iteration_mean": s.iteration_mean, "iteration_median": s.iteration_median,
        "iteration_std": s.iteration_std, "iteration_min": s.iteration_min,
        "iteration_max": s.iteration_max, "iteration_p95": s.iteration_p95,
        "iteration_p99": s.iteration_p99, "accuracy_mean": s.accuracy_mean,
        "accuracy_max": s.accuracy_max, "accuracy_std": s.accuracy_std, "hit_rate": s.hit_rate,
        "warp_divergence_proxy": s.warp_divergence_proxy,
        "depth_sum": float(s.depth_map.sum()),
    }


def gen_frames(tag, W, H, pairs, mc=None):
    mc = mc or MarchConfig()
    store, stats = {}, {}
    t0 = time.time()
    for sid, kid in pairs:
        scene, strategy, cam, lip, _ = wire(sid, kid, W, H)
        res = march_rows(scene, strategy, cam, mc, 0, H)
        pack(f"s{sid}_k{kid}_", res, cam, mc, lip, 0, H, store)
        stats[f"s{sid}_k{kid}"] = stats_dict(scene, strategy, res, W, H)
        print(f"  [{tag}] {scene.name} / {strategy.short_name}: hits={stats[f's{sid}_k{kid}']['hit_count']} "
              f"sum_iters={stats[f's{sid}_k{kid}']['sample_count']}  ({time.time() - t0:.0f}s)", flush=True)
    np.savez_compressed(os.path.join(OUT, f"frames_{tag}.npz"), **store)
    with open(os.path.join(OUT, f"stats_{tag}.json"), "w", encoding="utf-8") as f:
        json.dump(stats, f, indent=1, ensure_ascii=False)


def gen_rows1080(pairs, row0=536, rows=8):
    """Row-block samples of the 1920x1080 frame: pins full-resolution indexing."""
    mc = MarchConfig()
    store = {}
    for sid, kid in pairs:
        scene, strategy, cam, lip, _ = wire(sid, kid, 1920, 1080)
        res = march_rows(scene, strategy, cam, mc, row0, rows)
        pack(f"s{sid}_k{kid}_", res, cam, mc, lip, row0, rows, store)
        print(f"  [rows1080] {scene.name} / {strategy.short_name}", flush=True)
    np.savez_compressed(os.path.join(OUT, "frames_rows1080.npz"), **store)


def gen_leak():
    """The CLI reuses one RenderConfig across scenes (main.py:167,206): a scene without a
    suggested camera inherits the previous scene's.  Pin Cube rendered right after
    Grazing Plane (non-default, off-axis camera)."""
    mc = MarchConfig()
    store = {}
    rc = RenderConfig(width=64, height=48)
    wire(1, 0, 64, 48, rc)  # Grazing Plane mutates rc
    scene, strategy, cam, lip, _ = wire(2, 0, 64, 48, rc)
    res = march_rows(scene, strategy, cam, mc, 0, 48)
    pack("s2_k0_", res, cam, mc, lip, 0, 48, store)
    np.savez_compressed(os.path.join(OUT, "frames_leak.npz"), **store)


def leak_sequence(W, H, upto):
    """Walk `--scene all` in catalogue order with ONE shared RenderConfig, as cli() does (main.py:167,206):
    returns the RenderConfig as scene `upto` finds it (every earlier scene's suggestion applied)."""
    rc = RenderConfig(width=W, height=H)
    for sid in range(upto):
        wire(sid, 0, W, H, rc)
    return rc


# (scene, strategy) cells whose camera is NOT the scene's own in `--scene all --strategy all` order
# (scenes 2..9 see Grazing Plane's camera, 11 sees Mandelbulb's)
LEAK_CELLS = [(2, 10), (3, 4), (5, 9), (6, 3), (8, 10), (9, 6), (11, 0), (11, 10)]
LEAK_ROWS_1080 = [(2, 0), (9, 0), (11, 10)]


def gen_leakseq():
    """Cells of the CLI's leaked-camera sequence: whole frames at 64x48 and rows 536..543 of 1920x1080."""
    mc = MarchConfig()
    store, stats = {}, {}
    for sid, kid in LEAK_CELLS:
        rc = leak_sequence(64, 48, sid)
        scene, strategy, cam, lip, _ = wire(sid, kid, 64, 48, rc)
        res = march_rows(scene, strategy, cam, mc, 0, 48)
        pack(f"s{sid}_k{kid}_", res, cam, mc, lip, 0, 48, store)
        stats[f"s{sid}_k{kid}"] = stats_dict(scene, strategy, res, 64, 48)
        print(f"  [leakseq] {scene.name} / {strategy.short_name}: camera {rc.camera_position} -> {rc.camera_target}, "
              f"hits {stats[f's{sid}_k{kid}']['hit_count']}", flush=True)
    np.savez_compressed(os.path.join(OUT, "frames_leakseq.npz"), **store)
    with open(os.path.join(OUT, "stats_leakseq.json"), "w", encoding="utf-8") as f:
        json.dump(stats, f, indent=1, ensure_ascii=False)
    store = {}
    for sid, kid in LEAK_ROWS_1080:
        rc = leak_sequence(1920, 1080, sid)
        scene, strategy, cam, lip, _ = wire(sid, kid, 1920, 1080, rc)
        res = march_rows(scene, strategy, cam, mc, 536, 8)
        pack(f"s{sid}_k{kid}_", res, cam, mc, lip, 536, 8, store)
        print(f"  [leakrows1080] {scene.name} / {strategy.short_name}", flush=True)
    np.savez_compressed(os.path.join(OUT, "frames_leakrows1080.npz"), **store)


def gen_schema():
    """Header row and index column of the nine matrix_*.csv files the reference ships under example/
    (data files; BASELINE config 4 asks for CSVs identical in schema to these)."""
    import csv
    ex = os.path.join(REF, "example")
    out = {}
    for fn in sorted(os.listdir(ex)):
        if fn.startswith("matrix_") and fn.endswith(".csv"):
            with open(os.path.join(ex, fn), encoding="utf-8", newline="") as f:
                rows = list(csv.reader(f))
            out[fn] = {"header": rows[0], "index": [r[0] for r in rows[1:]]}
    with open(os.path.join(OUT, "example_matrix_schema.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
    print("example_matrix_schema.json:", len(out), "files")


# ---- non-default strategy parameters ---------------------------------------------------------------
# Parameter names / order of RmStrategyParams (include/rm_hip.h) = rmo_cfg (oracle/rm_oracle.c).
PARAM_ORDER = ["omega", "ar_omega_min", "ar_omega_max", "ar_smoothing", "ar_growth_rate", "ar_decay_rate", "beta",
               "overstep_min_step", "hybrid_stuck_step_ratio", "hybrid_min_step", "margin", "ar_omega_init",
               "overstep_bisection_steps", "hybrid_stuck_threshold", "segment_bisection_steps", "revaa_bisection_steps"]
PARAM_DEFAULTS = dict(omega=1.2, ar_omega_min=1.0, ar_omega_max=2.0, ar_smoothing=0.7, ar_growth_rate=1.05,
                      ar_decay_rate=0.7, beta=0.3, overstep_min_step=0.01, hybrid_stuck_step_ratio=0.001,
                      hybrid_min_step=0.005, margin=0.05, ar_omega_init=1.2, overstep_bisection_steps=16, hybrid_stuck_threshold=5,
                      segment_bisection_steps=8, revaa_bisection_steps=8)


def with_literal(cls, old, new):
    """The reference class with ONE literal of its march() replaced: the method is rebuilt from the reference's
    own code object with that constant swapped (types.CodeType.replace), nothing is re-typed.  Used for the four
    parameters the CPU strategies hold as literals (skipping_spheres.py:30 `margin = 0.05`, auto_relaxed.py:41
    `omega = 1.2`, segment_tracing.py:79 and rev_affine.py:70 `range(8)`); the GLSL seam exposes `margin` as a uniform (gpu/runner.py:115)."""
    import types
    code = cls.march.__code__
    assert sum(1 for c in code.co_consts if type(c) is type(old) and c == old) == 1, (cls.__name__, old, code.co_consts)
    consts = tuple(new if (type(c) is type(old) and c == old) else c for c in code.co_consts)
    fn = types.FunctionType(code.replace(co_consts=consts), cls.march.__globals__, "march", cls.march.__defaults__,
                            cls.march.__closure__)
    return type(cls.__name__ + "Lit", (cls,), {"march": fn})


# (strategy id, constructor kwargs / literal swaps, RmStrategyParams overrides): >= 3 non-default settings per
# tunable strategy; omega / margin values are the reference's own grid (param_grid.py:20-27)
PARAM_CASES = (
    [(1, dict(omega=w), None, dict(omega=w)) for w in (1.4, 1.6, 1.8)] +
    [(2, dict(omega_min=a, omega_max=b, smoothing=c, growth_rate=d, decay_rate=e), None,
      dict(ar_omega_min=a, ar_omega_max=b, ar_smoothing=c, ar_growth_rate=d, ar_decay_rate=e))
     for a, b, c, d, e in ((1.0, 1.6, 0.5, 1.1, 0.5), (1.1, 2.5, 0.9, 1.02, 0.8), (1.0, 3.0, 0.3, 1.2, 0.9))] +
    [(3, dict(beta=b), None, dict(beta=b)) for b in (0.1, 0.5, 0.9)] +
    [(6, dict(min_step_factor=m, bisection_steps=n), None, dict(overstep_min_step=m, overstep_bisection_steps=n))
     for m, n in ((0.02, 8), (0.005, 24), (0.05, 4), (0.01, 0))] +
    [(9, dict(stuck_threshold=k, stuck_step_ratio=r, min_step_factor=m), None,
      dict(hybrid_stuck_threshold=k, hybrid_stuck_step_ratio=r, hybrid_min_step=m))
     for k, r, m in ((3, 0.01, 0.01), (8, 0.0005, 0.002), (2, 0.005, 0.02))] +
    [(7, {}, (0.05, m), dict(margin=m)) for m in (0.02, 0.1, 0.2)] +
    [(2, {}, (1.2, w), dict(ar_omega_init=w)) for w in (1.4, 1.6, 1.8)] +
    [(10, {}, (8, n), dict(segment_bisection_steps=n)) for n in (3, 12, 0)] +
    [(8, {}, (8, n), dict(revaa_bisection_steps=n)) for n in (3, 12, 0)]
)
PARAM_SCENES = (0, 2, 9, 10, 12)


def gen_params(W=48, H=36):
    """Frames marched by the reference's strategy classes constructed with NON-default arguments."""
    mc = MarchConfig()
    store = {}
    n = 0
    for kid, kwargs, literal, overrides in PARAM_CASES:
        cls = STRATEGIES[STRAT_KEYS[kid]]
        if literal is not None:
            cls = with_literal(cls, *literal)
        for sid in PARAM_SCENES:
            scene, _, cam, _, _ = wire(sid, kid, W, H)
            strategy = cls(**kwargs)
            lip = 1.0
            if hasattr(strategy, "lipschitz"):                            # main.py:58-61
                bound = scene.known_lipschitz_bound()
                if bound is not None:
                    strategy.lipschitz = bound
                lip = float(strategy.lipschitz)
            res = march_rows(scene, strategy, cam, mc, 0, H)
            pre = f"c{n}_"
            pack(pre, res, cam, mc, lip, 0, H, store)
            prm = dict(PARAM_DEFAULTS, **overrides)
            store[pre + "ids"] = np.array([sid, kid], dtype=np.int32)
            store[pre + "prm"] = np.array([float(prm[k]) for k in PARAM_ORDER], dtype=np.float64)
            print(f"  [params] case {n}: {scene.name} / {strategy.short_name} {overrides}: hits "
                  f"{sum(1 for r in res if r.hit)} iterations {sum(r.iterations for r in res)}", flush=True)
            n += 1
    store["ncases"] = np.array([n], dtype=np.int32)
    np.savez_compressed(os.path.join(OUT, f"frames_params_{W}x{H}.npz"), **store)


def gen_sdf(n=2000):
    """Per-scene SDF values at seeded random points (same generator idea as the
    reference's tests/test_scene_parity.py:88-102)."""
    rng = random.Random(1234)
    pts = np.array([[rng.uniform(-3.5, 3.5) for _ in range(3)] for _ in range(n)], dtype=np.float64)
    store = {"pts": pts}
    for sid, scene in enumerate(SCENES):
        store[f"s{sid}"] = np.array([scene.sdf(Vec3(*p)) for p in pts], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "sdf_points.npz"), **store)


def gen_evals(W=48, H=36, scene_ids=(0, 1, 9, 10, 12, 15)):
    """SDF evaluations per ray: strategy.march is given a counting wrapper of scene.sdf, so the count is what
    the reference's own march() calls (the quantity its GLSL backend exposes as g_evals, scenes.glsl:10-12).
    All 11 strategies on a few scenes; iterations ride along to tie the two together."""
    mc = MarchConfig()
    store = {}
    for sid in scene_ids:
        for kid in range(len(STRAT_KEYS)):
            scene, strategy, cam, lip, _ = wire(sid, kid, W, H)
            calls = [0]

            def counted(p, _sdf=scene.sdf, _c=calls):
                _c[0] += 1
                return _sdf(p)
            evals, iters = [], []
            for py in range(H):
                for px in range(W):
                    calls[0] = 0
                    r = strategy.march(cam.get_ray(px, py), counted, mc)
                    evals.append(calls[0])
                    iters.append(r.iterations)
            pre = f"s{sid}_k{kid}_"
            store[pre + "evals"] = np.array(evals, dtype=np.int16).reshape(H, W)
            store[pre + "iters"] = np.array(iters, dtype=np.int16).reshape(H, W)
            store[pre + "cam"] = cam14(cam)
            store[pre + "meta"] = np.array([W, H, 0, H, mc.max_iterations, mc.hit_threshold, mc.max_distance, lip], dtype=np.float64)
            print(f"  [evals] {scene.name} / {strategy.short_name}: evals {sum(evals)} iterations {sum(iters)}", flush=True)
    np.savez_compressed(os.path.join(OUT, f"evals_{W}x{H}.npz"), **store)


def gen_analytic(W=80, H=60):
    """Closed-form depth / hit / normal of the reference's gpu/analytic.py (:74-208) for its four analytic scenes,
    on the CPU camera's pixel-centre rays (its intersect_* functions take ray arrays; the module is loaded by
    path because the gpu package's __init__ needs moderngl)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_analytic", os.path.join(REF, "raymarching_benchmark", "gpu", "analytic.py"))
    ref = importlib.util.module_from_spec(spec)
    ref.__package__ = "raymarching_benchmark.gpu"
    spec.loader.exec_module(ref)
    store = {}
    for sid in (0, 1, 2, 3):
        scene, _, cam, _, _ = wire(sid, 0, W, H)
        c = cam14(cam)
        u = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * c[12]
        v = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * c[13]
        d = c[3:6][None, None, :] + c[6:9][None, None, :] * u[None, :, None] + c[9:12][None, None, :] * v[:, None, None]
        d = d / np.sqrt((d * d).sum(2, keepdims=True))
        depth, hit, normal = ref.ANALYTIC_SCENES[scene.name](c[0:3].copy(), d)
        store[f"s{sid}_depth"] = depth.astype("<f8")
        store[f"s{sid}_hitbits"] = np.packbits(hit)
        store[f"s{sid}_normal"] = normal.astype("<f8")
        store[f"s{sid}_cam"] = c
        print(f"  [analytic] {scene.name}: {int(hit.sum())} hits", flush=True)
    np.savez_compressed(os.path.join(OUT, f"analytic_{W}x{H}.npz"), **store)


def gen_viewpoints():
    """The reference's curated viewpoints (viewpoints.py:41-140) for every catalogue scene, as data."""
    from raymarching_benchmark.viewpoints import viewpoints_for
    from raymarching_benchmark.scenes.catalog import get_all_scenes
    out = {}
    for sc in get_all_scenes():
        out[sc.name] = [[v.name, v.category, [float(c) for c in v.position], [float(c) for c in v.target],
                         [float(c) for c in v.up]] for v in viewpoints_for(sc)]
    with open(os.path.join(OUT, "viewpoints.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
    print("viewpoints.json:", sum(len(v) for v in out.values()), "viewpoints of", len(out), "scenes")


# ---- off-default march configurations, cameras, shapes and explicit rays --------------------------------------
# frames_config_<family>.npz hold the fields of frames_params_48x36.npz (ids, prm, meta, cam, iters, hitbits, sha_t,
# sha_fs) for some two thousand small frames.  They are stored BY COLUMN -- one array per field, one row per case --
# because a key per case and field costs about 200 bytes of zip directory and .npy header, twice the payload of such
# a frame.  Per file, N cases:
#   ids (N,2) int32 scene, strategy     prm (N,16) RmStrategyParams order     meta (N,8) as in pack()
#   cam (N,14) the reference camera's basis     view (N,10) its arguments: position, target, up, fov_degrees
#   iters int16, all frames concatenated row-major; off (N+1,) int64 ray offsets     hitbits uint8 packbits of all hits
#   sha_t, sha_fs (N,32)   sha_depth32 (N,32): sha256 of float32(t if hit else 0.0), the depth map of core/types.py:93
#   t_bits (N,64) uint64: the bits of t of the first 64 rays (0-padded), to locate a mismatch the hashes only detect
#   refstats (N,6) int64: total_rays, hit_count, miss_count, sample_count, iteration_min, iteration_max of the
#                         reference's RayMarchStats for whole frames of family D, -1 elsewhere
#   tag (N,) the generator's label of the case (family, sub-family, level), for the coverage test and for messages
# Everything is seeded by CONFIG_SEED; archives are written with fixed timestamps, so a rerun is byte-identical.
CONFIG_SEED = 20261016
HEAVY_SCENES = (9, 10, 15, 16)          # Menger, Mandelbulb, Bumpy Sphere, Gyroid: slow in pure Python
FRACTAL_SCENES = (9, 10)
BUDGET_EDGES = (0, 1, 2, 3, 15, 16, 17, 18)
FAMILIES = ("A", "B", "C", "D", "E")
# which RmStrategyParams a constructor argument is (PARAM_CASES spells the same pairs out by hand)
CTOR_TO_PRM = {1: dict(omega="omega"),
               2: dict(omega_min="ar_omega_min", omega_max="ar_omega_max", smoothing="ar_smoothing",
                       growth_rate="ar_growth_rate", decay_rate="ar_decay_rate"),
               3: dict(beta="beta"),
               6: dict(min_step_factor="overstep_min_step", bisection_steps="overstep_bisection_steps"),
               9: dict(stuck_threshold="hybrid_stuck_threshold", stuck_step_ratio="hybrid_stuck_step_ratio",
                       min_step_factor="hybrid_min_step")}
# the march() literal with_literal can swap per strategy: (its value in the reference, the RmStrategyParams field)
LITERAL_OF = {7: (0.05, "margin"), 2: (1.2, "ar_omega_init"), 10: (8, "segment_bisection_steps"), 8: (8, "revaa_bisection_steps")}


def save_npz(path, store):
    """np.savez_compressed with fixed member timestamps (numpy stamps the wall clock), so reruns are byte-identical."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def default_view(scene):
    """(position, target, up, fov) as run_once finds them: the scene's suggestion or RenderConfig's defaults."""
    rc = scene.suggested_camera() or RenderConfig()
    return (tuple(rc.camera_position), tuple(rc.camera_target), tuple(rc.camera_up), float(rc.fov_degrees))


def spec(tag, sid, kid, view, W, H, row0=0, rows=None, mi=512, thr=1e-4, far=100.0, lip=None, ctor=None, lit=None, stats=False):
    """One case.  lip None: main.py's wiring (the scene's bound if it has one); lit: new value of LITERAL_OF[kid]."""
    pos, tgt, up, fov = view
    return dict(tag=tag, sid=sid, kid=kid, view=[*map(float, pos), *map(float, tgt), *map(float, up), float(fov)], W=W, H=H,
                row0=row0, rows=H - row0 if rows is None else rows, mi=int(mi), thr=float(thr), far=float(far), lip=lip,
                ctor=dict(ctor or {}), lit=lit, stats=stats)


def build_strategy(scene, kid, ctor, lit, lip):
    cls = STRATEGIES[STRAT_KEYS[kid]]
    overrides = {CTOR_TO_PRM[kid][k]: v for k, v in ctor.items()}
    if lit is not None:
        old, field_name = LITERAL_OF[kid]
        if lit != old:
            cls = with_literal(cls, old, lit)
        overrides[field_name] = lit
    strategy = cls(**ctor)
    lipschitz = 1.0
    if hasattr(strategy, "lipschitz"):                                     # main.py:58-61
        if lip is None:
            bound = scene.known_lipschitz_bound()
            if bound is not None:
                strategy.lipschitz = bound
        else:
            strategy.lipschitz = lip
        lipschitz = float(strategy.lipschitz)
    return strategy, lipschitz, overrides


def run_spec(sp):
    """Worker: march one case with the reference.  Returns the case's columns, or its description and the exception."""
    try:
        scene = SCENES[sp["sid"]]
        strategy, lip, overrides = build_strategy(scene, sp["kid"], sp["ctor"], sp["lit"], sp["lip"])
        v = sp["view"]
        cam = Camera(position=Vec3(*v[0:3]), target=Vec3(*v[3:6]), up=Vec3(*v[6:9]), fov_degrees=v[9], width=sp["W"], height=sp["H"])
        mc = MarchConfig(max_iterations=sp["mi"], hit_threshold=sp["thr"], max_distance=sp["far"])
        res = march_rows(scene, strategy, cam, mc, sp["row0"], sp["rows"])
        one = {}
        pack("", res, cam, mc, lip, sp["row0"], sp["rows"], one)
        hit = np.array([bool(r.hit) for r in res], dtype=bool)
        t = np.array([float(r.t) for r in res], dtype="<f8")
        one.pop("t_hit")
        one["hit"] = hit
        one["sha_depth32"] = np.frombuffer(hashlib.sha256(np.where(hit, t, 0.0).astype("<f4").tobytes()).digest(), dtype=np.uint8)
        tb = np.zeros(64, dtype=np.uint64)
        tb[:min(64, len(t))] = t[:64].view(np.uint64)
        one["t_bits"] = tb
        prm = dict(PARAM_DEFAULTS, **overrides)
        one["prm"] = np.array([float(prm[k]) for k in PARAM_ORDER], dtype=np.float64)
        one["refstats"] = np.full(6, -1, dtype=np.int64)
        if sp["stats"] and sp["row0"] == 0 and sp["rows"] == sp["H"]:
            s = stats_dict(scene, strategy, res, sp["W"], sp["H"])
            one["refstats"] = np.array([s["total_rays"], s["hit_count"], s["miss_count"], s["sample_count"],
                                        s["iteration_min"], s["iteration_max"]], dtype=np.int64)
        return sp, one, None
    except Exception as e:                                                  # noqa: BLE001 -- the reference refused the case
        return sp, None, f"{type(e).__name__}: {e}"


def _vp_views(sid):
    from raymarching_benchmark.viewpoints import viewpoints_for
    return [(v.name, (tuple(v.position), tuple(v.target), tuple(v.up), 60.0)) for v in viewpoints_for(SCENES[sid])]


def sweep_levels():
    """DEFAULT_BUDGETS, DEFAULT_EPSILONS and RESIDUAL_CAP of the reference's sweep.py (:48-55), read from its text: the module
    imports moderngl (gpu/runner.py:3) and cannot be imported here."""
    import ast
    with open(os.path.join(REF, "raymarching_benchmark", "sweep.py"), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    found = {n.targets[0].id: ast.literal_eval(n.value) for n in tree.body
             if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
             and n.targets[0].id in ("DEFAULT_BUDGETS", "DEFAULT_EPSILONS", "RESIDUAL_CAP")}
    return found["DEFAULT_BUDGETS"], found["DEFAULT_EPSILONS"], found["RESIDUAL_CAP"]


def family_a(W=16, H=12):
    """The sweep's grid (sweep.py:48-55, :222-240): every level of both axes, from the curated viewpoints, fov 60.  A group
    is one (scene, viewpoint, strategy) with all levels of one axis -- what the sweep renders in one go."""
    DEFAULT_BUDGETS, DEFAULT_EPSILONS, RESIDUAL_CAP = sweep_levels()
    axes = {"budget": [(b, 1e-4) for b in DEFAULT_BUDGETS], "eps512": [(512, e) for e in DEFAULT_EPSILONS],
            "eps2048": [(RESIDUAL_CAP, e) for e in DEFAULT_EPSILONS]}
    entries = [(sid, name, view) for sid in range(len(SCENES)) if sid != 10 for name, view in _vp_views(sid)]
    used = {(e[0], e[1]): 0 for e in entries}
    mandel = _vp_views(10)
    out, g, m = [], 0, 0
    for kid in range(len(STRAT_KEYS)):
        for axis, levels in axes.items():
            chosen = []
            if axis != "eps2048":                                              # Mandelbulb: every strategy, both axes at 512
                name, view = mandel[m % len(mandel)]
                m += 1
                chosen.append((10, name, view))
            while len(chosen) < 3:
                # least-used eligible viewpoint of a scene this (strategy, axis) does not have yet; the 2048 cap stays off the
                # fractals (as the issue asks) and off the other slow scenes, which the two other axes therefore take first
                ok = [e for e in entries if e[0] not in [c[0] for c in chosen]
                      and not (axis == "eps2048" and e[0] in HEAVY_SCENES)]
                ok.sort(key=lambda e: (used[(e[0], e[1])], 0 if (axis != "eps2048" and e[0] in HEAVY_SCENES) else 1))
                chosen.append(ok[0])
                used[(ok[0][0], ok[0][1])] += 1
            for sid, name, view in chosen:
                for mi, thr in levels:
                    out.append(spec(f"A/{axis}/g{g}/{name}", sid, kid, view, W, H, mi=mi, thr=thr))
                g += 1
    assert all(n > 0 for n in used.values()), [k for k, n in used.items() if not n]
    return out


def family_b(W=12, H=8):
    """Budget edges: the empty loop, Overstep-Bisect's reserve (overstep_bisect.py:40-41), the bisection loops of Segment and
    RevAA, and bisection counts of 0, 1, the budget and one more.  Plus the two frames test_edge_cases used to assert on."""
    out = []
    for sid in (0, 9, 10, 12):
        view = default_view(SCENES[sid])
        for kid in range(len(STRAT_KEYS)):
            for b in BUDGET_EDGES:
                out.append(spec(f"B/budget/{b}", sid, kid, view, W, H, mi=b))
    for sid in (0, 9, 10):
        view = default_view(SCENES[sid])
        for kid in (6, 10, 8):
            for b in BUDGET_EDGES:
                for n in sorted({0, 1, b, b + 1}):
                    kw = dict(ctor=dict(bisection_steps=n)) if kid == 6 else dict(lit=n)
                    out.append(spec(f"B/steps/{b}/{n}", sid, kid, view, W, H, mi=b, **kw))
    edge_view = ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)
    out.append(spec("B/edge/0", 0, 0, edge_view, 8, 4, mi=0))
    out.append(spec("B/edge/10", 0, 6, edge_view, 8, 4, mi=10))
    return out


# constructor arguments and literals at both ends of their meaningful range: (strategy, ctor kwargs, literal)
PARAM_ENDS = (
    [(1, dict(omega=w), None) for w in (1.0, 2.5)] +
    [(2, dict(omega_min=a, omega_max=b, smoothing=c, growth_rate=d, decay_rate=e), None)
     for a, b, c, d, e in ((1.0, 1.0, 0.0, 1.0, 1.0), (1.0, 2.5, 1.0, 1.5, 0.1), (2.5, 2.5, 0.0, 1.05, 0.7), (1.0, 2.5, 0.0, 2.0, 0.0))] +
    [(2, {}, w) for w in (1.0, 2.0)] +
    [(3, dict(beta=b), None) for b in (0.0, 1.0)] +
    [(6, dict(min_step_factor=m, bisection_steps=n), None) for m, n in ((0.0, 16), (1.0, 16), (0.0, 64), (1.0, 1))] +
    [(9, dict(stuck_threshold=k, stuck_step_ratio=r, min_step_factor=m), None)
     for k, r, m in ((0, 0.001, 0.005), (1, 0.001, 0.005), (5, 0.0, 0.0), (5, 1.0, 1.0), (1, 1.0, 0.0), (20, 0.01, 1.0))] +
    [(7, {}, m) for m in (0.0, 1.0)] +
    [(10, {}, n) for n in (1, 64)] +
    [(8, {}, n) for n in (1, 64)]
)


def _center_t(sid, view):
    """t of the frame's central ray under the default configuration: places a far plane relative to the object."""
    scene = SCENES[sid]
    cam = Camera(position=Vec3(*view[0]), target=Vec3(*view[1]), up=Vec3(*view[2]), fov_degrees=view[3], width=1, height=1)
    r = STRATEGIES["Standard"]().march(cam.get_ray(0, 0), scene.sdf, MarchConfig())
    assert r.hit, (sid, view)
    return float(r.t)


def family_c(W=16, H=12):
    out = []
    for sid in (0, 3, 13):
        view = default_view(SCENES[sid])
        for kid in range(len(STRAT_KEYS)):
            for thr in (0.0, 1e-9, 0.5):                                      # nothing converges below 1e-9: the budget runs out
                out.append(spec(f"C/thr/{thr:g}", sid, kid, view, W, H, mi=200 if thr == 0.5 else 700, thr=thr))
    for mi in (542, 543, 544, 2048):                                         # around the last bin of a 544-bin iteration histogram
        for kid in (0, 4, 6, 10):
            out.append(spec(f"C/hist/{mi}", 0, kid, default_view(SCENES[0]), W, H, mi=mi, thr=0.0))
    for sid in (0, 2, 1):
        view = _vp_views(sid)[-1 if sid == 1 else 0][1]                    # the plane from its most grazing viewpoint
        tc = _center_t(sid, view)
        # below the camera's distance to the object; just past the central hit, so the far plane cuts between the object's
        # near and far surface and the silhouette rays' hits lie beyond it; then far planes only the plane's horizon reaches
        for what, far in (("below", round(0.5 * tc, 6)), ("between", round(1.02 * tc, 6)), ("1e4", 1e4), ("1e9", 1e9)):
            for kid in range(len(STRAT_KEYS)):
                out.append(spec(f"C/far/{what}", sid, kid, view, W, H, far=far, mi=2048 if sid == 1 else 512))
    for sid in (0, 11, 10, 9, 2):                                             # 10: no bound of its own; 11: bound 2.0
        for lip in (0.1, 0.5, 2.0, 4.0):
            out.append(spec(f"C/lip/{lip:g}", sid, 10, default_view(SCENES[sid]), W, H, lip=lip, mi=256))
    for kid, ctor, lit in PARAM_ENDS:
        for sid, mi, thr in ((0, 100, 1e-3), (9, 64, 1e-2), (10, 150, 1e-5), (12, 300, 3e-4)):
            out.append(spec(f"C/prm/{kid}", sid, kid, default_view(SCENES[sid]), W, H, mi=mi, thr=thr, ctor=ctor, lit=lit))
    return out


def family_d():
    out = []
    up = (0.0, 1.0, 0.0)
    cams = [("inside", ((0.0, 0.0, 0.3), (0.0, 0.0, -1.0), up, 60.0)),
            ("inside-offaxis", ((0.2, -0.1, 0.15), (1.0, 1.0, 1.0), up, 90.0)),
            ("on-surface-in", ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), up, 60.0)),       # sdf == 0 at the rays' origin, looking in
            ("on-surface-out", ((0.0, 0.0, 1.0), (0.0, 0.0, 3.0), up, 60.0)),      # ... and looking away
            ("on-surface-along", ((0.0, 0.0, 1.0), (0.0, 3.0, 1.0), (0.0, 0.0, 1.0), 60.0)),
            ("down-parallel-up", ((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), up, 60.0)),    # forward x up == 0: right and up are zero
            ("up-zero", ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 60.0)),
            ("no-forward", ((0.0, 0.0, 5.0), (0.0, 0.0, 5.0), up, 60.0)),          # target == position: every basis vector zero
            ("up+z", ((3.0, 3.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 60.0)),
            ("up+xy", ((0.0, 0.5, 4.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0), 60.0)),
            ("up-y", ((1.0, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), 60.0)),
            ("fov5", ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), up, 5.0)),
            ("fov150", ((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up, 150.0))]
    rot = 0
    for name, view in cams:
        for sid in (0, 2, 4, 11):
            if name.startswith("on-surface"):
                assert SCENES[sid].sdf(Vec3(*view[0])) == 0.0, (sid, view)
            for _ in range(3):
                kid = rot % len(STRAT_KEYS)
                rot += 1
                out.append(spec(f"D/cam/{name}", sid, kid, view, 12, 9, mi=128, stats=True))
    for kid in (0, 6, 10):
        out.append(spec("D/cam/inside", 10, kid, cams[0][1], 12, 9, mi=128, stats=True))
    shapes = [(1, 1, 0, 1), (1, 7, 0, 7), (9, 1, 0, 1), (63, 3, 0, 3), (64, 4, 0, 4), (65, 5, 0, 5),
              (20, 17, 3, 5), (20, 17, 1, 1), (20, 17, 6, 11), (33, 10, 7, 2)]
    for W, H, row0, rows in shapes:
        for sid, kid in ((0, 0), (9, 6), (10, 10), (12, 2), (1, 4)):
            out.append(spec(f"D/shape/{W}x{H}+{row0}+{rows}", sid, kid, default_view(SCENES[sid]), W, H, row0, rows, mi=256, stats=True))
    return out


def family_e(n=320):
    """Seeded draws over every scene, every strategy and every axis the other families pick values on by hand."""
    rng = random.Random(CONFIG_SEED)
    out = []
    for i in range(n):
        sid, kid = (i % 20, (i // 20 + i) % 11) if i < 220 else (rng.randrange(20), rng.randrange(11))   # every pair's scene and strategy met
        W, H = rng.randint(1, 24), rng.randint(1, 18)
        row0 = 0 if rng.random() < 0.7 else rng.randrange(H)
        rows = H - row0 if rng.random() < 0.7 else rng.randint(1, H - row0)
        pos, tgt, _, _ = default_view(SCENES[sid])
        s = rng.choice((0.3, 1.0, 1.0, 3.0, 12.0))
        pos = tuple(c * s + rng.gauss(0.0, 0.3) for c in pos)
        tgt = tuple(c + rng.gauss(0.0, 0.2) for c in tgt)
        upv = rng.choice(((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, -1.0, 0.0)))
        fov = rng.choice((5.0, 30.0, 60.0, 90.0, 150.0))
        mi = rng.choice((0, 1, 2, 3, 15, 16, 17, 32, 64, 128, 256, 512, 700, 2048))
        if sid in HEAVY_SCENES:
            mi = min(mi, 300)
        thr = rng.choice((0.0, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 1e-9, 0.5))
        far = rng.choice((0.5, 2.0, 9.0, 30.0, 100.0, 1e4, 1e9))
        lip = rng.choice((None, 0.1, 0.5, 1.0, 2.0, 4.0)) if kid == 10 else None
        ctor, lit = {}, None
        if rng.random() < 0.6:
            if kid == 1:
                ctor = dict(omega=rng.uniform(1.0, 2.5))
            elif kid == 2:
                ctor = dict(omega_min=rng.uniform(1.0, 1.3), omega_max=rng.uniform(1.3, 2.5), smoothing=rng.uniform(0.0, 1.0),
                            growth_rate=rng.uniform(1.0, 1.3), decay_rate=rng.uniform(0.3, 1.0))
                lit = rng.choice((None, 1.0, 1.7))
            elif kid == 3:
                ctor = dict(beta=rng.uniform(0.0, 1.0))
            elif kid == 6:
                ctor = dict(min_step_factor=rng.choice((0.0, 0.001, 0.01, 0.1, 1.0)), bisection_steps=rng.randint(0, 64))
            elif kid == 9:
                ctor = dict(stuck_threshold=rng.randint(0, 20), stuck_step_ratio=rng.choice((0.0, 1e-4, 1e-3, 1e-2, 1.0)),
                            min_step_factor=rng.choice((0.0, 0.005, 0.1, 1.0)))
            elif kid == 7:
                lit = rng.choice((0.0, 0.02, 0.1, 0.5))
            elif kid in (8, 10):
                lit = rng.randint(0, 64)
        out.append(spec(f"E/{i}", sid, kid, (pos, tgt, upv, fov), W, H, row0, rows, mi=mi, thr=thr, far=far, lip=lip, ctor=ctor, lit=lit))
    return out


def gen_config(jobs):
    import multiprocessing
    fams = {"A": family_a(), "B": family_b(), "C": family_c(), "D": family_d(), "E": family_e()}
    skipped, drawn = [], 0
    with multiprocessing.Pool(jobs) as pool:
        for fam, specs in fams.items():
            t0 = time.time()
            done = [(sp, one) for sp, one, err in pool.imap(run_spec, specs, chunksize=4)
                    if err is None or skipped.append(dict(sp, reason=err))]
            drawn += len(specs)
            store = {k: np.stack([one[k] for _, one in done]) for k in ("prm", "meta", "cam", "sha_t", "sha_fs", "sha_depth32", "t_bits", "refstats")}
            store["ids"] = np.array([[sp["sid"], sp["kid"]] for sp, _ in done], dtype=np.int32)
            store["view"] = np.array([sp["view"] for sp, _ in done], dtype=np.float64)
            store["iters"] = np.concatenate([one["iters"].reshape(-1) for _, one in done])
            store["off"] = np.cumsum([0] + [one["iters"].size for _, one in done]).astype(np.int64)
            store["hitbits"] = np.packbits(np.concatenate([one["hit"] for _, one in done]))
            store["tag"] = np.array([sp["tag"] for sp, _ in done])
            save_npz(os.path.join(OUT, f"frames_config_{fam}.npz"), store)
            print(f"  [config] family {fam}: {len(done)} cases of {len(specs)}, {int(store['off'][-1])} rays, "
                  f"{int(store['iters'].astype(np.int64).sum())} iterations, max {int(store['iters'].max())}  ({time.time() - t0:.0f}s)", flush=True)
    for s in skipped:
        print(f"  [config] SKIPPED (the reference raised) {s['tag']}: {s['reason']}", flush=True)
    with open(os.path.join(OUT, "frames_config_skipped.json"), "w", encoding="utf-8") as f:
        json.dump({"seed": CONFIG_SEED, "drawn": drawn, "skipped": skipped}, f, indent=1)


# (scene, strategy, MarchConfig arguments, constructor arguments, literal): Mandelbulb with three strategies is the team form
RAY_PAIRS = [(0, 0, dict(), {}, None), (2, 6, dict(max_iterations=64, hit_threshold=1e-3), dict(bisection_steps=5), None),
             (3, 10, dict(max_distance=9.0), {}, 3), (9, 4, dict(max_iterations=100), {}, None),
             (12, 9, dict(hit_threshold=1e-5, max_distance=30.0), dict(stuck_threshold=2), None),
             (1, 1, dict(max_iterations=2048, max_distance=1e4), dict(omega=1.6), None), (13, 7, dict(max_iterations=17), {}, 0.1),
             (16, 8, dict(max_iterations=200, hit_threshold=3e-3), {}, None),
             (10, 0, dict(max_iterations=300), {}, None), (10, 6, dict(max_iterations=40, hit_threshold=3e-4), {}, None),
             (10, 10, dict(max_iterations=128, max_distance=9.0), {}, 12)]


def ray_inputs(rng, scene, far, n=300):
    """Origins and directions as a caller of MarchStrategy.march may pass them: unit and un-normalised directions, exactly
    zero ones, lengths on both sides of Vec3.normalized()'s 1e-12, origins inside the object and beyond the far plane."""
    pos = default_view(scene)[0]

    def unit():
        while True:
            d = [rng.gauss(0.0, 1.0) for _ in range(3)]
            l = sum(c * c for c in d) ** 0.5
            if l > 0.1:
                return [c / l for c in d]

    def toward(o, spread):
        d = [-c for c in o]
        l = sum(c * c for c in d) ** 0.5 or 1.0
        return [c / l + rng.gauss(0.0, spread) for c in d]
    o, d = [], []
    for i in range(n):
        oi = [c + rng.gauss(0.0, 0.05) for c in pos]
        di = toward(oi, 0.25)
        if i < 100:                                                   # unit
            l = sum(c * c for c in di) ** 0.5
            di = [c / l for c in di]
        elif i < 170:                                                 # un-normalised, 1e-6 .. 1e6
            s = 10.0 ** rng.uniform(-6.0, 6.0)
            di = [c * s for c in di]
        elif i < 180:                                                 # exactly zero (one of them -0.0)
            di = [0.0, 0.0, -0.0 if i == 179 else 0.0]
        elif i < 200:                                                 # length just below 1e-12: normalises to the zero vector
            di = [c * rng.choice((0.999e-12, 0.9e-12, 1e-13, 1e-30)) for c in unit()]
        elif i < 220:                                                 # ... and just above
            di = [c * rng.choice((1.001e-12, 1.1e-12, 1e-11)) for c in unit()]
        elif i < 270:                                                 # origins in or near the object, any direction
            oi = [rng.uniform(-0.6, 0.6) for _ in range(3)]
            di = unit()
        else:                                                         # origins beyond the far plane, looking back
            u = unit()
            oi = [c * far * rng.uniform(1.01, 3.0) for c in u]
            di = toward(oi, 0.01)
        o.append(oi)
        d.append(di)
    return np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)


def run_ray_pair(args):
    from raymarching_benchmark.core.ray import Ray
    n, (sid, kid, mckw, ctor, lit) = args
    scene = SCENES[sid]
    strategy, lip, overrides = build_strategy(scene, kid, ctor, lit, None)
    mc = MarchConfig(**mckw)
    o, d = ray_inputs(random.Random(CONFIG_SEED + n), scene, mc.max_distance)
    res = [strategy.march(Ray(Vec3(*oi), Vec3(*di)), scene.sdf, mc) for oi, di in zip(o.tolist(), d.tolist())]
    prm = dict(PARAM_DEFAULTS, **overrides)
    pre = f"p{n}_"
    return {pre + "ids": np.array([sid, kid], dtype=np.int32), pre + "o": o, pre + "d": d,
            pre + "meta": np.array([mc.max_iterations, mc.hit_threshold, mc.max_distance, lip], dtype=np.float64),
            pre + "prm": np.array([float(prm[k]) for k in PARAM_ORDER], dtype=np.float64),
            pre + "hit": np.array([bool(r.hit) for r in res], dtype=np.uint8),
            pre + "iters": np.array([r.iterations for r in res], dtype=np.int32),
            pre + "t_bits": np.array([float(r.t) for r in res], dtype="<f8").view(np.uint64),
            pre + "fs_bits": np.array([float(r.final_sdf) for r in res], dtype="<f8").view(np.uint64)}


def gen_rays(jobs):
    """rays_config.npz: MarchStrategy.march on explicit Ray(origin, direction) objects (Ray.__init__ normalises, core/ray.py:11-13).
    Keys p{n}_: ids, meta (max_iterations, hit_threshold, max_distance, lipschitz), prm, o, d (inputs), hit, iters, t_bits, fs_bits."""
    import multiprocessing
    store = {}
    with multiprocessing.Pool(jobs) as pool:
        for part in pool.imap(run_ray_pair, list(enumerate(RAY_PAIRS))):
            store.update(part)
            n = next(iter(part)).split("_")[0]
            print(f"  [rays] pair {n}: hits {int(part[n + '_hit'].sum())} iterations {int(part[n + '_iters'].sum())}", flush=True)
    store["npairs"] = np.array([len(RAY_PAIRS)], dtype=np.int32)
    save_npz(os.path.join(OUT, "rays_config.npz"), store)


# ---- edge points of the scene SDFs -------------------------------------------------------------------------------------
# sdf_edges.npz / rays_edges.npz: layout, conditions and coverage are in tests/sdf_edge_cases.py, whose check_fixture
# runs here before anything is written.  A uniform draw (gen_sdf) never lands on a measure-zero edge; these do.
EDGE_SEED = 20261020
REGION = 3.5


def _edge_constants():
    """The lengths the catalogue is written with, read from its classes where they are attributes; the literals of its
    sdf() bodies are listed.  Returns (constants, sphere centres, spheres as (centre, radius))."""
    from raymarching_benchmark.scenes import catalog as C
    cloud = [(tuple(c), r) for c, r in C.SphereCloudScene.SPHERES]
    bumps = [(tuple(c), C.BumpySphereScene.BUMP_R) for c in C.BumpySphereScene.BUMPS]
    balls = [(tuple(c), r) for c, r in C.MetaballsScene.BALLS]
    single = [((0.0, 0.0, 0.0), r) for r in (1.0, 1.3, 2.0, C.BumpySphereScene.BASE_R, C.GyroidScene.RADIUS)]
    single += [((-1.01, 0.0, 0.0), 1.0), ((1.01, 0.0, 0.0), 1.0), ((-0.5, 0.0, 0.0), 0.8)]
    consts = {1.0, 0.5, 1.5, 0.05, 1.01, 1.3, 0.8, 0.6, 2.0, 0.1, 3.0, 0.15, 0.25, 0.01, 4.0, 2.5,
              C.BumpySphereScene.BASE_R, C.BumpySphereScene.BUMP_R, C.GyroidScene.FREQ, C.GyroidScene.LIP, C.GyroidScene.RADIUS,
              C.CappedTorusScene.RA, C.CappedTorusScene.RB, *C.CappedTorusScene.SC, C.BoxLatticeScene.C, C.BoxLatticeScene.L,
              C.BoxLatticeScene.BB, C.MetaballsScene.K}
    consts |= {r for _, r in cloud + balls}
    return sorted(consts), cloud, bumps, balls, single


def _rows(rng, rows):
    """points from rows of three entries; None is a coordinate drawn uniformly from the region"""
    a = rng.uniform(-REGION, REGION, size=(len(rows), 3))
    for i, r in enumerate(rows):
        for c in range(3):
            if r[c] is not None:
                a[i, c] = r[c]
    return a


def _with_neighbours(rng, a, share=0.5):
    """the points, and a copy of `share` of them with every coordinate moved one nextafter down, up or not at all"""
    pick = a[rng.random(len(a)) < share]
    step = rng.integers(-1, 2, size=pick.shape)
    return np.concatenate([a, np.nextafter(pick, np.where(step == 0, pick, np.where(step > 0, np.inf, -np.inf)))])


def _from_pools(rng, n, pools, weights, p_take=0.6, nudge=1.0 / 3.0):
    """The shared recipe: every coordinate is taken with probability p_take (at least one per point) from a pool chosen by
    weight, the others are uniform in the region; a share of all coordinates is nudged one nextafter either way."""
    a = rng.uniform(-REGION, REGION, size=(n, 3))
    take = rng.random((n, 3)) < p_take
    take[np.arange(n), rng.integers(0, 3, size=n)] = True
    which = rng.choice(len(pools), size=(n, 3), p=weights)
    for k, pool in enumerate(pools):
        pool = np.asarray(pool, dtype=np.float64)
        m = take & (which == k)
        a[m] = pool[rng.integers(0, len(pool), size=int(m.sum()))]
    step = rng.integers(0, 2, size=(n, 3)) * 2 - 1
    m = rng.random((n, 3)) < nudge
    a[m] = np.nextafter(a[m], step[m] * np.inf)
    return a, take


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def edge_points():
    """[(group name, points)] in fixture order"""
    rng = np.random.default_rng(EDGE_SEED)
    consts, cloud, bumps, balls, single = _edge_constants()
    pi = float(np.pi)
    signed = lambda v: [s * x for x in v for s in (1.0, -1.0)]                                    # noqa: E731
    core = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-12, -1e-12, 1e-13] + signed(consts)
    thirds = [k / s for s in (3.0, 9.0, 27.0) for k in range(-40, 41) if abs(k / s) <= REGION]
    sixths = [j * pi / 6.0 for j in range(-6, 7)]
    centres = [c for ctr, _ in cloud + bumps + balls for c in ctr]
    big = [100.0, -100.0, 1e3, -1e3, 1e4, 1e6]
    out = []
    out.append(("shared", _from_pools(rng, 1300, [core, thirds, sixths, centres, big], [0.4, 0.2, 0.1, 0.2, 0.1])[0]))

    # sphere-type scenes: every centre, and the surfaces along the axes (all six for the single spheres, two for the clouds)
    rows = [ctr for ctr, _ in cloud + bumps + balls + single]
    for n, (ctr, r) in enumerate(cloud + bumps + balls + single):
        few = n < len(cloud) + len(bumps)
        for ax in range(3):
            for s in ((1.0, -1.0) if not few else ((1.0 if n % 2 else -1.0,) if (n + ax) % 3 else ())):
                rows.append(tuple(ctr[c] + (s * r if c == ax else 0.0) for c in range(3)))
    out.append(("spheres", _with_neighbours(rng, _rows(rng, rows), 0.3)))

    # Near Miss: the tie plane x = +-0 (both spheres at one distance) and the +-0.01 gap
    rows = [(z, None, None) for z in (0.0, -0.0) * 15] + [(z, y, w) for z in (0.0, -0.0) for y in (0.0, 1e-300, 0.5) for w in (0.0, -1e-12)]
    rows += [(g, y, w) for g in (0.01, -0.01, 0.0) for y in (0.0, -0.0, 1e-13, 0.1) for w in (0.0, 0.05)]
    out.append(("near_miss", _with_neighbours(rng, _rows(rng, rows))))

    # planes: Grazing Plane's y = -0.5; Thin Planes' cell edges y = 0.25 + 0.5 k and sheets 0.5 k +- 0.01
    rows = [(None, -0.5, None)] * 6 + [(0.0, -0.5, 0.0), (1e6, -0.5, -1e6)]
    rows += [(None, 0.25 + 0.5 * k, None) for k in range(-8, 8) for _ in range(3)]
    rows += [(None, 0.5 * k + s, None) for k in range(-7, 8) for s in (0.01, -0.01, 0.0)]
    out.append(("planes", _with_neighbours(rng, _rows(rng, rows))))

    # boxes: faces, edges, corners and the q-tie diagonals (|x| - h == |y| - h) of half-extents 1 (Cube, Hollow Cube,
    # Menger), 0.6 about (0.5, 0, 0) (Smooth Blend) and 0.3 about a lattice node (Box Lattice)
    rows = []
    for h, ctr in ((1.0, (0.0, 0.0, 0.0)), (0.6, (0.5, 0.0, 0.0)), (0.3, (0.0, 0.0, 0.0)), (0.3, (1.0, -2.0, 2.0))):
        inside = lambda c: ctr[c] + float(rng.uniform(-h, h))                                   # noqa: E731
        sg = lambda: float(rng.choice((-1.0, 1.0)))                                             # noqa: E731
        for _ in range(10):                                                                       # faces
            ax = int(rng.integers(3))
            rows.append(tuple(ctr[c] + sg() * h if c == ax else inside(c) for c in range(3)))
        for _ in range(10):                                                                       # edges
            ax = int(rng.integers(3))
            rows.append(tuple(inside(c) if c == ax else ctr[c] + sg() * h for c in range(3)))
        rows += [tuple(ctr[c] + (h if (k >> c) & 1 else -h) for c in range(3)) for k in range(8)]   # corners
        for _ in range(18):                                                                       # diagonals: two or three equal |q|
            e = float(rng.choice((0.0, 0.25, -0.25, 0.5, 2.0 ** -30, -0.125)))
            three = rng.random() < 0.4
            ax = int(rng.integers(3))
            rows.append(tuple(inside(c) if (c == ax and not three) else ctr[c] + sg() * (h + e) for c in range(3)))
    out.append(("boxes", _with_neighbours(rng, _rows(rng, rows), 0.4)))

    # Thin Torus / Cylinder / Pillar Forest's cylinder: the axis, the caps y = +-1.5 and +-3, the rims
    rows = [(z, None, w) for z in (0.0, -0.0) for w in (0.0, -0.0) for _ in range(4)]
    rows += [(0.0, y, 0.0) for y in (0.0, -0.0, 1.5, -1.5, 3.0, -3.0, 0.05, 1e-300)]
    rows += [(float(rng.uniform(-0.7, 0.7)), y, float(rng.uniform(-0.7, 0.7))) for y in (1.5, -1.5, 3.0, -3.0) for _ in range(6)]
    rows += [(x, y, w) for y in (1.5, -1.5) for x, w in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.6, 0.8), (-0.8, 0.6))]
    rows += [(x, y, w) for y in (3.0, -3.0) for x, w in ((0.15, 0.0), (0.0, -0.15), (2.15, 2.0), (-2.0, 1.85))]
    th = rng.uniform(-pi, pi, size=16)
    rows += [(float(np.sin(t)), y, float(np.cos(t))) for t, y in zip(th, (1.5, -1.5) * 8)]
    out.append(("torus_cyl", _with_neighbours(rng, _rows(rng, rows))))

    # Thin Torus: the centre circle r = 1.5 of its tube
    th = rng.uniform(-pi, pi, size=32)
    rows = [(1.5 * float(np.sin(t)), y, 1.5 * float(np.cos(t))) for t, y in zip(th, (0.0, -0.0, 0.05, -0.05) * 8)]
    rows += [(x, y, w) for x, w in ((1.5, 0.0), (-1.5, 0.0), (0.0, 1.5), (0.0, -1.5), (0.9, 1.2), (1.2, -0.9)) for y in (0.0, -0.0, 0.05)]
    out.append(("thin_torus", _with_neighbours(rng, _rows(rng, rows))))

    # Onion Shell: the shells 2, 2 +- 0.1, 2 +- 0.1 +- 0.05 along the axes and in random directions
    radii = [2.0, 2.0 + 0.1, 2.0 - 0.1, 2.0 + 0.1 + 0.05, 2.0 + 0.1 - 0.05, 2.0 - 0.1 + 0.05, 2.0 - 0.1 - 0.05]
    rows = [tuple(s * r if c == ax else 0.0 for c in range(3)) for r in radii for ax in range(3) for s in (1.0, -1.0)]
    a = np.concatenate([_rows(rng, rows), _unit(rng, 56) * np.repeat(radii, 8)[:, None]])
    out.append(("onion", _with_neighbours(rng, a)))

    # Pillar Forest: cell edges at odd x, z (a zero remainder of `%`), pillar axes at even x, z
    odd, even = (-3.0, -1.0, 1.0, 3.0, 101.0), (-2.0, 0.0, -0.0, 2.0, 100.0)
    rows = [(float(rng.choice(odd)), None, None) for _ in range(15)] + [(None, None, float(rng.choice(odd))) for _ in range(15)]
    rows += [(float(rng.choice(odd)), y, float(rng.choice(odd))) for y in (None, 3.0, -3.0, 0.0) for _ in range(4)]
    rows += [(float(rng.choice(even)), y, float(rng.choice(even))) for y in (None, 3.0, -3.0, 0.0, None) for _ in range(5)]
    rows += [(float(rng.choice(even)) + s, None, float(rng.choice(even))) for s in (0.15, -0.15) for _ in range(5)]
    out.append(("pillars", _with_neighbours(rng, _rows(rng, rows))))

    # Menger: p * s an even integer for s = 1, 3, 9 (the jump of `%`), and +-1 / (3 s) beside it (the fold of the cross)
    planes = [v for s in (1.0, 3.0, 9.0) for k in range(-12, 13) for v in (2.0 * k / s, 2.0 * k / s + 1.0 / (3.0 * s), 2.0 * k / s - 1.0 / (3.0 * s))
              if abs(v) <= 1.5 or (s == 1.0 and abs(v) <= REGION)]
    out.append(("menger", _from_pools(rng, 220, [planes], [1.0], p_take=0.6, nudge=0.2)[0]))

    # Box Lattice: the ties x = k + 0.5 of floor(x + 0.5), the clamps |x| = 2.5 and beyond
    ties = [k + 0.5 for k in range(-4, 4)] + [2.5, -2.5, 2.6, -2.6, 3.2, -3.2, 3.5, -3.5, 100.0, -100.0, 2.2, -1.7, 0.3, -0.3, 1.3, 0.7]
    out.append(("lattice", _from_pools(rng, 160, [ties], [1.0], p_take=0.6, nudge=0.2)[0]))

    # Capped Torus: x = +-0 (the |x| kink), the branch line cos2 |x| = sin2 y, both arc ends
    from raymarching_benchmark.scenes.catalog import CappedTorusScene as CT
    s2, c2, ra, rb = CT.SC[0], CT.SC[1], CT.RA, CT.RB
    rows = [(z, None, w) for z in (0.0, -0.0) for w in (None, 0.0, -0.0) for _ in range(6)]
    rows += [(z, y, 0.0) for z in (0.0, -0.0) for y in (ra, -ra, ra + rb, ra - rb, 0.0, -0.0)]
    xs = np.concatenate([rng.uniform(-REGION, REGION, size=24), [1e-300, -1e-300, 5e-324, ra * s2, -ra * s2, 1.0]])
    rows += [(float(x), c2 * abs(float(x)) / s2, w) for x, w in zip(xs, (None, 0.0, -0.0) * 10)]
    rows += [(sx * (ra + e) * s2, (ra + e) * c2, w) for sx in (1.0, -1.0) for e in (0.0, rb, -rb) for w in (0.0, rb, -0.0)]
    out.append(("capped_torus", _with_neighbours(rng, _rows(rng, rows), 0.6)))
    # ... and 200 points of the centre circle of its tube, where p.p + ra^2 - 2 ra k cancels to +-1 ulp: the reference goes
    # complex where it rounds below zero
    th = rng.uniform(-2.0, 2.0, size=200)
    out.append(("ctorus_circle", np.stack([ra * np.sin(th), ra * np.cos(th), np.zeros(200)], axis=1)))

    # Gyroid: 3 x a multiple of pi / 2, the ball r = 2.2, coordinates on both sides of the sincos cut 105414336 / 3
    a, _ = _from_pools(rng, 60, [sixths], [1.0], p_take=0.7, nudge=0.3)
    R = 2.2
    rows = [tuple(s * R if c == ax else 0.0 for c in range(3)) for ax in range(3) for s in (1.0, -1.0)]
    b = np.concatenate([_rows(rng, rows), _unit(rng, 24) * R])
    cut = 105414336.0 / 3.0
    near = [cut, -cut, float(np.nextafter(cut, 0.0)), float(np.nextafter(cut, np.inf)), -float(np.nextafter(cut, 0.0)), cut - 1.0, cut + 1.0,
            cut - 0.125, 1e7, -3.5e7, 3.4e7]
    c, _ = _from_pools(rng, 44, [near], [1.0], p_take=0.5, nudge=0.0)
    out.append(("gyroid", np.concatenate([a, b, c])))

    # Mandelbulb: the origin, |p| on both sides of the 1e-12 clamps, the poles x = y = 0, the atan2 cut y = +-0 with x < 0,
    # x = +-0, and |p| = 1 and 4 (log r = 0, the bail-out) with neighbours on both sides
    rows = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0)]
    tiny = (1e-13, 9.99e-13, 1e-12, 1.0000001e-12, 2e-12, 5e-324, 1e-300, 1e-160, 1e-7)
    rows += [tuple(s * m if c == ax else z for c in range(3)) for m in tiny for ax in range(3) for s, z in ((1.0, 0.0), (-1.0, -0.0))]
    a = np.concatenate([_rows(rng, rows), _unit(rng, 24) * rng.choice(tiny, size=(24, 1))])
    rows = [(zx, zy, z) for zx in (0.0, -0.0) for zy in (0.0, -0.0) for z in (0.5, -0.5, 1.0, -1.0, 1.1, 4.0, -4.0, 1e-12, None, None)]
    rows += [(-abs(float(rng.uniform(0.05, 1.3))), zy, w) for zy in (0.0, -0.0) for w in (None, 0.0, -0.0, None, 0.3) for _ in range(3)]
    rows += [(zx, None, w) for zx in (0.0, -0.0) for w in (None, 0.0, -0.0, None, 0.3) for _ in range(3)]
    b = _rows(rng, rows)
    b[len(rows) - 60:] = np.clip(b[len(rows) - 60:], -1.3, 1.3)
    u = _unit(rng, 48)
    ring = [u[k] * (rad * (1.0 + (k - 24) * 2.0 ** -50)) for rad in (1.0, 4.0) for k in range(48)]
    for rad in (1.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0)), 4.0, float(np.nextafter(4.0, 0.0)), float(np.nextafter(4.0, 5.0))):
        ring += [np.array(r) for r in ((rad, 0.0, 0.0), (0.0, -rad, 0.0), (0.0, 0.0, rad), (-rad, -0.0, 0.0), (0.0, 0.0, -rad))]
    out.append(("mandelbulb", np.concatenate([a, b, np.array(ring)])))

    # huge: the shared recipe with magnitudes whose square leaves binary64's range or precision
    hugepool = [1e15, 2.0 ** 53, 1e100, 1e154, 1.4e154, 1e200, -1e200]
    a, take = _from_pools(rng, 380, [hugepool, core], [0.75, 0.25], nudge=0.1)
    none = ~(np.abs(a) >= 1e15).any(axis=1)
    a[none, 0] = np.asarray(hugepool)[rng.integers(0, len(hugepool), size=int(none.sum()))]
    out.append(("huge", a))
    return out


def _ref_sdf(scene, p):
    """(value, None) or (0.0, the exception's name); a complex value is the TypeError float() would raise"""
    try:
        v = scene.sdf(Vec3(float(p[0]), float(p[1]), float(p[2])))
        if isinstance(v, complex):
            return 0.0, "TypeError(complex)"
        return float(v), None
    except (OverflowError, TypeError, ValueError, ZeroDivisionError) as e:
        return 0.0, type(e).__name__


def _edge_cases_module():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import sdf_edge_cases
    return sdf_edge_cases


def gen_sdf_edges():
    ec = _edge_cases_module()
    groups = edge_points()
    names = [g for g, _ in groups]
    pts = np.ascontiguousarray(np.concatenate([a for _, a in groups]), dtype=np.float64)
    group = np.concatenate([np.full(len(a), i, dtype=np.int16) for i, (_, a) in enumerate(groups)])
    assert np.isfinite(pts).all()
    store = {"pts": pts, "group": group, "group_names": np.array(names)}
    want, raised = {}, {}
    for sid, scene in enumerate(SCENES):
        res = [_ref_sdf(scene, p) for p in pts]
        want[sid] = np.array([v for v, _ in res], dtype=np.float64)
        raised[sid] = np.array([e is not None for _, e in res], dtype=bool)
        kinds = {}
        for _, e in res:
            if e:
                kinds[e] = kinds.get(e, 0) + 1
        print(f"  [sdf_edges] {scene.name}: raised {int(raised[sid].sum())} {kinds}, NaN {int(np.isnan(want[sid]).sum())}, "
              f"-0.0 {int(((want[sid] == 0.0) & np.signbit(want[sid]) & ~raised[sid]).sum())}", flush=True)
        store[f"s{sid}"] = want[sid]
        store[f"raised_s{sid}"] = raised[sid]
    store["unclaimed_s16"] = ec.unclaimed_gyroid(pts)
    cov = ec.check_fixture(pts, group, names, want, raised)
    print(f"  [sdf_edges] {len(pts)} points, groups {dict(zip(names, np.bincount(group).tolist()))}")
    print(f"  [sdf_edges] coverage {cov}; minima {ec.MINIMA}")
    assert all(cov[k] >= v for k, v in ec.MINIMA.items()), (cov, ec.MINIMA)
    path = os.path.join(OUT, "sdf_edges.npz")
    save_npz(path, store)
    assert os.path.getsize(path) <= min(ec.LARGEST_FIXTURE_BEFORE, 1 << 20), os.path.getsize(path)
    print(f"  [sdf_edges] {os.path.getsize(path)} bytes")


def edge_rays(n=240):
    """Origins among the edge points of the non-huge groups where no scene's reference value is missing, every group met;
    directions by turns random, along an axis and aimed at the origin."""
    ec = _edge_cases_module()
    E = ec.Edges(np.load(os.path.join(OUT, "sdf_edges.npz")))
    rng = np.random.default_rng(EDGE_SEED + 1)
    ok = ~E.in_group("huge", "ctorus_circle")
    for sid in range(len(SCENES)):
        ok &= E.pinned(sid)
    ok &= (np.abs(E.pts) <= 1e4).all(axis=1)
    gids = [g for g in range(len(E.names)) if (ok & (E.group == g)).any()]
    o = []
    for k in range(n):
        cand = np.flatnonzero(ok & (E.group == gids[k % len(gids)]))
        o.append(E.pts[cand[rng.integers(len(cand))]])
    o = np.array(o)
    d = _unit(rng, n)
    for k in range(n):
        if k % 3 == 1:
            d[k] = 0.0
            d[k, (k // 3) % 3] = 1.0 if (k // 9) % 2 else -1.0
        elif k % 3 == 2 and np.abs(o[k]).sum() > 1e-6:
            d[k] = -o[k]                                  # un-normalised: Ray.__init__ normalises
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def run_edge_cells(sid):
    from raymarching_benchmark.core.ray import Ray
    ec = _edge_cases_module()
    scene = SCENES[sid]
    o, d = edge_rays()
    sha = np.zeros((len(STRAT_KEYS), len(ec.BUDGETS), 32), dtype=np.uint8)
    lips = np.zeros(len(STRAT_KEYS))
    for kid in range(len(STRAT_KEYS)):
        for bi, b in enumerate(ec.BUDGETS):
            strategy, lip, _ = build_strategy(scene, kid, {}, None, None)
            lips[kid] = lip
            mc = MarchConfig(max_iterations=b)
            res = [strategy.march(Ray(Vec3(*oi), Vec3(*di)), scene.sdf, mc) for oi, di in zip(o.tolist(), d.tolist())]   # a raise fails the run
            assert all(isinstance(r.t, float) and isinstance(r.final_sdf, float) for r in res), (sid, kid, b)
            sha[kid, bi] = np.frombuffer(ec.cell_hash(np.array([bool(r.hit) for r in res]), np.array([r.iterations for r in res]),
                                                      np.array([r.t for r in res]), np.array([r.final_sdf for r in res])), dtype=np.uint8)
    return sid, sha, lips


def gen_ray_edges(jobs):
    """rays_edges.npz: every scene x strategy x budget 0..3 marched by the reference's own march() from edge points; budget 0
    makes final_sdf the SDF at the origin itself, for every strategy."""
    import multiprocessing
    ec = _edge_cases_module()
    o, d = edge_rays()
    sha = np.zeros((len(SCENES), len(STRAT_KEYS), len(ec.BUDGETS), 32), dtype=np.uint8)
    lip = np.zeros((len(SCENES), len(STRAT_KEYS)))
    with multiprocessing.Pool(jobs) as pool:
        for sid, s, l in pool.imap(run_edge_cells, range(len(SCENES))):
            sha[sid], lip[sid] = s, l
            print(f"  [ray_edges] {SCENES[sid].name}: {s.shape[0] * s.shape[1]} cells of {len(o)} rays", flush=True)
    save_npz(os.path.join(OUT, "rays_edges.npz"), {"o": o, "d": d, "lip": lip, "budgets": np.array(ec.BUDGETS, dtype=np.int32), "sha": sha})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1), help="worker processes of --only config / rays / ray_edges")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    all_pairs = [(s, k) for s in range(len(SCENES)) for k in range(len(STRAT_KEYS))]
    graded9 = [0, 1, 2, 3, 4, 5, 6, 9, 10]  # the README's nine strategies (ids in STRATEGIES order)
    if a.only in ("all", "viewpoints"):
        gen_viewpoints()
    if a.only in ("all", "evals"):
        gen_evals()
    if a.only in ("all", "analytic"):
        gen_analytic()
    if a.only in ("all", "sdf"):
        gen_sdf()
    if a.only in ("all", "frames64"):
        gen_frames("64x48", 64, 48, all_pairs)
    if a.only in ("all", "frames160"):
        pairs = [(0, k) for k in graded9] + [(2, k) for k in graded9]
        pairs += [(s, k) for s in (9, 10) for k in (0, 4, 6)] + [(12, 0)]
        gen_frames("160x120", 160, 120, pairs)
    if a.only in ("all", "rows1080"):
        gen_rows1080([(0, 0), (2, 0), (9, 0), (10, 0), (10, 4), (10, 6), (12, 0)])
    if a.only in ("all", "leak"):
        gen_leak()
    if a.only in ("all", "leakseq"):
        gen_leakseq()
    if a.only in ("all", "params"):
        gen_params()
    if a.only in ("all", "schema"):
        gen_schema()
    if a.only in ("all", "config"):
        gen_config(a.jobs)
    if a.only in ("all", "rays"):
        gen_rays(a.jobs)
    if a.only in ("all", "sdf_edges"):
        gen_sdf_edges()
    if a.only in ("all", "ray_edges"):
        gen_ray_edges(a.jobs)
    if a.only in ("all", "small"):
        # max_iterations=100, 16x12: the configuration of the reference's own smoke test
        # (tests/test_smoke.py:31-43), every registry key on the Sphere.
        gen_frames("16x12_it100", 16, 12, [(0, k) for k in range(len(STRAT_KEYS))],
                   MarchConfig(max_iterations=100))


if __name__ == "__main__":
    main()
