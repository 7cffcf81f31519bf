#!/usr/bin/env python3
"""Cost of the discovery features on the GPU, in one process, per scene: the kernel time of rm_intrinsic_features at the
reference's sample counts (1500 points, 240 chords of 160 steps: 47 400 SDF evaluations per set) for nsets = 1 and 8
(hipEvent timing of the kernels without the copies, median of `--repeats` after `--warmup`) and the wall time of the whole
call (copies included); the wall time of the same features in NumPy over _native.sdf_eval
(features.intrinsic_features_numpy: seven round trips per Lipschitz estimate and one per chord); the kernel and wall time
of rm_view_features on the dense-march capture; and the wall time of that capture itself (rm_capture of the Dense-March
strategy, 40 000 iterations) -- the part of a `sweep.py --features` run that is the march, not the features.  The sample
box is the padded box of the capture's hit points, as in a sweep.  No time is gated.  Appends one JSON line per (scene,
nsets) to `--out` and prints a markdown table ("Discovery features").

Usage:  python tools/features_cost.py [--res 256] [--scenes Sphere,Pillar\\ Forest,Mandelbulb] [--repeats 15] [--warmup 3]
                                      [--out profiles/features/cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, features, registry  # noqa: E402
from raymarch_algo_compare_amd.viewpoints import viewpoints_for  # noqa: E402


def wall(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--scenes", default="Sphere,Pillar Forest,Mandelbulb")
    ap.add_argument("--counts", default="1,8")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features", "cost.jsonl"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    _native.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    print("| scene | res | nsets | intrinsic kernels ms | whole call ms | NumPy over sdf_eval ms | view kernels ms | view call ms | "
          "dense capture ms | statistics equal NumPy's |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for name in a.scenes.split(","):
            scene = registry.get_scene_by_name(name)
            vp = viewpoints_for(scene)[0]
            for _ in range(a.warmup):
                features.dense_capture(scene, vp, a.res, a.res)
            (cam, cap), capture_ms = wall(lambda: features.dense_capture(scene, vp, a.res, a.res), a.repeats)
            cams = cam.params14()[None]
            (view, vtm) = _native.view_features(cams, [cap], warmup=a.warmup, repeats=a.repeats)
            _, view_ms = wall(lambda: _native.view_features(cams, [cap]), a.repeats)
            v = features.view_features([cap], [cam])[0]
            if v["box"] is None:
                raise SystemExit(f"{scene.name}: fewer than {features.MIN_HITS} hits at {a.res}x{a.res}")
            lo, hi, diag = features.padded_box(*v["box"])
            rng = np.random.default_rng(0)
            for n in (int(c) for c in a.counts.split(",")):
                sets = [features.sample_sets(lo, hi, rng) for _ in range(n)]
                out, tm = features.intrinsic_features_device(scene.id, sets, warmup=a.warmup, repeats=a.repeats)
                _, call_ms = wall(lambda: features.intrinsic_features_device(scene.id, sets), a.repeats)
                want, numpy_ms = wall(lambda: features.intrinsic_features_numpy(scene.id, sets), a.numpy_repeats)
                same = all(np.array_equal([o["lipschitz_p99"], o["slab_median"]], [w["lipschitz_p99"], w["slab_median"]], equal_nan=True)
                           for o, w in zip(out, want))
                row = {"scene": scene.name, "viewpoint": vp.name, "res": a.res, "nsets": n, "repeats": a.repeats, "warmup": a.warmup,
                       "points_per_set": 6 * features._LIP_SAMPLES + features._CHORDS * features._CHORD_STEPS,
                       "kernels_ms": tm["ms_median"], "kernels_ms_each": tm["ms_each"], "call_ms": float(np.median(call_ms)),
                       "call_ms_each": call_ms, "numpy_ms": float(np.median(numpy_ms)), "numpy_ms_each": numpy_ms,
                       "view_kernels_ms": vtm["ms_median"], "view_kernels_ms_each": vtm["ms_each"],
                       "view_call_ms": float(np.median(view_ms)), "view_call_ms_each": view_ms,
                       "capture_ms": float(np.median(capture_ms)), "capture_ms_each": capture_ms, "hit_rate": view[0]["hit_rate"],
                       "lipschitz_p99": [o["lipschitz_p99"] for o in out], "thin_slab": [o["slab_median"] / diag for o in out],
                       "statistics_equal": bool(same)}
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(f"| {scene.name} | {a.res}x{a.res} | {n} | {row['kernels_ms']:.3f} | {row['call_ms']:.2f} | {row['numpy_ms']:.1f} | "
                      f"{row['view_kernels_ms']:.3f} | {row['view_call_ms']:.2f} | {row['capture_ms']:.2f} | {'yes' if same else 'NO'} |",
                      flush=True)


if __name__ == "__main__":
    main()
