#!/usr/bin/env python3
"""Per-frame cost of the exact first hit (rm_exact_render) on the GPU, per scene with an exact form -- catalogue ids 0-6,
8 and 14 and the program twins of Bad Lipschitz Sphere and Bumpy Sphere -- on the scene's default camera (its suggested
camera, else (0, 0, 5) looking at the origin; fov 60): ms per frame (hipEvent timing, median / min / max of `--repeats`
after `--warmup`), next to rm_interval_render of the same frame (tol 1e-5) and, for the four scenes analytic.py covers,
the wall time of analytic.analytic_depth on the host.  Appends one JSON line per scene to `--out` and prints a markdown
table (profiles/exact/README.md).

Usage:  python tools/exact_cost.py [--size 512x512] [--repeats 15] [--warmup 3] [--out profiles/exact/cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, analytic, registry, scene_program, sweep  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact", "cost.jsonl"))
    a = ap.parse_args()
    _native.init(0)
    W, H = (int(v) for v in a.size.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    print("| scene | size | leaves hit | exact ms (median) | min | max | interval ms (median) | analytic.py ms (host) | hit pixels | "
          "exact hits that are interval hits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for base in registry.get_all_scenes():
            scene = sweep.exact_scene(base, twins=True)          # the scene, else its program twin when that has an exact form
            if scene is None:
                continue
            pos = base.camera_position or (0.0, 0.0, 5.0)
            tgt = base.camera_target or (0.0, 0.0, 0.0)
            cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H)
            ex = _native.exact_render(scene.id, cam.params14(), W, H, _native.exact_config(t_max=100.0), warmup=a.warmup,
                                      repeats=a.repeats)
            iv = _native.interval_render(scene.id, cam.params14(), W, H, _native.interval_config(bound_radius=-1.0),
                                         warmup=a.warmup, repeats=a.repeats, want_normal=True)
            host_ms = None
            if analytic.has_analytic(base.name):
                t0 = time.perf_counter()
                analytic.analytic_depth(base.name, cam)
                host_ms = (time.perf_counter() - t0) * 1e3
            hit = ex["hit"] > 0
            row = {"scene": base.name, "width": W, "height": H, "leaves_hit": int(len(np.unique(ex["leaf"][hit]))) if hit.any() else 0,
                   "exact_ms_median": ex["timing"]["ms_median"], "exact_ms_min": ex["timing"]["ms_min"],
                   "exact_ms_max": ex["timing"]["ms_max"], "exact_ms_each": ex["timing"]["ms_each"],
                   "interval_ms_median": iv["timing"]["ms_median"], "interval_ms_each": iv["timing"]["ms_each"],
                   "analytic_host_ms": host_ms, "hit_pixels": int(hit.sum()),
                   "exact_hits_in_interval": int((hit & (iv["hit"] > 0)).sum()), "repeats": a.repeats, "warmup": a.warmup}
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(f"| {base.name} | {W}x{H} | {row['leaves_hit']} | {row['exact_ms_median']:.3f} | {row['exact_ms_min']:.3f} | "
                  f"{row['exact_ms_max']:.3f} | {row['interval_ms_median']:.3f} | "
                  f"{'-' if host_ms is None else format(host_ms, '.1f')} | {row['hit_pixels']} | {row['exact_hits_in_interval']} |",
                  flush=True)
    for sid in scene_program.catalogue_twins():          # the twins sweep.exact_scene registered on the way
        if registry.find_program_scene(scene_program.twin_name(sid)) is not None:
            scene_program.unregister_scene(scene_program.twin_name(sid))


if __name__ == "__main__":
    main()
