#!/usr/bin/env python3
"""Per-frame cost of the certified first hit (rm_certify_render) on the GPU next to rm_interval_render of the same frame,
per scene with an interval extension -- the 14 catalogue scenes and the five program twins -- on the scene's default camera
(its suggested camera, else (0, 0, 5) looking at the origin; fov 60): ms per frame (hipEvent timing, median / min / max of
`--repeats` after `--warmup`, one process), the steps per ray (median / p95 / max; a step is two walks over the program),
the counts per status and the interval oracle's false hits (certified_oracle.error_bar).  Both renders without a prune, the
interval render without normals, tol 1e-5; l_global is the scene's Lipschitz bound.  No time is asserted anywhere: the
ratio to the interval render is the finding.  Appends one JSON line per scene to `--out` and prints a markdown table
(profiles/certify/README.md).

Usage:  python tools/certify_cost.py [--size 512x512] [--repeats 15] [--warmup 3] [--out profiles/certify/cost.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, certified_oracle, registry, scene_program, sweep  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify", "cost.jsonl"))
    a = ap.parse_args()
    _native.init(0)
    W, H = (int(v) for v in a.size.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    print("| scene | size | certify ms (median) | min | max | interval ms (median) | ratio | steps median | p95 | max | MISS | HIT | OPEN | "
          "interval hits | of them proven free | t_hi - t_interval median | max |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for base in registry.get_all_scenes():
            scene = sweep.sound_scene(base, twins=True)          # the scene, else its program twin
            if scene is None:
                continue
            pos = base.camera_position or (0.0, 0.0, 5.0)
            tgt = base.camera_target or (0.0, 0.0, 0.0)
            cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H)
            cfg = _native.certify_config(bound_radius=-1.0, l_global=max(1.0, float(base.known_lipschitz_bound() or 1.0)))
            ce = _native.certify_render(scene.id, cam.params14(), W, H, cfg, warmup=a.warmup, repeats=a.repeats)
            iv = _native.interval_render(scene.id, cam.params14(), W, H, _native.interval_config(bound_radius=-1.0),
                                         warmup=a.warmup, repeats=a.repeats, want_normal=False)
            bar = certified_oracle.error_bar(ce, {"hit": iv["hit"] > 0, "depth": iv["depth"]})
            steps = ce["steps"].ravel()
            row = {"scene": base.name, "width": W, "height": H,
                   "certify_ms_median": ce["timing"]["ms_median"], "certify_ms_min": ce["timing"]["ms_min"],
                   "certify_ms_max": ce["timing"]["ms_max"], "certify_ms_each": ce["timing"]["ms_each"],
                   "interval_ms_median": iv["timing"]["ms_median"], "interval_ms_each": iv["timing"]["ms_each"],
                   "ratio": ce["timing"]["ms_median"] / iv["timing"]["ms_median"],
                   "steps_median": float(np.median(steps)), "steps_p95": float(np.percentile(steps, 95)), "steps_max": int(steps.max()),
                   "interval_steps_median": float(np.median(iv["steps"])), "interval_steps_max": int(iv["steps"].max()),
                   "error_bar": bar, "repeats": a.repeats, "warmup": a.warmup}
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(f"| {base.name} | {W}x{H} | {row['certify_ms_median']:.3f} | {row['certify_ms_min']:.3f} | {row['certify_ms_max']:.3f} | "
                  f"{row['interval_ms_median']:.3f} | {row['ratio']:.2f} | {row['steps_median']:.0f} | {row['steps_p95']:.0f} | "
                  f"{row['steps_max']} | {bar['n_miss']} | {bar['n_hit']} | {bar['n_open']} | {bar['n_oracle_hit']} | {bar['false_hits']} | "
                  f"{bar['lag_median']:.2e} | {bar['lag_max']:.2e} |", flush=True)
    for sid in scene_program.catalogue_twins():          # the twins sweep.sound_scene registered on the way
        if registry.find_program_scene(scene_program.twin_name(sid)) is not None:
            scene_program.unregister_scene(scene_program.twin_name(sid))


if __name__ == "__main__":
    main()
