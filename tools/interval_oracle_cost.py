#!/usr/bin/env python3
"""Per-frame cost of the interval oracle (rm_interval_render) on the GPU: ms per frame (hipEvent timing, median of
`--repeats` after `--warmup`) and steps per ray (mean / p99 / max over the rays that were not pruned) for the 14
catalogue scenes with an interval extension, on each scene's default camera (its suggested camera, else (0, 0, 5)
looking at the origin; fov 60), at the given sizes.  Prints a markdown table ("Interval oracle").

Usage:  python tools/interval_oracle_cost.py [--sizes 384x384,1920x1080] [--repeats 5] [--warmup 1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from raymarch_algo_compare_amd import _native, registry  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="384x384,1920x1080")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    _native.init(0)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    print("| scene | size | ms / frame (median) | steps / ray mean | p99 | max | hit pixels |")
    print("|---|---|---|---|---|---|---|")
    for scene in registry.get_all_scenes():
        if not _native.interval_supported(scene.id):
            continue
        pos = scene.camera_position or (0.0, 0.0, 5.0)
        tgt = scene.camera_target or (0.0, 0.0, 0.0)
        for W, H in sizes:
            cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H)
            out = _native.interval_render(scene.id, cam.params14(), W, H, warmup=a.warmup, repeats=a.repeats)
            st = out["steps"][out["steps"] > 0]
            st = st if st.size else np.zeros(1)
            print(f"| {scene.name} | {W}x{H} | {out['timing']['ms_median']:.3f} | {st.mean():.1f} | "
                  f"{np.percentile(st, 99):.0f} | {st.max()} | {int(out['hit'].sum())} |", flush=True)


if __name__ == "__main__":
    main()
