#!/usr/bin/env python3
"""How many fractal trips the evaluations of a Mandelbulb frame's longest rays take (CPU only).

The oracle renders the frame (Standard), the N rays with the most iterations are marched again in NumPy on top of the
host check build of SceneMandelbulb (tests/native/short_last_trip_check.cpp: begin / trip / value), and every
evaluation's trip count is tallied.  The short last trip (rm_scenes.h) saves time only on evaluations that take all
eight trips, and a team's loop runs as many trips as the slowest of the rays it carries: `rays` is the share of single
evaluations with eight trips, `steps(k)` the share of steps in which at least one of k rays marching side by side does.

    python tests/trip_counts.py [--width 1920 --height 1080 --rays 64 --threads 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # test infrastructure, lives under tests/: it loads oracle/


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--threads", type=int, default=4)
    args = ap.parse_args()
    import short_last_trip_cases as C
    from oracle import oracle
    W, H = args.width, args.height
    cam = C.frame_camera(W, H)
    fr = oracle.render(10, 0, cam, W, H, nthreads=args.threads)
    o, d = C.frame_rays(cam, W, H)
    it = fr.iters.ravel()
    top = np.argsort(-it, kind="stable")[:args.rays]
    its, trips = C.trace_standard(np.repeat(o[None], len(top), 0), d.reshape(-1, 3)[top])
    hist = np.bincount(trips[trips >= 0], minlength=9)
    out = {"frame": f"{W}x{H}", "rays": int(len(top)), "iterations min/max": [int(it[top].min()), int(it[top].max())],
           "evaluations": int(hist.sum()), "by_trips_0..8": hist.tolist(), "eight_trip_share_rays": round(float(hist[8] / hist.sum()), 4)}
    rng = np.random.default_rng(1)
    for k in (1, 2, 4, 8, 16, 64):
        if k > len(top):
            break
        shares = []
        for _ in range(32 if k < len(top) else 1):
            sel = rng.choice(len(top), k, replace=False)
            live = (trips[sel] >= 0).any(axis=0)
            shares.append(float(((trips[sel] == 8).any(axis=0) & live).sum() / live.sum()))
        out[f"eight_trip_share_steps({k})"] = round(float(np.mean(shares)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
