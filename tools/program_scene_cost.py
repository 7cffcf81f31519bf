#!/usr/bin/env python3
"""Cost of the scene-program interpreter: each of the 14 catalogue scenes restated as a program
(scene_program.catalogue_expressions) against its built-in kernel, 1920x1080, Standard, full = 0, the scene's
suggested camera.  Rounds interleave the two so both see the same clocks; the table reports the median of the
per-round medians and checks that both frames have the same iteration map.

  python tools/program_scene_cost.py [--rounds 5] [--repeats 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raymarch_algo_compare_amd import _native, registry  # noqa: E402
from raymarch_algo_compare_amd import scene_program as sp  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _native.init()
    W, H = a.width, a.height
    rows = []
    for sid, expr in sp.catalogue_expressions().items():
        s = registry.SCENES[sid]
        arr, n = sp.to_ctypes(expr)
        pid = _native.scene_program_create(arr, n, s.lipschitz or 1.0)
        try:
            cam = Camera(s.camera_position or (0.0, 0.0, 5.0), s.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                         W, H).params14()
            ms = {"builtin": [], "program": []}
            iters = {}
            for _ in range(a.rounds):
                for key, scene_id in (("builtin", sid), ("program", pid)):
                    out = _native.render(_native.make_desc(scene_id, 0, cam, W, H, full=False), warmup=3, repeats=a.repeats)
                    ms[key].append(out["timing"]["ms_median"])
                    iters[key] = out["iters"]
            same = bool(np.array_equal(iters["builtin"], iters["program"]))
            b, p = float(np.median(ms["builtin"])), float(np.median(ms["program"]))
            rows.append({"scene_id": sid, "scene": s.name, "ops": n, "builtin_ms": b, "program_ms": p, "ratio": p / b,
                         "same_iterations": same})
            print(f"{s.name:22s} ops {n:3d}   built-in {b:7.3f} ms   program {p:7.3f} ms   x{p / b:5.2f}   "
                  f"{'same' if same else 'DIFFERENT'} iterations", flush=True)
        finally:
            _native.scene_program_destroy(pid)
    if a.json:
        with open(a.json, "w", encoding="utf-8") as f:
            json.dump({"width": W, "height": H, "strategy": "Standard", "full": 0, "rows": rows}, f, indent=1)
    if not all(r["same_iterations"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
