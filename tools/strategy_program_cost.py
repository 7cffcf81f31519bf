#!/usr/bin/env python3
"""What the strategy-program interpreter costs: each twin of strategy_program.strategy_twins() next to the compiled
kernel it restates, on one MI355X.

  python tools/strategy_program_cost.py [--out profiles/strategy_program/cost.jsonl] [--width 1920 --height 1080]

Like is compared with like: the compiled kernel is forced to the plan a program frame always gets (rm_launch_plan.h,
plan_strategy_program) -- one plain render pass: no suspension, no single launch, whole evaluations, the static tile
order -- and its default plan is timed as a third column.  Device time of the frame (rm_bench_device-style timing through
rm_render_outputs: events around the launches, outputs on the device), 3 warm-up frames, the median of 15; the three
columns of a row are measured one after the other (program, compiled on the same plan, compiled on its default plan),
and that round is run twice; both rounds are written.  One JSON line per (scene, strategy, round):
ms_program, ms_compiled_plain, ms_compiled_default, ratio = ms_program / ms_compiled_plain, mean iterations and
evaluations per ray (equal by construction: the tool stops with an error if the program frame and the compiled frame
differ in any of iters, hit, depth or evals), and the overhead
per step in nanoseconds of frame time per evaluation, (ms_program - ms_compiled_plain) / evaluations.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, registry                      # noqa: E402
from raymarch_algo_compare_amd import strategy_program as sp                 # noqa: E402
from raymarch_algo_compare_amd.camera import Camera                          # noqa: E402

SCENES = [0, 12, 10]          # Sphere, Pillar Forest, Mandelbulb
PLAIN = dict(pipeline=1, suspend_after=(-1, -1), eval_mode=1, tile_order_mode=0, tile_rows=4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strategy_program", "cost.jsonl"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args(argv)
    _native.init()
    W, H = a.width, a.height
    twins = sp.strategy_twins()
    ids = {k: _native.strategy_program_create(p.to_ops(), len(p)) for k, p in twins.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    try:
        with open(a.out, "w", encoding="utf-8") as f:
            for sid in SCENES:
                scene = registry.SCENES[sid]
                cam = Camera(scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0),
                             60.0, W, H).params14()
                for key, pid in ids.items():
                    kid = registry.STRATEGIES[key]
                    descs = {"program": _native.make_desc(sid, pid, cam, W, H),
                             "compiled_plain": _native.make_desc(sid, kid, cam, W, H, **PLAIN),
                             "compiled_default": _native.make_desc(sid, kid, cam, W, H)}
                    for rnd in range(2):
                        row = {"scene": scene.name, "strategy": key, "round": rnd, "width": W, "height": H}
                        outs = {}
                        for col, d in descs.items():
                            outs[col] = _native.render(d, warmup=a.warmup, repeats=a.repeats, want_evals=True)
                            row["ms_" + col] = outs[col]["timing"]["ms_median"]
                        same = all(np.array_equal(outs["program"][k], outs["compiled_plain"][k]) for k in ("iters", "hit", "depth", "evals"))
                        if not same:
                            raise SystemExit(f"{scene.name} / {key}: the program frame differs from the compiled frame")
                        ev = float(outs["program"]["evals"].sum())
                        row.update(bit_identical=bool(same), iters_mean=float(outs["program"]["iters"].mean()),
                                   evals_per_ray=ev / (W * H), ratio=row["ms_program"] / row["ms_compiled_plain"],
                                   overhead_ns_per_eval=(row["ms_program"] - row["ms_compiled_plain"]) * 1e6 / max(ev, 1.0))
                        f.write(json.dumps(row) + "\n")
                        f.flush()
                        print(json.dumps(row))
    finally:
        for pid in ids.values():
            _native.strategy_program_destroy(pid)
    return 0


if __name__ == "__main__":
    sys.exit(main())
