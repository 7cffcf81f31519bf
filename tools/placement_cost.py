#!/usr/bin/env python3
"""Cost of the placement ops of scene programs (op_rotate, op_turn, op_mirror), 1920x1080, Standard, full = 0.

1. Regression check.  The five catalogue twins (scene_program.catalogue_twins) hold none of the new ops but run the
   kernels that gained them (SceneExtProgram).  They are timed with this tree's library and with a library built from the
   parent commit (--parent-lib), each in a fresh process, in rounds of parent, this, parent: the two parent runs of a round
   give the noise band, and this tree's time must lie inside the band of the parent's times over all rounds.
2. The price of the ops.  A union of six translated boxes against the same six boxes each under an op_rotate with three
   non-zero angles: ms per frame and SDF evaluations (the iteration maps differ: the solids do).

  python tools/placement_cost.py --parent-lib <parent>/raymarch_algo_compare_amd/librm_hip.so [--rounds 5] [--repeats 20]
                                 [--out profiles/placement/cost.jsonl]

Without --parent-lib only part 2 runs.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TWIN_IDS = [9, 11, 15, 16, 18]
BOXES = [((-1.6, 0.9, 0.2), (0.45, 0.3, 0.35), (0.4, -0.7, 0.3)), ((0.0, 1.0, -0.3), (0.35, 0.4, 0.3), (-0.5, 0.3, 0.9)),
         ((1.6, 0.8, 0.1), (0.4, 0.35, 0.45), (1.1, 0.6, -0.4)), ((-1.5, -0.8, 0.0), (0.5, 0.3, 0.3), (-0.3, -1.2, 0.5)),
         ((0.1, -0.9, 0.4), (0.3, 0.45, 0.4), (0.8, 0.2, 1.3)), ((1.5, -0.9, -0.2), (0.35, 0.35, 0.5), (-0.9, 0.7, -0.6))]


def _frame(_native, scene_id, cam, W, H, repeats):
    out = _native.render(_native.make_desc(scene_id, 0, cam, W, H, full=False), warmup=3, repeats=repeats)
    return out["timing"]["ms_median"], int(out["iters"].astype(np.int64).sum()), int((out["hit"] > 0).sum())


def time_twins(W, H, repeats):
    """{scene id: ms} of the five twins with the library RM_HIP_LIB names (the child of part 1)"""
    from raymarch_algo_compare_amd import _native, registry
    from raymarch_algo_compare_amd import scene_program as sp
    from raymarch_algo_compare_amd.camera import Camera
    _native.init()
    out = {}
    for sid in TWIN_IDS:
        s = registry.SCENES[sid]
        arr, n = sp.to_ctypes(sp.catalogue_twins()[sid])
        pid = _native.scene_program_create(arr, n, s.lipschitz or 1.0)
        cam = Camera(s.camera_position or (0.0, 0.0, 5.0), s.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                     W, H).params14()
        ms, evals, _ = _frame(_native, pid, cam, W, H, repeats)
        out[str(sid)] = {"ms": ms, "evals": evals}
        _native.scene_program_destroy(pid)
    return out


def child(lib, a):
    env = dict(os.environ)
    if lib:
        env["RM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("RM_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--width", str(a.width), "--height", str(a.height),
                        "--repeats", str(a.repeats)], env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(r.stdout.strip().splitlines()[-1])


def regression(a, rows):
    from raymarch_algo_compare_amd import registry
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):
        runs["parent"].append(child(a.parent_lib, a))
        runs["this"].append(child(None, a))
        runs["parent"].append(child(a.parent_lib, a))
    ok = True
    print("| twin | parent ms (min .. max of the runs) | this tree ms (median) | inside the band | evaluations |")
    print("|---|---|---|---|---|")
    for sid in TWIN_IDS:
        p = [r[str(sid)]["ms"] for r in runs["parent"]]
        t = [r[str(sid)]["ms"] for r in runs["this"]]
        same = runs["parent"][0][str(sid)]["evals"] == runs["this"][0][str(sid)]["evals"]
        med = float(np.median(t))
        inside = med <= max(p)                      # (faster than every parent run is no regression)
        ok = ok and inside and same
        name = registry.SCENES[sid].name
        rows.append({"part": "regression", "scene_id": sid, "scene": name, "parent_ms": p, "this_ms": t, "this_ms_median": med,
                     "inside_band": inside, "same_evaluations": same, "evals": runs["this"][0][str(sid)]["evals"]})
        print(f"| {name} | {float(np.median(p)):.3f} ({min(p):.3f} .. {max(p):.3f}) | {med:.3f} | {'yes' if inside else 'NO'} | "
              f"{runs['this'][0][str(sid)]['evals']}{'' if same else ' (parent differs)'} |", flush=True)
    return ok


def price(a, rows):
    from raymarch_algo_compare_amd import _native
    from raymarch_algo_compare_amd import scene_program as sp
    from raymarch_algo_compare_amd.camera import Camera
    _native.init()
    W, H = a.width, a.height
    cam = Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()

    def union(make):
        e = None
        for off, half, ang in BOXES:
            leaf = make(off, half, ang)
            e = leaf if e is None else sp.op_union(e, leaf)
        return e

    scenes = {
        "six translated boxes": union(lambda off, half, ang: sp.op_translate(off, sp.sd_box(half))),
        "six translated boxes, each under op_rotate": union(lambda off, half, ang: sp.op_translate(off, sp.op_rotate(ang, sp.sd_box(half)))),
    }
    ids = {}
    for name, e in scenes.items():
        arr, n = sp.to_ctypes(e)
        ids[name] = (_native.scene_program_create(arr, n, 1.0), n)
    ms = {name: [] for name in scenes}
    evals, hits = {}, {}
    for _ in range(a.rounds):
        for name, (pid, _) in ids.items():
            m, evals[name], hits[name] = _frame(_native, pid, cam, W, H, a.repeats)
            ms[name].append(m)
    print("\n| scene | ops | ms per frame | SDF evaluations | ns per evaluation | hit pixels |")
    print("|---|---|---|---|---|---|")
    for name, (pid, n) in ids.items():
        m = float(np.median(ms[name]))
        rows.append({"part": "price", "scene": name, "ops": n, "ms": ms[name], "ms_median": m, "evals": evals[name], "hits": hits[name]})
        print(f"| {name} | {n} | {m:.3f} | {evals[name]} | {1e6 * m / evals[name]:.4f} | {hits[name]} |", flush=True)
        _native.scene_program_destroy(pid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(time_twins(a.width, a.height, a.repeats)))
        return 0
    rows = []
    ok = regression(a, rows) if a.parent_lib else True
    price(a, rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            for r in rows:
                f.write(json.dumps({"width": a.width, "height": a.height, "strategy": "Standard", "full": 0, **r}) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
