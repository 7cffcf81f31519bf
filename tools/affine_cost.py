#!/usr/bin/env python3
"""Per-frame cost of the affine range's march (rm_affine_render, RM_RANGE_AFFINE and RM_RANGE_MEET) on the GPU next to the
interval oracle (rm_interval_render, without normals) of the same frame, in one process: kernel ms per frame (hipEvent
timing, median of `--repeats` after `--warmup`) and the SDF segment evaluations of each march, for the 14 catalogue scenes
with an interval extension (with `--twins` also the five program twins, `--only-twins` those alone), on each scene's
default camera (its suggested camera, else (0, 0, 5) looking at the origin; fov 60), at the given sizes.  No time is gated: the comparison is against rm_interval_render of the same build and
scene.  A meet probe walks the scene's program twice, so fewer evaluations need not mean less time: that trade is what
this tool measures.  Appends one JSON line per scene and size to `--out` and prints a markdown table (DESIGN.md section
3, "Affine range").

Usage:  python tools/affine_cost.py [--sizes 512x512,1920x1080] [--repeats 7] [--warmup 2] [--out profiles/affine/cost.jsonl] [--twins | --only-twins]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, registry, scene_program  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine", "cost.jsonl"))
    ap.add_argument("--label", default=None, help="what the library was built from (default: git's short HEAD)")
    ap.add_argument("--twins", action="store_true",
                    help="also the program twins of Menger, Bad Lipschitz Sphere, Bumpy Sphere, Gyroid and Box Lattice "
                         "(scene_program.register_twin)")
    ap.add_argument("--only-twins", action="store_true", help="the program twins alone")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    _native.init(0)
    label = a.label or commit()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    print("| scene | size | affine ms | meet ms | interval ms | affine evals | meet evals | interval evals | same hit map |")
    print("|---|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        scenes = [] if a.only_twins else [s for s in registry.get_all_scenes() if _native.affine_supported(s.id)]
        if a.twins or a.only_twins:
            scenes += [scene_program.register_twin(sid) for sid in sorted(scene_program.catalogue_twins())]
        for scene in scenes:
            pos = scene.camera_position or (0.0, 0.0, 5.0)
            tgt = scene.camera_target or (0.0, 0.0, 0.0)
            for W, H in sizes:
                cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H).params14()
                aff = _native.affine_render(scene.id, cam, W, H, _native.RM_RANGE_AFFINE, warmup=a.warmup, repeats=a.repeats)
                meet = _native.affine_render(scene.id, cam, W, H, _native.RM_RANGE_MEET, warmup=a.warmup, repeats=a.repeats)
                d = _native.make_desc(scene.id, 0, cam, W, H)
                ivl = _native.interval_render(scene.id, cam, W, H, warmup=a.warmup, repeats=a.repeats, want_normal=False)
                evals = {k: int(v["steps"].sum(dtype=np.int64)) for k, v in (("affine", aff), ("meet", meet), ("interval", ivl))}
                same = bool(np.array_equal(aff["hit"], ivl["hit"]) and np.array_equal(meet["hit"], ivl["hit"]))
                row = {"commit": label, "scene": scene.name, "width": int(d.width), "height": int(d.height), "repeats": a.repeats,
                       "warmup": a.warmup, "affine_ms": aff["timing"]["ms_median"], "affine_ms_each": aff["timing"]["ms_each"],
                       "meet_ms": meet["timing"]["ms_median"], "meet_ms_each": meet["timing"]["ms_each"],
                       "interval_ms": ivl["timing"]["ms_median"], "interval_ms_each": ivl["timing"]["ms_each"],
                       "affine_evals": evals["affine"], "meet_evals": evals["meet"],
                       "interval_evals": evals["interval"], "same_hit_map": same, "hit_pixels": int((ivl["hit"] > 0).sum())}
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(f"| {scene.name} | {W}x{H} | {row['affine_ms']:.3f} | {row['meet_ms']:.3f} | {row['interval_ms']:.3f} | "
                      f"{evals['affine']} | {evals['meet']} | {evals['interval']} | {'yes' if same else 'no'} |", flush=True)


if __name__ == "__main__":
    main()
