#!/usr/bin/env python3
"""Cost of capture on the device (rm_capture, rm_shade_frames) on the GPU, in one process, per scene and size:
  * the wall time of GPURunner.capture(device=False) -- the host path: fp64 maps down, NumPy rays and hit points, four
    points per hit up through rm_sdf_eval, NumPy shading -- against device=True (rm_capture: float maps down only);
  * the kernel time of the capture kernel alone (rm_shade_frames on the frame's own t, hipEvent timing without the
    copies) next to the Standard render of the same frame and to the two together (timed rm_capture);
  * the wall time of rm_shade_frames for N = 1 and N = 11 frames in one call against N runner.hit_normals calls (what
    sweep.ssim_columns does per kept row without --device-capture).
Medians of `--repeats` after `--warmup`.  No time is gated.  Appends one JSON line per row to `--out` and prints a
markdown table ("Capture on the device").

Usage:  python tools/capture_cost.py [--sizes 512x512,1920x1080] [--scenes Sphere,Mandelbulb] [--repeats 9] [--warmup 2]
                                     [--out profiles/capture/cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, registry  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig  # noqa: E402
from raymarch_algo_compare_amd.runner import GPURunner, hit_normals, ray_directions  # noqa: E402


def wall_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--scenes", default="Sphere,Mandelbulb")
    ap.add_argument("--counts", default="1,11")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture", "cost.jsonl"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    _native.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    runner, mc = GPURunner(), MarchConfig()
    print("| scene | size | host capture ms | device capture ms | render kernel ms | capture kernel ms | render + capture ms | "
          "N | N hit_normals ms | rm_shade_frames ms | shade kernel ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for name in a.scenes.split(","):
            scene = registry.get_scene_by_name(name)
            pos, tgt = scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0)
            for size in a.sizes.split(","):
                W, H = (int(v) for v in size.split("x"))
                rc = RenderConfig(width=W, height=H, camera_position=pos, camera_target=tgt)
                cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H)
                desc = _native.make_desc(scene.id, 0, cam.params14(), W, H, full=True)
                host_ms, host_each = wall_ms(lambda: runner.capture(scene.id, 0, rc, mc, device=False), a.warmup, a.repeats)
                dev_ms, dev_each = wall_ms(lambda: runner.capture(scene.id, 0, rc, mc, device=True), a.warmup, a.repeats)
                r = _native.render(desc, want_t_raw=True, want_final_sdf=True, want_evals=True, warmup=a.warmup, repeats=a.repeats)
                both = _native.capture(desc, warmup=a.warmup, repeats=a.repeats)
                shade = _native.shade_frames(scene.id, cam.params14(), r["hit"], t=r["t_raw"], warmup=a.warmup, repeats=a.repeats)
                hit = r["hit"] > 0
                depth = np.where(hit, r["t_raw"], 0.0)
                rd = ray_directions(cam)
                for n in (int(v) for v in a.counts.split(",")):
                    cams = np.stack([cam.params14()] * n)
                    hits, ts = np.stack([r["hit"]] * n), np.stack([r["t_raw"]] * n)
                    normals_ms, normals_each = wall_ms(lambda: [hit_normals(scene.id, cam, rd, depth, hit) for _ in range(n)],
                                                       a.warmup, a.repeats)
                    frames_ms, frames_each = wall_ms(lambda: _native.shade_frames(scene.id, cams, hits, t=ts), a.warmup, a.repeats)
                    frames_k = _native.shade_frames(scene.id, cams, hits, t=ts, warmup=a.warmup, repeats=a.repeats)["timing"]
                    row = {"scene": scene.name, "width": W, "height": H, "hits": int(hit.sum()), "repeats": a.repeats, "warmup": a.warmup,
                           "host_capture_ms": host_ms, "host_capture_ms_each": host_each,
                           "device_capture_ms": dev_ms, "device_capture_ms_each": dev_each,
                           "render_kernel_ms": r["timing"]["ms_median"], "render_kernel_ms_each": r["timing"]["ms_each"],
                           "capture_kernel_ms": shade["timing"]["ms_median"], "capture_kernel_ms_each": shade["timing"]["ms_each"],
                           "render_capture_kernels_ms": both["timing"]["ms_median"], "render_capture_kernels_ms_each": both["timing"]["ms_each"],
                           "n": n, "hit_normals_ms": normals_ms, "hit_normals_ms_each": normals_each,
                           "shade_frames_ms": frames_ms, "shade_frames_ms_each": frames_each,
                           "shade_frames_kernel_ms": frames_k["ms_median"], "shade_frames_kernel_ms_each": frames_k["ms_each"]}
                    f.write(json.dumps(row) + "\n")
                    f.flush()
                    print(f"| {scene.name} | {W}x{H} | {host_ms:.1f} | {dev_ms:.2f} | {row['render_kernel_ms']:.3f} | "
                          f"{row['capture_kernel_ms']:.3f} | {row['render_capture_kernels_ms']:.3f} | {n} | {normals_ms:.1f} | "
                          f"{frames_ms:.2f} | {row['shade_frames_kernel_ms']:.3f} |", flush=True)


if __name__ == "__main__":
    main()
