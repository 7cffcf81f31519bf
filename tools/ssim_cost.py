#!/usr/bin/env python3
"""Cost of the SSIM / colour-RMSE scoring (rm_ssim_scores) on the GPU, in one process: the kernel time of scoring N = 1
and N = 11 method captures against one reference (hipEvent timing of the three kernels without the copies, median of
`--repeats` after `--warmup`) and the wall time of the whole call (copies included), next to the wall time of the same
scores in NumPy (scipy.ndimage.uniform_filter over float64, seven channels, the 8-bit images given) and the kernel time
of a Standard render of the frame the captures come from.  The captures are GPURunner.capture frames of one scene
(Standard as the reference, the other strategies of the shader's numbering as methods, repeated up to N).  No time is
gated.  Appends one JSON line per N to `--out` and prints a markdown table ("SSIM scoring").

Usage:  python tools/ssim_cost.py [--size 512x512] [--scene Sphere] [--repeats 15] [--warmup 3] [--out profiles/ssim/cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.ndimage import uniform_filter

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, registry, ssim  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig  # noqa: E402
from raymarch_algo_compare_amd.runner import GPURunner  # noqa: E402

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def numpy_plane(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
    k = 49 / 48
    vx, vy = k * (uniform_filter(x * x, size=7) - ux * ux), k * (uniform_filter(y * y, size=7) - uy * uy)
    vxy = k * (uniform_filter(x * y, size=7) - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return float(S[3:-3, 3:-3].mean())


def numpy_scores(method, reference):
    dr = ssim.depth_range(reference)
    r, m = ssim.to_images(reference, dr), ssim.to_images(method, dr)
    return [numpy_plane(r["depth"], m["depth"]),
            float(np.mean([numpy_plane(r["normal"][..., c], m["normal"][..., c]) for c in range(3)])),
            float(np.mean([numpy_plane(r["color"][..., c], m["color"][..., c]) for c in range(3)])),
            float(np.sqrt(np.mean((r["color"].astype(np.float64) - m["color"]) ** 2)))]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--scene", default="Sphere")
    ap.add_argument("--counts", default="1,11")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim", "cost.jsonl"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    _native.init(0)
    W, H = (int(v) for v in a.size.split("x"))
    scene = registry.get_scene_by_name(a.scene)
    pos, tgt = scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0)
    rc, mc, runner = RenderConfig(width=W, height=H, camera_position=pos, camera_target=tgt), MarchConfig(), GPURunner()
    caps = [runner.capture(scene.id, k, rc, mc) for k in range(8)]
    reference = caps[0]
    cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H).params14()
    render = _native.render(_native.make_desc(scene.id, 0, cam, W, H, full=True), warmup=a.warmup, repeats=a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    print("| scene | size | N | kernels ms | whole call ms | NumPy ms | Standard render ms | max abs difference to NumPy |")
    print("|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for n in (int(v) for v in a.counts.split(",")):
            methods = [caps[1 + i % 7] for i in range(n)]
            out, tm = _native.ssim_scores(W, H, reference, methods, warmup=a.warmup, repeats=a.repeats)
            walls = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                _native.ssim_scores(W, H, reference, methods)
                walls.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want = np.array([numpy_scores(m, reference) for m in methods])
            numpy_ms = (time.perf_counter() - t0) * 1e3
            row = {"scene": scene.name, "width": W, "height": H, "n": n, "repeats": a.repeats, "warmup": a.warmup,
                   "kernels_ms": tm["ms_median"], "kernels_ms_each": tm["ms_each"], "call_ms": float(np.median(walls)),
                   "call_ms_each": walls, "numpy_ms": numpy_ms, "render_ms": render["timing"]["ms_median"],
                   "render_ms_each": render["timing"]["ms_each"], "max_abs_diff": float(np.abs(out - want).max())}
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(f"| {scene.name} | {W}x{H} | {n} | {row['kernels_ms']:.3f} | {row['call_ms']:.2f} | {numpy_ms:.0f} | "
                  f"{row['render_ms']:.3f} | {row['max_abs_diff']:.1e} |", flush=True)


if __name__ == "__main__":
    main()
