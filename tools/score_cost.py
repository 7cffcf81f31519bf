#!/usr/bin/env python3
"""Cost of the hit-mask / depth / normal scoring (rm_score_captures) on the GPU, in one process: the kernel time of scoring
N = 1 and N = 11 method captures against one reference (hipEvent timing of the kernels without the copies, median of
`--repeats` after `--warmup`) and the wall time of the whole call (copies included), next to the wall time of the same
reports in NumPy (scoring.score_capture + scoring.residual with its silhouette band, per method; median of `--repeats`)
and the kernel time of a Standard render of the frame the captures come from.  The captures are GPURunner.capture frames
of one scene (Standard as the reference, the other strategies of the shader's numbering as methods, repeated up to N),
float32 maps with normals.  No time is gated.  Appends one JSON line per N to `--out` and prints a markdown table
("Scoring on the device").

Usage:  python tools/score_cost.py [--size 512x512] [--scene Sphere] [--repeats 15] [--warmup 3] [--out profiles/score/cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import _native, registry, scoring  # noqa: E402
from raymarch_algo_compare_amd.camera import Camera  # noqa: E402
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig  # noqa: E402
from raymarch_algo_compare_amd.runner import GPURunner  # noqa: E402

BAND_K = 2


def numpy_reports(methods, reference):
    """what one rm_score_captures call replaces: both tiers and the residual of every method, the band made once"""
    band = scoring.silhouette_band(reference["hit"], BAND_K)
    return [(scoring.score_capture(m, reference), scoring.residual(m["hit"], m["depth"], reference["hit"], reference["depth"], band))
            for m in methods]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--scene", default="Sphere")
    ap.add_argument("--counts", default="1,11")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score", "cost.jsonl"))
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
    print("| scene | size | N | kernels ms | whole call ms | NumPy ms | Standard render ms | percentiles equal NumPy's |")
    print("|---|---|---|---|---|---|---|---|")
    with open(a.out, "a", encoding="utf-8") as f:
        for n in (int(v) for v in a.counts.split(",")):
            methods = [caps[1 + i % 7] for i in range(n)]
            out, tm = _native.score_captures(W, H, reference, methods, band_k=BAND_K, warmup=a.warmup, repeats=a.repeats)
            walls = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                _native.score_captures(W, H, reference, methods, band_k=BAND_K)
                walls.append((time.perf_counter() - t0) * 1e3)
            numpys = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                want = numpy_reports(methods, reference)
                numpys.append((time.perf_counter() - t0) * 1e3)
            same = all(np.array_equal([o["depth_p95"], o["depth_med"]], [w[0]["depth"]["p95"], w[1]["depth_med"]], equal_nan=True)
                       for o, w in zip(out, want))
            row = {"scene": scene.name, "width": W, "height": H, "n": n, "band_k": BAND_K, "repeats": a.repeats, "warmup": a.warmup,
                   "kernels_ms": tm["ms_median"], "kernels_ms_each": tm["ms_each"], "call_ms": float(np.median(walls)),
                   "call_ms_each": walls, "numpy_ms": float(np.median(numpys)), "numpy_ms_each": numpys,
                   "render_ms": render["timing"]["ms_median"], "render_ms_each": render["timing"]["ms_each"],
                   "percentiles_equal": bool(same)}
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(f"| {scene.name} | {W}x{H} | {n} | {row['kernels_ms']:.3f} | {row['call_ms']:.2f} | {row['numpy_ms']:.1f} | "
                  f"{row['render_ms']:.3f} | {'yes' if same else 'NO'} |", flush=True)


if __name__ == "__main__":
    main()
