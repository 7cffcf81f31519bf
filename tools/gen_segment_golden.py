#!/usr/bin/env python3
"""Generate the segment-tracer fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports /root/reference, as tools/gen_interval_golden.py does); writes data only.  The
reference's own gpu/interval_autodiff.py seed_segment, gpu/interval.py COMPONENT_SCENES and gpu/faithful_offline.py
segment_trace / _prune_candidates are applied to the rays of its CPU camera, so no reference code is restated here.
(gpu/faithful_offline.py imports the GLSL runner, which needs moderngl; an empty stand-in module is enough.)

  segment_dsdf.npz      per scene s (catalogue ids 0-3), prefix "s{s}_":
                        segs   float64 (N, 8)  origin, direction, t0, t1 (widths 1e-6 .. 10, some t0 == t1)
                        out    uint64  (N, 4)  bits of val.lo, val.hi, der.lo, der.hi
  segment_frames.npz    per scene s and case c ("default", "patched"), prefix "s{s}_{c}_":
                        cam    float64 (14,)   RmFrameDesc.cam
                        cfg    float64 (10,)   t_max, tol, h0, kappa, h_min, h_max, k_min, l_global, bound_radius, budget
                                               (RmSegmentConfig; bound_radius < 0: no prune)
                        hit    uint8 packbits of the W x H hit map
                        t      uint64          bits of t at the hit pixels, in pixel order
                        iters  int32 (W * H)   trips of every candidate ray (0: pruned)
                        W, H in "shape".
  segment_rays.npz      the ray sets of interval_rays.npz ("rand", "unit", "unnorm"), prefix "{k}_s{s}_":
                        o, d   float64 (M, 3); cfg as above; t uint64 (M,) bits of t_hit; iters int32 (M,)

"default": the reference's constants.  "patched": every module global of the tracer monkeypatched and tol, l_global,
t_max passed, no prune, so that every field of RmSegmentConfig is pinned.

Usage:  python tools/gen_segment_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.modules.setdefault("moderngl", types.ModuleType("moderngl"))

import gen_interval_golden as G  # noqa: E402  (puts the reference on sys.path; camera(), ray_sets(), SCENES)

from raymarching_benchmark.gpu import faithful_offline as FO  # noqa: E402
from raymarching_benchmark.gpu.interval import COMPONENT_SCENES  # noqa: E402
from raymarching_benchmark.gpu.interval_autodiff import seed_segment  # noqa: E402
from raymarching_benchmark.gpu.interval_oracle import SCENE_BOUND, _prune_candidates  # noqa: E402

OUT = G.OUT
SCENES = G.SCENES
W, H = G.W, G.H
DEFAULTS = dict(t_max=100.0, tol=1e-4, h0=0.1, kappa=1.5, h_min=1e-5, h_max=10.0, k_min=1e-6, l_global=1.0, budget=4096)
CASES = {
    "default": dict(DEFAULTS),
    "patched": dict(t_max=6.0, tol=1e-3, h0=0.05, kappa=2.0, h_min=1e-4, h_max=2.0, k_min=1e-3, l_global=0.75, budget=12,
                    no_prune=True),
}
N_SEGS = 2000
bits = G.bits


def patch(c):
    FO._H0, FO._KAPPA, FO._HMIN, FO._HMAX, FO._KMIN, FO._BUDGET = c["h0"], c["kappa"], c["h_min"], c["h_max"], c["k_min"], c["budget"]


def cfg_array(c, bound):
    return np.array([c["t_max"], c["tol"], c["h0"], c["kappa"], c["h_min"], c["h_max"], c["k_min"], c["l_global"], bound,
                     c["budget"]], np.float64)


def trace(name, ro, rd, c):
    patch(c)
    return FO.segment_trace(ro, rd, name, t_max=c["t_max"], tol=c["tol"], l_global=c["l_global"])


def dsdf(name, rng):
    o = np.repeat(rng.normal(size=(N_SEGS // 50, 3)), 50, axis=0)
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 5.0, size=(len(o), 1))
    d = -o + rng.normal(scale=1.0, size=o.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d[::7] *= rng.uniform(0.2, 3.0, size=(len(d[::7]), 1))            # some unnormalised directions
    t0 = rng.uniform(0.0, 8.0, size=len(o))
    t1 = t0 + 10.0 ** rng.uniform(-6.0, 1.0, size=len(o))
    t1[::10] = t0[::10]                                               # degenerate segments
    X, Y, Z = seed_segment(o.T, d, t0, t1)
    r = COMPONENT_SCENES[name](X, Y, Z)
    out = np.stack([np.broadcast_to(a, t0.shape) for a in (r.val.lo, r.val.hi, r.der.lo, r.der.hi)], axis=1)
    return np.concatenate([o, d, t0[:, None], t1[:, None]], axis=1), out


def frame(name, c):
    ro, rd, cam14 = G.camera(name)
    bound = None if c.get("no_prune") else SCENE_BOUND.get(name)
    cand = _prune_candidates(ro, rd, bound)
    t, it = trace(name, ro, rd[cand], c)
    idx = np.nonzero(cand)[0]
    got = np.isfinite(t)
    hit = np.zeros(H * W, dtype=bool)
    hit[idx[got]] = True
    iters = np.zeros(H * W, np.int32)
    iters[idx] = it
    return cam14, -1.0 if bound is None else 0.0, hit, t[got], iters


def main() -> None:
    rng = np.random.default_rng(20261017)
    ds = {}
    for sid, name in SCENES.items():
        segs, out = dsdf(name, rng)
        assert np.isfinite(out).all(), name
        ds[f"s{sid}_segs"], ds[f"s{sid}_out"] = segs, bits(out)
        print(f"{name:14s} segments {len(segs)}  K max {np.abs(out[:, 2:]).max():.3g}", flush=True)
    np.savez_compressed(os.path.join(OUT, "segment_dsdf.npz"), **ds)

    fr = {"shape": np.array([W, H], np.int64)}
    for sid, name in SCENES.items():
        for cname, c in CASES.items():
            cam14, bound, hit, t, iters = frame(name, c)
            p = f"s{sid}_{cname}_"
            fr[p + "cam"], fr[p + "cfg"] = cam14, cfg_array(c, bound)
            fr[p + "hit"], fr[p + "t"], fr[p + "iters"] = np.packbits(hit.astype(np.uint8)), bits(t), iters
            cand = iters > 0
            print(f"{name:14s} {cname:8s} hits {int(hit.sum())}  iters median {np.median(iters[hit]) if hit.any() else 0:.0f} "
                  f"max {int(iters.max())}  budget used up {int((cand & ~hit & (iters == c['budget'])).sum())}", flush=True)
    np.savez_compressed(os.path.join(OUT, "segment_frames.npz"), **fr)

    rs = {}
    for (k, sid), (o, d, ic) in G.ray_sets(np.random.default_rng(20261016)).items():
        c = dict(DEFAULTS, t_max=ic["t_max"], tol=10.0 * ic["tol"])      # the interval cases' horizon, this tracer's scale of tol
        t, it = np.empty(len(o)), np.empty(len(o), np.int32)
        for i in range(len(o)):
            ti, ii = trace(SCENES[sid], o[i], d[i][None, :], c)
            t[i], it[i] = ti[0], ii[0]
        p = f"{k}_s{sid}_"
        rs[p + "o"], rs[p + "d"], rs[p + "cfg"] = o, d, cfg_array(c, -1.0)
        rs[p + "t"], rs[p + "iters"] = bits(t), it
        print(f"{k:7s} {SCENES[sid]:14s} rays {len(o)} hits {int(np.isfinite(t).sum())} iters max {int(it.max())}", flush=True)
    np.savez_compressed(os.path.join(OUT, "segment_rays.npz"), **rs)
    for f in ("segment_dsdf.npz", "segment_frames.npz", "segment_rays.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
