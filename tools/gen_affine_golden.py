#!/usr/bin/env python3
"""Generate the affine-range fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports the reference, as tools/gen_interval_golden.py does); writes data only.  The
reference's own gpu/affine.py _aff_positions, _affine_range and march_count, gpu/interval.py COMPONENT_SCENES and
gpu/interval_oracle.py _prune_candidates are applied to the rays of its CPU camera, so no reference code is restated
here.  (gpu/affine.py's import chain reaches the GLSL runner, which needs moderngl; an empty stand-in module is enough.)

  affine_forms.npz     per scene s (catalogue ids 0-3), prefix "s{s}_":
                       segs   float64 (N, 8)  origin, direction, t0, t1 (widths 1e-6 .. 10, every tenth t0 == t1, some
                                              unnormalised directions)
                       out    uint64  (N, 5)  bits of x0, x1, e, lo, hi
  affine_frames.npz    per scene s and case c ("default", "patched"), prefix "s{s}_{c}_":
                       cam    float64 (14,)   RmFrameDesc.cam
                       cfg    float64 (8,)    t_max, tol, h0, growth, h_max, normal_eps, bound_radius, max_steps
                                              (RmIntervalConfig; bound_radius < 0: no prune)
                       hit    uint8 packbits of the W x H hit map
                       t      uint64          bits of t at the hit pixels, in pixel order
                       steps  int32 (W * H)   range evaluations of every candidate ray (0: pruned); their sum is the
                                              reference's eval count
                       score  float64 (2,)    the reference's residual of the affine capture against its interval
                                              capture of the same rays and constants: iou, core_iou (silhouette band k = 2)
                       W, H in "shape".
  affine_rays.npz      the ray sets of interval_rays.npz ("rand", "unit", "unnorm"), marched one ray at a time, prefix
                       "{k}_s{s}_": o, d float64 (M, 3); cfg as above; t uint64 (M,) bits of t_hit; steps int32 (M,)

"default": the reference's constants.  "patched": every march constant monkeypatched to a non-default value, t_max and tol
passed, no prune, so that every field of RmIntervalConfig the march reads is pinned.

march_count returns only the total of the evaluations.  The per-ray counts come out of the reference's own loop: the
directions travel with a fourth column holding the ray's index, and the range function handed to march_count strips
that column and counts the rays it is asked about.

Two properties are asserted, with their counts printed: every output is finite, and the reference's affine range
encloses its pointwise SDF (_scalar_sdf) at 33 samples of each segment within 1e-12 * (1 + |f|).

Usage:  python tools/gen_affine_golden.py
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

from raymarching_benchmark.gpu import affine as AF  # noqa: E402
from raymarching_benchmark.gpu import interval_oracle as IO  # noqa: E402
from raymarching_benchmark.gpu.interval import COMPONENT_SCENES  # noqa: E402
from raymarching_benchmark.gpu.oracle_calibration import residual, silhouette_band  # noqa: E402

OUT = G.OUT
SCENES = G.SCENES
W, H = G.W, G.H
bits = G.bits
CASES = {
    "default": dict(G.DEFAULTS),
    "patched": dict(G.DEFAULTS, t_max=8.0, tol=1e-3, h0=0.5, growth=2.0, h_max=4.0, max_steps=40, no_prune=True),
}
N_SEGS = 2000
N_SAMPLES = 33


def patch(c):
    G.patch(c)                                                         # the interval oracle's globals (the gold capture)
    AF._MAX_ITERS, AF._H0, AF._GROWTH, AF._HMAX = c["max_steps"], c["h0"], c["growth"], c["h_max"]   # gpu/affine.py's copies


def march(name, ro, rd, c):
    """march_count over the rays rd (M, 3) from ro: (t_hit, per-ray evaluations)"""
    patch(c)
    steps = np.zeros(len(rd), np.int64)

    def range_fn(o, d4, t0, t1):
        np.add.at(steps, d4[:, 3].astype(np.int64), 1)
        return AF._affine_range(name, o, np.ascontiguousarray(d4[:, :3]), t0, t1)

    d4 = np.concatenate([rd, np.arange(len(rd), dtype=np.float64)[:, None]], axis=1)
    t, total = AF.march_count(ro, d4, range_fn, t_max=c["t_max"], tol=c["tol"])
    assert total == int(steps.sum())
    return t, steps.astype(np.int32)


def forms(name, rng):
    """segments drawn as gen_segment_golden.dsdf draws them"""
    o = np.repeat(rng.normal(size=(N_SEGS // 50, 3)), 50, axis=0)
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 5.0, size=(len(o), 1))
    d = -o + rng.normal(scale=1.0, size=o.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d[::7] *= rng.uniform(0.2, 3.0, size=(len(d[::7]), 1))            # some unnormalised directions
    t0 = rng.uniform(0.0, 8.0, size=len(o))
    t1 = t0 + 10.0 ** rng.uniform(-6.0, 1.0, size=len(o))
    t1[::10] = t0[::10]                                               # degenerate segments
    f = COMPONENT_SCENES[name](*AF._aff_positions(o.T, d, t0, t1))
    lo, hi = f.range()
    out = np.stack([np.broadcast_to(a, t0.shape) for a in (f.x0, f.x1, f.e, lo, hi)], axis=1)
    # inclusion: the pointwise SDF at 33 samples of each segment
    u = np.linspace(0.0, 1.0, N_SAMPLES)
    tau = t0[:, None] + u[None, :] * (t1 - t0)[:, None]
    tau[:, -1] = t1
    pts = o[:, None, :] + tau[..., None] * d[:, None, :]
    g = IO._scalar_sdf(name, pts.reshape(-1, 3)).reshape(tau.shape)
    slack = 1e-12 * (1.0 + np.abs(g))
    bad = (g < lo[:, None] - slack) | (g > hi[:, None] + slack)
    return np.concatenate([o, d, t0[:, None], t1[:, None]], axis=1), out, int(bad.any(axis=1).sum())


def frame(name, c):
    ro, rd, cam14 = G.camera(name)
    bound = None if c.get("no_prune") else IO.SCENE_BOUND.get(name)
    cand = IO._prune_candidates(ro, rd, bound)
    idx = np.nonzero(cand)[0]
    t, st = march(name, ro, rd[cand], c)
    got = np.isfinite(t)
    hit = np.zeros(H * W, dtype=bool)
    hit[idx[got]] = True
    depth = np.zeros(H * W)
    depth[idx[got]] = t[got]
    steps = np.zeros(H * W, np.int32)
    steps[idx] = st
    # the interval capture of the same rays and constants (interval_capture's body, gen_interval_golden.frame)
    _, _, ghit, gt, _ = G.frame(name, c)
    gdepth = np.zeros(H * W)
    gdepth[ghit] = gt
    ghit2, hit2 = ghit.reshape(H, W), hit.reshape(H, W)
    res = residual(hit2, depth.reshape(H, W), ghit2, gdepth.reshape(H, W), silhouette_band(ghit2, k=2))
    return cam14, -1.0 if bound is None else 0.0, hit, t[got], steps, np.array([res["iou"], res["core_iou"]], np.float64)


def main() -> None:
    rng = np.random.default_rng(20261017)
    fo = {}
    for sid, name in SCENES.items():
        segs, out, violations = forms(name, rng)
        finite = bool(np.isfinite(out).all())
        print(f"{name:14s} segments {len(segs)}  non-finite outputs {int((~np.isfinite(out)).sum())}  "
              f"inclusion violations {violations}", flush=True)
        assert finite, name
        assert violations == 0, (name, violations)
        fo[f"s{sid}_segs"], fo[f"s{sid}_out"] = segs, bits(out)
    np.savez_compressed(os.path.join(OUT, "affine_forms.npz"), **fo)

    fr = {"shape": np.array([W, H], np.int64)}
    for sid, name in SCENES.items():
        for cname, c in CASES.items():
            cam14, bound, hit, t, steps, score = frame(name, c)
            assert np.isfinite(t).all() and np.isfinite(score).all(), (name, cname)
            p = f"s{sid}_{cname}_"
            fr[p + "cam"], fr[p + "cfg"] = cam14, G.cfg_array(c, bound)
            fr[p + "hit"], fr[p + "t"], fr[p + "steps"], fr[p + "score"] = np.packbits(hit.astype(np.uint8)), bits(t), steps, score
            print(f"{name:14s} {cname:8s} hits {int(hit.sum())}  evals {int(steps.sum())}  max {int(steps.max())}  "
                  f"iou {score[0]:.6f} core {score[1]:.6f}", flush=True)
    np.savez_compressed(os.path.join(OUT, "affine_frames.npz"), **fr)

    rs = {}
    for (k, sid), (o, d, c) in G.ray_sets(np.random.default_rng(20261016)).items():
        t, st = np.empty(len(o)), np.empty(len(o), np.int32)
        for i in range(len(o)):
            ti, si = march(SCENES[sid], o[i], d[i][None, :], c)
            t[i], st[i] = ti[0], si[0]
        p = f"{k}_s{sid}_"
        rs[p + "o"], rs[p + "d"], rs[p + "cfg"] = o, d, G.cfg_array(c, -1.0)
        rs[p + "t"], rs[p + "steps"] = bits(t), st
        print(f"{k:7s} {SCENES[sid]:14s} rays {len(o)} hits {int(np.isfinite(t).sum())} steps max {int(st.max())}", flush=True)
    np.savez_compressed(os.path.join(OUT, "affine_rays.npz"), **rs)
    for f in ("affine_forms.npz", "affine_frames.npz", "affine_rays.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
