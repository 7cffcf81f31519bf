#!/usr/bin/env python3
"""Generate the interval-oracle fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports /root/reference, which never travels to the GPU box); writes data only.  The
reference's own gpu/interval_oracle.py first_hit, _prune_candidates and _normals_fd and gpu/interval.py's
INTERVAL_SCENES (Sphere, Grazing Plane, Cube, Thin Torus) are applied to the rays of its CPU camera (core.camera.Camera,
core.ray.Ray -- the camera csrc/rm_camera.h reproduces), so no reference code is restated here.

  interval_frames.npz   per scene s (catalogue id) and case c ("default", "test", "patched"), key prefix "s{s}_{c}_":
                        cam    float64 (14,)  position, forward, right, up, half_width, half_height (RmFrameDesc.cam)
                        cfg    float64 (8,)   t_max, tol, h0, growth, h_max, normal_eps, bound_radius, max_steps
                                              (RmIntervalConfig; bound_radius < 0: no prune)
                        hit    uint8 packbits of the W x H hit map (row 0 = top)
                        t      uint64         bits of depth at the hit pixels, in pixel order
                        n_sha  uint8 (32,)    sha256 of the normal bits of every hit pixel (3 doubles each, pixel order)
                        n_bits uint64         the normal bits of the first 256 hit pixels
                        W, H in "shape".
  interval_rays.npz     explicit rays, per set k in ("rand", "unit", "unnorm") and scene s, prefix "{k}_s{s}_":
                        o, d   float64 (M, 3) origins and directions (directions as given: first_hit does not normalise)
                        cfg    as above
                        t      uint64 (M,)    bits of first_hit (+inf: a miss)
                        n      uint64 (M, 3)  bits of _normals_fd at o + t * d (0 for a miss)

Cases of the frames: "default" the reference's constants; "test" tol = 1e-6, t_max = 10 (its tests' settings);
"patched" _MAX_ITERS = 40, _H0 = 0.5, _GROWTH = 2.0, _HMAX = 4.0, _normals_fd eps = 2e-4 and no prune (monkeypatched
module globals), so that every field of RmIntervalConfig is pinned.

Usage:  python tools/gen_interval_golden.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from raymarching_benchmark.core.camera import Camera  # noqa: E402
from raymarching_benchmark.core.vec3 import Vec3  # noqa: E402
from raymarching_benchmark.gpu import interval_oracle as IO  # noqa: E402
from raymarching_benchmark.gpu.interval import INTERVAL_SCENES  # noqa: E402
from raymarching_benchmark.scenes.catalog import get_scene_by_name  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SCENES = {0: "Sphere", 1: "Grazing Plane", 2: "Cube", 3: "Thin Torus"}
W, H = 96, 72
DEFAULTS = dict(t_max=100.0, tol=1e-5, h0=0.25, growth=1.5, h_max=10.0, eps=1e-4, max_steps=20000)
CASES = {
    "default": dict(DEFAULTS),
    "test": dict(DEFAULTS, t_max=10.0, tol=1e-6),
    "patched": dict(DEFAULTS, max_steps=40, h0=0.5, growth=2.0, h_max=4.0, eps=2e-4, no_prune=True),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def patch(c):
    IO._MAX_ITERS, IO._H0, IO._GROWTH, IO._HMAX = c["max_steps"], c["h0"], c["growth"], c["h_max"]


def cfg_array(c, bound):
    return np.array([c["t_max"], c["tol"], c["h0"], c["growth"], c["h_max"], c["eps"], bound, c["max_steps"]], np.float64)


def camera(name):
    rc = get_scene_by_name(name).suggested_camera()      # main.py:50-53: the scene's camera, else RenderConfig's
    pos = rc.camera_position if rc else (0.0, 0.0, 5.0)
    tgt = rc.camera_target if rc else (0.0, 0.0, 0.0)
    up, fov = (rc.camera_up, rc.fov_degrees) if rc else ((0.0, 1.0, 0.0), 60.0)
    cam = Camera(Vec3(*pos), Vec3(*tgt), Vec3(*up), fov, W, H)
    v = lambda q: [q.x, q.y, q.z]      # noqa: E731
    cam14 = np.array(v(cam.position) + v(cam.forward) + v(cam.right) + v(cam.up) + [cam.half_width, cam.half_height])
    rd = np.empty((H * W, 3))
    for py in range(H):
        for px in range(W):
            r = cam.get_ray(px, py)
            rd[py * W + px] = v(r.direction)
    return np.array(v(cam.position)), rd, cam14


def frame(name, c):
    """interval_capture's body on the CPU camera's rays"""
    patch(c)
    ro, rd, cam14 = camera(name)
    bound = None if c.get("no_prune") else IO.SCENE_BOUND.get(name)
    cand = IO._prune_candidates(ro, rd, bound)
    t_cand = IO.first_hit(ro, rd[cand], INTERVAL_SCENES[name], c["t_max"], c["tol"])
    depth = np.zeros(H * W)
    hit = np.zeros(H * W, dtype=bool)
    idx = np.nonzero(cand)[0]
    got = np.isfinite(t_cand)
    hg = idx[got]
    depth[hg] = t_cand[got]
    hit[hg] = True
    P = ro[None, :] + depth[hg][:, None] * rd[hg]
    normal = IO._normals_fd(name, P, eps=c["eps"])
    return cam14, -1.0 if bound is None else 0.0, hit, depth[hg], normal


def rays(name, o, d, c):
    patch(c)
    t = np.empty(len(o))
    for i in range(len(o)):
        t[i] = IO.first_hit(o[i], d[i][None, :], INTERVAL_SCENES[name], c["t_max"], c["tol"])[0]
    n = np.zeros((len(o), 3))
    ok = np.isfinite(t)
    for i in np.nonzero(ok)[0]:
        n[i] = IO._normals_fd(name, (o[i] + t[i] * d[i])[None, :], eps=c["eps"])[0]
    return t, n


def ray_sets(rng):
    """(set name, o, d, case) per scene"""
    out = {}
    for sid in SCENES:
        # 512 random pairs: 16 origins on a shell around the object, 32 directions each aimed near the origin
        o = np.repeat(rng.normal(size=(16, 3)), 32, axis=0)
        o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(2.5, 6.0, size=(len(o), 1))
        d = -o + rng.normal(scale=1.2, size=o.shape)
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        out[("rand", sid)] = (o, d, CASES["default"])
        # a few unnormalised directions (first_hit uses them as given)
        o2 = np.array([[0.3, 0.8, 4.0], [2.5, 0.2, -3.0], [-4.0, 1.5, 0.5], [0.0, 3.0, 0.2], [1.4, 2.0, 0.1], [-2.0, -2.0, 2.0]])
        d2 = -o2 * np.array([[0.21], [0.5], [1.7], [3.0], [0.33], [2.5]]) + np.array([[0.02, -0.05, 0.0]])
        out[("unnorm", sid)] = (o2, d2, CASES["default"])
    # tests/test_interval.py: the straight-on sphere ray and the ray through the thin torus's tube
    out[("unit", 0)] = (np.array([[0.0, 0.0, 5.0]]), np.array([[0.0, 0.0, -1.0]]), CASES["test"])
    out[("unit", 3)] = (np.array([[1.5, 3.0, 0.0]]), np.array([[0.0, -1.0, 0.0]]), CASES["test"])
    return out


def main() -> None:
    fr = {"shape": np.array([W, H], np.int64)}
    for sid, name in SCENES.items():
        for cname, c in CASES.items():
            cam14, bound, hit, t, normal = frame(name, c)
            p = f"s{sid}_{cname}_"
            fr[p + "cam"] = cam14
            fr[p + "cfg"] = cfg_array(c, bound)
            fr[p + "hit"] = np.packbits(hit.astype(np.uint8))
            fr[p + "t"] = bits(t)
            fr[p + "n_sha"] = np.frombuffer(hashlib.sha256(bits(normal).tobytes()).digest(), np.uint8)
            fr[p + "n_bits"] = bits(normal[:256]).reshape(-1)
            print(f"{name:14s} {cname:8s} hits {int(hit.sum())}", flush=True)
    np.savez_compressed(os.path.join(OUT, "interval_frames.npz"), **fr)
    rs = {}
    for (k, sid), (o, d, c) in ray_sets(np.random.default_rng(20261016)).items():
        t, n = rays(SCENES[sid], o, d, c)
        p = f"{k}_s{sid}_"
        rs[p + "o"], rs[p + "d"], rs[p + "cfg"] = o, d, cfg_array(c, -1.0)
        rs[p + "t"], rs[p + "n"] = bits(t), bits(n)
        print(f"{k:7s} {SCENES[sid]:14s} rays {len(o)} hits {int(np.isfinite(t).sum())}", flush=True)
    np.savez_compressed(os.path.join(OUT, "interval_rays.npz"), **rs)
    for f in ("interval_frames.npz", "interval_rays.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
