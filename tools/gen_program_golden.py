#!/usr/bin/env python3
"""Generate the scene-program fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports /root/reference, which never travels to the GPU box); writes data only.
Every program is a seeded random expression tree in the JSON schema of raymarch_algo_compare_amd/scene_program.py,
and the reference evaluates it by calling its own scenes/primitives.py functions node by node (an SDFScene whose
sdf() walks the tree), so no reference code is restated here.

  programs_trees.json   {"trees": [<expression>, ...], "frame_trees": [tree index, ...], "W": .., "H": ..}
  programs_sdf.npz      npoints   int64 (1,)     N, the points of every tree (tools/program_fixture_points.py makes
                                                 them: the file holds results only)
                        t{i}_sha  uint8 (32,)    sha256 of sdf(p) over all N points (little-endian binary64)
                        t{i}_bits uint64 (K,)    the bits of sdf(p) at the first K = 250 points (a mismatch is
                                                 located here; the hash pins the rest)
                        t{i}_pts_sha uint8 (32,) sha256 of the points themselves (the generator has not drifted)
  programs_frames.npz   frames of the trees named by frame_trees at W x H for the 11 registry strategies, wired as
                        run_once does (fresh RenderConfig, Lipschitz bound 1.0), keys "s{tree}_k{strategy}_" in the
                        layout of frames_*.npz (oracle/gen_golden.py)

Usage:  python tools/gen_program_golden.py [--trees 40] [--points 2000] [--frames 10] [--jobs 8]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import random
import sys
import time
from multiprocessing import Pool

import numpy as np

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from raymarching_benchmark.config import MarchConfig, RenderConfig  # noqa: E402
from raymarching_benchmark.core.camera import Camera  # noqa: E402
from raymarching_benchmark.core.vec3 import Vec3  # noqa: E402
from raymarching_benchmark.scenes import primitives as P  # noqa: E402
from raymarching_benchmark.scenes.base import SDFScene  # noqa: E402
from raymarching_benchmark.strategies import STRATEGIES  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from program_fixture_points import fixture_points, sha256_f64  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
STRAT_KEYS = list(STRATEGIES.keys())


# ---- the reference's functions applied to a tree ----------------------------------------------------------------------

def v(t):
    return Vec3(*t)


def evaluate(n, p):
    op = n["op"]
    if op == "sd_sphere":
        return P.sd_sphere(p, n["radius"])
    if op == "sd_box":
        return P.sd_box(p, v(n["half_extents"]))
    if op == "sd_plane":
        return P.sd_plane(p, v(n["normal"]), n["offset"])
    if op == "sd_cylinder":
        return P.sd_cylinder(p, n["radius"], n["half_height"])
    if op == "sd_torus":
        return P.sd_torus(p, n["major_radius"], n["minor_radius"])
    if op == "sd_capsule":
        return P.sd_capsule(p, v(n["a"]), v(n["b"]), n["radius"])
    if op == "sd_capped_torus":
        return P.sd_capped_torus(p, tuple(n["sc"]), n["ra"], n["rb"])
    if op == "sd_cone":
        return P.sd_cone(p, n["angle_rad"], n["height"])
    if op in ("op_union", "op_subtract", "op_intersect"):
        return getattr(P, op)(evaluate(n["a"], p), evaluate(n["b"], p))
    if op in ("op_smooth_union", "op_smooth_subtract", "op_smooth_intersect"):
        return getattr(P, op)(evaluate(n["a"], p), evaluate(n["b"], p), n["k"])
    if op == "op_translate":
        return evaluate(n["child"], P.op_translate(p, v(n["offset"])))
    if op == "op_repeat":
        return evaluate(n["child"], P.op_repeat(p, v(n["spacing"])))
    if op == "op_round":
        return P.op_round(evaluate(n["child"], p), n["radius"])
    if op == "op_onion":
        return P.op_onion(evaluate(n["child"], p), n["thickness"])
    raise ValueError(op)


class TreeScene(SDFScene):
    def __init__(self, tree, name):
        self.tree, self._name = tree, name

    @property
    def name(self):
        return self._name

    @property
    def description(self):
        return "scene program fixture"

    def sdf(self, p):
        return evaluate(self.tree, p)


# ---- random trees -------------------------------------------------------------------------------------------------------

PRIMS = ["sd_sphere", "sd_box", "sd_plane", "sd_cylinder", "sd_torus", "sd_capsule", "sd_capped_torus", "sd_cone"]
BINARY = ["op_union", "op_subtract", "op_intersect", "op_smooth_union", "op_smooth_subtract", "op_smooth_intersect"]
OTHERS = BINARY + ["op_round", "op_onion", "op_translate", "op_repeat"]
SPACINGS = [0.0, 0.3, 1.7, 2.0, 0.5, 1.0, 0.75, 1.3]


def rnd(r, lo, hi):
    return round(r.uniform(lo, hi), 4)


def vec(r, lo, hi):
    return [rnd(r, lo, hi) for _ in range(3)]


def prim(r, op):
    if op == "sd_sphere":
        return {"op": op, "radius": rnd(r, 0.2, 1.5)}
    if op == "sd_box":
        return {"op": op, "half_extents": vec(r, 0.1, 1.2)}
    if op == "sd_plane":
        nrm = r.choice([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.8, 0.0], [0.0, -0.6, 0.8]])
        return {"op": op, "normal": nrm, "offset": rnd(r, -1.5, 0.5)}
    if op == "sd_cylinder":
        return {"op": op, "radius": rnd(r, 0.1, 1.0), "half_height": rnd(r, 0.2, 1.5)}
    if op == "sd_torus":
        return {"op": op, "major_radius": rnd(r, 0.5, 1.5), "minor_radius": rnd(r, 0.05, 0.4)}
    if op == "sd_capsule":
        return {"op": op, "a": vec(r, -1.0, 1.0), "b": vec(r, -1.0, 1.0), "radius": rnd(r, 0.1, 0.5)}
    if op == "sd_capped_torus":
        h = rnd(r, 0.3, 2.8)
        return {"op": op, "sc": [math.sin(h), math.cos(h)], "ra": rnd(r, 0.6, 1.4), "rb": rnd(r, 0.05, 0.3)}
    return {"op": "sd_cone", "angle_rad": rnd(r, 0.2, 1.2), "height": rnd(r, 0.5, 2.0)}


def tree(r, depth, points, need):
    """A random tree of at most `depth` levels, `points` nested transforms allowed; `need` = ops still to cover."""
    if depth <= 1:
        want = [o for o in PRIMS if o in need]          # list order: set order would follow the string hash seed
        op = want[0] if want and r.random() < 0.7 else r.choice(PRIMS)
        need.discard(op)
        return prim(r, op)
    want = [o for o in OTHERS if o in need and (points > 0 or o not in ("op_translate", "op_repeat"))]
    kinds = BINARY + ["op_round", "op_onion"] + (["op_translate", "op_repeat"] if points > 0 else []) + ["prim"]
    op = want[0] if want and r.random() < 0.6 else r.choice(kinds)
    if op == "prim":
        return tree(r, 1, points, need)
    need.discard(op)
    if op in BINARY:
        n = {"op": op, "a": tree(r, depth - 1, points, need), "b": tree(r, depth - 1, points, need)}
        if op.startswith("op_smooth"):
            n["k"] = r.choice([0.1, 0.25, 0.3, 0.5])
        return n
    if op in ("op_round", "op_onion"):
        key = "radius" if op == "op_round" else "thickness"
        return {"op": op, "child": tree(r, depth - 1, points, need), key: rnd(r, 0.01, 0.2)}
    if op == "op_translate":
        return {"op": op, "offset": vec(r, -1.5, 1.5), "child": tree(r, depth - 1, points - 1, need)}
    sp = [r.choice(SPACINGS) for _ in range(3)]
    if not any(sp):
        sp[1] = 1.7
    return {"op": "op_repeat", "spacing": sp, "child": tree(r, depth - 1, points - 1, need)}


def gen_trees(n, frames, seed=20261015):
    r = random.Random(seed)
    trees = []
    for i in range(n):
        need = set(PRIMS + BINARY + ["op_round", "op_onion", "op_translate", "op_repeat"])
        # the frame trees are shallower: the reference marches them in pure Python
        trees.append(tree(r, 4 if i < frames else r.randint(3, 6), 4, need))
    return trees


# ---- fixtures ---------------------------------------------------------------------------------------------------------------

KEEP_BITS = 250


def sdf_case(args):
    i, t, npts = args
    xyz = fixture_points(i, npts)
    out = np.array([evaluate(t, Vec3(float(a), float(b), float(c))) for a, b, c in xyz], dtype="<f8")
    return i, sha256_f64(xyz), sha256_f64(out), out[:KEEP_BITS].view(np.uint64).copy()


def frame_case(args):
    i, t, kid, W, H = args
    scene = TreeScene(t, f"tree{i}")
    strategy = STRATEGIES[STRAT_KEYS[kid]]()
    render = RenderConfig(width=W, height=H)
    lip = 1.0
    if hasattr(strategy, "lipschitz"):
        strategy.lipschitz = scene.known_lipschitz_bound()
        lip = float(strategy.lipschitz)
    cam = Camera(position=Vec3(*render.camera_position), target=Vec3(*render.camera_target), up=Vec3(*render.camera_up),
                 fov_degrees=render.fov_degrees, width=W, height=H)
    mc = MarchConfig()
    res = [strategy.march(cam.get_ray(px, py), scene.sdf, mc) for py in range(H) for px in range(W)]
    iters = np.array([x.iterations for x in res], dtype=np.int32).reshape(H, W)
    hit = np.array([bool(x.hit) for x in res], dtype=bool)
    tt = np.array([float(x.t) for x in res], dtype="<f8")
    fs = np.array([float(x.final_sdf) for x in res], dtype="<f8")
    pre = f"s{i}_k{kid}_"
    cam14 = np.array([*cam.position.to_tuple(), *cam.forward.to_tuple(), *cam.right.to_tuple(), *cam.up.to_tuple(),
                      cam.half_width, cam.half_height], dtype=np.float64)
    return {pre + "iters": iters.astype(np.int16), pre + "hitbits": np.packbits(hit), pre + "t_hit": tt[hit],
            pre + "sha_t": np.frombuffer(hashlib.sha256(tt.tobytes()).digest(), dtype=np.uint8),
            pre + "sha_fs": np.frombuffer(hashlib.sha256(fs.tobytes()).digest(), dtype=np.uint8),
            pre + "cam": cam14,
            pre + "meta": np.array([W, H, 0, H, mc.max_iterations, mc.hit_threshold, mc.max_distance, lip], dtype=np.float64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=40)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--height", type=int, default=24)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    trees = gen_trees(a.trees, a.frames)
    frame_trees = list(range(a.frames))
    with open(os.path.join(OUT, "programs_trees.json"), "w", encoding="utf-8") as f:
        json.dump({"trees": trees, "frame_trees": frame_trees, "W": a.width, "H": a.height}, f)
    t0 = time.time()
    with Pool(a.jobs) as pool:
        store = {"npoints": np.array([a.points], dtype=np.int64)}
        for i, psha, sha, bits in pool.imap_unordered(sdf_case, [(i, t, a.points) for i, t in enumerate(trees)]):
            store[f"t{i}_pts_sha"] = np.frombuffer(psha, dtype=np.uint8)
            store[f"t{i}_sha"] = np.frombuffer(sha, dtype=np.uint8)
            store[f"t{i}_bits"] = bits
        np.savez_compressed(os.path.join(OUT, "programs_sdf.npz"), **dict(sorted(store.items())))
        print(f"sdf fixtures: {len(trees)} trees x {a.points} points ({time.time() - t0:.0f}s)", flush=True)
        store = {}
        jobs = [(i, trees[i], k, a.width, a.height) for i in frame_trees for k in range(len(STRAT_KEYS))]
        for rec in pool.imap_unordered(frame_case, jobs):
            store.update(rec)
        np.savez_compressed(os.path.join(OUT, "programs_frames.npz"), **dict(sorted(store.items())))
        print(f"frame fixtures: {len(jobs)} frames ({time.time() - t0:.0f}s)", flush=True)


if __name__ == "__main__":
    main()
