#!/usr/bin/env python3
"""Generate tests/golden/features_intrinsic.npz by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports the reference, as tools/gen_interval_golden.py does); writes data only.  The
reference's own report/features.py _intrinsic_features(scene, corners, default_rng(seed)) is called with the 8 corners of
a box as its hit points, so no reference code is restated here.  (report/features.py imports the GLSL runner, which needs
moderngl; an empty stand-in module is enough.)  The same seed is then replayed through this package's sample_sets and
intrinsic_features_numpy over the reference's own point evaluation (_sdf_at) to record the samples and the intermediate
values; nothing is written unless the replay reproduces the reference's two outputs bit for bit.

Per case c, key prefix "c{c}_":
    meta        int64 (5,)     scene id, seed, n_lip, n_chords, chord_steps
    box         float64 (2, 3) the corners' lo and hi (the unpadded box)
    pts         float64 (n_lip, 3), chords (n_chords, 6: a, b), seglen (n_chords,), ts (chord_steps,), diag (1,)
    gmag        uint64 (n_lip,)     bits of |grad f| per point
    slab_counts int32 (n_chords,)   solid runs per chord
    want        uint64 (2,)    bits of the reference's lipschitz_p99 and thin_slab
"ncases" holds their number, "names" the scene names.

Cases: all 20 scenes in the box +-1.5 with the reference's sample counts lowered (through its module attributes) to 300
points and 48 chords; Sphere, Thin Torus and Mandelbulb at its full counts; a second box +-0.4 for Onion Shell and Thin
Planes Stack.  A case whose chords all miss the solid (the reference answers NaN) takes its seed + 1000, + 2000, ...: a
fixture case must hold a slab.  The one exception is Onion Shell in +-0.4, which holds no solid at all (its shells lie at
radius 1.85 .. 2.15): the reference answers NaN for thin_slab there, and the case pins the empty sample.

Usage:  python tools/gen_features_golden.py
"""
from __future__ import annotations

import itertools
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.modules.setdefault("moderngl", types.ModuleType("moderngl"))

import gen_interval_golden as G  # noqa: E402  (puts the reference on sys.path)

from raymarching_benchmark.report import features as F  # noqa: E402
from raymarching_benchmark.scenes.catalog import get_all_scenes  # noqa: E402

from raymarch_algo_compare_amd import features, registry  # noqa: E402

OUT = G.OUT
SMALL = (300, 48)
FULL = (F._LIP_SAMPLES, F._CHORDS)
MAX_SEED_TRIES = 40      # a thin scene's 48 chords can all miss it: the case's seed then moves on by 1000
bits = G.bits


def cases():
    scenes = get_all_scenes()
    assert [s.name for s in scenes] == [s.name for s in registry.get_all_scenes()]
    by_name = {s.name: i for i, s in enumerate(scenes)}
    for i in range(len(scenes)):
        yield i, 1.5, 100 + i, SMALL, True
    for name in ("Sphere", "Thin Torus", "Mandelbulb"):
        yield by_name[name], 1.5, 200 + by_name[name], FULL, True
    for name in ("Onion Shell", "Thin Planes Stack"):
        yield by_name[name], 0.4, 300 + by_name[name], SMALL, name != "Onion Shell"      # its shells lie at radius 1.85 .. 2.15


def main():
    scenes = get_all_scenes()
    assert (features._LIP_SAMPLES, features._CHORDS, features._CHORD_STEPS, features._LIP_EPS, features.GRAZING_COS) == \
        (F._LIP_SAMPLES, F._CHORDS, F._CHORD_STEPS, F._LIP_EPS, F.GRAZING_COS)
    z = {}
    names = []
    for c, (sid, half, seed, (n_lip, n_chords), solid) in enumerate(cases()):
        scene = scenes[sid]
        F._LIP_SAMPLES, F._CHORDS = n_lip, n_chords
        corners = np.array(list(itertools.product((-half, half), repeat=3)), np.float64)
        lo, hi, diag = features.padded_box(corners.min(axis=0), corners.max(axis=0))
        for seed in range(seed, seed + 1000 * MAX_SEED_TRIES, 1000):
            want = F._intrinsic_features(scene, corners, np.random.default_rng(seed))
            if not solid or want["thin_slab"] == want["thin_slab"]:      # some chord met the solid
                break
        s = features.sample_sets(lo, hi, np.random.default_rng(seed), n_lip, n_chords, F._CHORD_STEPS)
        got = features.intrinsic_features_numpy(sid, [s], F._LIP_EPS, sdf=lambda p: F._sdf_at(scene, p))[0]
        thin = float(np.float64(got["slab_median"]) / diag)
        assert bits(got["lipschitz_p99"]) == bits(want["lipschitz_p99"]), (scene.name, got["lipschitz_p99"], want["lipschitz_p99"])
        assert bits(thin) == bits(want["thin_slab"]), (scene.name, thin, want["thin_slab"])
        assert got["n_finite"] == n_lip, (scene.name, got["n_finite"])
        assert (got["n_slabs"] > 0) == solid, scene.name
        p = f"c{c}_"
        z[p + "meta"] = np.array([sid, seed, n_lip, n_chords, F._CHORD_STEPS], np.int64)
        z[p + "box"] = np.stack([corners.min(axis=0), corners.max(axis=0)])
        z[p + "pts"], z[p + "chords"], z[p + "seglen"], z[p + "ts"] = s["pts"], s["chords"], s["seglen"], s["ts"]
        z[p + "diag"] = np.array([diag])
        z[p + "gmag"] = bits(got["gmag"])
        z[p + "slab_counts"] = got["slab_counts"].astype(np.int32)
        z[p + "want"] = np.array([bits(want["lipschitz_p99"]), bits(want["thin_slab"])], np.uint64).reshape(2)
        names.append(scene.name)
        print(f"case {c}: {scene.name} +-{half} n_lip {n_lip} chords {n_chords}: p99 {want['lipschitz_p99']!r} thin {want['thin_slab']!r} "
              f"slabs {got['n_slabs']}")
    z["ncases"] = np.array([len(names)], np.int64)
    z["names"] = np.array(names)
    path = os.path.join(OUT, "features_intrinsic.npz")
    np.savez_compressed(path, **z)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
