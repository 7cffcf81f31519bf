#!/usr/bin/env python3
"""Generate tests/golden/ssim_images.npz by RUNNING THE REFERENCE's data/capture_io.py (depth_to_image, normal_to_image,
color_to_image and, through them, _to_u8) on a few small random captures.  Writes data only; no reference code is
restated here.  The fixture pins the quantisation of csrc/rm_ssim.h and ssim.to_images bit for bit.

No SSIM VALUE comes from the reference: it takes them from skimage, which is not installed where this tool runs (nor used
by this project).  The SSIM arithmetic is checked against a float64 restatement with scipy.ndimage.uniform_filter
instead (tests/test_ssim_host.py); this fixture covers the one step that restatement cannot vouch for.

  ssim_images.npz   cases "c0" .. "c{n-1}" (n in "ncases"), prefix "c{k}_":
                    depth  float32 (H, W)     beyond the range on both sides, NaN-free (c0 .. c3)
                    normal float32 (H, W, 3)  unit-ish vectors; some components exactly +1 / -1 / 0
                    color  float32 (H, W, 3)  0, 1, the rounding edges k/255 -+ 1e-7, values outside [0, 1], some NaN / inf
                    hit    uint8   (H, W)     with misses
                    drange float64 (2,)       the depth range handed to depth_to_image (not this capture's own: a
                                              method's image uses its reference capture's range); c2: an all-miss
                                              capture with (0, 1); c3: a range below the 1e-6 floor
                    img_depth uint8 (H, W), img_normal, img_color uint8 (H, W, 3): the reference's images
                    c4 and later (appended, so the random stream leaves c0 .. c3 as they were) are the plain case with
                    what a degenerate normal or a broken frame puts into a capture, all 16 x 12 but c4:
                      c4  badnormal   40 x 33; NaN, +inf, -inf (one component or all three) and all-zero normals, on hits
                                      and on misses
                      c5  nan_late    depth NaN on the 6th hit (row-major), NaN / +-inf on misses
                      c6  nan_first   depth NaN on the first hit, NaN / +-inf on misses
                      c7  posinf      depth +inf on two hits, NaN / +-inf on misses
                      c8  neginf      depth -inf on two hits, NaN / +-inf on misses
                      c9  huge        depth +3.4e38 and -3.4e38 on hits (their difference overflows binary32)
                      c10 onehit      exactly one hit
                      c11 equaldepth  every hit at depth 4.25, the misses' depths random
                    and carry two more arrays:
                    own_drange    float64 (2,)  the reference's depth_range_of(capture): NaN on a hit gives (nan, nan)
                    img_depth_own uint8 (H, W)  depth_to_image with that range, the image a REFERENCE capture gets

Usage:  python tools/gen_ssim_golden.py <path of the reference checkout>
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capture_io(ref_root: str):
    path = os.path.join(ref_root, "raymarching_benchmark", "data", "capture_io.py")
    spec = importlib.util.spec_from_file_location("reference_capture_io", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(rng: np.random.Generator, W: int, H: int, kind: str) -> dict:
    f32 = np.float32
    hit = rng.random((H, W)) < 0.7
    depth = rng.uniform(1.0, 9.0, (H, W)).astype(f32)
    drange = (float(f32(2.5)), float(f32(7.25)))                    # depths fall below, inside and above it
    if kind == "allmiss":
        hit[:] = False
        drange = (0.0, 1.0)
    elif kind == "flat":
        depth = (f32(3.0) + rng.integers(0, 3, (H, W)).astype(f32) * f32(2.4e-7)).astype(f32)
        drange = (float(depth.min()), float(depth.min()) + 2.4e-7)   # below the floor of 1e-6
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    normal = n.astype(f32)
    axis = rng.integers(0, 3, (H, W))
    sign = rng.choice(np.array([-1.0, 1.0], f32), (H, W))
    pick = rng.random((H, W)) < 0.2                                  # exactly +-1 in one component, 0 in the others
    normal[pick] = 0.0
    normal[pick, axis[pick]] = sign[pick]
    k = rng.integers(0, 256, (H, W, 3)).astype(np.float64)
    edge = rng.choice(np.array([-1e-7, 0.0, 1e-7]), (H, W, 3))
    color = (k / 255.0 + edge).astype(f32)                           # the rounding edges of x * 255
    u = rng.random((H, W, 3))
    color[u < 0.05] = 0.0
    color[(u >= 0.05) & (u < 0.10)] = 1.0
    color[(u >= 0.10) & (u < 0.13)] = f32(-0.25)
    color[(u >= 0.13) & (u < 0.16)] = f32(1.5)
    color[(u >= 0.16) & (u < 0.17)] = np.nan
    color[(u >= 0.17) & (u < 0.18)] = np.inf
    color[(u >= 0.18) & (u < 0.19)] = -np.inf
    color[(u >= 0.19) & (u < 0.40)] = rng.random(int(((u >= 0.19) & (u < 0.40)).sum())).astype(f32)
    return {"depth": depth, "normal": normal, "color": color, "hit": hit, "drange": drange}


SPECIAL = ("badnormal", "nan_late", "nan_first", "posinf", "neginf", "huge", "onehit", "equaldepth")


def make_special(rng: np.random.Generator, W: int, H: int, kind: str) -> dict:
    """the plain case with one kind of trouble put in; drange stays the plain case's"""
    f32 = np.float32
    c = make_case(rng, W, H, "plain")
    depth, normal, hit = c["depth"], c["normal"], c["hit"]
    if kind == "onehit":
        hit[:] = False
        hit[H // 2, W // 3] = True
    hits, misses = np.flatnonzero(hit), np.flatnonzero(~hit)
    flat = depth.reshape(-1)
    if kind == "badnormal":
        bad = np.array([[np.nan, np.nan, np.nan], [np.nan, 0.5, -0.5], [0.0, np.inf, 0.0], [-np.inf, 0.0, 1.0],
                        [np.inf, np.inf, -np.inf], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1.0, np.nan, -1.0]], f32)
        nf = normal.reshape(-1, 3)
        for idx in (hits, misses):                                   # every kind on hits and on misses
            where = rng.choice(idx, 3 * len(bad), replace=False)
            nf[where] = np.tile(bad, (3, 1))
    elif kind == "equaldepth":
        flat[hits] = f32(4.25)
    else:
        special = {"nan_late": [(5, np.nan)], "nan_first": [(0, np.nan)], "posinf": [(2, np.inf), (-1, np.inf)],
                   "neginf": [(0, -np.inf), (7, -np.inf)], "huge": [(1, 3.4e38), (4, -3.4e38), (-2, 3.4e38)], "onehit": []}[kind]
        for i, v in special:                                         # i: which hit, row-major
            flat[hits[i]] = f32(v)
        m = rng.choice(misses, 6, replace=False)                     # on a miss they must not matter
        flat[m] = np.array([np.nan, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38], f32)
    return c


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__.strip().splitlines()[-1], file=sys.stderr)
        return 2
    io = capture_io(argv[1])
    rng = np.random.default_rng(20240607)
    out = {}
    cases = [(16, 12, "plain"), (40, 33, "plain"), (16, 12, "allmiss"), (16, 12, "flat")]
    cases += [(40, 33, "badnormal")] + [(16, 12, kind) for kind in SPECIAL[1:]]
    for i, (W, H, kind) in enumerate(cases):
        if kind in SPECIAL:
            c = make_special(rng, W, H, kind)
        else:
            c = make_case(rng, W, H, kind)
            assert np.isfinite(c["depth"]).all()
        p = f"c{i}_"
        out[p + "depth"], out[p + "normal"], out[p + "color"] = c["depth"], c["normal"], c["color"]
        out[p + "hit"] = c["hit"].astype(np.uint8)
        out[p + "drange"] = np.array(c["drange"], np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            out[p + "img_depth"] = io.depth_to_image(c["depth"], c["hit"], c["drange"])
            out[p + "img_normal"] = io.normal_to_image(c["normal"], c["hit"])
            out[p + "img_color"] = io.color_to_image(c["color"])
            if kind in SPECIAL:
                own = io.depth_range_of(c)
                out[p + "own_drange"] = np.array(own, np.float64)
                out[p + "img_depth_own"] = io.depth_to_image(c["depth"], c["hit"], own)
                assert out[p + "img_depth_own"].dtype == np.uint8
        for k in ("img_depth", "img_normal", "img_color"):
            assert out[p + k].dtype == np.uint8
        print(f"case {i} {W}x{H} {kind}: hits {int(c['hit'].sum())}, depth image values {len(np.unique(out[p + 'img_depth']))}, "
              f"colour image values {len(np.unique(out[p + 'img_color']))}")
    out["ncases"] = np.array([len(cases)], np.int32)
    path = os.path.join(ROOT, "tests", "golden", "ssim_images.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
