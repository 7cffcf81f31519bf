"""Inputs shared by tests/test_scene_program_ext_host.py and tests/test_gpu_scene_program_ext.py: the programs (the five
catalogue twins and each of the four new ops alone under a translate), the points, boxes and ray segments they are
evaluated on, and the ctypes front of the host build (tests/native/program_ext_check.cpp).  Everything is seeded: the
CPU and the GPU test see the same arrays."""
import ctypes
import math
import os

import numpy as np

from conftest import GOLDEN, build_native

from raymarch_algo_compare_amd import scene_program as sp

TWIN_IDS = [9, 11, 15, 16, 18]
REGION = 3.5

# each new op alone, under a translate (the primitives fuse with it: `translate, primitive, pop point` is one word).  The
# children are cylinders: sd_sphere, sd_box and sd_torus are the three ops whose interval form takes a square root where the
# point form takes `** 0.5` ("Interval oracle"), so a tree without them is bit-identical at a point.
SINGLE = {
    "scale": ((0.3, -0.2, 0.1), lambda: sp.op_scale(sp.sd_cylinder(0.6, 0.9), 2.5)),
    "limited_repeat": ((0.25, -0.4, 0.15),
                       lambda: sp.op_limited_repeat((1.0, 0.7, 0.0), (2.0, 1.0, 3.0), sp.sd_cylinder(0.2, 0.25))),
    "menger_cross": ((0.1, 0.2, -0.3), lambda: sp.sd_menger_cross(3.0)),
    "gyroid": ((0.2, -0.1, 0.4), lambda: sp.sd_gyroid(3.0, 10.5)),
}


def programs():
    """[(name, expression, translate offset)]: the twins by catalogue id, then the single ops"""
    twins = sp.catalogue_twins()
    out = [(f"twin{sid}", twins[sid], (0.0, 0.0, 0.0)) for sid in TWIN_IDS]
    out += [(name, sp.op_translate(off, make()), off) for name, (off, make) in SINGLE.items()]
    return out


NAMES = [f"twin{sid}" for sid in TWIN_IDS] + list(SINGLE)


def special_coordinates():
    """Coordinates where an op takes another path: cell edges of the lattices (k + 0.5, spacing 0.7 too), the clamped outer
    cells (|x| > 2.5), Menger jump and fold planes for s = 1, 3, 9 (p * s an even integer, +-1/3 of a period beside it),
    the gyroid's extrema (freq * x a multiple of pi / 2), and 0."""
    v = [0.0]
    v += [k + 0.5 for k in range(-4, 4)] + [0.7 * (k + 0.5) for k in range(-3, 3)]
    v += [2.6, -2.6, 3.2, -3.2, 2.5, -2.5]
    for s in (1.0, 3.0, 9.0):
        for k in range(-3, 4):
            e = 2.0 * k / s
            v += [e, e + 1.0 / (3.0 * s), e - 1.0 / (3.0 * s), e + 1.0 / s]
    v += [j * math.pi / 6.0 for j in range(-6, 7)]
    return np.array(sorted(set(x for x in v if abs(x) <= REGION)))


def special_points(offset=(0.0, 0.0, 0.0)):
    """Points with one, two or three special coordinates (of the op's own frame and of the world frame), the others random;
    negative coordinates included (Python's `%` sign)."""
    rng = np.random.default_rng(11)
    sc = special_coordinates()
    sc = np.unique(np.concatenate([sc, sc + offset[0], sc + offset[1], sc + offset[2]]))
    n = 1500
    pts = rng.uniform(-REGION, REGION, size=(n, 3))
    pick = rng.integers(0, len(sc), size=(n, 3))
    mask = rng.random((n, 3)) < 0.5
    mask[np.arange(n), rng.integers(0, 3, size=n)] = True
    pts[mask] = sc[pick][mask]
    nudge = rng.integers(-1, 2, size=(n, 3)) * (rng.random((n, 3)) < 0.3)
    return np.ascontiguousarray(np.nextafter(pts, pts + nudge))


def parity_points():
    """tests/golden/sdf_points.npz's points (the reference evaluated the catalogue there), 2000 default_rng(0) points in
    [-3.5, 3.5]^3 and the special points"""
    z = np.load(os.path.join(GOLDEN, "sdf_points.npz"))
    rnd = np.random.default_rng(0).uniform(-REGION, REGION, size=(2000, 3))
    return z, np.ascontiguousarray(np.concatenate([z["pts"], rnd, special_points()]))


def boxes(seed, offset):
    """4000 boxes (lo, hi): 500 degenerate, 2000 with edges 1e-6 .. 4, 1000 astride a special coordinate (edges 1e-9 ..
    0.1), 500 wider than the gyroid's period 2 pi / 3"""
    rng = np.random.default_rng(seed)
    c0 = np.concatenate([special_points(offset)[:250], rng.uniform(-REGION, REGION, size=(250, 3))])
    c1 = rng.uniform(-REGION, REGION, size=(2000, 3))
    e1 = 10.0 ** rng.uniform(-6.0, math.log10(4.0), size=(2000, 3))
    c2 = special_points(offset)[250:1250]
    e2 = 10.0 ** rng.uniform(-9.0, -1.0, size=(1000, 3))
    c2 = c2 + e2 * rng.uniform(-0.5, 0.5, size=(1000, 3)) * (rng.random((1000, 3)) < 0.5)
    c3 = rng.uniform(-REGION, REGION, size=(500, 3))
    e3 = rng.uniform(2.0 * math.pi / 3.0, 4.0, size=(500, 3))
    c = np.concatenate([c0, c1, c2, c3])
    e = np.concatenate([np.zeros((500, 3)), e1, e2, e3])
    return np.ascontiguousarray(c - 0.5 * e), np.ascontiguousarray(c + 0.5 * e)


def box_samples(seed, lo, hi, n=64):
    """(boxes, n + 8, 3): n random points of each box and its corners"""
    rng = np.random.default_rng(seed)
    u = rng.random((len(lo), n, 3))
    corners = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], dtype=np.float64)
    u = np.concatenate([u, np.broadcast_to(corners, (len(lo), 8, 3))], axis=1)
    p = lo[:, None, :] + u * (hi - lo)[:, None, :]
    return np.clip(p, lo[:, None, :], hi[:, None, :])


def segments(seed, n=2000):
    """n ray segments (n x 8: origin, unit direction, t0, t1) with lengths 1e-5 .. 2 through [-3, 3]^3"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3.0, 3.0, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    length = 10.0 ** rng.uniform(-5.0, math.log10(2.0), size=n)
    t0 = rng.uniform(0.0, 4.0, size=n)
    return np.ascontiguousarray(np.concatenate([a - t0[:, None] * d, d, t0[:, None], (t0 + length)[:, None]], axis=1))


# ops whose degenerate interval value may differ from the point walk's in the last place (tests/test_interval_host.py)
DIFFERING_OPS = {"sd_sphere", "sd_box", "sd_torus"}


def uses(expr, names):
    return expr.op in names or any(uses(c, names) for c in expr.children)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Host:
    """The host build of the four evaluations."""

    def __init__(self):
        self.L = ctypes.CDLL(build_native("program_ext_check"))
        self.why = ctypes.create_string_buffer(256)

    @staticmethod
    def _dp(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def _ok(self, rc):
        assert rc == 0, (rc, self.why.value)

    def encode(self, rows):
        from raymarch_algo_compare_amd import _native
        arr = (_native.RmSceneOp * max(1, len(rows)))()
        for i, (op, f) in enumerate(rows):
            arr[i].op, arr[i].arg = op, 0
            for j, v in enumerate(f):
                arr[i].f[j] = v
        return self.L.rmx_encode(arr, len(rows), self.why, 256), self.why.value.decode()

    def point(self, expr, pts):
        ops, n = sp.to_ctypes(expr)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        self._ok(self.L.rmx_point(ops, n, self._dp(pts), ctypes.c_size_t(len(pts)), self._dp(out), self.why, 256))
        return out

    def interval(self, expr, lo, hi):
        ops, n = sp.to_ctypes(expr)
        out = np.empty((len(lo), 2))
        self._ok(self.L.rmx_interval(ops, n, self._dp(lo), self._dp(hi), ctypes.c_size_t(len(lo)), self._dp(out), self.why, 256))
        return out

    def dual(self, expr, segs):
        ops, n = sp.to_ctypes(expr)
        dual, box = np.empty((len(segs), 4)), np.empty((len(segs), 2))
        self._ok(self.L.rmx_dual(ops, n, self._dp(segs), ctypes.c_size_t(len(segs)), self._dp(dual), self._dp(box), self.why, 256))
        return dual, box

    def affine(self, expr, mode, segs):
        ops, n = sp.to_ctypes(expr)
        out = np.empty((len(segs), 2))
        self._ok(self.L.rmx_affine(ops, n, int(mode), self._dp(segs), ctypes.c_size_t(len(segs)), self._dp(out), self.why, 256))
        return out

    def interval_render(self, expr, cam14, width, height, cfg=None):
        ops, n = sp.to_ctypes(expr)
        cam14 = np.ascontiguousarray(cam14, dtype=np.float64)
        npx = width * height
        depth, hit, steps = np.empty(npx), np.empty(npx, np.uint8), np.empty(npx, np.int32)
        self._ok(self.L.rmx_interval_render(ops, n, ctypes.byref(cfg) if cfg is not None else None, self._dp(cam14), width, height,
                                            self._dp(depth), hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            steps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.why, 256))
        return depth.reshape(height, width), hit.reshape(height, width), steps.reshape(height, width)
