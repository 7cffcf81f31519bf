"""Inputs shared by tests/test_scene_placement_host.py and tests/test_gpu_scene_placement.py: programs with the placement ops
(op_rotate, op_turn, op_mirror), the NumPy statement of what the ops do to a point, the points they are evaluated on and
the ctypes front of the host build (tests/native/placement_check.cpp).  Boxes, box samples and segments are
program_ext_cases'.  Everything is seeded: the CPU and the GPU test see the same arrays."""
import ctypes
import functools
import math

import numpy as np

from conftest import build_native

from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p

# largest t_exact - t_interval over the co-hit pixels of the tilted scene, 64 x 48, default camera, interval tol 1e-5, both from
# the host build.  Printed by
#   python -m pytest tests/test_scene_placement_host.py -k exact_against_interval -s
# (the lag is the length of the interval oracle's last probe, at most tol, lengthened where the ray grazes or where the
# wrapping effect under a rotation widens the last enclosures; tests/exact_cases.py has 4.23e-5 for the catalogue frames)
TILTED_LAG_MEASURED = 2.20e-5

A1, A2, A3, A4 = (0.3, -0.5, 0.7), (-1.1, 0.4, 0.25), (0.0, 0.9, 0.0), (2.0, -0.3, -1.7)
OFF = (0.35, -0.2, 0.15)
A5 = (0.15, 0.6, -0.1)             # the extra rotation of the conjugation tests: gentle enough to keep the floor's horizon in view


def conjugate_camera(angles, W=64, H=48):
    """the default camera, its position, target and up sent through op_rotate(angles, .)'s point transform: what it sees of
    a scene is what the default camera sees of op_rotate(angles, scene)"""
    c = rot_consts(angles)
    return Camera(tuple(np_rotate(np.array([0.0, 0.0, 5.0]), c)), tuple(np_rotate(np.zeros(3), c)),
                  tuple(np_rotate(np.array([0.0, 1.0, 0.0]), c)), 60.0, W, H)


def cyl():
    return sp.sd_cylinder(0.6, 0.9)


def rot_consts(angles):
    """cx, sx, cy, sy, cz, sz by the host's libm; exactly (1, 0) for an angle of 0"""
    out = []
    for a in angles:
        out += [1.0, 0.0] if a == 0.0 else [math.cos(a), math.sin(a)]
    return tuple(out)


QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def turn_consts(quarters):
    return tuple(v for q in quarters for v in QUARTER[q % 4])


# name -> (chain of transforms from the outermost in, the child they apply to).  A transform is (kind, argument).
def chains():
    return {
        "rot_x": ([("rotate", (0.4, 0.0, 0.0))], cyl()),
        "rot_y": ([("rotate", (0.0, -0.8, 0.0))], cyl()),
        "rot_z": ([("rotate", (0.0, 0.0, 1.3))], cyl()),
        "rot_xyz": ([("rotate", A1)], cyl()),
        "turn": ([("turn", (1, 2, 3))], cyl()),
        "mirror": ([("mirror", (1, 0, 1))], sp.op_translate((0.5, 0.2, 0.3), cyl())),
        "rot_of_translate": ([("rotate", A1), ("translate", OFF)], cyl()),          # the fused word inside a rotated frame
        "translate_of_rot": ([("translate", OFF), ("rotate", A1)], cyl()),          # not fused
        "nested4": ([("rotate", A1), ("rotate", A2), ("rotate", A3), ("rotate", A4)], cyl()),      # a rotate in every point slot
        "mirror_in_rot": ([("rotate", A2), ("mirror", (0, 1, 1)), ("translate", OFF), ("turn", (0, 0, 1))], cyl()),
    }


def wrap(kind, arg, child):
    if kind == "rotate":
        return sp.op_rotate(arg, child)
    if kind == "turn":
        return sp.op_turn(arg, child)
    if kind == "mirror":
        return sp.op_mirror(arg, child)
    return sp.op_translate(arg, child)


def build(chain, child):
    e = child
    for kind, arg in reversed(chain):
        e = wrap(kind, arg, e)
    return e


def np_rotate(p, consts):
    """The point transform of RM_SOP_ROTATE as include/rm_hip.h states it: per plane the four products, then one add and one
    subtract, both from the old pair (NumPy does not fuse); a pair that is exactly (1, 0) is skipped."""
    x, y, z = p[..., 0].copy(), p[..., 1].copy(), p[..., 2].copy()
    cx, sx, cy, sy, cz, sz = consts
    if (cz, sz) != (1.0, 0.0):
        x, y = cz * x + sz * y, cz * y - sz * x
    if (cy, sy) != (1.0, 0.0):
        z, x = cy * z + sy * x, cy * x - sy * z
    if (cx, sx) != (1.0, 0.0):
        y, z = cx * y + sx * z, cx * z - sx * y
    return np.stack([x, y, z], axis=-1)


def np_unrotate(v, consts):
    """the transpose: the planes in the reverse order with the sines negated (frame of the child -> world)"""
    x, y, z = v[..., 0].copy(), v[..., 1].copy(), v[..., 2].copy()
    cx, sx, cy, sy, cz, sz = consts
    y, z = cx * y - sx * z, cx * z + sx * y
    z, x = cy * z - sy * x, cy * x + sy * z
    x, y = cz * x - sz * y, cz * y + sz * x
    return np.stack([x, y, z], axis=-1)


def np_transform(kind, arg, p):
    if kind == "rotate":
        return np_rotate(p, rot_consts(arg))
    if kind == "turn":
        return np_rotate(p, turn_consts(arg))
    if kind == "mirror":
        q = p.copy()
        for a in range(3):
            if arg[a]:
                q[..., a] = np.abs(q[..., a])
        return q
    return p - np.array(arg, dtype=np.float64)


def np_chain(chain, p):
    for kind, arg in chain:
        p = np_transform(kind, arg, p)
    return p


def tilted():
    """A hard-CSG scene no axis-aligned program can state: a rotated box minus a rotated cylinder, a torus turned to face
    the default camera, a floor."""
    body = sp.op_subtract(sp.op_rotate((0.5, 0.3, -0.4), sp.sd_box((0.9, 0.6, 0.7))),
                          sp.op_rotate((0.2, 0.0, 1.1), sp.sd_cylinder(0.4, 1.5)))
    ring = sp.op_turn((1, 0, 0), sp.sd_torus(1.5, 0.15))
    return sp.op_union(sp.op_union(body, ring), sp.sd_plane((0.0, 1.0, 0.0), -1.8))


def programs():
    """{name: expression}: the chains and the tilted scene"""
    out = {name: build(chain, child) for name, (chain, child) in chains().items()}
    out["tilted"] = tilted()
    return out


NAMES = list(chains()) + ["tilted"]
LANE_COUNTS = (1, 63, 64, 65)


def points():
    """0, -0, the smallest denormals and +-1 ulp beside other values on either side of the mirror planes, points on each axis,
    1400 random points of [-3, 3]^3 with some coordinates replaced by those values"""
    rng = np.random.default_rng(23)
    tiny = 5e-324
    sc = np.array([0.0, -0.0, tiny, -tiny, np.nextafter(0.5, 1.0), np.nextafter(-0.5, -1.0), 1.0, -1.0, 0.35, -0.2, 0.15, 2.5, -2.5])
    grid = np.array([[a, b, c] for a in sc[:6] for b in sc[:6] for c in sc[:6]])
    axes = np.array([[s * v if i == a else 0.0 for i in range(3)] for a in range(3) for v in (0.3, 1.0, 2.0) for s in (1.0, -1.0)])
    pts = rng.uniform(-3.0, 3.0, size=(1400, 3))
    pick = rng.integers(0, len(sc), size=pts.shape)
    mask = rng.random(pts.shape) < 0.25
    pts[mask] = sc[pick][mask]
    return np.ascontiguousarray(np.concatenate([grid, axes, pts]))


def default_camera(W=64, H=48):
    return Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H)


def exact_rays(seed=5, n=4096, half=1.2):
    """n rays through the box [-half, half]^3: from a point outside it towards a point inside, directions not normalised"""
    rng = np.random.default_rng(seed)
    inside = rng.uniform(-half, half, size=(n, 3))
    o = rng.normal(size=(n, 3))
    o *= (rng.uniform(3.0, 6.0, size=n) * half / np.linalg.norm(o, axis=1))[:, None]
    d = (inside - o) * rng.uniform(0.2, 3.0, size=n)[:, None]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rows_of(expr):
    return [(op, list(f)) for op, f in sp.compile_ops(expr)]


def ops_array(rows):
    arr = (_native.RmSceneOp * max(1, len(rows)))()
    for i, (op, f) in enumerate(rows):
        arr[i].op, arr[i].arg = op, 0
        for j, v in enumerate(f):
            arr[i].f[j] = v
    return arr


class Host:
    """The host build of the five evaluations (tests/native/placement_check.cpp)."""

    def __init__(self):
        self.L = ctypes.CDLL(build_native("placement_check"))
        self.why = ctypes.create_string_buffer(256)

    def _ok(self, rc):
        assert rc == 0, (rc, self.why.value)

    def encode(self, rows):
        """(0 / -1, reason, encoded words)"""
        words, n = (ctypes.c_uint32 * 256)(), ctypes.c_int32(0)
        rc = self.L.rmp_encode(ops_array(rows), len(rows), words, 256, ctypes.byref(n), self.why, 256)
        return rc, self.why.value.decode(), list(words[:n.value]) if rc == 0 else []

    def point(self, expr, pts):
        ops, n = sp.to_ctypes(expr)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        self._ok(self.L.rmp_point(ops, n, pts.ctypes.data_as(dp), ctypes.c_size_t(len(pts)), out.ctypes.data_as(dp), self.why, 256))
        return out

    def interval(self, expr, lo, hi):
        ops, n = sp.to_ctypes(expr)
        lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
        out = np.empty((len(lo), 2))
        self._ok(self.L.rmp_interval(ops, n, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), ctypes.c_size_t(len(lo)),
                                     out.ctypes.data_as(dp), self.why, 256))
        return out

    def dual(self, expr, segs):
        ops, n = sp.to_ctypes(expr)
        segs = np.ascontiguousarray(segs, np.float64)
        dual, box = np.empty((len(segs), 4)), np.empty((len(segs), 2))
        self._ok(self.L.rmp_dual(ops, n, segs.ctypes.data_as(dp), ctypes.c_size_t(len(segs)), dual.ctypes.data_as(dp),
                                 box.ctypes.data_as(dp), self.why, 256))
        return dual, box

    def affine(self, expr, mode, segs, want_form=False):
        ops, n = sp.to_ctypes(expr)
        segs = np.ascontiguousarray(segs, np.float64)
        out, form = np.empty((len(segs), 2)), np.empty((len(segs), 3))
        self._ok(self.L.rmp_affine(ops, n, int(mode), segs.ctypes.data_as(dp), ctypes.c_size_t(len(segs)), out.ctypes.data_as(dp),
                                   form.ctypes.data_as(dp), self.why, 256))
        return (out, form) if want_form else out

    def exact_supported(self, expr):
        ops, n = sp.to_ctypes(expr)
        return self.L.rmp_exact_supported(ops, n, self.why, 256), self.why.value.decode()

    def exact_march(self, expr, o, d, t_min=0.0, t_max=0.0):
        ops, n = sp.to_ctypes(expr)
        o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
        m = len(d)
        t, nrm, leaf = np.empty(m), np.empty((m, 3)), np.empty(m, np.int32)
        cfg = _native.exact_config(t_min=t_min, t_max=t_max)
        self._ok(self.L.rmp_exact_march(ops, n, ctypes.byref(cfg), o.ctypes.data_as(dp), d.ctypes.data_as(dp), ctypes.c_size_t(m),
                                        t.ctypes.data_as(dp), nrm.ctypes.data_as(dp), leaf.ctypes.data_as(vp), self.why, 256))
        return t, nrm, leaf

    def exact_render(self, expr, cam14, W, H, t_max=100.0):
        ops, n = sp.to_ctypes(expr)
        cam = np.ascontiguousarray(cam14, np.float64)
        depth, hit, nrm, leaf = np.empty(W * H), np.empty(W * H, np.uint8), np.empty((W * H, 3)), np.empty(W * H, np.int32)
        cfg = _native.exact_config(t_max=t_max)
        self._ok(self.L.rmp_exact_render(ops, n, ctypes.byref(cfg), cam.ctypes.data_as(dp), W, H, depth.ctypes.data_as(dp),
                                         hit.ctypes.data_as(vp), nrm.ctypes.data_as(dp), leaf.ctypes.data_as(vp), self.why, 256))
        return {"depth": depth.reshape(H, W), "hit": hit.reshape(H, W) > 0, "normal": nrm.reshape(H, W, 3), "leaf": leaf.reshape(H, W)}

    def interval_render(self, expr, cam14, W, H, tol=1e-5, t_max=100.0):
        ops, n = sp.to_ctypes(expr)
        cam = np.ascontiguousarray(cam14, np.float64)
        depth, hit, steps = np.empty(W * H), np.empty(W * H, np.uint8), np.empty(W * H, np.int32)
        cfg = _native.interval_config(t_max=t_max, tol=tol, bound_radius=-1.0)
        self._ok(self.L.rmp_interval_render(ops, n, ctypes.byref(cfg), cam.ctypes.data_as(dp), W, H, depth.ctypes.data_as(dp),
                                            hit.ctypes.data_as(vp), steps.ctypes.data_as(vp), self.why, 256))
        return {"depth": depth.reshape(H, W), "hit": hit.reshape(H, W) > 0, "steps": steps.reshape(H, W)}

    def affine_render(self, expr, mode, cam14, W, H, tol=1e-5, t_max=100.0):
        ops, n = sp.to_ctypes(expr)
        cam = np.ascontiguousarray(cam14, np.float64)
        depth, hit, steps = np.empty(W * H), np.empty(W * H, np.uint8), np.empty(W * H, np.int32)
        cfg = _native.interval_config(t_max=t_max, tol=tol, bound_radius=-1.0)
        self._ok(self.L.rmp_affine_render(ops, n, int(mode), ctypes.byref(cfg), cam.ctypes.data_as(dp), W, H, depth.ctypes.data_as(dp),
                                          hit.ctypes.data_as(vp), steps.ctypes.data_as(vp), self.why, 256))
        return {"depth": depth.reshape(H, W), "hit": hit.reshape(H, W) > 0, "steps": steps.reshape(H, W)}


@functools.lru_cache(maxsize=None)
def host():
    return Host()


@functools.lru_cache(maxsize=None)
def tilted_frames():
    """(exact, interval) captures of the tilted scene by the host build, 64 x 48, default camera (computed once; read only)"""
    cam = default_camera().params14()
    return host().exact_render(tilted(), cam, 64, 48), host().interval_render(tilted(), cam, 64, 48)
