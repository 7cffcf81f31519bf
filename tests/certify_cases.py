"""Shared by tests/test_certify_host.py and tests/test_gpu_certify.py: the g++ build of csrc/rm_certify.h
(tests/native/certify_check.cpp), the frames and programs the certified first hit is checked on, the constructed rays, and
the measured bound."""
import ctypes
import functools
import json
import os

import numpy as np

from conftest import GOLDEN, build_native
import exact_cases as ec

from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p
MISS, HIT, OPEN = _native.RM_CERTIFY_MISS, _native.RM_CERTIFY_HIT, _native.RM_CERTIFY_OPEN
CATALOGUE_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 17, 19]
TWIN_IDS = sorted(sp.catalogue_twins())
T_MAX = 100.0
WIDTH_REL = 1e-10            # a HIT's bracket: t_hi - t_lo <= 1e-10 (1 + t_lo)
PILLAR_FOREST, HOLLOW_CUBE = 12, 6

# The largest amount by which an exact first hit of the eleven frames lies outside its bracket, max(t_lo - t_exact,
# t_exact - t_hi, 0), the bracket by the host build of rm_certify.h and the hit by the host build of rm_exact.h
# (tests/test_certify_host.py prints it; DESIGN.md section 3 records it).  The tests assert 4 x this value.
BRACKET_SLACK_MEASURED = 0.0
# pixels the interval oracle (tol 1e-5, no prune) reports as hits whose bracket ends MISS or has t_lo more than 1e-3 past
# the oracle's t, at 64 x 48 with the default camera: the oracle's false hits
FALSE_HITS_MEASURED = {PILLAR_FOREST: 2232, HOLLOW_CUBE: 0}


@functools.lru_cache(maxsize=None)
def lib():
    """tests/native/certify_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("certify_check"))
    L.rmc_march.argtypes = [vp, ctypes.c_int32, vp, dp, dp, ctypes.c_size_t, dp, dp, vp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rmc_render.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_double, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             dp, dp, vp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rmc_resolve.argtypes = [vp, ctypes.c_double, dp, ctypes.c_char_p, ctypes.c_int]
    L.rmc_scene_bound.restype = ctypes.c_double
    L.rmc_scene_bound.argtypes = [ctypes.c_int]
    L.rmc_sizeof_config.restype = ctypes.c_size_t
    L.rmc_offsetof_config.restype = ctypes.c_size_t
    L.rmc_offsetof_config.argtypes = [ctypes.c_int]
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_march(expr, o, d, cfg=None):
    """(t_lo, t_hi, status, steps) of the host build over explicit rays (directions as given)"""
    ops, n = sp.to_ctypes(expr)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, np.float64), d.shape))
    m = len(d)
    t_lo, t_hi, status, steps = np.empty(m), np.empty(m), np.empty(m, np.uint8), np.empty(m, np.int32)
    why = ctypes.create_string_buffer(256)
    rc = lib().rmc_march(ops, n, ctypes.byref(cfg) if cfg is not None else None, o.ctypes.data_as(dp), d.ctypes.data_as(dp), m,
                         t_lo.ctypes.data_as(dp), t_hi.ctypes.data_as(dp), status.ctypes.data, steps.ctypes.data, why, 256)
    assert rc == 0, (rc, why.value)
    return t_lo, t_hi, status, steps


def host_render(expr, cam14, W, H, cfg=None, scene_bound=-1.0, row0=0, rows=None):
    """{t_lo, t_hi, status, steps} (rows, W) of the host build on the library's camera rays"""
    ops, n = sp.to_ctypes(expr)
    rows = H - row0 if rows is None else rows
    cam = np.ascontiguousarray(cam14, np.float64)
    m = W * rows
    t_lo, t_hi, status, steps = np.empty(m), np.empty(m), np.empty(m, np.uint8), np.empty(m, np.int32)
    why = ctypes.create_string_buffer(256)
    rc = lib().rmc_render(ops, n, ctypes.byref(cfg) if cfg is not None else None, scene_bound, cam.ctypes.data_as(dp), W, H, row0,
                          rows, t_lo.ctypes.data_as(dp), t_hi.ctypes.data_as(dp), status.ctypes.data, steps.ctypes.data, why, 256)
    assert rc == 0, (rc, why.value)
    return {"t_lo": t_lo.reshape(rows, W), "t_hi": t_hi.reshape(rows, W), "status": status.reshape(rows, W),
            "steps": steps.reshape(rows, W)}


def same(a, b):
    """two results {t_lo, t_hi, status, steps} agree bit for bit"""
    return (np.array_equal(bits(a["t_lo"]), bits(b["t_lo"])) and np.array_equal(bits(a["t_hi"]), bits(b["t_hi"]))
            and np.array_equal(a["status"], b["status"]) and np.array_equal(a["steps"], b["steps"]))


# ---- the frames: every catalogue program and every twin at 64 x 48 (Thin Torus 128 x 96), default camera -------------------

def frame_keys():
    """("c", id) for the 14 catalogue programs, ("t", id) for the five twins"""
    return [("c", sid) for sid in CATALOGUE_IDS] + [("t", sid) for sid in TWIN_IDS]


def frame_expression(key):
    kind, sid = key
    return sp.catalogue_twins()[sid] if kind == "t" else sp.catalogue_expressions()[sid]


def frame_size(key):
    return (128, 96) if key == ("c", 3) else (64, 48)


def exact_key(sid):
    """the frame of an exact_cases.EXACT_IDS scene"""
    return ("t", sid) if sid in ec.TWIN_IDS else ("c", sid)


def frame_camera(key):
    """the eleven frames with an exact form: exact_cases' camera, (0, 0, 5) -> 0; the others: the scene's own default"""
    W, H = frame_size(key)
    scene = registry.SCENES[key[1]]
    if key[1] in ec.EXACT_IDS or scene.camera_position is None:
        return ec.default_camera(W, H)
    return Camera(scene.camera_position, scene.camera_target, (0.0, 1.0, 0.0), 60.0, W, H)


def frame_config(key, **kw):
    """the default configuration with l_global = the scene's Lipschitz bound (2 for Bad Lipschitz Sphere, else 1)"""
    return _native.certify_config(l_global=float(registry.SCENES[key[1]].lipschitz), **kw)


@functools.lru_cache(maxsize=None)
def host_frame(key):
    """the host build's brackets of the frame, no prune (computed once; read only)"""
    W, H = frame_size(key)
    return host_render(frame_expression(key), frame_camera(key).params14(), W, H, frame_config(key))


@functools.lru_cache(maxsize=None)
def host_interval_frame(key):
    """the host interval oracle on the same rays (tol 1e-5, no prune)"""
    W, H = frame_size(key)
    return ec.host_interval_render(frame_expression(key), frame_camera(key).params14(), W, H)


def frame_rays(key):
    W, H = frame_size(key)
    o, d = ec.camera_rays(frame_camera(key).params14(), W, H)
    return o, d.reshape(-1, 3)


# ---- the 40 fixture trees: rays inside one cell of a tree that repeats ---------------------------------------------------------

def trees():
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        return [sp.expr_from_json(t) for t in json.load(f)["trees"]]


REGION = 3.0


def one_cell(expr):
    """The world-space box inside which no op_repeat of the tree wraps (as tests/test_segment_host.py's): None for a tree
    without op_repeat."""
    lo, hi, found = np.full(3, -REGION), np.full(3, REGION), [False]

    def walk(e, offset):
        if e.op == "op_translate":
            offset = offset + np.array(e.param("offset"))
        elif e.op == "op_repeat":
            found[0] = True
            for ax, s in enumerate(e.param("spacing")):
                if s > 0.0:
                    lo[ax] = max(lo[ax], offset[ax] - 0.5 * s)
                    hi[ax] = min(hi[ax], offset[ax] + 0.5 * s)
        for c in e.children:
            walk(c, offset)

    walk(expr, np.zeros(3))
    return (lo, hi) if found[0] else None


def tree_rays(idx, expr, n=96):
    """(o, d, t_max) for tree idx: n rays between two random points of the region (of the tree's one cell when it repeats),
    unit directions, t_max the distance between the points, so that a ray never leaves the cell"""
    rng = np.random.default_rng(7000 + idx)
    cell = one_cell(expr)
    lo, hi = (np.full(3, -REGION), np.full(3, REGION)) if cell is None else cell
    w = hi - lo
    assert np.all(w > 0.0), (idx, "the repeats of this tree share no cell")
    p = rng.uniform(lo + 1e-9 * w, hi - 1e-9 * w, size=(n, 3))
    q = rng.uniform(lo + 1e-9 * w, hi - 1e-9 * w, size=(n, 3))
    length = np.linalg.norm(q - p, axis=1)
    return p, (q - p) / length[:, None], length


# ---- the user program of the device comparison: rotate, mirror and limited repeat --------------------------------------------

def rotated_program():
    body = sp.op_union(sp.sd_box((0.35, 0.25, 0.3)), sp.op_translate((0.2, 0.3, 0.0), sp.sd_sphere(0.3)))
    body = sp.op_limited_repeat((1.1, 0.0, 1.3), (1.0, 0.0, 1.0), body)
    return sp.op_rotate((0.3, -0.5, 0.2), sp.op_mirror((1, 0, 0), body))


# ---- explicit rays with every outcome in one wave -------------------------------------------------------------------------------

INSIDE = {14: (-0.6017, -1.1893, 1.0755), 12: (0.0, 0.0, 0.0)}      # a point well inside a solid: a cloud sphere, the central pillar


def mixed_rays(n, seed, inside=None):
    """n rays towards the origin from a shell of radius 6 (hits and misses), every fifth from within 0.05 of `inside` (an eye
    in a solid; without one, from the cube of half edge 0.5), every seventh a tangent of the unit sphere at (0, 1, 0), every
    ninth unnormalised"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o *= 6.0 / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.normal(scale=1.2, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[::5] = rng.uniform(-0.5, 0.5, size=o[::5].shape) if inside is None else np.asarray(inside) + rng.uniform(-0.05, 0.05, size=o[::5].shape)
    o[1::7] = (-5.0, 1.0, 0.0)
    d[1::7] = (1.0, 0.0, 0.0)
    d[::9] *= 0.5
    return o, d
