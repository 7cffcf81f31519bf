"""Shared by tests/test_exact_host.py and tests/test_gpu_exact.py: the g++ builds of csrc/rm_exact.h
(tests/native/exact_check.cpp) and csrc/rm_interval.h (tests/native/interval_check.cpp), the scenes with an exact form,
the fixture of the reference's closed forms (tests/golden/exact_reference.npz) and the measured bounds."""
import ctypes
import functools
import os

import numpy as np

from conftest import GOLDEN, build_native

from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p

# The scenes with an exact form: catalogue ids 0-6, 8 and 14 and the program twins of 11 and 15.
EXACT_IDS = [0, 1, 2, 3, 4, 5, 6, 8, 14, 11, 15]
TWIN_IDS = (11, 15)
NAMES = {0: "Sphere", 1: "Grazing Plane", 2: "Cube", 3: "Thin Torus", 4: "Cylinder", 5: "Near Miss", 6: "Hollow Cube (CSG)",
         8: "Onion Shell", 14: "Sphere Cloud", 11: "Bad Lipschitz Sphere", 15: "Bumpy Sphere"}
T_MAX = 100.0

# ---- the four values the host build measured (tests/test_exact_host.py prints them; DESIGN.md section 3 records them) ----
# largest |depth - reference's intersect_torus depth| over the torus fixtures; the reference's own eigenvalue error
TORUS_DEPTH_MEASURED = 7.12e-12
# largest t_exact - t_interval over the co-hit pixels of the eleven frames (tol 1e-5: the interval hit is the start of a
# segment of length <= tol that reaches the surface, lengthened where the ray grazes)
INTERVAL_LAG_MEASURED = 4.23e-5
# largest |f(p_hit)| over the eleven frames, f by the pointwise interpreter
ROOT_RESIDUAL_MEASURED = 3.0e-14
# interval-hit / exact-miss pixels over the eleven frames (all of them in the k = 2 silhouette band of the exact mask)
INTERVAL_ONLY_PIXELS = 0


def expression(sid: int):
    return sp.catalogue_twins()[sid] if sid in TWIN_IDS else sp.catalogue_expressions()[sid]


def frame_size(sid: int):
    return (128, 96) if sid == 3 else (64, 48)


def default_camera(W: int, H: int) -> Camera:
    return Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H)


# a user program mixing box, cylinder, capsule, torus, subtract, and onion over a sphere
def mixed_program():
    body = sp.op_union(sp.sd_box((0.9, 0.6, 0.7)), sp.op_translate((0.0, 0.9, 0.0), sp.sd_cylinder(0.5, 0.6)))
    body = sp.op_union(body, sp.sd_capsule((-1.4, -0.5, 0.2), (1.3, 0.8, -0.3), 0.25))
    body = sp.op_union(body, sp.op_translate((0.0, -0.2, 0.0), sp.sd_torus(1.6, 0.2)))
    body = sp.op_subtract(body, sp.op_translate((0.3, 0.1, 0.8), sp.op_onion(sp.sd_sphere(0.7), 0.08)))
    return body


@functools.lru_cache(maxsize=None)
def exact_lib():
    """tests/native/exact_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("exact_check"))
    L.rme_catalogue.argtypes = [ctypes.c_int, vp, ctypes.c_int]
    L.rme_supported.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int]
    L.rme_march.argtypes = [vp, ctypes.c_int32, vp, dp, dp, ctypes.c_size_t, dp, vp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rme_render.argtypes = [vp, ctypes.c_int32, vp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, vp, dp, vp,
                             ctypes.c_char_p, ctypes.c_int]
    L.rme_sizeof_config.restype = ctypes.c_size_t
    L.rme_offsetof_config.restype = ctypes.c_size_t
    L.rme_offsetof_config.argtypes = [ctypes.c_int]
    return L


@functools.lru_cache(maxsize=None)
def interval_lib():
    """tests/native/interval_check.cpp built by g++ (the host interval oracle)"""
    L = ctypes.CDLL(build_native("interval_check"))
    L.rmi_render.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_double, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp,
                             vp, dp, vp, ctypes.c_char_p, ctypes.c_int]
    return L


@functools.lru_cache(maxsize=None)
def program_lib():
    """tests/native/program_check.cpp built by g++ (the pointwise interpreter)"""
    L = ctypes.CDLL(build_native("program_check"))
    L.rmp_eval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, ctypes.c_char_p, ctypes.c_int]
    return L


def _cfg(t_min=0.0, t_max=T_MAX):
    return _native.exact_config(t_min=t_min, t_max=t_max)


def host_supported(expr):
    """(1 / 0 / -1, reason) of exact_supported for the expression's program"""
    ops, n = sp.to_ctypes(expr)
    why = ctypes.create_string_buffer(256)
    return exact_lib().rme_supported(ops, n, why, 256), why.value.decode()


def host_march(expr, o, d, t_min=0.0, t_max=0.0):
    """(t, normals, leaf) of the host build over explicit rays (t_max 0: no limit)"""
    ops, n = sp.to_ctypes(expr)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, np.float64), d.shape))
    m = len(d)
    t, nrm, leaf = np.empty(m), np.empty((m, 3)), np.empty(m, np.int32)
    why = ctypes.create_string_buffer(256)
    cfg = _cfg(t_min, t_max)
    rc = exact_lib().rme_march(ops, n, ctypes.byref(cfg), o.ctypes.data_as(dp), d.ctypes.data_as(dp), m, t.ctypes.data_as(dp),
                               nrm.ctypes.data, leaf.ctypes.data, why, 256)
    assert rc == 0, (rc, why.value)
    return t, nrm, leaf


def host_render(expr, cam14, W, H, row0=0, rows=None, t_max=T_MAX):
    """{depth, hit (bool), normal, leaf} of the host build on the library's camera rays"""
    ops, n = sp.to_ctypes(expr)
    rows = H - row0 if rows is None else rows
    cam = np.ascontiguousarray(cam14, np.float64)
    depth, hit, nrm, leaf = np.empty(W * rows), np.empty(W * rows, np.uint8), np.empty((W * rows, 3)), np.empty(W * rows, np.int32)
    why = ctypes.create_string_buffer(256)
    cfg = _cfg(0.0, t_max)
    rc = exact_lib().rme_render(ops, n, ctypes.byref(cfg), cam.ctypes.data_as(dp), W, H, row0, rows, depth.ctypes.data_as(dp),
                                hit.ctypes.data, nrm.ctypes.data_as(dp), leaf.ctypes.data, why, 256)
    assert rc == 0, (rc, why.value)
    return {"depth": depth.reshape(rows, W), "hit": hit.reshape(rows, W) > 0, "normal": nrm.reshape(rows, W, 3),
            "leaf": leaf.reshape(rows, W)}


def host_interval_render(expr, cam14, W, H, tol=1e-5, t_max=T_MAX):
    """{depth, hit (bool)} of the host interval oracle on the same rays (no prune)"""
    ops, n = sp.to_ctypes(expr)
    cam = np.ascontiguousarray(cam14, np.float64)
    depth, hit, nrm, steps = np.empty(W * H), np.empty(W * H, np.uint8), np.empty((W * H, 3)), np.empty(W * H, np.int32)
    why = ctypes.create_string_buffer(256)
    cfg = _native.interval_config(t_max=t_max, tol=tol, bound_radius=-1.0)
    rc = interval_lib().rmi_render(ops, n, ctypes.byref(cfg), -1.0, cam.ctypes.data_as(dp), W, H, 0, H, depth.ctypes.data_as(dp),
                                   hit.ctypes.data, nrm.ctypes.data_as(dp), steps.ctypes.data, why, 256)
    assert rc == 0, (rc, why.value)
    return {"depth": depth.reshape(H, W), "hit": hit.reshape(H, W) > 0}


def pointwise(expr, pts):
    """f at the points, by the pointwise interpreter"""
    ops, n = sp.to_ctypes(expr)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    out = np.empty(len(pts))
    why = ctypes.create_string_buffer(256)
    assert program_lib().rmp_eval(ops, n, pts.ctypes.data_as(dp), len(pts), out.ctypes.data_as(dp), why, 256) == 0, why.value
    return out


@functools.lru_cache(maxsize=None)
def host_frame(sid: int):
    """the host build's frame of an EXACT_IDS scene at its test size with the default camera (computed once; read only)"""
    W, H = frame_size(sid)
    return host_render(expression(sid), default_camera(W, H).params14(), W, H)


@functools.lru_cache(maxsize=None)
def host_interval_frame(sid: int):
    W, H = frame_size(sid)
    return host_interval_render(expression(sid), default_camera(W, H).params14(), W, H)


def angle(a, b):
    """the angle between unit vectors (..., 3), accurate near 0 (atan2 of |a x b| and a . b)"""
    c = np.cross(a, b)
    return np.arctan2(np.sqrt((c * c).sum(-1)), (a * b).sum(-1))


def reference_cases():
    """tests/golden/exact_reference.npz (tools/gen_exact_golden.py): {case: {scene, W, H, cam, hit, depth, normal}}"""
    z = np.load(os.path.join(GOLDEN, "exact_reference.npz"))
    out = {}
    for name in str(z["cases"]).split(";"):
        W, H = (int(v) for v in z[name + "_shape"])
        hit = np.unpackbits(z[name + "_hit"])[:W * H].reshape(H, W) > 0
        depth, normal = np.zeros((H, W)), np.zeros((H, W, 3))
        depth[hit] = z[name + "_t"]
        normal[hit] = z[name + "_n"]
        out[name] = {"scene": int(z[name + "_scene"][0]), "W": W, "H": H, "cam": z[name + "_cam"].copy(), "hit": hit,
                     "depth": depth, "normal": normal}
    return out


def camera_rays(cam14, W, H):
    """(origin (3,), unit directions (H, W, 3)) of the camera's pixel-centre rays, as analytic.camera_rays"""
    c = np.asarray(cam14, np.float64)
    u = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * c[12]
    v = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * c[13]
    d = c[3:6][None, None, :] + c[6:9][None, None, :] * u[None, :, None] + c[9:12][None, None, :] * v[:, None, None]
    return c[0:3].copy(), d / np.sqrt((d * d).sum(2, keepdims=True))
