"""The exact first hit without a GPU: csrc/rm_exact.h compiled for the host by g++ (tests/native/exact_check.cpp) against
analytic.py, against the reference's own closed forms (tests/golden/exact_reference.npz, written by
tools/gen_exact_golden.py), against the host interval oracle (tests/native/interval_check.cpp) and the pointwise
interpreter (tests/native/program_check.cpp), on constructed rays, and the host-only behaviour of the C ABI.

Measured by this file on the host build (printed by the tests, recorded in exact_cases.py and DESIGN.md section 3):
torus depth against the reference's roots 7.12e-12 at the most (asserted: 4x); t_exact - t_interval between 1.7e-8 and
4.23e-5 (asserted: <= 4x the largest); |f(p_hit)| 3.0e-14 at the most (asserted: 4x); interval-hit / exact-miss pixels: 0."""
import ctypes
import math
import subprocess
import sys

import numpy as np
import pytest

import exact_cases as ec
from conftest import ROOT

from raymarch_algo_compare_amd import _native, analytic, scoring, sweep
from raymarch_algo_compare_amd import exact_oracle as xo
from raymarch_algo_compare_amd import scene_program as sp

ref = ctypes.byref
OK, BAD_SCENE, NO_DEVICE, BAD_ARG = 0, _native.RM_E_BAD_SCENE, _native.RM_E_NO_DEVICE, _native.RM_E_BAD_ARG
INF = float("inf")


def rel(depth):
    return 1e-12 * (1.0 + depth)


# ---- against analytic.py -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", [0, 1, 2])
def test_equals_analytic_py(sid):
    """Sphere, Grazing Plane and Cube at 64x48: equal masks, |d depth| <= 1e-12 (1 + depth), normals within 1e-9 rad"""
    W, H = 64, 48
    cam = ec.default_camera(W, H)
    ex = ec.host_frame(sid)
    depth, hit, normal = analytic.analytic_depth(ec.NAMES[sid], cam)
    assert np.array_equal(ex["hit"], hit)
    gap = np.abs(ex["depth"] - depth)[hit]
    print(f"{ec.NAMES[sid]}: {int(hit.sum())} hits, max |d depth| {gap.max():.3g}")
    assert (gap <= rel(depth[hit])).all()
    assert ec.angle(ex["normal"][hit], normal[hit]).max() <= 1e-9
    assert (ex["depth"][~hit] == 0.0).all() and (ex["normal"][~hit] == 0.0).all() and (ex["leaf"][~hit] == -1).all()
    assert (ex["leaf"][hit] == 0).all()


# ---- against the reference's closed forms ----------------------------------------------------------------------------------

REFERENCE = ec.reference_cases()


@pytest.mark.parametrize("case", sorted(REFERENCE))
def test_equals_the_reference_fixture(case):
    c = REFERENCE[case]
    ex = ec.host_render(ec.expression(c["scene"]), c["cam"], c["W"], c["H"])
    assert np.array_equal(ex["hit"], c["hit"])
    hit = c["hit"]
    gap = np.abs(ex["depth"] - c["depth"])[hit]
    print(f"{case}: {int(hit.sum())} hits, max |d depth| {gap.max():.3g}")
    if c["scene"] == 3:         # the reference's eigenvalue roots carry the error: 4x the largest difference measured
        assert gap.max() <= 4.0 * ec.TORUS_DEPTH_MEASURED
    else:
        assert (gap <= rel(c["depth"][hit])).all()
    assert ec.angle(ex["normal"][hit], c["normal"][hit]).max() <= 1e-9


def test_torus_roots_are_no_worse_than_the_reference_s():
    """|sd_torus(p_hit)| over all torus fixtures: the bracketing solver's largest against the eigenvalue solver's"""
    mine = theirs = 0.0
    for name, c in REFERENCE.items():
        if c["scene"] != 3:
            continue
        ex = ec.host_render(ec.expression(3), c["cam"], c["W"], c["H"])
        o, d = ec.camera_rays(c["cam"], c["W"], c["H"])
        hit = c["hit"]
        mine = max(mine, np.abs(ec.pointwise(ec.expression(3), o + ex["depth"][hit][:, None] * d[hit])).max())
        theirs = max(theirs, np.abs(ec.pointwise(ec.expression(3), o + c["depth"][hit][:, None] * d[hit])).max())
    print(f"torus residual: {mine:.3g} (the reference's roots: {theirs:.3g})")
    assert mine <= theirs


# ---- against the host interval oracle and the pointwise interpreter ---------------------------------------------------------

@pytest.mark.parametrize("sid", ec.EXACT_IDS)
def test_agrees_with_the_host_interval_oracle(sid):
    """tol 1e-5, t_max 100, default camera: every exact hit is an interval hit; an interval hit the exact form misses lies in
    the k = 2 silhouette band; the interval depth is not later than the exact one and lags by a bounded amount"""
    ex, iv = ec.host_frame(sid), ec.host_interval_frame(sid)
    assert not (ex["hit"] & ~iv["hit"]).any()
    only = iv["hit"] & ~ex["hit"]
    assert not (only & ~scoring.silhouette_band(ex["hit"], 2)).any()
    both = ex["hit"] & iv["hit"]
    te, ti = ex["depth"][both], iv["depth"][both]
    print(f"{ec.NAMES[sid]}: {int(both.sum())} co-hits, interval-only {int(only.sum())}, t_exact - t_interval in "
          f"[{(te - ti).min():.3g}, {(te - ti).max():.3g}]")
    assert (ti <= te + rel(te)).all()
    assert (te - ti).max() <= 4.0 * ec.INTERVAL_LAG_MEASURED


def test_interval_only_pixels_are_counted():
    n = sum(int((ec.host_interval_frame(s)["hit"] & ~ec.host_frame(s)["hit"]).sum()) for s in ec.EXACT_IDS)
    print(f"interval-hit / exact-miss pixels over the eleven frames: {n}")
    assert n == ec.INTERVAL_ONLY_PIXELS


@pytest.mark.parametrize("sid", ec.EXACT_IDS)
def test_the_hit_is_a_root_of_the_program(sid):
    W, H = ec.frame_size(sid)
    ex = ec.host_frame(sid)
    o, d = ec.camera_rays(ec.default_camera(W, H).params14(), W, H)
    f = np.abs(ec.pointwise(ec.expression(sid), o + ex["depth"][ex["hit"]][:, None] * d[ex["hit"]]))
    print(f"{ec.NAMES[sid]}: max |f(p_hit)| {f.max():.3g}")
    assert f.max() <= 4.0 * ec.ROOT_RESIDUAL_MEASURED


def test_normals_face_the_ray_on_entry():
    """outward normals: every pixel of these frames is an entry (the eye is outside), so n . d < 0 up to grazing"""
    for sid in ec.EXACT_IDS:
        W, H = ec.frame_size(sid)
        ex = ec.host_frame(sid)
        _, d = ec.camera_rays(ec.default_camera(W, H).params14(), W, H)
        nd = (ex["normal"] * d).sum(-1)[ex["hit"]]
        assert (nd <= 1e-9).all(), ec.NAMES[sid]
        assert np.abs(np.sqrt((ex["normal"] ** 2).sum(-1))[ex["hit"]] - 1.0).max() <= 1e-12


# ---- constructed rays ----------------------------------------------------------------------------------------------------

def one(expr, o, d, **kw):
    t, n, leaf = ec.host_march(expr, o, [d], **kw)
    return float(t[0]), n[0], int(leaf[0])


def test_tangent_contact_counts():
    """Near Miss's spheres moved to touch at the origin: the ray through the contact point has discriminant 0 on both"""
    touching = sp.op_union(sp.op_translate((-1.0, 0.0, 0.0), sp.sd_sphere(1.0)), sp.op_translate((1.0, 0.0, 0.0), sp.sd_sphere(1.0)))
    t, n, leaf = one(touching, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert t == 5.0 and leaf == 1
    assert np.allclose(n, (1.0, 0.0, 0.0), atol=0) or np.allclose(n, (-1.0, 0.0, 0.0), atol=0)
    assert one(touching, (0.0, 1e-3, 5.0), (0.0, 0.0, -1.0))[0] == INF


def test_eye_inside_a_box_hits_the_exit_face():
    t, n, _ = one(sp.sd_box((1.0, 2.0, 3.0)), (0.25, 0.5, 0.0), (0.0, 0.0, -1.0))
    assert t == 3.0 and tuple(n) == (0.0, 0.0, -1.0)
    t, n, _ = one(sp.sd_box((1.0, 2.0, 3.0)), (0.25, 0.5, 0.0), (1.0, 0.0, 0.0))
    assert t == 0.75 and tuple(n) == (1.0, 0.0, 0.0)


def test_eye_inside_the_removed_sphere_of_hollow_cube():
    """from the centre the removed sphere (radius 1.3) reaches past the faces (1.0) but not the edges: along an axis nothing
    is left, towards an edge the shell begins on the sphere (normal towards the eye) and ends on the box"""
    hollow = ec.expression(6)
    assert one(hollow, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))[0] == INF
    d = np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0)
    t, n, leaf = one(hollow, (0.0, 0.0, 0.0), d)
    assert abs(t - 1.3) <= 1e-15 and leaf == 1
    assert ec.angle(n, -d) <= 1e-12
    t, n, leaf = one(hollow, (0.0, 0.0, 0.0), d, t_min=1.31)
    assert abs(t - math.sqrt(2.0)) <= 1e-15 and leaf == 0


def test_ray_parallel_to_a_box_slab():
    box = sp.sd_box((1.0, 1.0, 1.0))
    t, n, _ = one(box, (0.5, 0.5, 5.0), (0.0, 0.0, -1.0))             # inside the x and y slabs
    assert t == 4.0 and tuple(n) == (0.0, 0.0, 1.0)
    assert one(box, (1.5, 0.5, 5.0), (0.0, 0.0, -1.0))[0] == INF      # outside the x slab
    assert one(box, (1.0, 0.5, 5.0), (0.0, 0.0, -1.0))[0] == 4.0      # on its face: the slab is closed


def test_direction_is_used_as_given():
    for s in (0.5, 3.0, 1e-3):
        t, n, _ = one(ec.expression(0), (0.0, 0.0, 5.0), (0.0, 0.0, -s))
        assert abs(t - 4.0 / s) <= 1e-15 * (4.0 / s) and tuple(n) == (0.0, 0.0, 1.0)
    assert one(ec.expression(0), (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))[0] == INF


def test_t_max_and_t_min_cut_at_a_root():
    sphere = ec.expression(0)
    o, d = (0.0, 0.0, 5.0), (0.0, 0.0, -1.0)
    assert one(sphere, o, d, t_max=4.0)[0] == 4.0                       # t <= t_max
    assert one(sphere, o, d, t_max=math.nextafter(4.0, 0.0))[0] == INF
    assert one(sphere, o, d, t_min=4.0)[0] == 6.0                       # t > t_min: the exit
    assert one(sphere, o, d, t_min=math.nextafter(4.0, 0.0))[0] == 4.0
    assert one(sphere, o, d, t_min=4.0, t_max=5.9)[0] == INF


def test_subtracting_a_solid_from_itself_leaves_the_shell():
    a = sp.op_translate((0.25, 0.0, 0.0), sp.sd_sphere(1.0))
    t, _, _ = one(sp.op_subtract(a, a), (0.25, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert t == 4.0
    assert one(sp.op_subtract(a, a), (0.25, 0.0, 5.0), (0.0, 0.0, -1.0), t_min=4.0)[0] == 6.0


def test_nested_onion_radii_are_exactly_ordered():
    """Onion Shell along an axis: shells |r - 2| in [0.05, 0.15], boundaries at 2.15, 2.05, 1.95, 1.85; the seams at 2.1 and
    1.9, where two level ranges meet, are no boundaries"""
    onion = ec.expression(8)
    o, d = (0.0, 0.0, 5.0), (0.0, 0.0, -1.0)
    want = [(2.0 + 0.1) + 0.05, (2.0 + 0.1) - 0.05, (2.0 - 0.1) + 0.05, (2.0 - 0.1) - 0.05]
    t_min, got, signs = 0.0, [], []
    for _ in range(8):
        t, n, _ = one(onion, o, d, t_min=t_min)
        got.append(t)
        signs.append(n[2])
        t_min = t
    radii = [abs(5.0 - t) for t in got]
    assert got == sorted(got) and len(set(got)) == 8
    for r, w in zip(radii[:4], want):
        assert abs(r - w) <= 4e-16 * 5.0
    assert np.abs(np.array(radii[4:]) - radii[3::-1]).max() <= 4e-16 * 5.0      # (5 - t and t - 5 round on their own)
    assert signs == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0]      # outward of the shell: outer side, inner side, ...
    assert one(onion, o, d, t_min=got[-1])[0] == INF


def test_full_stacks():
    """eight leaves on the value stack and four nested translates: a row of unit-spaced spheres, each reached through one
    more translate than the one before"""
    def sphere_at(i):
        return sp.op_translate((float(i), 0.0, 0.0), sp.sd_sphere(0.25))
    leaves = [sp.op_translate((1.0, 0.0, 0.0), sp.op_translate((1.0, 0.0, 0.0), sp.op_translate(
        (1.0, 0.0, 0.0), sp.op_translate((1.0, 0.0, 0.0), sp.sd_sphere(0.25)))))] + [sphere_at(i) for i in (0, 1, 2, 3, 5, 6, 7)]

    def fold(xs):                  # right-nested unions: all eight values are on the stack before the first union
        return xs[0] if len(xs) == 1 else sp.op_union(xs[0], fold(xs[1:]))
    row = fold(leaves)
    assert ec.host_supported(row) == (1, "")
    for i in range(8):
        t, n, _ = one(row, (float(i), 0.0, 5.0), (0.0, 0.0, -1.0))
        assert t == 4.75 and tuple(n) == (0.0, 0.0, 1.0), i
    assert one(row, (0.5, 0.0, 5.0), (0.0, 0.0, -1.0))[0] == INF
    t, _, _ = one(row, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    assert t == 2.75


def test_capsule_cylinder_and_torus_leaves():
    cap = sp.sd_capsule((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.5)
    assert one(cap, (0.3, 0.0, 5.0), (0.0, 0.0, -1.0))[0] == 4.5                     # the side
    assert abs(one(cap, (-5.0, 0.0, 0.0), (1.0, 0.0, 0.0))[0] - 3.5) <= 1e-15         # an end sphere
    assert one(cap, (1.6, 0.0, 5.0), (0.0, 0.0, -1.0))[0] == INF
    t, n, _ = one(sp.op_round(cap, 0.25), (0.3, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert t == 4.25 and tuple(n) == (0.0, 0.0, 1.0)
    cyl = ec.expression(4)                                                             # radius 1, half height 1.5
    t, n, _ = one(cyl, (0.0, 5.0, 0.0), (0.0, -1.0, 0.0))
    assert t == 3.5 and tuple(n) == (0.0, 1.0, 0.0)                                   # along the axis: the cap
    t, n, _ = one(cyl, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert t == 4.0 and tuple(n) == (0.0, 0.0, 1.0)
    tor = sp.sd_torus(1.5, 0.25)
    ts, t_min = [], 0.0
    for _ in range(4):                                                                 # through both tubes
        t, _, _ = one(tor, (5.0, 0.0, 0.0), (-1.0, 0.0, 0.0), t_min=t_min)
        ts.append(t)
        t_min = t
    assert np.abs(np.array(ts) - [3.25, 3.75, 6.25, 6.75]).max() <= 2e-15
    assert one(tor, (0.0, 5.0, 0.0), (0.0, -1.0, 0.0))[0] == INF                      # through the hole


# ---- the support check -----------------------------------------------------------------------------------------------------

S = sp.sd_sphere(1.0)
REFUSED = [
    ("smooth union", sp.op_smooth_union(S, S, 0.5), "a smooth combinator has no exact form"),
    ("smooth subtract", sp.op_smooth_subtract(S, S, 0.5), "a smooth combinator has no exact form"),
    ("smooth intersect", sp.op_smooth_intersect(S, S, 0.5), "a smooth combinator has no exact form"),
    ("repeat", sp.op_repeat((2.0, 0.0, 2.0), S), "a repeat needs a cell traversal"),
    ("limited repeat", sp.op_limited_repeat((1.0, 1.0, 1.0), (2.0, 2.0, 2.0), S), "a repeat needs a cell traversal"),
    ("cone", sp.sd_cone(0.5, 1.0), "sd_cone has no exact form"),
    ("capped torus", sp.sd_capped_torus((math.sin(2.0), math.cos(2.0)), 1.2, 0.2), "sd_capped_torus has no exact form"),
    ("menger cross", sp.op_intersect(S, sp.sd_menger_cross(1.0)), "sd_menger_cross has no exact form"),
    ("gyroid", sp.op_intersect(sp.sd_gyroid(3.0, 10.0), S), "sd_gyroid has no exact form"),
    ("round over a box", sp.op_round(sp.sd_box((1.0, 1.0, 1.0)), 0.1), "op_round over a box, which is cut at level 0 only"),
    ("onion over a box", sp.op_onion(sp.sd_box((1.0, 1.0, 1.0)), 0.1), "op_onion over a box, which is cut at level 0 only"),
    ("round over a cylinder", sp.op_round(sp.sd_cylinder(1.0, 1.0), 0.1), "op_round over a cylinder, which is cut at level 0 only"),
    ("onion over a cylinder", sp.op_onion(sp.sd_cylinder(1.0, 1.0), 0.1), "op_onion over a cylinder, which is cut at level 0 only"),
    ("scale over a box", sp.op_scale(sp.sd_box((1.0, 1.0, 1.0)), 2.0), "op_scale over a box, which is cut at level 0 only"),
    ("round over a union", sp.op_round(sp.op_union(S, S), 0.1), "op_round over a combinator's result"),
    ("four onions", sp.op_onion(sp.op_onion(sp.op_onion(sp.op_onion(S, 0.2), 0.1), 0.05), 0.02), "more than 3 onions over one leaf"),
    ("a torus without a hole", sp.op_round(sp.sd_torus(1.0, 0.5), 0.5), "the torus is cut where its tube closes the hole"),
]


@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_programs_carry_their_reason(row):
    _, expr, reason = row
    rc, why = ec.host_supported(expr)
    assert rc == 0 and reason in why, why
    ops, nops = sp.to_ctypes(expr)
    L = _native.load()
    sid = ctypes.c_int32(-1)
    assert L.rm_scene_program_create(ops, nops, 1.0, ref(sid)) == OK
    try:
        assert L.rm_exact_supported(sid.value) == 0 and reason.encode() in L.rm_last_error()
        assert L.rm_exact_march_rays(sid.value, None, None, None, 4, None, None, None) == BAD_SCENE
        assert reason.encode() in L.rm_last_error()
    finally:
        assert L.rm_scene_program_destroy(sid.value) == OK


def test_supported_programs():
    for expr in (ec.mixed_program(), sp.op_round(sp.op_onion(sp.op_scale(sp.sd_torus(1.5, 0.1), 2.0), 0.05), 0.01),
                 sp.op_translate((1.0, 0.0, 0.0), sp.op_onion(sp.sd_plane((0.0, 1.0, 0.0), 0.0), 0.1))):
        assert ec.host_supported(expr) == (1, "")


def test_exact_supported_over_the_catalogue_and_a_live_program():
    L = _native.load()
    assert [s for s in range(20) if L.rm_exact_supported(s) == 1] == [0, 1, 2, 3, 4, 5, 6, 8, 14]
    assert [L.rm_exact_supported(s) for s in (-1, 20, 99, 5000)] == [0, 0, 0, 0]
    assert xo.has_exact("Sphere") and xo.has_exact(6) and not xo.has_exact("Metaballs") and not xo.has_exact("no such scene")
    assert xo.why_not("Onion Shell") is None and "smooth combinator" in xo.why_not("Metaballs")
    assert "no composition of primitives" in xo.why_not("Mandelbulb")
    ops, nops = sp.to_ctypes(ec.mixed_program())
    sid = ctypes.c_int32(-1)
    assert L.rm_scene_program_create(ops, nops, 1.0, ref(sid)) == OK
    assert L.rm_exact_supported(sid.value) == 1
    assert L.rm_scene_program_destroy(sid.value) == OK
    assert L.rm_exact_supported(sid.value) == 0 and b"does not exist" in L.rm_last_error()
    assert L.rm_exact_march_rays(sid.value, None, None, None, 4, None, None, None) == BAD_SCENE


def test_the_twins_of_11_and_15_have_an_exact_form():
    for sid in ec.TWIN_IDS:
        assert ec.host_supported(ec.expression(sid)) == (1, "")
    assert ec.host_supported(sp.catalogue_twins()[9])[0] == 0


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------

def test_config_layout_matches_gcc():
    L = ec.exact_lib()
    assert ctypes.sizeof(_native.RmExactConfig) == L.rme_sizeof_config() == 24
    for i, name in enumerate(("t_min", "t_max", "reserved")):
        assert getattr(_native.RmExactConfig, name).offset == L.rme_offsetof_config(i), name


def _desc(scene=0, **kw):
    cam = np.asarray(ec.default_camera(16, 12).params14(), np.float64)
    return _native.make_desc(scene, 0, cam, kw.pop("w", 16), kw.pop("h", 12), kw.pop("row0", 0), kw.pop("rows", None))


def _bad_cfgs():
    for field, v in (("t_min", -1.0), ("t_min", math.nan), ("t_max", -1e-300), ("t_max", math.nan)):
        c = _native.RmExactConfig()
        setattr(c, field, v)
        yield f"{field} {v}", c, f"RmExactConfig: {field} is negative or NaN"
    for i in (0, 1):
        c = _native.RmExactConfig()
        c.reserved[i] = 1
        yield f"reserved[{i}]", c, "RmExactConfig: reserved must be 0"


def test_bad_arguments_and_scenes_come_without_a_device():
    L = _native.load()
    for what, cfg, text in _bad_cfgs():
        assert L.rm_exact_march_rays(0, ref(cfg), None, None, 4, None, None, None) == BAD_ARG, what
        assert text.encode() in L.rm_last_error(), (what, L.rm_last_error())
        assert L.rm_exact_render(ref(_desc()), ref(cfg), None, None, None, None, None) == BAD_ARG, what
    for scene in (7, 9, 12, 17, 19, 20, -1, 99, 4096):
        assert L.rm_exact_march_rays(scene, None, None, None, 4, None, None, None) == BAD_SCENE, scene
        assert L.rm_exact_render(ref(_desc(scene)), None, None, None, None, None, None) == BAD_SCENE, scene
    # the scene is looked at before the configuration
    bad = next(_bad_cfgs())[1]
    assert L.rm_exact_march_rays(7, ref(bad), None, None, 4, None, None, None) == BAD_SCENE
    assert L.rm_exact_render(None, None, None, None, None, None, None) == BAD_ARG and b"desc is NULL" in L.rm_last_error()


NO_DEVICE_SCRIPT = """
import ctypes, sys
import numpy as np
from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd.camera import Camera
L = _native.load()
cam = np.asarray(Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 16, 12).params14(), np.float64)
d = _native.make_desc(0, 0, cam, 16, 12, 0, None)
got = [L.rm_exact_march_rays(0, None, None, None, 4, None, None, None),
       L.rm_exact_render(ctypes.byref(d), None, None, None, None, None, None),
       L.rm_exact_march_rays(7, None, None, None, 4, None, None, None)]
print(got)
sys.exit(0 if got == [_native.RM_E_NO_DEVICE, _native.RM_E_NO_DEVICE, _native.RM_E_BAD_SCENE] else 1)
"""


def test_no_device_from_a_fresh_process():
    """a process that sees no device (none present, or all hidden from it): the calls that pass the scene and argument
    checks return RM_E_NO_DEVICE"""
    import os
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", NO_DEVICE_SCRIPT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout, out.stderr)


def test_sweep_accepts_the_exact_oracle_and_refuses_an_unknown_one():
    assert sweep.ORACLES == ("interval", "exact")
    with pytest.raises(ValueError, match="unknown oracle"):
        sweep.run_sweep(["Sphere"], ["Standard"], oracle="analytic")
    with pytest.raises(SystemExit):
        sweep.main(["--oracle", "analytic"])
    # accepted: the next check (an unknown scene) is reached, still before the device
    with pytest.raises(KeyError, match="unknown scene"):
        sweep.run_sweep(["no such scene"], ["Standard"], oracle="exact")


def test_a_negative_half_extent_is_the_empty_set():
    """sd_box with a negative half extent and sd_cylinder with a negative half height are positive everywhere: no hit on a
    diagonal ray through where the solid of the absolute values would be, and none along the axes"""
    o, d = np.array([3.0, 2.5, 3.5]), -np.array([3.0, 2.5, 3.5]) / np.linalg.norm([3.0, 2.5, 3.5])
    for expr in (sp.sd_box((-0.5, 1.0, 1.0)), sp.sd_box((1.0, -0.5, 1.0)), sp.sd_box((1.0, 1.0, -0.5)), sp.sd_cylinder(1.0, -0.5),
                 sp.sd_cylinder(-1.0, 0.5)):
        assert ec.host_supported(expr) == (1, "")
        assert (ec.pointwise(expr, o + np.linspace(0.0, 10.0, 101)[:, None] * d) > 0.0).all()
        for oo, dd in ((o, d), ((0.0, 0.0, 5.0), (0.0, 0.0, -1.0)), ((0.0, 5.0, 0.0), (0.0, -1.0, 0.0)), ((5.0, 0.0, 0.0), (-1.0, 0.0, 0.0))):
            assert one(expr, oo, dd)[0] == INF
    # ... and takes nothing away, or everything, as an operand
    assert one(sp.op_subtract(S, sp.sd_box((-0.5, 1.0, 1.0))), (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))[0] == 4.0
    assert one(sp.op_intersect(S, sp.sd_cylinder(1.0, -0.5)), (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))[0] == INF


def test_capsule_normal_on_a_segment_shorter_than_its_clamp():
    """sd_capsule divides by max(|ab|^2, 1e-12): the gradient uses the same projection, so a nearly degenerate capsule's
    normal is the one of its distance function"""
    cap = sp.sd_capsule((0.0, 0.0, 0.0), (1e-7, 0.0, 0.0), 1.0)
    t, n, _ = one(cap, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert abs(t - 4.0) <= 1e-12 and ec.angle(n, np.array([0.0, 0.0, 1.0])) <= 1e-6
