"""User-defined scenes (scene programs) without a GPU: the builder, its JSON and its encoding, the library's validation
of programs (rm_scene_program_create needs no device), the name rules of registration, the RmSceneOp layout, and the
interpreter of csrc/rm_scene_program.h compiled for the host by g++ (tests/native/program_check.cpp) against the
reference's own values (tests/golden/programs_*, written by tools/gen_program_golden.py)."""
import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, build_native

from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import scene_program as sp


def _trees():
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        return json.load(f)


def _fixture_points():
    """tools/program_fixture_points.py: the fixture stores results only, the points are rebuilt here"""
    spec = importlib.util.spec_from_file_location("program_fixture_points",
                                                  os.path.join(ROOT, "tools", "program_fixture_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sdf_fixture():
    """[(tree, points, sha256 of all results, bits of the first results)] of tests/golden/programs_sdf.npz"""
    fp = _fixture_points()
    z = np.load(os.path.join(GOLDEN, "programs_sdf.npz"))
    n = int(z["npoints"][0])
    out = []
    for i, t in enumerate(_trees()["trees"]):
        pts = fp.fixture_points(i, n)
        assert fp.sha256_f64(pts) == z[f"t{i}_pts_sha"].tobytes(), f"the fixture points of tree {i} have drifted"
        out.append((t, pts, z[f"t{i}_sha"].tobytes(), z[f"t{i}_bits"]))
    return out, fp.sha256_f64


def _ops(rows):
    """RmSceneOp array from [(op, [f...], arg)] rows (arg optional)."""
    arr = (_native.RmSceneOp * max(1, len(rows)))()
    for i, row in enumerate(rows):
        arr[i].op = row[0]
        arr[i].arg = row[2] if len(row) > 2 else 0
        for j, v in enumerate(row[1]):
            arr[i].f[j] = v
    return arr


@pytest.fixture
def registered():
    """Register scenes through this fixture: every one is unregistered (and its program destroyed) at teardown."""
    names = []

    def reg(name, expr, **kw):
        info = sp.register_scene(name, expr, **kw)
        names.append(name)
        return info

    yield reg
    for n in names:
        if registry.find_program_scene(n) is not None:
            sp.unregister_scene(n)


# ---- builder, JSON, encoding ------------------------------------------------------------------------------------------

def two_boxes():
    return sp.op_smooth_union(sp.sd_box((1, 1, 1)), sp.op_translate((1.5, 0, 0), sp.sd_sphere(0.7)), 0.3)


def test_encoding_is_postfix_with_point_pops():
    assert sp.compile_ops(two_boxes()) == [
        (1, (1.0, 1.0, 1.0)), (14, (1.5, 0.0, 0.0)), (0, (0.7,)), (16, ()), (11, (0.3,))]
    e = sp.op_onion(sp.op_repeat((0, 0.5, 0), sp.sd_plane((0, 1, 0), 0.0)), 0.01)
    assert sp.compile_ops(e) == [(15, (0.0, 0.5, 0.0)), (2, (0.0, 1.0, 0.0, 0.0)), (16, ()), (18, (0.01,))]
    # sd_cone: cos / sin of the angle by Python's math (the reference's libm), then the height
    assert sp.compile_ops(sp.sd_cone(0.4, 1.5)) == [(7, (math.cos(0.4), math.sin(0.4), 1.5))]
    assert [o for o, _ in sp.compile_ops(sp.op_subtract(sp.sd_sphere(1), sp.op_round(sp.sd_torus(1, .2), .1)))] == [0, 4, 17, 9]


def test_json_round_trip():
    e = two_boxes()
    assert sp.loads(sp.dumps(e)) == e
    for t in _trees()["trees"]:
        assert sp.expr_from_json(t).to_json() == t
    with pytest.raises(ValueError):
        sp.expr_from_json({"op": "sd_sphere"})                      # missing radius
    with pytest.raises(ValueError):
        sp.expr_from_json({"op": "sd_sphere", "radius": 1.0, "r": 2.0})
    with pytest.raises(ValueError):
        sp.expr_from_json({"op": "op_twist", "child": {"op": "sd_sphere", "radius": 1.0}})
    with pytest.raises(TypeError):
        sp.sd_box((1, 1))


def test_scene_op_ctypes_layout_matches_header():
    L = ctypes.CDLL(build_native("program_check"))
    L.rmp_sizeof_op.restype = L.rmp_offsetof_f.restype = ctypes.c_size_t
    assert ctypes.sizeof(_native.RmSceneOp) == L.rmp_sizeof_op() == 72
    assert _native.RmSceneOp.f.offset == L.rmp_offsetof_f() == 8


# ---- validation (the library, no device) ------------------------------------------------------------------------------

SPHERE = (0, [1.0])
UNION = (8, [])
TRANSLATE = (14, [0.5, 0.0, 0.0])
POP = (16, [])

BAD_PROGRAMS = {
    "empty": [],
    "too long": [SPHERE] + [(17, [0.01])] * 256,
    "opcode below range": [(-1, [])],
    "opcode above range": [(19, [])],
    "reserved arg": [(0, [1.0], 7)],
    "nan constant": [(0, [float("nan")])],
    "inf constant": [(1, [1.0, float("inf"), 1.0])],
    "unused constant set": [(0, [1.0, 2.0])],
    "value stack overflow": [SPHERE] * 9 + [UNION] * 8,
    "combinator underflow": [SPHERE, UNION],
    "modifier on empty stack": [(17, [0.1])],
    "two values left": [SPHERE, SPHERE],
    "point stack overflow": [TRANSLATE] * 5 + [SPHERE] + [POP] * 5,
    "pop without transform": [SPHERE, POP],
    "open transform": [TRANSLATE, SPHERE],
    "smooth k zero": [SPHERE, SPHERE, (11, [0.0])],
}


@pytest.mark.parametrize("case", sorted(BAD_PROGRAMS))
def test_malformed_programs_are_rejected_on_the_host(case):
    rows = BAD_PROGRAMS[case]
    L = _native.load()
    sid = ctypes.c_int32(-1)
    rc = L.rm_scene_program_create(_ops(rows), len(rows), 1.0, ctypes.byref(sid))
    assert rc == -6, (case, rc)
    assert L.rm_last_error().decode()
    assert sid.value == -1


def test_limits_are_accepted_and_ids_are_never_reused():
    L = _native.load()
    ok = [[SPHERE] * 8 + [UNION] * 7, [TRANSLATE] * 4 + [SPHERE] + [POP] * 4, [SPHERE] + [(17, [0.01])] * 255]
    ids = []
    for rows in ok:
        ids.append(_native.scene_program_create(_ops(rows), len(rows), 1.0))
    assert all(i >= _native.RM_SCENE_PROGRAM_BASE for i in ids) and ids == sorted(ids) and len(set(ids)) == 3
    for i in ids:
        _native.scene_program_destroy(i)
    with pytest.raises(_native.RmError) as e:
        _native.scene_program_destroy(ids[0])
    assert e.value.code == -1
    again = _native.scene_program_create(_ops([SPHERE]), 1, 1.0)
    assert again > ids[-1]
    _native.scene_program_destroy(again)
    for lip in (0.0, -1.0, float("nan"), float("inf")):
        sid = ctypes.c_int32(-1)
        assert L.rm_scene_program_create(_ops([SPHERE]), 1, lip, ctypes.byref(sid)) == -6
    assert L.rm_scene_program_create(None, 1, 1.0, ctypes.byref(ctypes.c_int32())) == -6
    assert L.rm_num_scenes() == 20


def test_native_encoder_agrees_with_the_library():
    """The g++ build of program_encode accepts and rejects exactly what the library does."""
    L = ctypes.CDLL(build_native("program_check"))
    L.rmp_sizeof_image.restype = ctypes.c_size_t
    img = ctypes.create_string_buffer(L.rmp_sizeof_image())
    why = ctypes.create_string_buffer(256)
    for case, rows in BAD_PROGRAMS.items():
        assert L.rmp_encode(_ops(rows), len(rows), img, why, 256) == -1, case
    assert L.rmp_encode(_ops([SPHERE]), 1, img, why, 256) == 0


# ---- registration and names -----------------------------------------------------------------------------------------

def test_names_of_registered_scenes(registered):
    n0 = len(registry.get_all_scenes())
    for clash in ("Sphere", "sphere", "S phere", "HOLLOWCUBE(CSG)", "Menger Sponge (iter=3)"):
        with pytest.raises(ValueError):
            registered(clash, sp.sd_sphere(1.0))
    info = registered("Two Boxes", two_boxes(), lipschitz=1.0, camera_position=(0, 1, 6))
    assert info.id >= _native.RM_SCENE_PROGRAM_BASE
    assert registry.get_scene_by_name("two boxes") is info
    assert registry.get_scene_by_name("TwoB") is info               # starts-with, after the catalogue's names
    assert registry.get_scene_by_name("Sph").name == "Sphere"       # the catalogue first
    assert registry.find_scene_exact("Two Boxes") is info and registry.get_scene_by_id(info.id) is info
    assert info.suggested_camera().camera_position == (0.0, 1.0, 6.0)
    with pytest.raises(ValueError):
        registered("twoboxes", sp.sd_sphere(1.0))
    assert len(registry.get_all_scenes()) == n0 == len(registry.SCENES) == 20
    with pytest.raises(ValueError):                                  # the library refuses the program
        registered("Too Deep", sp.op_union(sp.sd_sphere(1), sp.op_union(sp.sd_sphere(1), sp.op_union(
            sp.sd_sphere(1), sp.op_union(sp.sd_sphere(1), sp.op_union(sp.sd_sphere(1), sp.op_union(sp.sd_sphere(1), sp.op_union(
                sp.sd_sphere(1), sp.op_union(sp.sd_sphere(1), sp.sd_sphere(1))))))))))
    assert registry.get_scene_by_name("Too Deep") is None
    sp.unregister_scene("Two Boxes")
    assert registry.get_scene_by_name("Two Boxes") is None
    with pytest.raises(KeyError):
        sp.unregister_scene("Two Boxes")


def test_scene_file_round_trip(registered, tmp_path):
    registered("Two Boxes", two_boxes(), description="smooth union", camera_position=(0, 0, 6), camera_target=(0.5, 0, 0))
    path = str(tmp_path / "s.json")
    sp.save_scene_file(path, ["Two Boxes"])
    expr = sp.expression_of("Two Boxes")
    sp.unregister_scene("Two Boxes")
    infos = sp.load_scene_file(path)
    try:
        assert [i.name for i in infos] == ["Two Boxes"]
        assert sp.expression_of("Two Boxes") == expr == two_boxes()
        assert infos[0].camera_target == (0.5, 0.0, 0.0) and infos[0].description == "smooth union"
    finally:
        sp.unregister_scene("Two Boxes")


# ---- the interpreter, host build, against the reference's values -----------------------------------------------------

def test_host_interpreter_matches_reference_bits():
    L = ctypes.CDLL(build_native("program_check"))
    dp = ctypes.POINTER(ctypes.c_double)
    cases, sha = sdf_fixture()
    assert len(cases) >= 40 and all(len(c[1]) == 2000 for c in cases)
    why = ctypes.create_string_buffer(256)
    for i, (t, xyz, want_sha, want_bits) in enumerate(cases):
        arr, n = sp.to_ctypes(sp.expr_from_json(t))
        xyz = np.ascontiguousarray(xyz)
        out = np.empty(len(xyz))
        assert L.rmp_eval(arr, n, xyz.ctypes.data_as(dp), len(xyz), out.ctypes.data_as(dp), why, 256) == 0, why.value
        k = len(want_bits)
        bad = np.flatnonzero(out[:k].view(np.uint64) != want_bits)
        assert bad.size == 0, (i, bad.size, xyz[bad[0]], out[bad[0]], want_bits[bad[0]].view(np.float64))
        assert sha(out) == want_sha, (i, "a result beyond the stored bits differs")


def test_fixture_trees_cover_every_op():
    seen = set()

    def walk(n):
        seen.add(n["op"])
        for k in sp._SPEC[n["op"]][1]:          # subtree fields (sd_capsule's a / b are points)
            walk(n[k])
    for t in _trees()["trees"]:
        walk(t)
    assert seen == set(sp.OPCODES) - {"pop_point"}


def test_restated_catalogue_scenes_match_reference_bits():
    """The 14 catalogue scenes restated as programs (scene_program.catalogue_expressions) give the reference's own
    values (tests/golden/sdf_points.npz, oracle/gen_golden.py) through the host build of the interpreter."""
    L = ctypes.CDLL(build_native("program_check"))
    dp = ctypes.POINTER(ctypes.c_double)
    z = np.load(os.path.join(GOLDEN, "sdf_points.npz"))
    xyz = np.ascontiguousarray(z["pts"])
    why = ctypes.create_string_buffer(256)
    exprs = sp.catalogue_expressions()
    assert sorted(exprs) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 17, 19]
    for sid, e in exprs.items():
        arr, n = sp.to_ctypes(e)
        out = np.empty(len(xyz))
        assert L.rmp_eval(arr, n, xyz.ctypes.data_as(dp), len(xyz), out.ctypes.data_as(dp), why, 256) == 0, why.value
        assert (out.view(np.uint64) == z[f"s{sid}"].view(np.uint64)).all(), registry.SCENES[sid].name
