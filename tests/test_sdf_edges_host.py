"""The 20 scene SDFs at their edge points, without a GPU: the oracle (oracle/rm_oracle.c), the host build of the kernel
headers (tests/native/host_check.cpp) and the host build of the program interpreter (tests/native/program_check.cpp: the
14 restated scenes and the 5 twins) against what the REFERENCE computes at tests/golden/sdf_edges.npz, and the oracle's and
the headers' march against the reference's own march() from such points (tests/golden/rays_edges.npz; both written by
oracle/gen_golden.py --only sdf_edges / ray_edges, layout in tests/sdf_edge_cases.py).  Bit for bit, NaN as one class.

Where the reference raises there is no value to pin; there the three builds are held to each other.  Capped Torus on the
centre circle of its tube (p.p + ra^2 - 2 ra k rounds below zero, the reference's `** 0.5` goes complex): all three
return NaN (include/rm_hip.h).  Gyroid beyond the sincos cut: the headers return NaN by contract,
the oracle calls libm as the reference does."""
import ctypes

import numpy as np
import pytest

import sdf_edge_cases as ec
from conftest import build_native
from oracle import oracle

from raymarch_algo_compare_amd import scene_program as sp

DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def E():
    return ec.edges()


@pytest.fixture(scope="module")
def hostlib():
    L = ctypes.CDLL(build_native("host_check"))
    L.rmh_sdf_eval.argtypes = [ctypes.c_int, DP, ctypes.c_size_t, DP]
    L.rmh_march_rays.argtypes = ([ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.c_int, DP, DP, ctypes.c_size_t]
                                 + [ctypes.c_void_p, DP, ctypes.c_void_p, DP, DP])
    return L


def headers_sdf(L, sid, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.empty(len(pts))
    assert L.rmh_sdf_eval(sid, pts.ctypes.data_as(DP), len(pts), out.ctypes.data_as(DP)) == 0
    return out


@pytest.fixture(scope="module")
def interpreter():
    L = ctypes.CDLL(build_native("program_check"))
    why = ctypes.create_string_buffer(256)
    exprs = {**sp.catalogue_expressions(), **sp.catalogue_twins()}
    assert sorted(exprs) == sorted(ec.RESTATED + ec.TWINS)

    def run(sid, pts):
        arr, n = sp.to_ctypes(exprs[sid])
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        out = np.empty(len(pts))
        assert L.rmp_eval(arr, n, pts.ctypes.data_as(DP), len(pts), out.ctypes.data_as(DP), why, 256) == 0, why.value
        return out
    return run


# ---- against the fixture -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", range(ec.NSCENES))
def test_oracle_matches_reference(E, sid):
    got = oracle.sdf_eval(sid, E.pts)
    # the oracle calls libm where the reference does, so it is held to the reference beyond the sincos cut as well
    report = ec.mismatches(E, sid, got, where=~E.raised[sid])
    assert not report, "oracle\n" + report


@pytest.mark.parametrize("sid", range(ec.NSCENES))
def test_kernel_headers_match_reference(E, hostlib, sid):
    report = ec.mismatches(E, sid, headers_sdf(hostlib, sid, E.pts))
    assert not report, "kernel headers\n" + report


@pytest.mark.parametrize("sid", ec.RESTATED + ec.TWINS)
def test_interpreter_matches_reference(E, interpreter, sid):
    report = ec.mismatches(E, sid, interpreter(sid, E.pts))
    assert not report, "program interpreter\n" + report


def _cells(march):
    R = ec.rays()
    bad = []
    for sid in range(ec.NSCENES):
        for kid in range(ec.NSTRATEGIES):
            for bi, b in enumerate(R["budgets"]):
                hit, t, it, fs = march(sid, kid, R["o"], R["d"], b, float(R["lip"][sid, kid]))
                if ec.cell_hash(hit, it, t, fs) != R["sha"][sid, kid, bi].tobytes():
                    bad.append((sid, kid, b))
    return bad


def test_oracle_rays_match_reference():
    bad = _cells(lambda sid, kid, o, d, b, lip: oracle.march_rays(sid, kid, o, d, max_iterations=b, lipschitz=lip))
    assert not bad, ("(scene, strategy, budget) cells whose hash differs from the reference's", bad[:20], len(bad))


def test_kernel_headers_rays_match_reference(hostlib):
    prm = np.array([float(oracle.DEFAULT_PARAMS[n]) for n, _, _ in oracle.PARAM_FIELDS])

    def march(sid, kid, o, d, b, lip):
        n = len(o)
        hit, t, it, fs = np.empty(n, np.uint8), np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.float64)
        rc = hostlib.rmh_march_rays(sid, kid, b, 1e-4, 100.0, lip, 1, o.ctypes.data_as(DP), d.ctypes.data_as(DP), n, hit.ctypes.data,
                                    t.ctypes.data_as(DP), it.ctypes.data, fs.ctypes.data_as(DP), prm.ctypes.data_as(DP))
        assert rc == 0
        return hit, t, it, fs
    bad = _cells(march)
    assert not bad, ("(scene, strategy, budget) cells whose hash differs from the reference's", bad[:20], len(bad))


def test_budget_zero_is_the_sdf_at_the_origin(E):
    """What makes the ray fixture an SDF fixture: with no iterations final_sdf is the scene's value at ray.at(0) -- the origin
    itself, but for the sign of a zero coordinate (o + 0 * d: -0.0 + 0.0 is +0.0)."""
    R = ec.rays()
    start = R["o"] + R["d"] * 0.0
    assert (start == R["o"]).all()
    for sid in range(ec.NSCENES):
        want = oracle.sdf_eval(sid, start)
        for kid in range(ec.NSTRATEGIES):
            hit, t, it, fs = oracle.march_rays(sid, kid, R["o"], R["d"], max_iterations=0, lipschitz=float(R["lip"][sid, kid]))
            assert ec.same_bits(fs, want) and not hit.any() and not it.any(), (sid, kid)


# ---- where the reference raises --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", range(ec.NSCENES))
def test_builds_agree_where_the_reference_raises(E, hostlib, interpreter, sid):
    """Oracle, kernel headers and interpreter return the same bits where the reference has none to give: +inf from
    Cylinder's `** 2` that leaves binary64 (libm's pow overflows; sd_cylinder selects the same value, since rm_pow claims
    nothing for 512 <= |y log x|), hence the floor's distance in Pillar Forest, and NaN on Capped Torus' centre circle."""
    m = E.raised[sid]
    if not m.any():
        assert sid not in (4, 12, 17)             # Cylinder, Pillar Forest (overflow) and Capped Torus (complex) do raise
        return
    pts = E.pts[m]
    o, h = oracle.sdf_eval(sid, pts), headers_sdf(hostlib, sid, pts)
    bad = np.flatnonzero(ec.bits(o) != ec.bits(h))
    assert not len(bad), ("oracle and kernel headers", sid, len(bad), pts[bad[0]].tolist(), float(o[bad[0]]), float(h[bad[0]]))
    if sid in ec.RESTATED + ec.TWINS:
        p = interpreter(sid, pts)
        bad = np.flatnonzero(ec.bits(p) != ec.bits(h))
        assert not len(bad), ("interpreter and kernel headers", sid, len(bad), pts[bad[0]].tolist(), float(p[bad[0]]), float(h[bad[0]]))
    print(f"scene {sid}: {int(m.sum())} raised points, values there: NaN {int(np.isnan(h).sum())}, +inf {int((h == np.inf).sum())}, "
          f"other {int((np.isfinite(h)).sum())}")


def test_capped_torus_circle_is_nan_where_the_reference_goes_complex(E, hostlib, interpreter):
    m = E.raised[17] & E.in_group("ctorus_circle")
    assert m.sum() >= 20
    for name, got in (("oracle", oracle.sdf_eval(17, E.pts[m])), ("kernel headers", headers_sdf(hostlib, 17, E.pts[m])),
                      ("interpreter", interpreter(17, E.pts[m]))):
        assert np.isnan(got).all(), (name, int((~np.isnan(got)).sum()))


def test_gyroid_beyond_the_cut_is_nan_by_contract(E, hostlib, interpreter):
    """|3 x| >= 105414336 in any coordinate: sin and cos of the library are NaN there (include/rm_hip.h), and so is the
    scene (Python's max keeps its first argument, the sheet, when the comparison with NaN fails)"""
    m = E.unclaimed[16]
    assert (m == ec.unclaimed_gyroid(E.pts)).all() and m.sum() >= 40
    assert (m & ~E.in_group("huge")).sum() >= 20 and (~m & E.in_group("gyroid") & (np.abs(E.pts) > 3e7).any(axis=1)).sum() >= 5
    for name, got in (("kernel headers", headers_sdf(hostlib, 16, E.pts[m])), ("interpreter", interpreter(16, E.pts[m]))):
        assert np.isnan(got).all(), (name, int((~np.isnan(got)).sum()))


# ---- the fixture itself ---------------------------------------------------------------------------------------------------

def test_fixture_keeps_its_conditions_and_edges(E):
    import os
    cov = ec.check_fixture(E.pts, E.group, E.names, E.want, E.raised)
    print("coverage", cov)
    for k, least in ec.MINIMA.items():
        assert cov[k] >= least, (k, cov[k], least)
    assert np.isfinite(E.pts).all()
    for name in ("sdf_edges.npz", "rays_edges.npz"):
        assert os.path.getsize(os.path.join(ec.GOLDEN, name)) <= min(ec.LARGEST_FIXTURE_BEFORE, 1 << 20), name
    # NaN is a value of the reference at 1e200 (inf - inf in the smooth unions): one class in every comparison
    assert np.isnan(E.want[7]).any() and np.isnan(E.want[19]).any()
    for sid in range(ec.NSCENES):
        assert len(ec.chosen(E, sid)) == 64 and E.pinned(sid)[ec.chosen(E, sid)].all(), sid
    R = ec.rays()
    assert len(R["o"]) == 240 and R["sha"].shape == (ec.NSCENES, ec.NSTRATEGIES, len(ec.BUDGETS), 32) and tuple(R["budgets"]) == ec.BUDGETS
    assert (np.abs(R["o"]) <= 1e4).all()
    on = (R["o"][:, None, :] == E.pts[None, :, :]).all(axis=2)
    assert on.any(axis=1).all(), "every ray starts on an edge point"
