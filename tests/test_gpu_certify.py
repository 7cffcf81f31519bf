"""The certified first hit on the MI355X: rm_certify_render and rm_certify_march_rays against the host build of
csrc/rm_certify.h (tests/native/certify_check.cpp) bit for bit -- t_lo, t_hi, status and steps -- on the frames of
tests/certify_cases.py, a band of rows, explicit rays with every outcome in one wave and a user program; certified_oracle.py;
and the sweep's cert_* columns.

Every launch is bounded by max_steps (at most RM_INTERVAL_MAX_STEPS probes per ray).  Every program made here is destroyed by
the fixture that made it."""
import numpy as np
import pytest

import certify_cases as cc
from certify_cases import HIT, MISS, OPEN

from raymarch_algo_compare_amd import _native, certified_oracle, registry, scoring, sweep
from raymarch_algo_compare_amd import interval_oracle as io
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu


@pytest.fixture
def programs():
    """program ids made through this fixture are destroyed at teardown"""
    made = []

    def make(expr):
        ops, n = sp.to_ctypes(expr)
        made.append(_native.scene_program_create(ops, n))
        return made[-1]
    yield make
    for pid in made:
        try:
            _native.scene_program_destroy(pid)
        except _native.RmError:
            pass


def rays_dict(r):
    return dict(zip(("t_lo", "t_hi", "status", "steps"), r))


def where_differs(a, b):
    for k in ("t_lo", "t_hi"):
        bad = np.argwhere(cc.bits(a[k]) != cc.bits(b[k]))
        if len(bad):
            return k, bad[:4].tolist()
    for k in ("status", "steps"):
        bad = np.argwhere(a[k] != b[k])
        if len(bad):
            return k, bad[:4].tolist()
    return None


@pytest.mark.parametrize("key", cc.frame_keys(), ids=[f"{k}{i}" for k, i in cc.frame_keys()])
def test_render_equals_host(key, programs):
    """the frames of the host tests (64 x 48, Thin Torus 128 x 96), without a prune and, for a catalogue scene, with the
    library's own; a twin runs as a user program"""
    W, H = cc.frame_size(key)
    cam = cc.frame_camera(key).params14()
    expr = cc.frame_expression(key)
    sid = key[1] if key[0] == "c" else programs(expr)
    dev = _native.certify_render(sid, cam, W, H, cc.frame_config(key, bound_radius=-1.0))
    assert cc.same(dev, cc.host_frame(key)), (key, where_differs(dev, cc.host_frame(key)))
    assert dev["t_lo"].dtype == np.float64 and dev["status"].dtype == np.uint8 and dev["steps"].dtype == np.int32
    if key[0] == "c" and cc.lib().rmc_scene_bound(sid) > 0.0:
        dev = _native.certify_render(sid, cam, W, H, cc.frame_config(key))
        host = cc.host_render(expr, cam, W, H, cc.frame_config(key), cc.lib().rmc_scene_bound(sid))
        assert cc.same(dev, host), (key, "pruned", where_differs(dev, host))
        assert (dev["steps"] == 0).any()


def test_rows_timing_and_lifecycle(programs):
    key = ("c", cc.PILLAR_FOREST)
    W, H = cc.frame_size(key)
    cam = cc.frame_camera(key).params14()
    whole = cc.host_frame(key)
    part = _native.certify_render(cc.PILLAR_FOREST, cam, W, H, cc.frame_config(key), row0=7, rows=11)
    assert cc.same(part, {k: v[7:18] for k, v in whole.items()})
    last = _native.certify_render(cc.PILLAR_FOREST, cam, W, H, cc.frame_config(key), row0=H - 1, rows=1)
    assert cc.same(last, {k: v[H - 1:] for k, v in whole.items()})
    pid = programs(cc.frame_expression(key))
    timed = _native.certify_render(pid, cam, W, H, cc.frame_config(key), repeats=3, warmup=1)
    tm = timed.pop("timing")
    assert cc.same(timed, whole)
    assert tm["repeats"] == 3 and len(tm["ms_each"]) == 3 and all(x > 0 for x in tm["ms_each"])
    _native.scene_program_destroy(pid)
    for call in (lambda: _native.certify_render(pid, cam, W, H), lambda: _native.certify_march_rays(pid, [[0, 0, 5]], [[0, 0, -1]]),
                 lambda: _native.certify_render(registry.get_scene_by_name("Mandelbulb").id, cam, W, H)):
        with pytest.raises(_native.RmError) as e:
            call()
        assert e.value.code == _native.RM_E_BAD_SCENE
    assert certified_oracle.certified_capture("Mandelbulb", Camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 60.0, 8, 8)) is None


@pytest.mark.parametrize("sid", [14, cc.PILLAR_FOREST], ids=["Sphere Cloud", "Pillar Forest"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_march_rays_equals_host(sid, n):
    """hits, misses, OPEN (tangents of a sphere the cloud's rays graze; too few steps) and eyes inside a solid in one wave;
    n below, at and above the wave and the workgroup"""
    expr = sp.catalogue_expressions()[sid]
    o, d = cc.mixed_rays(n, 100 * sid + n, cc.INSIDE[sid])
    seen = set()
    for cfg in (None, _native.certify_config(max_steps=24)):
        host = rays_dict(cc.host_march(expr, o, d, cfg))
        dev = rays_dict(_native.certify_march_rays(sid, o, d, cfg))
        assert cc.same(dev, host), (sid, n, where_differs(dev, host))
        seen |= set(np.unique(host["status"]).tolist())
    assert host["steps"][0] == 0 and host["status"][0] == HIT          # the eye in a solid
    if n == 257:
        assert seen == {MISS, HIT, OPEN}


def test_user_program_equals_host(programs):
    """rotate, mirror and limited repeat in one program: explicit rays and a frame"""
    expr = cc.rotated_program()
    pid = programs(expr)
    o, d = cc.mixed_rays(300, 5)
    host = rays_dict(cc.host_march(expr, o, d))
    dev = rays_dict(_native.certify_march_rays(pid, o, d))
    assert cc.same(dev, host), where_differs(dev, host)
    assert (host["status"] == HIT).sum() > 50 and (host["status"] == MISS).sum() > 50
    cam = Camera((2.5, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 64, 48).params14()
    dev, host = _native.certify_render(pid, cam, 64, 48), cc.host_render(expr, cam, 64, 48)
    assert cc.same(dev, host), where_differs(dev, host)
    t_lo, t_hi, status, steps = certified_oracle.certified_first_hit(o, d, pid)
    assert cc.same(rays_dict((t_lo, t_hi, status, steps)), rays_dict(cc.host_march(expr, o, d)))


def test_capture_and_error_bar():
    """certified_capture and oracle_error_bar on Pillar Forest: the capture dict scores with scoring.py, the error bar is the
    host's (the same frames bit for bit), l_global comes from the scene (Bad Lipschitz Sphere's twin: 2)"""
    key = ("c", cc.PILLAR_FOREST)
    W, H = cc.frame_size(key)
    cam = cc.frame_camera(key)
    cert = certified_oracle.certified_capture("Pillar Forest", cam, bound_radius=-1.0)
    assert cc.same(cert, cc.host_frame(key))
    cap = cert["capture"]
    assert np.array_equal(cap["hit"], cert["status"] == HIT) and np.array_equal(cap["depth"][cap["hit"]], cert["t_hi"][cap["hit"]])
    assert np.all(cap["depth"][~cap["hit"]] == 0.0)
    iv = io.interval_capture("Pillar Forest", cam)
    res = scoring.residual(iv["hit"], iv["depth"], cap["hit"], cap["depth"], scoring.silhouette_band(cap["hit"], k=2))
    assert 0.0 < res["iou"] < 1.0 and res["n_analytic_hit"] == int(cap["hit"].sum())      # the oracle hits more than is there
    bar = certified_oracle.oracle_error_bar("Pillar Forest", cam)
    assert bar == certified_oracle.error_bar(cc.host_frame(key), cc.host_interval_frame(key))
    assert bar["false_hits"] == cc.FALSE_HITS_MEASURED[cc.PILLAR_FOREST]
    mine = registry.find_program_scene(sp.twin_name(11)) is None
    twin = sp.register_twin(registry.SCENES[11])
    try:
        cert = certified_oracle.certified_capture(twin, cc.frame_camera(("t", 11)), bound_radius=-1.0)
        assert cc.same(cert, cc.host_frame(("t", 11)))
    finally:
        if mine:
            sp.unregister_scene(twin.name)


def test_sweep_certify_columns(tmp_path, monkeypatch):
    W, H = 48, 36
    calls = []
    real = sweep.certify_columns

    def spy(frame, cert):
        calls.append((frame, cert, real(frame, cert)))
        return calls[-1][2]
    monkeypatch.setattr(sweep, "certify_columns", spy)
    rows = sweep.run_sweep(["Sphere", "Pillar Forest"], ["Standard", "Relaxed"], "budget", W, H, budgets=[16, 64], oracle="interval",
                           certify=True, out_path=str(tmp_path / "c.csv"))
    assert len(rows) == len(calls) > 0
    for r, (frame, cert, cols) in zip(rows, calls):
        assert list(r) == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS + sweep.CERTIFY_FIELDS
        assert all(r[k] is not None for k in sweep.CERTIFY_FIELDS) and {k: r[k] for k in sweep.CERTIFY_FIELDS} == cols
        # without the interval oracle: the IoU over the pixels the certificate decides lies between the two bounds
        decided = cert["status"] != OPEN
        free_iou = scoring._hit_metrics(frame["hit"][decided], (cert["status"] == HIT)[decided])["iou"]
        print(f"{r['scene']} {r['strategy']} {r['viewpoint']} budget {r['max_iterations']}: cert_iou_lo {r['cert_iou_lo']:.4f} <= "
              f"{free_iou:.4f} <= cert_iou_hi {r['cert_iou_hi']:.4f}; oracle_iou {r['oracle_iou']:.4f}, open "
              f"{r['cert_open_frac']:.4f}, depth mae {r['cert_depth_mae']:.3e}")
        assert 0.0 <= r["cert_iou_lo"] <= free_iou <= r["cert_iou_hi"] <= 1.0
        assert r["cert_open_frac"] == pytest.approx(float((~decided).mean()))
        assert frame["hit"].shape == cert["status"].shape == (H, W)
    text = (tmp_path / "c.csv").read_text().splitlines()
    assert text[0].split(",") == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS + sweep.CERTIFY_FIELDS and len(text) == len(rows) + 1
    plain = sweep.run_sweep(["Sphere"], ["Standard"], "budget", W, H, budgets=[16], oracle="interval", out_path=str(tmp_path / "p.csv"))
    assert list(plain[0]) == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS
    assert (tmp_path / "p.csv").read_text().splitlines()[0].split(",") == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS
