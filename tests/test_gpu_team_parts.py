"""Wavefront teams with per-part trip loops (rm_kernels.h team_trips): raw t, final_sdf, iterations and hits, bit for bit
against the oracle -- through rm_march_rays_team and through the single launch (rm_pipeline.h team role).

The ray sets are built so that the first evaluation of every lane starts in a chosen place of the part chains:
bail-out after each trip 1..8, each band of acos (Taylor, table, 1/sqrt) on z.z / r, small and large atan2 ratios in
all four quadrants, and the three argument ranges of sincos on 8 * theta and 8 * phi."""
import math

import numpy as np
import pytest


def _trips(p):
    """fractal iterations of one Mandelbulb evaluation at p (catalog.py:266-293; begin / trip of rm_scenes.h)"""
    z = p
    r = math.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2])
    i = 0
    while r <= 4.0 and i < 8:
        theta = math.acos(max(-1.0, min(1.0, z[2] / max(r, 1e-12)))) * 8.0
        phi = math.atan2(z[1], z[0]) * 8.0
        zr = r ** 8.0
        z = (zr * math.sin(theta) * math.cos(phi) + p[0], zr * math.sin(theta) * math.sin(phi) + p[1],
             zr * math.cos(theta) + p[2])
        i += 1
        r = math.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2])
    return i


def _band_points():
    """origins on the chosen bands of the three chains (the ray's first evaluation is at its origin)"""
    pts = []
    # acos on c = z.z / r: Taylor |c| < 1/8, table 1/8 <= |c| < 0.96875, 1/sqrt band 0.96875 <= |c| < 1, and c = +-1;
    # c > 0.9943 also puts 8 * theta in sincos range 1 (|x| < 0.855), 0.9 in range 2, the rest in range 3
    for c in (0.01, -0.1, 0.2, -0.45, 0.7, -0.9, 0.95, 0.97, -0.99, 0.9995, 1.0, -1.0):
        for az in (0.3, 2.0, -2.6, -0.9):
            s = math.sqrt(max(0.0, 1.0 - c * c))
            for rad in (0.6, 1.1):
                pts.append((rad * s * math.cos(az), rad * s * math.sin(az), rad * c))
    # atan2(y, x): ratio |y / x| (or |x / y|) below 1/16 and above it, in all four quadrants; small angles also give
    # 8 * phi in sincos ranges 1 and 2
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for ratio in (0.01, 0.05, 0.3, 0.9, 3.0, 40.0):
                x, y = sx * 0.8, sy * 0.8 * ratio
                n = math.hypot(x, y) / 0.9
                pts.append((x / n, y / n, 0.3))
    return pts


def _rays(n_live, seed):
    """n_live rays: origins with first evaluations that bail out after each trip count 1..8 and on every band above,
    aimed past the bulb's centre (some hit, some escape, some march to the iteration limit near the surface)"""
    rng = np.random.default_rng(seed)
    by_trips = {k: [] for k in range(1, 9)}
    while any(len(v) < 4 for v in by_trips.values()):
        p = tuple(rng.uniform(-1.3, 1.3, 3))
        k = _trips(p)
        if k >= 1 and len(by_trips[k]) < 4:
            by_trips[k].append(p)
    pts = [p for k in range(1, 9) for p in by_trips[k]] + _band_points()
    rng.shuffle(pts)
    o = np.array(pts[:n_live] if n_live <= len(pts) else [pts[i % len(pts)] for i in range(n_live)], dtype=np.float64)
    aim = rng.normal(0.0, 0.35, o.shape)
    d = aim - o
    return o, d


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def test_bail_out_trips_cover_one_to_eight():
    by = {_trips(p) for p in (tuple(np.random.default_rng(s).uniform(-1.3, 1.3, 3)) for s in range(4000))}
    assert set(range(1, 9)) <= by


@pytest.mark.gpu
@pytest.mark.parametrize("n_live", [1, 17, 64, 64 * 3 + 5])
@pytest.mark.parametrize("kid", [0, 4])
def test_march_rays_team_mandelbulb_bit_exact(hip, n_live, kid):
    from oracle import oracle
    o, d = _rays(n_live, 1000 + n_live)
    for team in (True, False):
        hit, t, it, fs = hip.march_rays(10, kid, o, d, team=team)
        rh, rt, ri, rf = oracle.march_rays(10, kid, o, d)
        assert _same(hit, rh) and _same(it, ri), (team, int((it != ri).sum()))
        assert _same(t, rt) and _same(fs, rf), team


@pytest.mark.gpu
@pytest.mark.parametrize("sid", [14, 15])
def test_march_rays_team_unions_bit_exact(hip, sid):
    from oracle import oracle
    rng = np.random.default_rng(sid)
    for n in (1, 17, 64, 130):
        o = rng.uniform(-3.0, 3.0, (n, 3))
        d = rng.normal(0.0, 0.5, (n, 3)) - o
        hit, t, it, fs = hip.march_rays(sid, 0, o, d, team=True)
        rh, rt, ri, rf = oracle.march_rays(sid, 0, o, d)
        assert _same(hit, rh) and _same(it, ri) and _same(t, rt) and _same(fs, rf), (sid, n)


@pytest.mark.gpu
@pytest.mark.parametrize("sid,kid", [(10, 0), (10, 4), (14, 0), (15, 0)])
def test_single_launch_teams_bit_exact(hip, sid, kid):
    """small frames whose rays are handed to the teams after a few trips (suspend_after), every ray against the oracle"""
    from oracle import oracle
    from raymarch_algo_compare_amd import registry
    from raymarch_algo_compare_amd.camera import Camera
    sc = registry.SCENES[sid]
    W, H = 96, 64
    cam = Camera(sc.camera_position or (0.0, 0.0, 5.0), sc.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W,
                 H).params14()
    ref = oracle.render(sid, kid, cam, W, H)
    for sched in (dict(suspend_after=(2, 6)), dict(suspend_after=(3, 0)), dict(suspend_after=(2, 9), team_grid=1)):
        out = hip.render(hip.make_desc(sid, kid, cam, W, H, full=True, pipeline=2, **sched), want_t_raw=True,
                         want_final_sdf=True)
        assert (out["iters"] == ref.iters).all() and (out["hit"] == ref.hit).all(), sched
        assert _same(out["t_raw"], ref.t) and _same(out["final_sdf"], ref.final_sdf), sched
