"""The edge-point fixtures of the 20 scene SDFs, shared by tests/test_sdf_edges_host.py and tests/test_gpu_sdf_edges.py (and
by oracle/gen_golden.py --only sdf_edges / ray_edges, which asserts check_fixture before it writes): the loader, the bit
comparison, the coverage the fixture must keep, and the wave layouts of the device test.

tests/golden/sdf_edges.npz (values of the REFERENCE itself):
  pts (N, 3)            the points: measure-zero edges of the scenes' arithmetic (zero remainders, .5 ties, clamps, signed
                        zeros on the poles, |p| == 4, min / max ties, branch lines, length(0), the sincos cut) and magnitudes
                        from subnormal to 1e200
  group (N,) int16      index into group_names: the recipe that made the point
  group_names           "shared", one group per scene family, "ctorus_circle", "huge"
  s{sid} (N,)           the reference's value; 0.0 where it raised
  raised_s{sid} (N,)    the reference raised an exception there (OverflowError, or a complex result: TypeError)
  unclaimed_s16 (N,)    Gyroid: a coordinate with |3 x| >= 105414336, where the library returns NaN by contract
                        (include/rm_hip.h) and the reference a value

tests/golden/rays_edges.npz: o, d (R, 3) origins (edge points) and directions, lip (20, 11) the Lipschitz constant of
main.py's wiring, budgets (4,), sha (20, 11, 4, 32) sha256 of one cell = scene x strategy x budget marched by the
reference's own march() (cell_hash below)."""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NSCENES, NSTRATEGIES = 20, 11
BUDGETS = (0, 1, 2, 3)
SINCOS_CUT = 105414336.0                 # 0x1.921fbp+26: rm_sincos is NaN from here on (csrc/rm_math_trig.h)
RESTATED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 17, 19)      # scene_program.catalogue_expressions
TWINS = (9, 11, 15, 16, 18)                                      # scene_program.catalogue_twins
TEAM_SCENES = (10, 14, 15)               # scenes with a wavefront-team form (rm_march_rays_team)
LARGEST_FIXTURE_BEFORE = 1200132         # frames_64x48.npz
CANONICAL_NAN = np.uint64(0x7FF8000000000000)

# the groups whose points were made for a scene (the shared and the huge group serve every scene)
SCENE_GROUPS = {0: ("spheres",), 1: ("planes",), 2: ("boxes",), 3: ("thin_torus", "torus_cyl"), 4: ("torus_cyl",),
                5: ("near_miss", "spheres"), 6: ("boxes", "spheres"), 7: ("boxes", "spheres"), 8: ("onion",),
                9: ("menger", "boxes"), 10: ("mandelbulb",), 11: ("spheres",), 12: ("pillars", "torus_cyl"), 13: ("planes",),
                14: ("spheres",), 15: ("spheres",), 16: ("gyroid",), 17: ("capped_torus", "ctorus_circle"), 18: ("lattice", "boxes"),
                19: ("spheres",)}

# What the fixture must keep holding: half of what the generated set holds (the counts are printed by the generator and by
# test_sdf_edges_host.py::test_fixture_keeps_its_edges).  Generated: menger_plane 279, lattice_tie 234, r_is_4 14,
# on_z_axis 136, negative_zero 51, circle_raised 35, circle_defined 165; the two counts of the Capped Torus circle are
# held to 20 each whatever the set holds.
MINIMA = {"menger_plane": 139, "lattice_tie": 117, "r_is_4": 7, "on_z_axis": 68, "negative_zero": 25,
          "circle_raised": 20, "circle_defined": 20}


def bits(a):
    """the bits of float64 values with every NaN replaced by one canonical NaN: NaN is one class"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = CANONICAL_NAN
    return b


def cell_hash(hit, iters, t, fs):
    """sha256 of one marched cell: hit (uint8), iterations (int32), the bits of t and of final_sdf, NaN canonical"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(hit).astype(np.uint8).tobytes())
    h.update(np.ascontiguousarray(iters).astype("<i4").tobytes())
    h.update(bits(t).astype("<u8").tobytes())
    h.update(bits(fs).astype("<u8").tobytes())
    return h.digest()


class Edges:
    def __init__(self, z):
        self.pts = np.ascontiguousarray(z["pts"])
        self.group = z["group"].astype(np.int64)
        self.names = [str(s) for s in z["group_names"]]
        self.want = {sid: z[f"s{sid}"] for sid in range(NSCENES)}
        self.raised = {sid: z[f"raised_s{sid}"].astype(bool) for sid in range(NSCENES)}
        self.unclaimed = {sid: np.zeros(len(self.pts), bool) for sid in range(NSCENES)}
        self.unclaimed[16] = z["unclaimed_s16"].astype(bool)

    def in_group(self, *names):
        return np.isin(self.group, [self.names.index(n) for n in names])

    def pinned(self, sid):
        """the points where the reference's value of scene sid holds for the library"""
        return ~self.raised[sid] & ~self.unclaimed[sid]

    def describe(self, i, sid):
        return (f"point {i} {self.pts[i].tolist()} ({[float.hex(float(c)) for c in self.pts[i]]}), group "
                f"{self.names[self.group[i]]}, scene {sid}")


@functools.lru_cache(maxsize=None)
def edges():
    return Edges(np.load(os.path.join(GOLDEN, "sdf_edges.npz")))


@functools.lru_cache(maxsize=None)
def rays():
    z = np.load(os.path.join(GOLDEN, "rays_edges.npz"))
    return {"o": np.ascontiguousarray(z["o"]), "d": np.ascontiguousarray(z["d"]), "lip": z["lip"], "budgets": [int(b) for b in z["budgets"]],
            "sha": z["sha"]}


def mismatches(E, sid, got, idx=None, where=None, lanes=None):
    """The points where `got` differs from the reference's value of scene sid, as a report ('' if there are none).  idx: the
    fixture index of every evaluated point (default: fixture order); where: compare only these; lanes: lane of each."""
    idx = np.arange(len(got)) if idx is None else np.asarray(idx)
    sel = E.pinned(sid)[idx] if where is None else where
    bad = np.flatnonzero((bits(got) != bits(E.want[sid][idx])) & sel)
    if not len(bad):
        return ""
    lines = [f"{len(bad)} of {int(sel.sum())} values differ from the reference"]
    for k in bad[:8]:
        lane = f", lane {int(lanes[k])}" if lanes is not None else f", position {int(k)} (lane {int(k) % 64})"
        lines.append(f"  {E.describe(int(idx[k]), sid)}{lane}: got {float(got[k])!r} ({float.hex(float(got[k]))}), want "
                     f"{float(E.want[sid][idx[k]])!r} ({float.hex(float(E.want[sid][idx[k]]))})")
    return "\n".join(lines)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


# ---- what the fixture promises ----------------------------------------------------------------------------------------

def coverage(pts, group, names, want, raised):
    """the counts of MINIMA, from the arrays of the fixture"""
    huge = group == names.index("huge")
    circle = group == names.index("ctorus_circle")
    p = pts[~huge]
    with np.errstate(all="ignore"):
        jump = np.zeros(len(p), bool)
        for s in (1.0, 3.0, 9.0):
            jump |= (((p * s) % 2.0 == 0.0) & (p != 0.0) & (np.abs(p) <= 3.5)).any(axis=1)
        tie = ((p - np.floor(p) == 0.5) & (np.abs(p) < 3.0)).any(axis=1)
        r4 = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2]) ** 0.5 == 4.0
    negzero = np.zeros(len(pts), bool)
    for sid in range(NSCENES):
        negzero |= (want[sid] == 0.0) & np.signbit(want[sid]) & ~raised[sid]
    return {"menger_plane": int(jump.sum()), "lattice_tie": int(tie.sum()), "r_is_4": int(r4.sum()),
            "on_z_axis": int(((pts[:, 0] == 0.0) & (pts[:, 1] == 0.0)).sum()), "negative_zero": int(negzero.sum()),
            "circle_raised": int(raised[17][circle].sum()), "circle_defined": int((~raised[17][circle]).sum())}


def unclaimed_gyroid(pts):
    q = 3.0 * pts
    return (~(np.abs(q) < SINCOS_CUT)).any(axis=1)


def check_fixture(pts, group, names, want, raised, out=print):
    """The conditions and the coverage of the fixture; returns the coverage counts."""
    n = len(pts)
    assert 3500 <= n <= 4500, n
    huge = group == names.index("huge")
    circle = group == names.index("ctorus_circle")
    assert huge.sum() <= 0.10 * n, int(huge.sum())
    assert int(circle.sum()) == 200
    for sid in range(NSCENES):
        assert raised[sid].sum() <= 0.05 * n, (sid, int(raised[sid].sum()))
        stray = np.flatnonzero(raised[sid] & ~huge & ~circle)
        for i in stray:
            out(f"scene {sid}: the reference raised at point {int(i)} {pts[i].tolist()} of group {names[group[i]]}")
        assert len(stray) <= 2, (sid, stray)
        assert not np.isnan(want[sid][raised[sid]]).any() and (want[sid][raised[sid]] == 0.0).all()
    cov = coverage(pts, group, names, want, raised)
    return cov


# ---- wave layouts of the device test -------------------------------------------------------------------------------------

PREFIXES = (1, 63, 64, 65)
LANES = (0, 13, 31, 32, 63)
PERMUTATION_SEED = 20261020


def permutation(n):
    return np.random.default_rng(PERMUTATION_SEED).permutation(n)


def chosen(E, sid, limit=64):
    """Up to `limit` edge points of scene sid: evenly spaced through the points of its own groups where the reference's
    value holds, a few of the shared and of the huge group at the end."""
    own = np.flatnonzero(E.in_group(*SCENE_GROUPS[sid]) & E.pinned(sid))
    rest = np.flatnonzero(E.in_group("shared", "huge") & E.pinned(sid))
    k = limit - 8
    pick = own[np.linspace(0, len(own) - 1, min(k, len(own))).astype(np.int64)] if len(own) else own
    tail = rest[np.linspace(0, len(rest) - 1, limit - len(pick)).astype(np.int64)]
    return np.unique(np.concatenate([pick, tail]))[:limit]


def ordinary(E, sid, n=63):
    """n unremarkable points for the other lanes of a wave: uniform in [-3.5, 3.5]^3, seeded; no fixture value is needed
    for them"""
    return np.random.default_rng(1000 + sid).uniform(-3.5, 3.5, size=(n, 3))


def wave_of_copies(E, idx):
    """one wave of 64 copies per chosen point: (points, fixture index of each, lane of each)"""
    rep = np.repeat(idx, 64)
    return E.pts[rep], rep, np.tile(np.arange(64), len(idx))


def alone_in_wave(E, sid, idx):
    """Each chosen point alone among 63 ordinary ones, its lane rotating over LANES: (points, the positions of the edge
    points, their fixture indices, their lanes)"""
    other = ordinary(E, sid)
    waves = np.empty((len(idx), 64, 3))
    lanes = np.array([LANES[k % len(LANES)] for k in range(len(idx))])
    for k, i in enumerate(idx):
        waves[k, np.arange(64) != lanes[k]] = other
        waves[k, lanes[k]] = E.pts[i]
    pos = np.arange(len(idx)) * 64 + lanes
    return waves.reshape(-1, 3), pos, np.asarray(idx), lanes
