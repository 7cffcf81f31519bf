"""Inputs shared by tests/test_ssim_host.py and tests/test_gpu_ssim.py where the quantisation of csrc/rm_ssim.h can go
wrong: float32 values at the rounding edges of `x * 255`, outside [0, 1] and non-finite, normals at exactly +-1 / 0, hit
depths that are NaN, +-inf or +-3.4e38, captures with no hit, one hit or one depth, images of the strongest contrast, and
captures that differ in one pixel at a tile seam.  Everything is seeded: the CPU and the GPU test see the same arrays."""
import numpy as np

F32 = np.float32
TILE_W, TILE_H = 32, 8      # kSsimTileW, kSsimTileH of csrc/rm_ssim.h: a tile's output pixels (its windows reach 6 further)
# (W, H).  As tests/test_gpu_ssim.py: one window; barely more; several tiles; no multiple of the tile; one tile plus one
# pixel each way.  Then: exactly one tile, no overhang; exactly 2 x 2 tiles; one output column, many tiles; one output row,
# many tiles; two tiles across with 7 output columns in the second, and rows 14 of 21 left over
SHAPES = [(7, 7), (8, 9), (64, 48), (100, 37), (TILE_W + 6 + 1, TILE_H + 6 + 1),
          (TILE_W + 6, TILE_H + 6), (2 * TILE_W + 6, 2 * TILE_H + 6), (7, 120), (200, 7), (45, 21)]
HUGE = F32(3.4e38)
# (a, b) of the constant images: test_ssim_host.test_constant_images_match_the_closed_form
CONSTANT_PAIRS = ((0, 255), (10, 200), (128, 129), (255, 254), (0, 1))


def k255_neighbours():
    """float32: the nearest float32 of every k/255, the float32 below it and the two above it"""
    k = (np.arange(256) / 255.0).astype(F32)
    up = np.nextafter(k, F32(2.0))
    return np.concatenate([k, np.nextafter(k, F32(-1.0)), up, np.nextafter(up, F32(2.0))])


def special_values():
    """float32 values off the k/255 grid: zeros and the smallest numbers, the largest, NaN, +-inf, 1 and 254.5/255 ..
    255.5/255 from both sides, and plain values outside [0, 1]"""
    tiny = np.nextafter(F32(0.0), F32(1.0))
    return np.array([-0.0, tiny, -tiny, np.finfo(F32).tiny, HUGE, -HUGE, np.nan, np.inf, -np.inf, 1.0 - 2.0 ** -24,
                     1.0 + 2.0 ** -23, 254.5 / 255.0, 255.5 / 255.0, -0.25, 1.5], F32)


def edge_values():
    return np.concatenate([k255_neighbours(), special_values()])


def _draw(rng, n):
    """n edge values: the specials first (every one is there from n = 15 on), then k/255 neighbours without repetition
    until they run out"""
    sp, nb = special_values(), k255_neighbours()
    picks = [sp]
    while sum(len(p) for p in picks) < n:
        picks.append(rng.permutation(nb))
    v = np.concatenate(picks)[:n]
    return v[rng.permutation(n)]


def edge_capture(W, H, seed, nan="late", posinf=True, neginf=True, huge=True, all_miss=False, one_hit=False, equal_depth=False,
                 color=True, normal=True):
    """A capture of edge values.  nan: None, or a NaN depth on the "first" or a "late" (6th) hit in row-major order;
    posinf / neginf / huge: +inf, -inf, +-3.4e38 on further hits.  All of them also lie on misses, where they must not
    matter.  one_hit and equal_depth keep the hit depths finite."""
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W)) < 0.7
    if all_miss:
        hit[:] = False
    if one_hit:
        hit[:] = False
        hit[H // 2, W // 3] = True
    depth = rng.uniform(1.0, 9.0, (H, W)).astype(F32)
    flat, hits, misses = depth.reshape(-1), np.flatnonzero(hit), np.flatnonzero(~hit)
    if equal_depth:
        flat[hits] = F32(4.25)
    elif not one_hit and len(hits):
        assert len(hits) >= 10, "too few hits for the special depths"
        if nan:
            flat[hits[0 if nan == "first" else 5]] = np.nan
        if posinf:
            flat[hits[2]] = np.inf
        if neginf:
            flat[hits[7]] = -np.inf
        if huge:
            flat[hits[1]], flat[hits[4]] = HUGE, -HUGE
    bad = np.array([np.nan, np.inf, -np.inf, HUGE, -HUGE, np.nan], F32)
    flat[misses[:len(bad)]] = bad[:len(misses)]
    c = {"hit": hit, "depth": depth}
    if normal:
        with np.errstate(over="ignore", invalid="ignore"):
            n = (F32(2.0) * _draw(rng, 3 * W * H) - F32(1.0)).reshape(H, W, 3)      # n * 0.5 + 0.5 comes back to the edges
        pick = rng.random((H, W)) < 0.2                                           # exactly +-1 on one axis, 0 on the others
        axis, sign = rng.integers(0, 3, (H, W)), rng.choice(np.array([-1.0, 1.0], F32), (H, W))
        n[pick] = 0.0
        n[pick, axis[pick]] = sign[pick]
        if len(hits) > 3:                                                         # degenerate normals on hits, whatever was drawn
            nf = n.reshape(-1, 3)
            nf[hits[3]] = np.nan
            nf[hits[-1]] = (np.inf, 0.0, -np.inf)
            nf[hits[-2]] = 0.0
        c["normal"] = n
    if color:
        c["color"] = _draw(rng, 3 * W * H).reshape(H, W, 3)
    return c


def require_classes(c):
    """`c` itself, after asserting that it holds every class of input the edge tests are about"""
    hit = np.asarray(c["hit"]) != 0
    d, n, col = c["depth"][hit], c["normal"][hit], c["color"]
    assert np.isnan(d).any(), "no NaN on a hit depth"
    assert np.isinf(d).any(), "no inf on a hit depth"
    assert np.isnan(n).any(), "no NaN normal on a hit"
    assert ((np.abs(n) == 1.0).sum(axis=1) == 1).any() and (n == 0.0).all(axis=1).any(), "no axis or zero normal on a hit"
    assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any(), "colour lacks NaN, +inf or -inf"
    with np.errstate(invalid="ignore"):
        assert (col < 0.0).any() and (col > 1.0).any(), "no colour below 0 or above 1"
    distinct = len(np.intersect1d(col[np.isfinite(col)], k255_neighbours()))
    need = min(200, col.size // 2)      # a 7 x 7 capture has 147 colour values
    assert distinct >= need, f"{distinct} distinct k/255 neighbours in the colour, {need} wanted"
    return c


def edge_pairs(W, H):
    """[(name, method, reference)]: what both the host and the GPU test score.  `noisy`: tests/test_ssim_host.capture"""
    from test_ssim_host import capture
    edge, other = require_classes(edge_capture(W, H, 41)), require_classes(edge_capture(W, H, 42, nan="first"))
    finite = edge_capture(W, H, 43, nan=None, posinf=False, neginf=False, huge=False)
    return [("noisy against edge", capture(W, H, 44), edge),
            ("edge against noisy", edge, capture(W, H, 44)),
            ("edge against edge", other, edge),
            ("edge against finite-depth edge", edge, finite),
            ("edge against +inf-depth edge", edge, edge_capture(W, H, 45, nan=None, neginf=False, huge=False)),
            ("edge against -inf-depth edge", edge, edge_capture(W, H, 46, nan=None, posinf=False, huge=False)),
            ("edge against huge-depth edge", edge, edge_capture(W, H, 47, nan=None, posinf=False, neginf=False)),
            ("edge against all-miss", edge, edge_capture(W, H, 48, all_miss=True)),
            ("all-miss against edge", edge_capture(W, H, 48, all_miss=True), finite),
            ("one-hit", edge, edge_capture(W, H, 49, one_hit=True)),
            ("one-hit both", edge_capture(W, H, 50, one_hit=True), edge_capture(W, H, 49, one_hit=True)),
            ("equal-depth", edge, edge_capture(W, H, 51, equal_depth=True)),
            ("NaN depth at a late hit of the reference", finite, edge_capture(W, H, 52, posinf=False, neginf=False, huge=False)),
            ("NaN depth at the first hit of the reference", finite,
             edge_capture(W, H, 53, nan="first", posinf=False, neginf=False, huge=False)),
            ("no colour", edge_capture(W, H, 54, color=False), edge_capture(W, H, 55, color=False)),
            ("depth only", edge_capture(W, H, 56, color=False, normal=False), edge_capture(W, H, 57, color=False, normal=False))]


# ---- the strongest contrasts ---------------------------------------------------------------------------------------------

def _from_level(level, depth):
    """a capture, every pixel a hit, whose colour and normal images are `level` (H, W; in 8-bit units, k + 0.5 for the
    byte k so that no rounding edge is near) in all three channels"""
    v = (np.asarray(level, np.float64) / 255.0).astype(F32)
    three = np.repeat(v[..., None], 3, axis=2)
    return {"hit": np.ones(v.shape, bool), "depth": np.asarray(depth, F32), "color": three, "normal": F32(2.0) * three - F32(1.0)}


def contrast_pairs(W, H):
    """[(name, method, reference, (a, b) or None)]: 0/1 checkerboards of period 1 and 7 against their inverses (the depth
    images too), all-0 against all-1, and constant images of bytes a against b (the depth images equal)"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for period in (1, 7):
        p = ((xx // period + yy // period) % 2).astype(np.float64)
        out.append((f"checkerboard of period {period}", _from_level(255.0 * p, 3.0 + p), _from_level(255.0 * (1.0 - p), 4.0 - p), None))
    flat = np.full((H, W), 3.0)
    out.append(("all-0 against all-1", _from_level(np.zeros((H, W)), flat), _from_level(np.full((H, W), 255.0), flat), (0, 255)))
    for a, b in CONSTANT_PAIRS:
        out.append((f"constant {a} against {b}", _from_level(np.full((H, W), a + 0.5), flat), _from_level(np.full((H, W), b + 0.5), flat), (a, b)))
    return out


# ---- one pixel apart ---------------------------------------------------------------------------------------------------

ONE_HOT_BYTES = ((0, 255), (255, 0), (17, 18), (200, 100), (128, 127))      # (reference, method) byte of the one pixel


def one_hot_places(W, H):
    """(x, y) once each: the corners, the last three columns and rows (the pixels the cropping leaves to the last tile),
    and both sides of every tile seam of the staged blocks (a tile's output block ends at 31 / 7, its halo at 37 / 13)"""
    seam_x, seam_y = [x for x in (31, 32, 37, 38) if x < W], [y for y in (7, 8, 13, 14) if y < H]
    places = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    places += [(W - k, H // 2) for k in (1, 2, 3)] + [(W // 2, H - k) for k in (1, 2, 3)]
    places += [(x, H // 2) for x in seam_x] + [(W // 2, y) for y in seam_y] + [(x, y) for x in seam_x for y in seam_y]
    return list(dict.fromkeys(places))


def one_hot_pairs(W, H):
    """[(name, method, reference, d)]: two captures equal but for one pixel of one colour channel, whose bytes differ by d"""
    rng = np.random.default_rng(61)
    base = _from_level(rng.integers(0, 256, (H, W)) + 0.5, rng.uniform(1.0, 9.0, (H, W)))
    out = []
    for i, (x, y) in enumerate(one_hot_places(W, H)):
        r, m = ONE_HOT_BYTES[i % len(ONE_HOT_BYTES)]
        ref, met = dict(base, color=base["color"].copy()), dict(base, color=base["color"].copy())
        ref["color"][y, x, i % 3], met["color"][y, x, i % 3] = F32((r + 0.5) / 255.0), F32((m + 0.5) / 255.0)
        out.append((f"({x}, {y}) channel {i % 3}", met, ref, m - r))
    return out
