// rm_score.h -- the primary and secondary tiers of capture scoring and the calibration residual: hit-mask counts (with and
// without the reference's silhouette band), depth error and normal angle over the co-hit pixels, with exact percentiles.
// Shared by the gfx950 kernels (rm_score.hip), the C ABI (rm_score_captures) and the host check build
// (tests/native/score_check.cpp): the per-pixel values, the band, the rank rules and the summation order are written
// once, here, so the host build and the device give the same bits.  scoring.py is the NumPy statement of the same thing.
//
// Inputs per capture: depth (W*H), normal (W*H*3 interleaved, absent on both sides or on neither), hit (W*H bytes, non-zero
// = hit).  depth and normal are binary64 or binary32 per capture (ScoreMaps.fp64); binary32 is widened on read, which is
// exact: what np.asarray(..., float64) gives.
//
// Counts (int64), m = method hit, r = reference hit:
//   n_method_hit |m|, n_reference_hit |r|, n_co_hit |m & r|, n_union |m | r|,
//   n_co_hit_core, n_union_core   the same two over the pixels outside the band,
//   n_nan_depth, n_nan_angle      co-hit pixels whose depth gap / normal angle is NaN.
// Rates (IoU, false hit, false miss) are not formed here: Python divides the counts exactly as scoring.py does.
//
// Silhouette band (scoring.silhouette_band(reference hit, k)): a pixel is an EDGE pixel if its hit flag differs from that of
// any of its 4-neighbours that lie inside the image (pixels beyond the image are not neighbours: they do not count as
// misses); a pixel is in the band if an edge pixel lies within L1 distance k of it.  Inside a rectangle that equals k
// dilations by the 4-neighbourhood, since a shortest L1 path between two pixels of a rectangle stays inside it.  k in
// [0, kScoreMaxBand]; k < 0: no band, the core counts equal the full counts.  Made once per call, from the reference.
//
// Depth, over the n = n_co_hit co-hit pixels, gap = depth_m - depth_r:
//   depth_mae = sum|gap| / n, depth_rmse = rm_sqrt(sum(gap * gap) / n), depth_signed = sum(gap) / n,
//   depth_p95 and depth_med of |gap|; all NaN when n = 0.
// Normal angle, over the same pixels, when the captures carry normals:
//   cos = (a0 * b0 + a1 * b1) + a2 * b2 (unfused), clamped to [-1, 1] by np_max(-1, .) then np_min(1, .), which let a NaN
//   through as np.minimum(np.maximum(., -1), 1) does; angle = rm_acos<false>(cos) * 57.29577951308232;
//   normal_mean_deg = sum(angle) / n, normal_p95_deg; NaN when n = 0 or without normals.
//
// Percentiles are exact order statistics under NumPy's `linear` rule (np.percentile(x, 95)), s the ascending sample:
//   v = (double)(n - 1) * 0.95, j = floor(v), g = v - j, a = s[j], b = s[min(j + 1, n - 1)], d = b - a,
//   p95 = g < 0.5 ? a + d * g : b - d * (1 - g).
// The median is np.median, which is not the q = 50 case of that rule: s[n / 2] for odd n, (s[n / 2 - 1] + s[n / 2]) / 2.0
// for even n.  One NaN in a sample makes its percentile and median NaN (n_nan_* says so before any selection is read).
// Samples are non-negative, so their bit patterns order as uint64 (score_key); a pixel outside the sample carries
// kScoreNoKey, above every double.  The device selects s[j] by a most-significant-digit radix select over the keys and
// takes s[j + 1] from it (score_next_rank); the host check build sorts.
//
// Sums have the SSIM path's fixed order (rm_ssim.h): tiles of kSsimTileW x kSsimTileH pixels over the whole image, a
// tile's values row-major with +0.0 for a pixel outside the sample or the image, each tile folded by halves (ssim_fold),
// the tiles' partial sums added in tile index order (ssim_sum_in_order).  Every NaN output is the one quiet NaN
// 0x7ff8000000000000, whatever payload or sign the arithmetic of the host or the device would have left.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rm_interval.h"      // np_min, np_max
#include "rm_ssim.h"          // the tile size and the summation order

namespace rm {

constexpr int kScoreMaxBand = 8;                            // largest band_k
constexpr int kScoreMaxMethods = 65535;                     // a grid's z extent
constexpr uint64_t kScoreNoKey = ~0ull;                     // the key of a pixel outside the sample
constexpr int kScoreSums = 4;                               // per method: sum|gap|, sum gap^2, sum gap, sum angle
constexpr int kScoreSelects = 3;                            // per method: depth p95, depth median, angle p95
constexpr int kScoreCounts = 8;
constexpr double kScoreDegrees = 57.29577951308232;         // np.rad2deg

// one capture's maps (RmScoreMaps of the C ABI; device or host pointers)
struct ScoreMaps {
    const void* depth;
    const void* normal;
    const uint8_t* hit;
    int32_t fp64;
};

// RmScoreResult of the C ABI, field for field
struct ScoreResult {
    int64_t n_method_hit, n_reference_hit, n_co_hit, n_union, n_co_hit_core, n_union_core, n_nan_depth, n_nan_angle;
    double depth_mae, depth_rmse, depth_signed, depth_p95, depth_med, normal_mean_deg, normal_p95_deg;
};

enum { SC_METHOD = 0, SC_REFERENCE, SC_CO, SC_UNION, SC_CO_CORE, SC_UNION_CORE, SC_NAN_DEPTH, SC_NAN_ANGLE };

RM_HD double score_load(const void* map, size_t i, int fp64)
{
    return fp64 ? ((const double*)map)[i] : (double)((const float*)map)[i];
}

RM_HD uint64_t score_key(double nonneg)
{
    union { double d; uint64_t u; } c;
    c.d = nonneg;
    return c.u;
}

RM_HD double score_unkey(uint64_t key)
{
    union { double d; uint64_t u; } c;
    c.u = key;
    return c.d;
}

// every NaN becomes the quiet NaN 0x7ff8000000000000; decided on the bit pattern, which no floating-point rewrite of a
// compiler touches (`x != x ? nan : x` left the sign of a device NaN as it was)
RM_HD double score_canonical(double x)
{
    return (score_key(x) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull ? score_unkey(0x7ff8000000000000ull) : x;
}

// ---- the per-pixel values ------------------------------------------------------------------------------------------------

struct ScorePixel {
    bool mine, truth, core;        // method hit, reference hit, outside the band
    double gap, mag, angle;        // on a co-hit pixel: depth gap, |gap|, normal angle in degrees (0 without normals)
};

RM_HD double score_angle(const ScoreMaps& m, const ScoreMaps& r, size_t p)
{
    const double a0 = score_load(m.normal, 3 * p, m.fp64), a1 = score_load(m.normal, 3 * p + 1, m.fp64),
                 a2 = score_load(m.normal, 3 * p + 2, m.fp64);
    const double b0 = score_load(r.normal, 3 * p, r.fp64), b1 = score_load(r.normal, 3 * p + 1, r.fp64),
                 b2 = score_load(r.normal, 3 * p + 2, r.fp64);
    const double cosine = np_min(1.0, np_max(-1.0, (a0 * b0 + a1 * b1) + a2 * b2));      // a NaN stays
    return rm_acos<false>(cosine) * kScoreDegrees;
}

// pixel p of a method against the reference; band: the reference's band map, NULL without one
RM_HD ScorePixel score_pixel(const ScoreMaps& m, const ScoreMaps& r, const uint8_t* band, bool has_normal, size_t p)
{
    ScorePixel px;
    px.mine = m.hit[p] != 0;
    px.truth = r.hit[p] != 0;
    px.core = !band || !band[p];
    px.gap = px.mag = px.angle = 0.0;
    if (px.mine && px.truth) {
        px.gap = score_load(m.depth, p, m.fp64) - score_load(r.depth, p, r.fp64);
        px.mag = rm_fabs(px.gap);
        if (has_normal) px.angle = score_angle(m, r, p);
    }
    return px;
}

// ---- the silhouette band -------------------------------------------------------------------------------------------------

// c: a pixel's hit flag (0 / 1); l, r, u, d: its 4-neighbours' flags, 2 for a neighbour beyond the image
RM_HD bool score_is_edge(int c, int l, int r, int u, int d)
{
    return (l != 2 && l != c) || (r != 2 && r != c) || (u != 2 && u != c) || (d != 2 && d != c);
}

// edge(x, y): is pixel (x, y) an edge pixel (false beyond the image); true if one lies within L1 distance k of (x, y)
template <class Edge>
RM_HD bool score_in_band(const Edge& edge, int x, int y, int k)
{
    bool in = false;
    for (int dy = -k; dy <= k; ++dy) {
        const int w = k - (dy < 0 ? -dy : dy);
        for (int dx = -w; dx <= w; ++dx) in = in || edge(x + dx, y + dy);
    }
    return in;
}

// ---- ranks and the interpolation rules -------------------------------------------------------------------------------------

// the lower rank j each selection of a sample of n needs (its upper rank is min(j + 1, n - 1)); 0 for an empty sample
RM_HD int64_t score_rank_p95(int64_t n) { return n > 0 ? (int64_t)rm_floor((double)(n - 1) * 0.95) : 0; }
RM_HD int64_t score_rank_med(int64_t n) { return n > 0 ? (n % 2 ? n / 2 : n / 2 - 1) : 0; }

// s[j + 1] from s[j] without a second selection: `le` keys are <= s[j]; `above` is the least key greater than s[j]
// (kScoreNoKey without one)
RM_HD uint64_t score_next_rank(uint64_t sj, int64_t j, int64_t n, int64_t le, uint64_t above)
{
    if (j + 1 > n - 1) return sj;            // min(j + 1, n - 1) = j
    return le > j + 1 ? sj : above;
}

RM_HD double score_p95(double a, double b, int64_t n)
{
    const double v = (double)(n - 1) * 0.95, g = v - rm_floor(v), d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

RM_HD double score_median(double a, double b, int64_t n) { return n % 2 ? a : (a + b) / 2.0; }

// ---- tiles and the final combination -------------------------------------------------------------------------------------

RM_HD int score_tiles_x(int width) { return (width + kSsimTileW - 1) / kSsimTileW; }
RM_HD int score_tiles_y(int height) { return (height + kSsimTileH - 1) / kSsimTileH; }

// what the selections leave per method: s[j] and s[min(j + 1, n - 1)] of each of the kScoreSelects samples, as keys
struct ScoreRanks {
    uint64_t lo[kScoreSelects], hi[kScoreSelects];
};

// counts: kScoreCounts values (SC_*); sums: kScoreSums values in the fixed order
RM_HD void score_combine(const int64_t* counts, const double* sums, const ScoreRanks& k, bool has_normal, ScoreResult* out)
{
    const double nan = score_unkey(0x7ff8000000000000ull);
    out->n_method_hit = counts[SC_METHOD]; out->n_reference_hit = counts[SC_REFERENCE];
    out->n_co_hit = counts[SC_CO]; out->n_union = counts[SC_UNION];
    out->n_co_hit_core = counts[SC_CO_CORE]; out->n_union_core = counts[SC_UNION_CORE];
    out->n_nan_depth = counts[SC_NAN_DEPTH]; out->n_nan_angle = counts[SC_NAN_ANGLE];
    const int64_t n = counts[SC_CO];
    out->depth_mae = out->depth_rmse = out->depth_signed = out->depth_p95 = out->depth_med = nan;
    out->normal_mean_deg = out->normal_p95_deg = nan;
    if (n == 0) return;
    const double dn = (double)n;
    out->depth_mae = score_canonical(sums[0] / dn);
    out->depth_rmse = score_canonical(rm_sqrt(sums[1] / dn));
    out->depth_signed = score_canonical(sums[2] / dn);
    if (counts[SC_NAN_DEPTH] == 0) {
        out->depth_p95 = score_canonical(score_p95(score_unkey(k.lo[0]), score_unkey(k.hi[0]), n));
        out->depth_med = score_canonical(score_median(score_unkey(k.lo[1]), score_unkey(k.hi[1]), n));
    }
    if (!has_normal) return;
    out->normal_mean_deg = score_canonical(sums[3] / dn);
    if (counts[SC_NAN_ANGLE] == 0) out->normal_p95_deg = score_canonical(score_p95(score_unkey(k.lo[2]), score_unkey(k.hi[2]), n));
}

// ---- the device call (rm_score_captures and its launch_score, both in rm_score.hip) ---------------------------------------

// the state of one radix selection: the digits chosen so far, the rank left inside their group, the keys below the
// group and, after the last pass, the keys equal to the selected one
struct ScoreSelect {
    uint64_t prefix;
    int64_t rank, below, equal;
};

// Everything in device memory.  caps: nmethods + 1 ScoreMaps, the reference last.  band: W*H bytes (unused with band_k <
// 0).  keys: nmethods x (has_normal ? 2 : 1) x W*H sample keys (|gap|, then angle).  counts: nmethods x kScoreCounts.
// part: nmethods x kScoreSums x tiles.  sel: nmethods x kScoreSelects; hist: 256 bins for each; above: one key for each.
struct ScoreLaunch {
    int width, height, nmethods, has_normal, band_k;
    const ScoreMaps* caps;
    uint8_t* band;
    uint64_t* keys;
    unsigned long long* counts;
    double* part;
    ScoreSelect* sel;
    uint32_t* hist;
    unsigned long long* above;
    ScoreResult* out;
};

}  // namespace rm
