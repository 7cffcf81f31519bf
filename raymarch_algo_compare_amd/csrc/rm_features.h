// rm_features.h -- the strategy-independent discovery features of a (scene, viewpoint): five view features of a dense-march
// capture and two intrinsic features of the scene's SDF sampled in the box of the visible geometry (the reference's
// report/features.py).  Shared by the gfx950 kernels (rm_features.hip), the C ABI (rm_intrinsic_features,
// rm_view_features) and the host check build (tests/native/features_check.cpp): the per-element bodies, the run detection,
// the rank rules, the summation order, the limits and the argument checks are written once, here, so the host build and
// the device give the same bits.  features.py holds the NumPy statement of the same thing.
//
// Intrinsic features, per sample set (a set = n_lip points, n_chords chords a -> b with their lengths, shared ts):
//   Points.  Each Lipschitz sample p gives six points, k = 2 * axis + (0: plus, 1: minus): p + e and p - e componentwise
//   with e = eps on the axis and +0.0 on the other two (NumPy's `pts + e`: the sum with +0.0 turns a -0.0 coordinate into
//   +0.0, the difference leaves it).  Each chord gives chord_steps points a + ts[i] * (b - a), unfused.  All sets' offset
//   points come first in the one xyz buffer (set, sample, k), then all chord points (set, chord, step).
//   Gradient.  g_axis = (f(p + e) - f(p - e)) / (2 * eps), 2 * eps formed once; gmag = sqrt((gx * gx + gy * gy) + gz * gz).
//   A non-finite gmag leaves the sample.  lipschitz_p99 = np.percentile(gmag, 99): rm_score.h's rule with 0.99.
//   Chords.  inside = f < 0 (a NaN is outside).  A run is a maximal stretch of inside samples [start, end); its length is
//   (double)(end - start) * (seglen / (double)(chord_steps - 1)).  A chord has at most ceil(chord_steps / 2) runs; run r of
//   chord c of set s sits in slot (s * n_chords + c) * feat_max_runs(chord_steps) + r, the chord's count beside it.
//   slab_median = np.median of all run lengths of the set (not divided by the box diagonal: the caller does that).
//   Both samples are non-negative (seglen is a length: an element that is NaN or has its sign bit set is refused, +inf is
//   valid), so their bit patterns order as uint64 (score_key).  An empty sample gives the one quiet
//   NaN 0x7ff8000000000000 and a count of 0.
//
// View features, per capture of width x height pixels (depth, normal xyz, evals as binary32; hit bytes, non-zero = hit),
// with (o, rd) = camera_ray of the pixel (rm_camera.h: the ray the march shot):
//   n_hit; n_grazing: hit and |(rd.x * (double)n.x + rd.y * (double)n.y) + rd.z * (double)n.z| < 0.20; n_perimeter: hit with
//   a non-hit 4-neighbour, a neighbour beyond the image being a non-hit; sum_evals: the exact integer sum of evals over hits;
//   box: per-axis min / max of o + (double)depth * rd over hits (+inf / -inf without a hit).
//   Evals are counts: integers in [0, 2^24], every one of which a binary32 holds.  feat_evals_count turns the float into the
//   integer that is summed, averaged and deviated from: a NaN or a negative value is 0, a value above 2^24 (+inf too) is
//   2^24, anything else is truncated; a count keeps every bit.  (The reference reads evals from its own integer map and
//   has no treatment of other values.)
//   A box axis over which any hit point's coordinate is NaN -- a NaN depth, or an infinite one times a zero ray component --
//   is the quiet NaN 0x7ff8000000000000 in box_lo and in box_hi, wherever the pixel sits (NumPy's min / max); feat_box_min
//   and feat_box_max are the one statement of it, for a tile's fold, the fold over tiles and the host build's loop.
//   hit_rate = n_hit / (W * H); grazing_frac = n_grazing / n_hit; silhouette_cplx = n_perimeter / sqrt(n_hit);
//   hardness_mean = sum_evals / n_hit (exact sum, one rounding: what np.mean gives while the sum is below 2^53);
//   hardness_cv = sqrt(sum((evals - mean)^2) / n_hit) / mean, 0 when the mean is 0; all four 0 without a hit.
//   The one floating-point sum has rm_ssim.h's fixed order: tiles of kSsimTileW x kSsimTileH pixels, a tile's values
//   row-major with +0.0 off the sample, folded by halves, the tiles' partial sums added in tile index order.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "rm_camera.h"
#include "rm_score.h"         // score_key, the rank rules, the tile helpers

namespace rm {

constexpr int kFeatMaxSets = 256;
constexpr int kFeatMaxLip = 65536;
constexpr int kFeatMaxChords = 4096;
constexpr int kFeatMinSteps = 2, kFeatMaxSteps = 1024;
constexpr int kFeatMaxViews = 65535;                        // a grid's y extent
constexpr int kFeatMaxChunks = kFeatMaxSteps / 64;          // ballots per chord
constexpr double kFeatGrazingCos = 0.20;
constexpr double kFeatLipQuantile = 0.99;

// RmIntrinsicFeatures of the C ABI, field for field
struct IntrinsicFeatures {
    double lipschitz_p99, slab_median;
    int64_t n_finite, n_slabs;
};

// RmViewMaps of the C ABI (device or host pointers)
struct ViewMaps {
    const float* depth;
    const float* normal;
    const float* evals;
    const uint8_t* hit;
};

// RmViewFeatures of the C ABI, field for field
struct ViewFeatures {
    int64_t n_hit, n_grazing, n_perimeter, sum_evals;
    double hit_rate, grazing_frac, silhouette_cplx, hardness_mean, hardness_cv;
    double box_lo[3], box_hi[3];
};

RM_HD double feat_nan() { return score_unkey(0x7ff8000000000000ull); }
RM_HD double feat_inf(bool negative) { return score_unkey(negative ? 0xfff0000000000000ull : 0x7ff0000000000000ull); }
RM_HD bool feat_is_finite(double x) { return (score_key(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// ---- argument checks (the reason, or NULL for valid arguments) ---------------------------------------------------------

inline const char* feat_check_intrinsic(int32_t nsets, int32_t n_lip, const double* pts, double lip_eps, int32_t n_chords,
                                        const double* chords, const double* seglen, int32_t chord_steps, const double* ts,
                                        const void* out)
{
    if (nsets < 1 || nsets > kFeatMaxSets) return "nsets outside [1, 256]";
    if (n_lip < 0 || n_lip > kFeatMaxLip) return "n_lip outside [0, 65536]";
    if (n_chords < 0 || n_chords > kFeatMaxChords) return "n_chords outside [0, 4096]";
    if (chord_steps < kFeatMinSteps || chord_steps > kFeatMaxSteps) return "chord_steps outside [2, 1024]";
    if (!feat_is_finite(lip_eps) || !(lip_eps > 0.0)) return "lip_eps is not a positive finite number";
    if (!out) return "out is NULL";
    if (n_lip > 0 && !pts) return "pts is NULL";
    if (n_chords > 0 && (!chords || !seglen)) return "chords or seglen is NULL";
    if (!ts) return "ts is NULL";
    return nullptr;
}

// The second half of rm_intrinsic_features' argument check, for arguments feat_check_intrinsic has passed: it reads the
// nsets x n_chords lengths.  seglen is a length: the key order needs a clear sign bit (-0.0 is refused with the negatives)
// and a NaN has no place in it; +inf is a length.  The reason names the first refused element.
inline const char* feat_check_seglen(int32_t nsets, int32_t n_chords, const double* seglen)
{
    for (size_t i = 0; i < (size_t)nsets * (size_t)n_chords; ++i)
        if (score_key(seglen[i]) > 0x7ff0000000000000ull) {
            static thread_local char why[64];
            snprintf(why, sizeof why, "seglen[%zu] is NaN or negative", i);
            return why;
        }
    return nullptr;
}

inline const char* feat_check_view(int32_t nviews, const double* cams, const void* maps, const void* out)
{
    if (!cams || !maps || !out) return "cams, maps or out is NULL";
    if (nviews < 1 || nviews > kFeatMaxViews) return "nviews outside [1, 65535]";
    return nullptr;
}

// ---- the sample points -------------------------------------------------------------------------------------------------

RM_HD int feat_max_runs(int chord_steps) { return (chord_steps + 1) / 2; }
RM_HD size_t feat_lip_points(int nsets, int n_lip) { return (size_t)nsets * (size_t)n_lip * 6; }
RM_HD size_t feat_chord_points(int nsets, int n_chords, int chord_steps) { return (size_t)nsets * (size_t)n_chords * (size_t)chord_steps; }

// offset point k (2 * axis + minus) of the sample p
RM_HD void feat_offset_point(const double* p, double eps, int k, double* out)
{
    const int axis = k >> 1;
    const bool minus = (k & 1) != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double e = j == axis ? eps : 0.0;
        out[j] = minus ? p[j] - e : p[j] + e;
    }
}

// sample `t` of the chord ab (a, then b)
RM_HD void feat_chord_point(const double* ab, double t, double* out)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = ab[j] + t * (ab[3 + j] - ab[j]);
}

// point i of the xyz buffer of a call (feat_lip_points, then feat_chord_points)
RM_HD void feat_point(size_t i, int nsets, int n_lip, int n_chords, int chord_steps, double eps, const double* pts, const double* chords,
                      const double* ts, double* out)
{
    const size_t nl = feat_lip_points(nsets, n_lip);
    if (i < nl) {
        feat_offset_point(pts + (i / 6) * 3, eps, (int)(i % 6), out);
        return;
    }
    const size_t j = i - nl;
    feat_chord_point(chords + (j / (size_t)chord_steps) * 6, ts[j % (size_t)chord_steps], out);
}

// ---- the gradient ------------------------------------------------------------------------------------------------------

// f: the six values of a sample's offset points; two_eps = 2.0 * eps
RM_HD double feat_gmag(const double* f, double two_eps)
{
    const double gx = (f[0] - f[1]) / two_eps, gy = (f[2] - f[3]) / two_eps, gz = (f[4] - f[5]) / two_eps;
    return rm_sqrt((gx * gx + gy * gy) + gz * gz);
}

// ---- runs of inside samples ----------------------------------------------------------------------------------------------

// bit i of a mask = sample 64 * chunk + i is inside.  prev: the last bit of the chunk before (0 for the first chunk);
// next: the first bit of the chunk after (0 for the last one).  A run starts at a set bit whose predecessor is clear and
// ends after a set bit whose successor is clear.
RM_HD uint64_t feat_run_starts(uint64_t mask, uint64_t prev) { return mask & ~((mask << 1) | (prev & 1ull)); }
RM_HD uint64_t feat_run_ends(uint64_t mask, uint64_t next) { return mask & ~((mask >> 1) | ((next & 1ull) << 63)); }

RM_HD int feat_popcount(uint64_t x) { return __builtin_popcountll(x); }
RM_HD int feat_chunks(int chord_steps) { return (chord_steps + 63) / 64; }

RM_HD double feat_step_length(double seglen, int chord_steps) { return seglen / (double)(chord_steps - 1); }
RM_HD double feat_run_length(int start, int end, double step_len) { return (double)(end - start) * step_len; }

// The runs of one chord from its masks (bits beyond chord_steps clear), on one thread: writes their lengths as keys in
// order and returns their number.  The device finds the same (start, end) pairs a lane per sample (chord_kernel).
inline int feat_chord_runs(const uint64_t* masks, int chord_steps, double seglen, uint64_t* keys)
{
    const int nchunks = feat_chunks(chord_steps);
    const double step_len = feat_step_length(seglen, chord_steps);
    int nstart = 0, nend = 0, start[kFeatMaxSteps / 2 + 1];
    for (int c = 0; c < nchunks; ++c) {
        uint64_t s = feat_run_starts(masks[c], c ? masks[c - 1] >> 63 : 0);
        for (; s; s &= s - 1) start[nstart++] = 64 * c + __builtin_ctzll(s);
    }
    for (int c = 0; c < nchunks; ++c) {
        uint64_t e = feat_run_ends(masks[c], c + 1 < nchunks ? masks[c + 1] : 0);
        for (; e; e &= e - 1, ++nend) keys[nend] = score_key(feat_run_length(start[nend], 64 * c + __builtin_ctzll(e) + 1, step_len));
    }
    return nend;
}

// ---- ranks and the two statistics -----------------------------------------------------------------------------------------

// rm_score.h's percentile rule with q in place of 0.95
RM_HD int64_t feat_rank_quantile(int64_t n, double q) { return n > 0 ? (int64_t)rm_floor((double)(n - 1) * q) : 0; }
RM_HD double feat_quantile(double a, double b, int64_t n, double q)
{
    const double v = (double)(n - 1) * q, g = v - rm_floor(v), d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

// selection 0: the p99 of gmag; selection 1: the median of the run lengths.  lo, hi: the keys s[j] and s[min(j + 1, n - 1)]
RM_HD int64_t feat_rank(int sel, int64_t n) { return sel == 0 ? feat_rank_quantile(n, kFeatLipQuantile) : score_rank_med(n); }
RM_HD double feat_statistic(int sel, uint64_t lo, uint64_t hi, int64_t n)
{
    if (n == 0) return feat_nan();
    const double a = score_unkey(lo), b = score_unkey(hi);
    return score_canonical(sel == 0 ? feat_quantile(a, b, n, kFeatLipQuantile) : score_median(a, b, n));
}

// ---- the view features -----------------------------------------------------------------------------------------------------

struct ViewPixel {
    bool hit, grazing, perimeter;
    int64_t evals;             // on a hit, else 0
    double p[3];               // the hit point
};

constexpr int64_t kFeatMaxEvals = 1 << 24;

// the count a pixel's evals stand for (the header comment): a NaN fails both comparisons
RM_HD int64_t feat_evals_count(float evals) { return evals >= (float)kFeatMaxEvals ? kFeatMaxEvals : evals >= 0.0f ? (int64_t)evals : 0; }

// one step of a box corner's fold; a NaN on either side stays
RM_HD double feat_box_min(double m, double p) { return m != m || p != p ? feat_nan() : (p < m ? p : m); }
RM_HD double feat_box_max(double m, double p) { return m != m || p != p ? feat_nan() : (p > m ? p : m); }

RM_HD ViewPixel feat_view_pixel(const ViewMaps& m, const CameraParams& cam, int width, int height, int x, int y)
{
    const size_t i = (size_t)y * (size_t)width + (size_t)x;
    ViewPixel px;
    px.hit = m.hit[i] != 0;
    px.grazing = px.perimeter = false;
    px.evals = 0;
    px.p[0] = px.p[1] = px.p[2] = 0.0;
    if (!px.hit) return px;
    vec3 o, rd;
    camera_ray(cam, width, height, x, y, o, rd);
    const double cosine = (rd.x * (double)m.normal[3 * i] + rd.y * (double)m.normal[3 * i + 1]) + rd.z * (double)m.normal[3 * i + 2];
    px.grazing = rm_fabs(cosine) < kFeatGrazingCos;
    px.perimeter = x == 0 || y == 0 || x == width - 1 || y == height - 1 || !m.hit[i - 1] || !m.hit[i + 1] ||
                   !m.hit[i - (size_t)width] || !m.hit[i + (size_t)width];
    px.evals = feat_evals_count(m.evals[i]);
    const double t = (double)m.depth[i];
    px.p[0] = o.x + t * rd.x; px.p[1] = o.y + t * rd.y; px.p[2] = o.z + t * rd.z;
    return px;
}

enum { VC_HIT = 0, VC_GRAZING, VC_PERIMETER, VC_EVALS, kViewCounts };

RM_HD double feat_mean_evals(int64_t sum_evals, int64_t n_hit) { return (double)sum_evals / (double)n_hit; }

// counts: kViewCounts integers; ssq: the sum of (evals - mean)^2 over hits in the fixed order; lo, hi: the box
RM_HD void feat_view_combine(int width, int height, const int64_t* counts, double ssq, const double* lo, const double* hi, ViewFeatures* out)
{
    const int64_t n = counts[VC_HIT];
    out->n_hit = n; out->n_grazing = counts[VC_GRAZING]; out->n_perimeter = counts[VC_PERIMETER]; out->sum_evals = counts[VC_EVALS];
    out->hit_rate = (double)n / (double)((int64_t)width * (int64_t)height);
    out->grazing_frac = out->silhouette_cplx = out->hardness_mean = out->hardness_cv = 0.0;
    for (int j = 0; j < 3; ++j) { out->box_lo[j] = n ? lo[j] : feat_inf(false); out->box_hi[j] = n ? hi[j] : feat_inf(true); }
    if (n == 0) return;
    const double dn = (double)n, mean = feat_mean_evals(counts[VC_EVALS], n);
    out->grazing_frac = (double)counts[VC_GRAZING] / dn;
    out->silhouette_cplx = (double)counts[VC_PERIMETER] / rm_sqrt(dn);
    out->hardness_mean = mean;
    out->hardness_cv = mean > 0.0 ? rm_sqrt(ssq / dn) / mean : 0.0;
}

// ---- the device calls (rm_features.hip) ------------------------------------------------------------------------------------

// Everything in device memory.  xyz: 3 doubles per point, f: one per point (feat_lip_points + feat_chord_points).  gkeys:
// nsets x n_lip keys of gmag (kScoreNoKey: left out).  slabs: nsets x n_chords x feat_max_runs keys, counts: nsets x n_chords.
// gmag_out (optional): nsets x n_lip doubles, NaN = left out.
struct IntrinsicLaunch {
    int nsets, n_lip, n_chords, chord_steps;
    double eps;
    const double *pts, *chords, *seglen, *ts;
    double* xyz;
    double* f;
    uint64_t* gkeys;
    uint64_t* slabs;
    int32_t* counts;
    double* gmag_out;
    IntrinsicFeatures* out;
};

// maps: nviews ViewMaps, cams: nviews CameraParams.  icounts: nviews x kViewCounts x tiles integers, box: nviews x 6 x tiles
// (lo xyz, hi xyz), mean: nviews doubles, part: nviews x tiles partial sums of (evals - mean)^2.
struct ViewLaunch {
    int width, height, nviews;
    const ViewMaps* maps;
    const CameraParams* cams;
    long long* icounts;
    double* box;
    double* mean;
    double* part;
    ViewFeatures* out;
};

}  // namespace rm
