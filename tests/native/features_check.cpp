// Host-only check build of the discovery features (csrc/rm_features.h) -- compiled by g++ for tests ONLY, so the sample
// points, the gradient, the run detection, the rank rules and the view features the gfx950 kernels are built from can be
// compared with the reference's recorded results, with features.py and with the device in a container without a GPU.  Never
// loaded by the product.  The SDF values come from the caller (the CPU oracle's point evaluation).
//
// The loops below walk the data as rm_features.hip's kernels do: a chord's masks 64 samples at a time, the image tile by
// tile with a tile's 256 values folded by halves and the tiles' partial sums added in index order.  A plain sort stands in
// for the radix select: s[j] is read from the sorted keys and s[j + 1] is taken from it by score_next_rank exactly as the
// device takes it; the calls answer 2 if that is not the sorted sample's next element.  rmft_runs_by_lanes finds the runs
// the way feat_chord_kernel does, a lane per sample, and must agree with feat_chord_runs.
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../raymarch_algo_compare_amd/csrc/rm_features.h"

using namespace rm;

namespace {

// selection `sel` of the keys (sorted here); 0, or 2 when score_next_rank disagrees with the sorted sample
int select(int sel, std::vector<uint64_t>& keys, double* value)
{
    std::sort(keys.begin(), keys.end());
    const int64_t n = (int64_t)keys.size();
    if (n == 0) { *value = feat_statistic(sel, 0, 0, 0); return 0; }
    const int64_t j = feat_rank(sel, n);
    const uint64_t sj = keys[(size_t)j];
    const auto up = std::upper_bound(keys.begin(), keys.end(), sj);
    const uint64_t hi = score_next_rank(sj, j, n, (int64_t)(up - keys.begin()), up == keys.end() ? kScoreNoKey : *up);
    *value = feat_statistic(sel, sj, hi, n);
    return hi == keys[(size_t)std::min(j + 1, n - 1)] ? 0 : 2;
}

void masks_of(int steps, const uint8_t* inside, uint64_t* masks)
{
    for (int c = 0; c <= kFeatMaxChunks; ++c) masks[c] = 0;
    for (int i = 0; i < steps; ++i)
        if (inside[i]) masks[i / 64] |= 1ull << (i % 64);
}

}  // namespace

extern "C" {

// the reason an argument set of rm_intrinsic_features is refused, NULL for a valid one
const char* rmft_check_intrinsic(int32_t nsets, int32_t n_lip, const double* pts, double lip_eps, int32_t n_chords, const double* chords,
                                 const double* seglen, int32_t chord_steps, const double* ts, const void* out)
{
    return feat_check_intrinsic(nsets, n_lip, pts, lip_eps, n_chords, chords, seglen, chord_steps, ts, out);
}

// ... and of its lengths, which rm_intrinsic_features checks once the arguments above are in order
const char* rmft_check_seglen(int32_t nsets, int32_t n_chords, const double* seglen) { return feat_check_seglen(nsets, n_chords, seglen); }

size_t rmft_num_points(int nsets, int n_lip, int n_chords, int steps) { return feat_lip_points(nsets, n_lip) + feat_chord_points(nsets, n_chords, steps); }

// the xyz buffer of a call: 3 doubles per point
void rmft_points(int nsets, int n_lip, int n_chords, int steps, double eps, const double* pts, const double* chords, const double* ts,
                 double* xyz)
{
    const size_t n = rmft_num_points(nsets, n_lip, n_chords, steps);
    for (size_t i = 0; i < n; ++i) feat_point(i, nsets, n_lip, n_chords, steps, eps, pts, chords, ts, xyz + 3 * i);
}

// the rest of rm_intrinsic_features from the values f of those points; gmag_out and counts_out may be NULL
int rmft_intrinsic(int nsets, int n_lip, int n_chords, int steps, double eps, const double* seglen, const double* f, IntrinsicFeatures* out,
                   double* gmag_out, int32_t* counts_out)
{
    int rc = 0;
    const double* fc = f + feat_lip_points(nsets, n_lip);
    for (int s = 0; s < nsets; ++s) {
        std::vector<uint64_t> gk, sk;
        for (int i = 0; i < n_lip; ++i) {
            const size_t at = (size_t)s * n_lip + i;
            const double g = feat_gmag(f + 6 * at, 2.0 * eps);
            const bool keep = feat_is_finite(g);
            if (keep) gk.push_back(score_key(g));
            if (gmag_out) gmag_out[at] = keep ? g : feat_nan();
        }
        for (int c = 0; c < n_chords; ++c) {
            const size_t chord = (size_t)s * n_chords + c;
            uint64_t masks[kFeatMaxChunks + 1] = { 0 }, keys[kFeatMaxSteps / 2 + 1];
            for (int i = 0; i < steps; ++i)
                if (fc[chord * steps + i] < 0.0) masks[i / 64] |= 1ull << (i % 64);
            const int runs = feat_chord_runs(masks, steps, seglen[chord], keys);
            if (runs > feat_max_runs(steps)) rc = 3;
            sk.insert(sk.end(), keys, keys + runs);
            if (counts_out) counts_out[chord] = runs;
        }
        out[s].n_finite = (int64_t)gk.size();
        out[s].n_slabs = (int64_t)sk.size();
        rc |= select(0, gk, &out[s].lipschitz_p99);
        rc |= select(1, sk, &out[s].slab_median);
    }
    return rc;
}

// the runs of one chord from its inside flags: lengths in order, the count returned
int rmft_runs(int steps, const uint8_t* inside, double seglen, double* lengths)
{
    uint64_t masks[kFeatMaxChunks + 1], keys[kFeatMaxSteps / 2 + 1];
    masks_of(steps, inside, masks);
    const int n = feat_chord_runs(masks, steps, seglen, keys);
    for (int i = 0; i < n; ++i) lengths[i] = score_unkey(keys[i]);
    return n;
}

// the same, found as feat_chord_kernel finds them: every lane looks at its own bit of each mask
int rmft_runs_by_lanes(int steps, const uint8_t* inside, double seglen, double* lengths)
{
    uint64_t mask[kFeatMaxChunks + 1];
    masks_of(steps, inside, mask);
    const int nchunks = feat_chunks(steps);
    const double step_len = feat_step_length(seglen, steps);
    int start[kFeatMaxSteps / 2 + 1], nstart = 0, nend = 0;
    for (int c = 0; c < nchunks; ++c) {
        const uint64_t s = feat_run_starts(mask[c], c ? mask[c - 1] >> 63 : 0);
        for (int lane = 0; lane < 64; ++lane)
            if ((s >> lane) & 1ull) start[nstart + feat_popcount(s & ((1ull << lane) - 1ull))] = 64 * c + lane;
        nstart += feat_popcount(s);
    }
    for (int c = 0; c < nchunks; ++c) {
        const uint64_t e = feat_run_ends(mask[c], mask[c + 1]);
        for (int lane = 0; lane < 64; ++lane)
            if ((e >> lane) & 1ull) {
                const int r = nend + feat_popcount(e & ((1ull << lane) - 1ull));
                if (r >= nstart) return -1;
                lengths[r] = feat_run_length(start[r], 64 * c + lane + 1, step_len);
            }
        nend += feat_popcount(e);
    }
    return nend == nstart ? nend : -1;
}

// selection 0 (p99) or 1 (median) of n non-negative values
int rmft_select(int sel, int64_t n, const double* values, double* out)
{
    std::vector<uint64_t> keys;
    for (int64_t i = 0; i < n; ++i) keys.push_back(score_key(values[i]));
    return select(sel, keys, out);
}

// rm_view_features of one capture
int rmft_view(int W, int H, const double* cam14, const float* depth, const float* normal, const float* evals, const uint8_t* hit,
              ViewFeatures* out)
{
    if (W <= 0 || H <= 0 || feat_check_view(1, cam14, depth, out) || !depth || !normal || !evals || !hit) return -1;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ViewMaps m = { depth, normal, evals, hit };
    const int tx = score_tiles_x(W), ty = score_tiles_y(H);
    int64_t counts[kViewCounts] = { 0, 0, 0, 0 };
    double lo[3] = { feat_inf(false), feat_inf(false), feat_inf(false) }, hi[3] = { feat_inf(true), feat_inf(true), feat_inf(true) };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const ViewPixel px = feat_view_pixel(m, cam, W, H, x, y);
            counts[VC_HIT] += px.hit; counts[VC_GRAZING] += px.grazing; counts[VC_PERIMETER] += px.perimeter;
            counts[VC_EVALS] += px.evals;
            if (!px.hit) continue;
            for (int j = 0; j < 3; ++j) { lo[j] = feat_box_min(lo[j], px.p[j]); hi[j] = feat_box_max(hi[j], px.p[j]); }
        }
    const double mean = counts[VC_HIT] ? feat_mean_evals(counts[VC_EVALS], counts[VC_HIT]) : 0.0;
    std::vector<double> part((size_t)tx * ty);
    for (int t = 0; t < tx * ty; ++t) {
        const int x0 = (t % tx) * kSsimTileW, y0 = (t / tx) * kSsimTileH;
        double v[kSsimTile];
        for (int i = 0; i < kSsimTile; ++i) {
            const int x = x0 + i % kSsimTileW, y = y0 + i / kSsimTileW;
            v[i] = 0.0;
            if (x >= W || y >= H || !hit[(size_t)y * W + x]) continue;
            const double d = (double)feat_evals_count(evals[(size_t)y * W + x]) - mean;
            v[i] = d * d;
        }
        part[t] = ssim_fold(v);
    }
    feat_view_combine(W, H, counts, ssim_sum_in_order(part.data(), tx * ty), lo, hi, out);
    return 0;
}

}
