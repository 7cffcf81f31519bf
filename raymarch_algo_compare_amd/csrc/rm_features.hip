// rm_features.hip -- the discovery features of a (scene, viewpoint) on the device (rm_features.h; rm_intrinsic_features and
// rm_view_features in include/rm_hip.h).
//
// Intrinsic features, all on one stream; the scene's own sdf_eval launcher runs between the first two (rm_intrinsic_features):
//   feat_points_kernel    one point per thread: the six offset points of every Lipschitz sample, then every chord sample
//   feat_grad_kernel      one Lipschitz sample per thread: gmag and its key (kScoreNoKey when it is not finite)
//   feat_chord_kernel     one wavefront per chord: `f < 0` as one ballot per 64 samples, run starts and ends from the masks
//                         by bit operations, each run's length into the chord's own slots and the run count beside them
//   feat_select_kernel    one workgroup per (selection, set): counts the sample, then a most-significant-digit radix select
//                         over its keys, 8 bits a pass, with the histogram in LDS; s[j + 1] from the least key above s[j]
//                         (score_next_rank); the p99 of gmag and the median of the run lengths
// View features:
//   view_tile_kernel      one workgroup per (tile, view), one pixel per thread: the pixel's flags (ballot + popcount per
//                         wave), its evals as a count (feat_evals_count), the hit point's box (feat_box_min / _max: a NaN
//                         coordinate stays); per-tile integers and boxes into fixed slots
//   view_mean_kernel      one workgroup per view: the tiles' integers and boxes in tile order; the mean of evals
//   view_var_kernel       one workgroup per (tile, view): (evals - mean)^2 folded by halves into the tile's partial sum
//   view_finish_kernel    one thread per view: the partial sums in tile order, feat_view_combine
// No atomics on floating-point values, no slot that depends on scheduling: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "rm_features.h"
#include "rm_capi_internal.h"

namespace rm {

static_assert(kSsimTile == 256, "one pixel per thread of a 256-thread workgroup");
static_assert(kFeatMaxChunks == 16, "a chord's masks fit 16 ballots");

// ---- intrinsic -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void feat_points_kernel(IntrinsicLaunch a, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double p[3];
    feat_point(i, a.nsets, a.n_lip, a.n_chords, a.chord_steps, a.eps, a.pts, a.chords, a.ts, p);
    a.xyz[3 * i] = p[0]; a.xyz[3 * i + 1] = p[1]; a.xyz[3 * i + 2] = p[2];
}

__global__ __launch_bounds__(256) void feat_grad_kernel(IntrinsicLaunch a, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = a.f[6 * i + k];
    const double g = feat_gmag(f, 2.0 * a.eps);
    const bool keep = feat_is_finite(g);
    a.gkeys[i] = keep ? score_key(g) : kScoreNoKey;
    if (a.gmag_out) a.gmag_out[i] = keep ? g : feat_nan();
}

// one 64-thread workgroup (one wavefront) per chord
__global__ __launch_bounds__(64) void feat_chord_kernel(IntrinsicLaunch a)
{
    const int lane = (int)threadIdx.x;
    const size_t chord = blockIdx.x;                                     // set * n_chords + chord of the set
    const int steps = a.chord_steps, nchunks = feat_chunks(steps), max_runs = feat_max_runs(steps);
    const double* f = a.f + feat_lip_points(a.nsets, a.n_lip) + chord * (size_t)steps;
    __shared__ uint64_t mask[kFeatMaxChunks + 1];
    __shared__ int start[kFeatMaxSteps / 2 + 1];
    for (int c = 0; c < nchunks; ++c) {
        const int i = 64 * c + lane;
        const uint64_t m = __ballot(i < steps && f[i] < 0.0);
        if (lane == 0) mask[c] = m;
    }
    if (lane == 0) mask[nchunks] = 0;
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;                        // the lanes before this one
    int nstart = 0;
    for (int c = 0; c < nchunks; ++c) {
        const uint64_t s = feat_run_starts(mask[c], c ? mask[c - 1] >> 63 : 0);
        if ((s >> lane) & 1ull) start[nstart + feat_popcount(s & below)] = 64 * c + lane;
        nstart += feat_popcount(s);
    }
    __syncthreads();
    const double step_len = feat_step_length(a.seglen[chord], steps);
    uint64_t* keys = a.slabs + chord * (size_t)max_runs;
    int nend = 0;
    for (int c = 0; c < nchunks; ++c) {
        const uint64_t e = feat_run_ends(mask[c], mask[c + 1]);
        if ((e >> lane) & 1ull) {
            const int r = nend + feat_popcount(e & below);               // r < nstart <= max_runs: every end has its start
            keys[r] = score_key(feat_run_length(start[r], 64 * c + lane + 1, step_len));
        }
        nend += feat_popcount(e);
    }
    if (lane == 0) a.counts[chord] = nend;
}

// key i of selection `sel` of set `set`; kScoreNoKey for an element outside the sample
__device__ __forceinline__ uint64_t feat_key(const IntrinsicLaunch& a, int sel, int set, size_t i, int max_runs)
{
    if (sel == 0) return a.gkeys[(size_t)set * (size_t)a.n_lip + i];
    const size_t chord = (size_t)set * (size_t)a.n_chords + i / (size_t)max_runs;
    const int r = (int)(i % (size_t)max_runs);
    return r < a.counts[chord] ? a.slabs[chord * (size_t)max_runs + (size_t)r] : kScoreNoKey;
}

__global__ __launch_bounds__(256) void feat_select_kernel(IntrinsicLaunch a)
{
    const int t = (int)threadIdx.x, sel = (int)blockIdx.x, set = (int)blockIdx.y;
    const int max_runs = feat_max_runs(a.chord_steps);
    const size_t items = sel == 0 ? (size_t)a.n_lip : (size_t)a.n_chords * (size_t)max_runs;
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long least[256];
    __shared__ uint64_t prefix;
    __shared__ long long rank, below, equal, total;

    hist[t] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (size_t i = t; i < items; i += 256) mine += feat_key(a, sel, set, i, max_runs) != kScoreNoKey;
    hist[t] = mine;
    __syncthreads();
    if (t == 0) {
        long long n = 0;
        for (int b = 0; b < 256; ++b) n += hist[b];
        total = n; prefix = 0; below = 0; equal = 0;
        rank = feat_rank(sel, n);
    }
    __syncthreads();
    const long long n = total;
    if (n == 0) {                                                        // uniform: every thread read the same word
        if (t == 0) {
            if (sel == 0) { a.out[set].lipschitz_p99 = feat_nan(); a.out[set].n_finite = 0; }
            else { a.out[set].slab_median = feat_nan(); a.out[set].n_slabs = 0; }
        }
        return;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        const uint64_t pre = prefix;
        for (size_t i = t; i < items; i += 256) {
            const uint64_t key = feat_key(a, sel, set, i, max_runs);
            if (key == kScoreNoKey) continue;
            if (shift == 56 || (key >> (shift + 8)) == pre) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (t == 0) {
            long long seen = 0;
            for (int b = 0; b < 256; ++b) {
                const long long c = hist[b];
                if (c && seen <= rank && rank < seen + c) {
                    prefix = (pre << 8) | (uint64_t)b;
                    rank -= seen; below += seen; equal = c;
                    break;
                }
                seen += c;
            }
        }
        __syncthreads();
    }
    const uint64_t sj = prefix;
    uint64_t above = kScoreNoKey;
    for (size_t i = t; i < items; i += 256) {
        const uint64_t key = feat_key(a, sel, set, i, max_runs);
        if (key > sj && key < above) above = key;                        // kScoreNoKey is never below `above`
    }
    least[t] = above;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h && least[t + h] < least[t]) least[t] = least[t + h];
        __syncthreads();
    }
    if (t != 0) return;
    const int64_t j = feat_rank(sel, n);
    const uint64_t hi = score_next_rank(sj, j, n, below + equal, (uint64_t)least[0]);
    const double v = feat_statistic(sel, sj, hi, n);
    if (sel == 0) { a.out[set].lipschitz_p99 = v; a.out[set].n_finite = n; }
    else { a.out[set].slab_median = v; a.out[set].n_slabs = n; }
}

// the kernels before the scene's sdf_eval: the points
static hipError_t launch_feature_points(const IntrinsicLaunch& a, hipStream_t s)
{
    const size_t n = feat_lip_points(a.nsets, a.n_lip) + feat_chord_points(a.nsets, a.n_chords, a.chord_steps);
    if (n) hipLaunchKernelGGL(feat_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, n);
    return hipGetLastError();
}

// ... and after it: gradients, runs, selections
static hipError_t launch_feature_reduce(const IntrinsicLaunch& a, hipStream_t s)
{
    const size_t nl = (size_t)a.nsets * (size_t)a.n_lip, nc = (size_t)a.nsets * (size_t)a.n_chords;
    if (nl) hipLaunchKernelGGL(feat_grad_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, a, nl);
    if (nc) hipLaunchKernelGGL(feat_chord_kernel, dim3((unsigned)nc), dim3(64), 0, s, a);
    hipLaunchKernelGGL(feat_select_kernel, dim3(2, (unsigned)a.nsets), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- view ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int view_tiles(const ViewLaunch& a) { return score_tiles_x(a.width) * score_tiles_y(a.height); }

__global__ __launch_bounds__(kSsimTile) void view_tile_kernel(ViewLaunch a)
{
    const int t = (int)threadIdx.x, tile = (int)blockIdx.x, v = (int)blockIdx.y;
    const int tiles_x = score_tiles_x(a.width), ntiles = view_tiles(a);
    const int x = (tile % tiles_x) * kSsimTileW + t % kSsimTileW, y = (tile / tiles_x) * kSsimTileH + t / kSsimTileW;
    ViewPixel px;
    px.hit = px.grazing = px.perimeter = false;
    px.evals = 0;
    px.p[0] = px.p[1] = px.p[2] = 0.0;
    if (x < a.width && y < a.height) px = feat_view_pixel(a.maps[v], a.cams[v], a.width, a.height, x, y);

    __shared__ int cnt[3][kSsimTile / 64];
    __shared__ long long ev[kSsimTile];
    __shared__ double lo[3][kSsimTile], hi[3][kSsimTile];
    const bool flags[3] = { px.hit, px.grazing, px.perimeter };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long b = __ballot(flags[c]);
        if ((t & 63) == 0) cnt[c][t >> 6] = __popcll(b);
    }
    ev[t] = px.evals;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        lo[j][t] = px.hit ? px.p[j] : feat_inf(false);
        hi[j][t] = px.hit ? px.p[j] : feat_inf(true);
    }
    __syncthreads();
    for (int h = kSsimTile / 2; h > 0; h >>= 1) {
        if (t < h) {
            ev[t] += ev[t + h];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j][t] = feat_box_min(lo[j][t], lo[j][t + h]);
                hi[j][t] = feat_box_max(hi[j][t], hi[j][t + h]);
            }
        }
        __syncthreads();
    }
    long long* ic = a.icounts + (size_t)v * kViewCounts * (size_t)ntiles;
    double* box = a.box + (size_t)v * 6 * (size_t)ntiles;
    if (t < 3) ic[(size_t)t * ntiles + tile] = (long long)(cnt[t][0] + cnt[t][1] + cnt[t][2] + cnt[t][3]);
    if (t == 3) ic[(size_t)VC_EVALS * ntiles + tile] = ev[0];
    if (t >= 4 && t < 7) box[(size_t)(t - 4) * ntiles + tile] = lo[t - 4][0];
    if (t >= 7 && t < 10) box[(size_t)(t - 4) * ntiles + tile] = hi[t - 7][0];
}

// one 64-thread workgroup per view: thread c < 4 adds count c over the tiles, threads 4 .. 9 fold the box; the totals
// take the place of tile 0's
__global__ __launch_bounds__(64) void view_mean_kernel(ViewLaunch a)
{
    const int t = (int)threadIdx.x, v = (int)blockIdx.x, ntiles = view_tiles(a);
    long long* ic = a.icounts + (size_t)v * kViewCounts * (size_t)ntiles;
    double* box = a.box + (size_t)v * 6 * (size_t)ntiles;
    __shared__ long long tot[kViewCounts];
    if (t < kViewCounts) {
        tot[t] = ssim_sum_in_order(ic + (size_t)t * ntiles, ntiles);
        ic[(size_t)t * ntiles] = tot[t];
    } else if (t < kViewCounts + 6) {
        double* b = box + (size_t)(t - kViewCounts) * ntiles;
        const bool low = t - kViewCounts < 3;
        double m = b[0];
        for (int i = 1; i < ntiles; ++i) m = low ? feat_box_min(m, b[i]) : feat_box_max(m, b[i]);
        b[0] = m;
    }
    __syncthreads();
    if (t == 0) a.mean[v] = tot[VC_HIT] ? feat_mean_evals(tot[VC_EVALS], tot[VC_HIT]) : 0.0;
}

__global__ __launch_bounds__(kSsimTile) void view_var_kernel(ViewLaunch a)
{
    const int t = (int)threadIdx.x, tile = (int)blockIdx.x, v = (int)blockIdx.y;
    const int tiles_x = score_tiles_x(a.width);
    const int x = (tile % tiles_x) * kSsimTileW + t % kSsimTileW, y = (tile / tiles_x) * kSsimTileH + t / kSsimTileW;
    __shared__ double red[kSsimTile];
    double d2 = 0.0;
    if (x < a.width && y < a.height) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        const ViewMaps m = a.maps[v];
        if (m.hit[i]) {
            const double d = (double)feat_evals_count(m.evals[i]) - a.mean[v];
            d2 = d * d;
        }
    }
    red[t] = d2;
    __syncthreads();
    for (int h = kSsimTile / 2; h > 0; h >>= 1) {                         // ssim_fold
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) a.part[(size_t)v * (size_t)view_tiles(a) + (size_t)tile] = red[0];
}

__global__ __launch_bounds__(64) void view_finish_kernel(ViewLaunch a)
{
    const int v = (int)(blockIdx.x * 64 + threadIdx.x), ntiles = view_tiles(a);
    if (v >= a.nviews) return;
    const long long* ic = a.icounts + (size_t)v * kViewCounts * (size_t)ntiles;
    const double* box = a.box + (size_t)v * 6 * (size_t)ntiles;
    int64_t counts[kViewCounts];
    double lo[3], hi[3];
    for (int c = 0; c < kViewCounts; ++c) counts[c] = ic[(size_t)c * ntiles];
    for (int j = 0; j < 3; ++j) { lo[j] = box[(size_t)j * ntiles]; hi[j] = box[(size_t)(3 + j) * ntiles]; }
    const double ssq = ssim_sum_in_order(a.part + (size_t)v * (size_t)ntiles, ntiles);
    feat_view_combine(a.width, a.height, counts, ssq, lo, hi, a.out + v);
}

// rm_view_features has validated the arguments: sides >= 1, nviews in [1, kFeatMaxViews], every buffer sized for them
static hipError_t launch_view_features(const ViewLaunch& a, hipStream_t s)
{
    const unsigned ntiles = (unsigned)(score_tiles_x(a.width) * score_tiles_y(a.height)), nv = (unsigned)a.nviews;
    hipLaunchKernelGGL(view_tile_kernel, dim3(ntiles, nv), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(view_mean_kernel, dim3(nv), dim3(64), 0, s, a);
    hipLaunchKernelGGL(view_var_kernel, dim3(ntiles, nv), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(view_finish_kernel, dim3((nv + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace rm

// ---- rm_intrinsic_features and rm_view_features of the C ABI --------------------------------------------------------------

static_assert(sizeof(RmIntrinsicFeatures) == sizeof(rm::IntrinsicFeatures) && offsetof(RmIntrinsicFeatures, n_slabs) == offsetof(rm::IntrinsicFeatures, n_slabs),
              "rm::IntrinsicFeatures is RmIntrinsicFeatures");
static_assert(sizeof(RmViewFeatures) == sizeof(rm::ViewFeatures) && offsetof(RmViewFeatures, hit_rate) == offsetof(rm::ViewFeatures, hit_rate) &&
              offsetof(RmViewFeatures, box_hi) == offsetof(rm::ViewFeatures, box_hi), "rm::ViewFeatures is RmViewFeatures");
static_assert(sizeof(RmViewMaps) == sizeof(rm::ViewMaps), "rm::ViewMaps is RmViewMaps");

using namespace rm::capi;

namespace {

WsBuf feat_in[4], feat_xyz, feat_f, feat_keys, feat_slabs;   // rm_intrinsic_features: pts / chords / seglen / ts, points, values, keys
WsBuf feat_counts, feat_gmag, feat_out;                      // its run counts, optional gmag, results
WsBuf view_map[4], view_tab, view_cams, view_small;          // rm_view_features: depth / normal / evals / hit, the table, partials + results

}  // namespace

extern "C" {

int rm_intrinsic_features(int scene_id, int32_t nsets, int32_t n_lip, const double* pts, double lip_eps, int32_t n_chords,
                          const double* chords, const double* seglen, int32_t chord_steps, const double* ts, RmIntrinsicFeatures* out,
                          double* gmag_out, int32_t* slab_counts_out, RmTiming* timing)
{
    if (const char* why = rm::feat_check_intrinsic(nsets, n_lip, pts, lip_eps, n_chords, chords, seglen, chord_steps, ts, out))
        return fail(RM_E_BAD_ARG, "rm_intrinsic_features: %s", why);
    if (const char* why = rm::feat_check_seglen(nsets, n_chords, seglen)) return fail(RM_E_BAD_ARG, "rm_intrinsic_features: %s", why);
    int rc = check_scene(scene_id);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const hipStream_t s = lib_stream();
    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    const size_t ns = (size_t)nsets, nl = ns * (size_t)n_lip, nc = ns * (size_t)n_chords;
    const size_t npts = rm::feat_lip_points(nsets, n_lip) + rm::feat_chord_points(nsets, n_chords, chord_steps);
    Staged st(e);
    rm::IntrinsicLaunch a;
    memset(&a, 0, sizeof a);
    a.nsets = nsets; a.n_lip = n_lip; a.n_chords = n_chords; a.chord_steps = chord_steps; a.eps = lip_eps;
    if (nl) a.pts = st.in(feat_in[0], pts, nl * 24);
    if (nc) a.chords = st.in(feat_in[1], chords, nc * 48);
    if (nc) a.seglen = st.in(feat_in[2], seglen, nc * 8);
    a.ts = st.in(feat_in[3], ts, (size_t)chord_steps * 8);
    a.xyz = st.scratch<double>(feat_xyz, npts * 24, 16);
    a.f = st.scratch<double>(feat_f, npts * 8, 16);
    a.gkeys = st.scratch<uint64_t>(feat_keys, nl * 8, 16);
    a.slabs = st.scratch<uint64_t>(feat_slabs, nc * (size_t)rm::feat_max_runs(chord_steps) * 8, 16);
    a.counts = nc && slab_counts_out ? st.out(feat_counts, slab_counts_out, nc * 4) : st.scratch<int32_t>(feat_counts, nc * 4, 16);
    a.gmag_out = nl ? st.out(feat_gmag, gmag_out, nl * 8) : nullptr;
    a.out = (rm::IntrinsicFeatures*)st.out(feat_out, out, ns * sizeof(RmIntrinsicFeatures));
    if ((rc = st.begin())) return rc;
    const SdfEval sdf_eval = sdf_eval_of(scene_id);
    rc = once_or_timed(e, timing, s, [&] {
        HIP_TRY(rm::launch_feature_points(a, s));
        HIP_TRY(sdf_eval(a.xyz, npts, a.f, data, s));
        HIP_TRY(rm::launch_feature_reduce(a, s));
        return (int)RM_OK;
    });
    if (rc) return rc;
    return st.finish();
}

int rm_view_features(int32_t width, int32_t height, int32_t nviews, const double* cams, const RmViewMaps* maps, RmViewFeatures* out,
                     RmTiming* timing)
{
    if (const char* why = rm::feat_check_view(nviews, cams, maps, out)) return fail(RM_E_BAD_ARG, "rm_view_features: %s", why);
    if (width <= 0 || height <= 0) return fail(RM_E_BAD_DIMS, "a %dx%d image has no pixel", width, height);
    if ((long long)width * height > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "image too large");
    for (int v = 0; v < nviews; ++v)
        if (!maps[v].depth || !maps[v].normal || !maps[v].evals || !maps[v].hit)
            return fail(RM_E_BAD_ARG, "rm_view_features: view %d: depth, normal, evals and hit are required", v);
    for (size_t i = 0; i < (size_t)nviews * 14; ++i)
        if (!rm::feat_is_finite(cams[i])) return fail(RM_E_BAD_ARG, "rm_view_features: camera %zu: field %zu is not finite", i / 14, i % 14);
    int rc = timing ? check_timing(timing) : RM_OK;
    if (rc) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const hipStream_t s = lib_stream();
    const size_t npix = (size_t)width * (size_t)height, nv = (size_t)nviews;
    const size_t ntiles = (size_t)rm::score_tiles_x(width) * (size_t)rm::score_tiles_y(height);
    const size_t o_counts = 0, o_box = align256(o_counts + nv * rm::kViewCounts * ntiles * 8), o_mean = align256(o_box + nv * 6 * ntiles * 8);
    const size_t o_part = align256(o_mean + nv * 8), o_out = align256(o_part + nv * ntiles * 8), small = o_out + nv * sizeof(rm::ViewFeatures);
    static_assert(sizeof(rm::CameraParams) == 14 * sizeof(double), "cams is an array of CameraParams");
    if ((rc = view_map[0].ensure(nv * npix * 4)) || (rc = view_map[1].ensure(nv * npix * 12)) || (rc = view_map[2].ensure(nv * npix * 4)) ||
        (rc = view_map[3].ensure(nv * npix)) || (rc = view_tab.ensure(nv * sizeof(rm::ViewMaps))) ||
        (rc = view_cams.ensure(nv * sizeof(rm::CameraParams))) || (rc = view_small.ensure(small)))
        return rc;
    std::vector<rm::ViewMaps> table(nv);
    for (size_t v = 0; v < nv; ++v) {
        rm::ViewMaps& d = table[v];
        d.depth = (const float*)view_map[0].p + v * npix;
        d.normal = (const float*)view_map[1].p + v * npix * 3;
        d.evals = (const float*)view_map[2].p + v * npix;
        d.hit = (const uint8_t*)view_map[3].p + v * npix;
        HIP_TRY(hipMemcpyAsync((void*)d.depth, maps[v].depth, npix * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((void*)d.normal, maps[v].normal, npix * 12, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((void*)d.evals, maps[v].evals, npix * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((void*)d.hit, maps[v].hit, npix, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(view_tab.p, table.data(), nv * sizeof(rm::ViewMaps), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(view_cams.p, cams, nv * sizeof(rm::CameraParams), hipMemcpyHostToDevice, s));
    rm::ViewLaunch a;
    a.width = width; a.height = height; a.nviews = nviews;
    a.maps = (const rm::ViewMaps*)view_tab.p;
    a.cams = (const rm::CameraParams*)view_cams.p;
    char* sm = (char*)view_small.p;
    a.icounts = (long long*)(sm + o_counts); a.box = (double*)(sm + o_box); a.mean = (double*)(sm + o_mean);
    a.part = (double*)(sm + o_part); a.out = (rm::ViewFeatures*)(sm + o_out);
    rc = once_or_timed(e, timing, s, [&] {
        HIP_TRY(rm::launch_view_features(a, s));
        return (int)RM_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, a.out, nv * sizeof(rm::ViewFeatures), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RM_OK;
}

}  // extern "C"
