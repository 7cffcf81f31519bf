// rm_features.hip -- the discovery features of a (scene, viewpoint) on the device (rm_features.h; rm_intrinsic_features and
// rm_view_features in include/rm_hip.h).
//
// Intrinsic features, all on one stream; the scene's own sdf_eval launcher runs between the first two (rm_capi.hip):
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

#include "rm_features.h"

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
hipError_t launch_feature_points(const IntrinsicLaunch& a, hipStream_t s)
{
    const size_t n = feat_lip_points(a.nsets, a.n_lip) + feat_chord_points(a.nsets, a.n_chords, a.chord_steps);
    if (n) hipLaunchKernelGGL(feat_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, n);
    return hipGetLastError();
}

// ... and after it: gradients, runs, selections
hipError_t launch_feature_reduce(const IntrinsicLaunch& a, hipStream_t s)
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

// rm_capi.hip has validated the arguments: sides >= 1, nviews in [1, kFeatMaxViews], every buffer sized for them
hipError_t launch_view_features(const ViewLaunch& a, hipStream_t s)
{
    const unsigned ntiles = (unsigned)(score_tiles_x(a.width) * score_tiles_y(a.height)), nv = (unsigned)a.nviews;
    hipLaunchKernelGGL(view_tile_kernel, dim3(ntiles, nv), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(view_mean_kernel, dim3(nv), dim3(64), 0, s, a);
    hipLaunchKernelGGL(view_var_kernel, dim3(ntiles, nv), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(view_finish_kernel, dim3((nv + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace rm
