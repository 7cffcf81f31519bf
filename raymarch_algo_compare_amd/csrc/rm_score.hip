// rm_score.hip -- hit-mask counts, depth and normal error and exact percentiles of captures on the device (rm_score.h;
// rm_score_captures in include/rm_hip.h).
//
// Kernels, all on one stream:
//   score_reset_kernel    clears the counts, the digit histograms and the "least key above" words
//   score_band_kernel     one workgroup per 32 x 8 tile: stages the reference's hit flags with a halo of band_k + 1 in LDS
//                         (2 = beyond the image), marks the edge pixels of the tile and a halo of band_k, and writes the
//                         band of the tile's pixels (skipped with band_k < 0)
//   score_tile_kernel     one workgroup per (tile, method), one pixel per thread: the per-pixel values of rm_score.h, the
//                         eight counts (a ballot and a popcount per wave, one integer add per workgroup), the sample keys
//                         of |gap| and of the angle, and the tile's four sums folded by halves into partials
//   score_select_kernel   the rank each selection looks for, from the co-hit count
//   score_hist_kernel     one pass of the most-significant-digit radix select, 8 bits per pass: the histogram of the next
//   + score_pick_kernel   digit over the keys that carry the digits chosen so far (LDS, then integer adds), and the digit
//                         that holds the rank; eight passes leave s[j] and how many keys are below it and equal to it
//   score_above_kernel    the least key greater than s[j] (an integer min), from which score_next_rank takes s[j + 1]
//   score_finish_kernel   one workgroup per method: four threads add a sum's partials in tile index order each, one
//                         combines counts, sums and order statistics into the result
// No atomics on floating-point values and no order that depends on scheduling: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <vector>

#include "rm_score.h"
#include "rm_capi_internal.h"

namespace rm {

static_assert(kSsimTile == 256, "one pixel per thread of a 256-thread workgroup");
static_assert(kScoreCounts <= 64 && kScoreSums <= 64, "the finishing workgroup has 64 threads");

constexpr int kScoreHalo = kScoreMaxBand + 1;
constexpr int kScoreStageW = kSsimTileW + 2 * kScoreHalo, kScoreStageH = kSsimTileH + 2 * kScoreHalo;
constexpr int kScoreDigitBits = 8, kScoreBins = 1 << kScoreDigitBits, kScorePasses = 64 / kScoreDigitBits;
constexpr unsigned kScoreMaxChunks = 256;                  // workgroups of a histogram pass per (method, selection)

__device__ __forceinline__ int score_nsel(const ScoreLaunch& a) { return a.has_normal ? kScoreSelects : kScoreSelects - 1; }
__device__ __forceinline__ size_t score_npix(const ScoreLaunch& a) { return (size_t)a.width * (size_t)a.height; }

// the keys of selection s of method m: |gap| for the two depth selections, the angle for the third
__device__ __forceinline__ const uint64_t* score_keys_of(const ScoreLaunch& a, int m, int s)
{
    const size_t planes = a.has_normal ? 2 : 1;
    return a.keys + ((size_t)m * planes + (size_t)(s == 2)) * score_npix(a);
}

__global__ __launch_bounds__(256) void score_reset_kernel(ScoreLaunch a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t sels = (size_t)a.nmethods * kScoreSelects;
    if (i < (size_t)a.nmethods * kScoreCounts) a.counts[i] = 0;
    if (i < sels) a.above[i] = kScoreNoKey;
    if (i < sels * kScoreBins) a.hist[i] = 0;
}

__global__ __launch_bounds__(kSsimTile) void score_band_kernel(ScoreLaunch a)
{
    const int t = (int)threadIdx.x, tiles_x = score_tiles_x(a.width);
    const int halo = a.band_k + 1;
    const int sx0 = (int)(blockIdx.x % tiles_x) * kSsimTileW - halo, sy0 = (int)(blockIdx.x / tiles_x) * kSsimTileH - halo;
    const int sw = kSsimTileW + 2 * halo, sh = kSsimTileH + 2 * halo;
    __shared__ uint8_t flag[kScoreStageH][kScoreStageW], edge[kScoreStageH][kScoreStageW];
    const uint8_t* hit = a.caps[a.nmethods].hit;
    for (int i = t; i < sw * sh; i += kSsimTile) {
        const int ly = i / sw, lx = i % sw, ix = sx0 + lx, iy = sy0 + ly;
        const bool inside = ix >= 0 && ix < a.width && iy >= 0 && iy < a.height;
        flag[ly][lx] = inside ? (uint8_t)(hit[(size_t)iy * (size_t)a.width + (size_t)ix] != 0) : (uint8_t)2;
    }
    __syncthreads();
    for (int i = t; i < sw * sh; i += kSsimTile) {
        const int ly = i / sw, lx = i % sw;
        bool e = false;
        if (lx >= 1 && lx < sw - 1 && ly >= 1 && ly < sh - 1 && flag[ly][lx] != 2)
            e = score_is_edge(flag[ly][lx], flag[ly][lx - 1], flag[ly][lx + 1], flag[ly - 1][lx], flag[ly + 1][lx]);
        edge[ly][lx] = (uint8_t)e;
    }
    __syncthreads();
    // the pixels within band_k of a tile pixel lie at staged columns 1 .. sw - 2 and rows 1 .. sh - 2
    const int ix = sx0 + halo + t % kSsimTileW, iy = sy0 + halo + t / kSsimTileW;
    if (ix < a.width && iy < a.height)
        a.band[(size_t)iy * (size_t)a.width + (size_t)ix] =
            (uint8_t)score_in_band([&](int x, int y) { return edge[y - sy0][x - sx0] != 0; }, ix, iy, a.band_k);
}

__global__ __launch_bounds__(kSsimTile) void score_tile_kernel(ScoreLaunch a)
{
    const int t = (int)threadIdx.x, tile = (int)blockIdx.x, m = (int)blockIdx.y;
    const int tiles_x = score_tiles_x(a.width);
    const int ix = (tile % tiles_x) * kSsimTileW + t % kSsimTileW, iy = (tile / tiles_x) * kSsimTileH + t / kSsimTileW;
    const size_t npix = score_npix(a), p = (size_t)iy * (size_t)a.width + (size_t)ix;
    const bool inside = ix < a.width && iy < a.height, has_normal = a.has_normal != 0;

    __shared__ int cnt[kScoreCounts];
    __shared__ double red[kScoreSums][kSsimTile];
    if (t < kScoreCounts) cnt[t] = 0;
    __syncthreads();

    ScorePixel px;
    px.mine = px.truth = px.core = false;
    px.gap = px.mag = px.angle = 0.0;
    if (inside) px = score_pixel(a.caps[m], a.caps[a.nmethods], a.band_k >= 0 ? a.band : nullptr, has_normal, p);
    const bool co = px.mine && px.truth, un = px.mine || px.truth;
    if (inside) {
        const size_t planes = has_normal ? 2 : 1;
        uint64_t* keys = a.keys + (size_t)m * planes * npix;
        keys[p] = co ? score_key(px.mag) : kScoreNoKey;
        if (has_normal) keys[npix + p] = co ? score_key(px.angle) : kScoreNoKey;
    }

    const bool flags[kScoreCounts] = { px.mine, px.truth, co, un, co && px.core, un && px.core, co && px.gap != px.gap,
                                       co && px.angle != px.angle };
#pragma unroll
    for (int c = 0; c < kScoreCounts; ++c) {
        const unsigned long long b = __ballot(flags[c]);
        if ((t & 63) == 0 && b) atomicAdd(&cnt[c], __popcll(b));
    }
    red[0][t] = co ? px.mag : 0.0;
    red[1][t] = co ? px.gap * px.gap : 0.0;
    red[2][t] = co ? px.gap : 0.0;
    red[3][t] = co ? px.angle : 0.0;
    __syncthreads();
    if (t < kScoreCounts && cnt[t]) atomicAdd(&a.counts[(size_t)m * kScoreCounts + (size_t)t], (unsigned long long)cnt[t]);
    for (int h = kSsimTile / 2; h > 0; h >>= 1) {                         // ssim_fold, one pair per thread and sum
        if (t < h) {
#pragma unroll
            for (int q = 0; q < kScoreSums; ++q) red[q][t] += red[q][t + h];
        }
        __syncthreads();
    }
    if (t < kScoreSums) {
        const size_t ntiles = (size_t)tiles_x * (size_t)score_tiles_y(a.height);
        a.part[((size_t)m * kScoreSums + (size_t)t) * ntiles + (size_t)tile] = red[t][0];
    }
}

__global__ __launch_bounds__(256) void score_select_kernel(ScoreLaunch a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)a.nmethods * kScoreSelects) return;
    const int64_t n = (int64_t)a.counts[(i / kScoreSelects) * kScoreCounts + SC_CO];
    ScoreSelect st;
    st.prefix = 0;
    st.rank = i % kScoreSelects == 1 ? score_rank_med(n) : score_rank_p95(n);
    st.below = st.equal = 0;
    a.sel[i] = st;
}

// pass with digit at bit `shift` (56, 48, ... 0): keys outside the sample are skipped, so an empty sample leaves an empty
// histogram and score_pick_kernel leaves its selection alone (score_combine does not read it)
__global__ __launch_bounds__(256) void score_hist_kernel(ScoreLaunch a, int shift)
{
    const int t = (int)threadIdx.x, s = (int)blockIdx.y, m = (int)blockIdx.z;
    const size_t idx = (size_t)m * kScoreSelects + (size_t)s, npix = score_npix(a);
    __shared__ uint32_t h[kScoreBins];
    h[t] = 0;
    __syncthreads();
    const uint64_t prefix = a.sel[idx].prefix;
    const uint64_t* keys = score_keys_of(a, m, s);
    const bool first = shift == 64 - kScoreDigitBits;
    for (size_t p = (size_t)blockIdx.x * 256 + (size_t)t; p < npix; p += (size_t)gridDim.x * 256) {
        const uint64_t key = keys[p];
        if (key == kScoreNoKey) continue;
        if (first || (key >> (shift + kScoreDigitBits)) == prefix) atomicAdd(&h[(key >> shift) & (kScoreBins - 1)], 1u);
    }
    __syncthreads();
    if (h[t]) atomicAdd(&a.hist[idx * kScoreBins + (size_t)t], h[t]);
}

__global__ __launch_bounds__(kScoreBins) void score_pick_kernel(ScoreLaunch a)
{
    const int t = (int)threadIdx.x;
    const size_t idx = (size_t)blockIdx.y * kScoreSelects + (size_t)blockIdx.x;
    const ScoreSelect st = a.sel[idx];                                    // every thread reads before the one write below
    const uint32_t c = a.hist[idx * kScoreBins + (size_t)t];
    a.hist[idx * kScoreBins + (size_t)t] = 0;                             // clean for the next pass
    __shared__ uint32_t scan[kScoreBins];
    scan[t] = c;
    __syncthreads();
    for (int off = 1; off < kScoreBins; off <<= 1) {                      // inclusive prefix sums of the bins
        const uint32_t v = t >= off ? scan[t - off] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const int64_t incl = (int64_t)scan[t], excl = incl - (int64_t)c;
    if (c && excl <= st.rank && st.rank < incl) {                         // at most one bin
        ScoreSelect nx;
        nx.prefix = (st.prefix << kScoreDigitBits) | (uint64_t)t;
        nx.rank = st.rank - excl;
        nx.below = st.below + excl;
        nx.equal = (int64_t)c;
        a.sel[idx] = nx;
    }
}

__global__ __launch_bounds__(256) void score_above_kernel(ScoreLaunch a)
{
    const int t = (int)threadIdx.x, s = (int)blockIdx.y, m = (int)blockIdx.z;
    const size_t idx = (size_t)m * kScoreSelects + (size_t)s, npix = score_npix(a);
    const uint64_t sj = a.sel[idx].prefix;
    const uint64_t* keys = score_keys_of(a, m, s);
    uint64_t least = kScoreNoKey;
    for (size_t p = (size_t)blockIdx.x * 256 + (size_t)t; p < npix; p += (size_t)gridDim.x * 256) {
        const uint64_t key = keys[p];
        if (key > sj && key < least) least = key;
    }
    __shared__ uint64_t red[256];
    red[t] = least;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h && red[t + h] < red[t]) red[t] = red[t + h];
        __syncthreads();
    }
    if (t == 0 && red[0] != kScoreNoKey) atomicMin(&a.above[idx], (unsigned long long)red[0]);
}

__global__ __launch_bounds__(64) void score_finish_kernel(ScoreLaunch a)
{
    const int m = (int)blockIdx.x, t = (int)threadIdx.x;
    const int ntiles = score_tiles_x(a.width) * score_tiles_y(a.height);
    __shared__ double sums[kScoreSums];
    if (t < kScoreSums) sums[t] = ssim_sum_in_order(a.part + ((size_t)m * kScoreSums + (size_t)t) * (size_t)ntiles, ntiles);
    __syncthreads();
    if (t != 0) return;
    int64_t counts[kScoreCounts];
    for (int c = 0; c < kScoreCounts; ++c) counts[c] = (int64_t)a.counts[(size_t)m * kScoreCounts + (size_t)c];
    const int64_t n = counts[SC_CO];
    ScoreRanks k;
    for (int s = 0; s < kScoreSelects; ++s) {
        const size_t idx = (size_t)m * kScoreSelects + (size_t)s;
        const ScoreSelect st = a.sel[idx];
        const int64_t j = s == 1 ? score_rank_med(n) : score_rank_p95(n);
        k.lo[s] = st.prefix;
        k.hi[s] = score_next_rank(st.prefix, j, n, st.below + st.equal, (uint64_t)a.above[idx]);
    }
    score_combine(counts, sums, k, a.has_normal != 0, a.out + m);
}

// rm_score_captures has validated the arguments: sides >= 1, nmethods in [1, kScoreMaxMethods], band_k <= kScoreMaxBand,
// every buffer sized for them
static hipError_t launch_score(const ScoreLaunch& a, hipStream_t s)
{
    const size_t npix = (size_t)a.width * (size_t)a.height;
    const unsigned ntiles = (unsigned)(score_tiles_x(a.width) * score_tiles_y(a.height));
    const unsigned nm = (unsigned)a.nmethods, nsel = a.has_normal ? kScoreSelects : kScoreSelects - 1;
    const size_t words = (size_t)nm * kScoreSelects * kScoreBins;
    const size_t want = (npix + 2047) / 2048;                             // eight keys per thread
    const unsigned chunks = (unsigned)(want < kScoreMaxChunks ? want : kScoreMaxChunks);
    hipLaunchKernelGGL(score_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a);
    if (a.band_k >= 0) hipLaunchKernelGGL(score_band_kernel, dim3(ntiles), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(score_tile_kernel, dim3(ntiles, nm), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(score_select_kernel, dim3((nm * kScoreSelects + 255) / 256), dim3(256), 0, s, a);
    for (int pass = 0; pass < kScorePasses; ++pass) {
        hipLaunchKernelGGL(score_hist_kernel, dim3(chunks, nsel, nm), dim3(256), 0, s, a, 64 - kScoreDigitBits * (pass + 1));
        hipLaunchKernelGGL(score_pick_kernel, dim3(nsel, nm), dim3(kScoreBins), 0, s, a);
    }
    hipLaunchKernelGGL(score_above_kernel, dim3(chunks, nsel, nm), dim3(256), 0, s, a);
    hipLaunchKernelGGL(score_finish_kernel, dim3(nm), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace rm

// ---- rm_score_captures of the C ABI ---------------------------------------------------------------------------------------

static_assert(sizeof(RmScoreResult) == sizeof(rm::ScoreResult) && offsetof(RmScoreResult, depth_mae) == offsetof(rm::ScoreResult, depth_mae) &&
              offsetof(RmScoreResult, normal_p95_deg) == offsetof(rm::ScoreResult, normal_p95_deg), "rm::ScoreResult is RmScoreResult");

using namespace rm::capi;

namespace {

WsBuf score_depth, score_normal, score_hit, score_caps;   // the methods' maps, then the reference's
WsBuf score_band, score_keys, score_small, score_part;    // the band, sample keys, counts / selections / results, partial sums

int score_check_maps(const RmScoreMaps& c, const RmScoreMaps& ref, const char* who, int index)
{
    if (!c.depth || !c.hit) return fail(RM_E_BAD_ARG, "%s %d: depth and hit are required", who, index);
    if (!c.normal != !ref.normal) return fail(RM_E_BAD_ARG, "%s %d: normal is NULL on one side only", who, index);
    return RM_OK;
}

}  // namespace

extern "C" int rm_score_captures(int32_t width, int32_t height, int32_t band_k, const RmScoreMaps* reference, const RmScoreMaps* methods,
                                 int32_t nmethods, RmScoreResult* out, RmTiming* timing)
{
    if (!reference || !methods || !out) return fail(RM_E_BAD_ARG, "reference, methods or out is NULL");
    if (nmethods <= 0 || nmethods > rm::kScoreMaxMethods)
        return fail(RM_E_BAD_ARG, "nmethods %d outside [1, %d]", nmethods, rm::kScoreMaxMethods);
    if (band_k > rm::kScoreMaxBand) return fail(RM_E_BAD_ARG, "band_k %d above %d", band_k, rm::kScoreMaxBand);
    if (width <= 0 || height <= 0) return fail(RM_E_BAD_DIMS, "a %dx%d image has no pixel", width, height);
    if ((long long)width * height > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "image too large");
    int rc = score_check_maps(*reference, *reference, "reference", 0);
    for (int m = 0; !rc && m < nmethods; ++m) rc = score_check_maps(methods[m], *reference, "method", m);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const hipStream_t s = lib_stream();
    const size_t npix = (size_t)width * (size_t)height, nm = (size_t)nmethods, caps = nm + 1;   // the reference is capture `nmethods`
    const size_t ntiles = (size_t)rm::score_tiles_x(width) * (size_t)rm::score_tiles_y(height);
    const bool has_normal = reference->normal != nullptr;
    // one small buffer: counts, selections, histograms, least keys above, results
    const size_t o_counts = 0, o_sel = align256(o_counts + nm * rm::kScoreCounts * 8);
    const size_t o_hist = align256(o_sel + nm * rm::kScoreSelects * sizeof(rm::ScoreSelect));
    const size_t o_above = align256(o_hist + nm * rm::kScoreSelects * 256 * 4);
    const size_t o_out = align256(o_above + nm * rm::kScoreSelects * 8), small = o_out + nm * sizeof(rm::ScoreResult);
    // every capture has a slot of W*H doubles (and 3 W*H for the normals), whichever type it holds
    if ((rc = score_depth.ensure(caps * npix * 8)) || (rc = score_hit.ensure(caps * npix)) ||
        (has_normal && (rc = score_normal.ensure(caps * npix * 24))) || (rc = score_caps.ensure(caps * sizeof(rm::ScoreMaps))) ||
        (band_k >= 0 && (rc = score_band.ensure(npix))) || (rc = score_keys.ensure(nm * (has_normal ? 2 : 1) * npix * 8)) ||
        (rc = score_small.ensure(small)) || (rc = score_part.ensure(nm * rm::kScoreSums * ntiles * 8)))
        return rc;
    std::vector<rm::ScoreMaps> table(caps);
    for (size_t m = 0; m < caps; ++m) {
        const RmScoreMaps& c = m < nm ? methods[m] : *reference;
        const size_t elem = c.fp64 ? 8 : 4;
        rm::ScoreMaps& d = table[m];
        d.depth = (char*)score_depth.p + m * npix * 8;
        d.normal = has_normal ? (char*)score_normal.p + m * npix * 24 : nullptr;
        d.hit = (uint8_t*)score_hit.p + m * npix;
        d.fp64 = c.fp64 != 0;
        HIP_TRY(hipMemcpyAsync((void*)d.depth, c.depth, npix * elem, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((void*)d.hit, c.hit, npix, hipMemcpyHostToDevice, s));
        if (has_normal) HIP_TRY(hipMemcpyAsync((void*)d.normal, c.normal, npix * 3 * elem, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(score_caps.p, table.data(), caps * sizeof(rm::ScoreMaps), hipMemcpyHostToDevice, s));
    rm::ScoreLaunch a;
    a.width = width; a.height = height; a.nmethods = nmethods; a.has_normal = has_normal; a.band_k = band_k < 0 ? -1 : band_k;
    a.caps = (const rm::ScoreMaps*)score_caps.p;
    a.band = (uint8_t*)score_band.p;
    a.keys = (uint64_t*)score_keys.p;
    char* sm = (char*)score_small.p;
    a.counts = (unsigned long long*)(sm + o_counts); a.sel = (rm::ScoreSelect*)(sm + o_sel); a.hist = (uint32_t*)(sm + o_hist);
    a.above = (unsigned long long*)(sm + o_above); a.out = (rm::ScoreResult*)(sm + o_out);
    a.part = (double*)score_part.p;
    rc = once_or_timed(e, timing, s, [&] {
        HIP_TRY(rm::launch_score(a, s));
        return (int)RM_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, a.out, nm * sizeof(rm::ScoreResult), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RM_OK;
}
