// rm_ssim.hip -- SSIM and colour-RMSE scoring of captures on the device (rm_ssim.h; rm_ssim_scores in include/rm_hip.h).
//
// Three kernels on one stream:
//   ssim_reference_kernel   the reference capture's seven 8-bit planes, quantised once for all methods
//   ssim_tile_kernel        one workgroup per (tile, channel, method): quantises the method's float map on the fly, stages
//                           both images' tile + halo in LDS, forms the five window sums as integers (a row pass, then a
//                           column pass), evaluates S in fp64 and folds the tile's 256 values by halves into one partial;
//                           a colour channel also leaves its tile's exact sum of squared differences
//   ssim_finish_kernel      one workgroup per method: ten threads add the partials of a channel each in tile index order,
//                           one combines them into the four scores
// No atomics on floating-point values and no order that depends on scheduling: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "rm_ssim.h"
#include "rm_capi_internal.h"

namespace rm {

static_assert(kSsimTile == 256, "one output pixel per thread of a 256-thread workgroup");

__global__ __launch_bounds__(256) void ssim_reference_kernel(SsimLaunch a)
{
    const size_t npix = (size_t)a.width * (size_t)a.height;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    for (int c = 0; c < kSsimChannels; ++c) {
        if ((c >= 1 && c < kSsimColor0 && !a.has_normal) || (c >= kSsimColor0 && !a.has_color)) continue;
        a.ref_img[(size_t)c * npix + p] = ssim_channel_u8(c, a.ref_depth, a.ref_normal, a.ref_color, a.ref_hit, p, a.range);
    }
}

__global__ __launch_bounds__(kSsimTile) void ssim_tile_kernel(SsimLaunch a)
{
    const int c = (int)blockIdx.y, m = (int)blockIdx.z, tile = (int)blockIdx.x;
    if ((c >= 1 && c < kSsimColor0 && !a.has_normal) || (c >= kSsimColor0 && !a.has_color)) return;   // workgroup-uniform
    const int t = (int)threadIdx.x;
    const int tiles_x = ssim_tiles_x(a.width), tiles_y = ssim_tiles_y(a.height);
    const int tix = tile % tiles_x, tiy = tile / tiles_x;
    const int x0 = tix * kSsimTileW, y0 = tiy * kSsimTileH;
    const size_t npix = (size_t)a.width * (size_t)a.height;

    __shared__ uint8_t sx[kSsimStageH][kSsimStageW + 2], sy[kSsimStageH][kSsimStageW + 2];
    __shared__ int32_t rows[5][kSsimStageH][kSsimTileW];
    __shared__ double red[kSsimTile];
    __shared__ int32_t ssd_tile;
    if (t == 0) ssd_tile = 0;
    __syncthreads();

    // stage the tile and its halo: the reference's plane as it is, the method's map quantised here; 0 beyond the image
    // (only outputs that are masked below read those)
    const uint8_t* ref = a.ref_img + (size_t)c * npix;
    const float* depth = a.depth + (size_t)m * npix;
    const float* normal = a.has_normal ? a.normal + (size_t)m * npix * 3 : nullptr;
    const float* color = a.has_color ? a.color + (size_t)m * npix * 3 : nullptr;
    const uint8_t* hit = a.hit + (size_t)m * npix;
    const bool last_x = tix == tiles_x - 1, last_y = tiy == tiles_y - 1;
    int32_t ssd = 0;                                                      // at most 3 pixels x 255^2
    for (int i = t; i < kSsimStageH * kSsimStageW; i += kSsimTile) {
        const int ly = i / kSsimStageW, lx = i % kSsimStageW;
        const int ix = x0 + lx, iy = y0 + ly;
        uint8_t x = 0, y = 0;
        if (ix < a.width && iy < a.height) {
            const size_t p = (size_t)iy * (size_t)a.width + (size_t)ix;
            x = ref[p];
            y = ssim_channel_u8(c, depth, normal, color, hit, p, a.range);
            if (c >= kSsimColor0 && ssim_owns(lx, ly, last_x, last_y)) {
                const int32_t d = (int32_t)x - (int32_t)y;
                ssd += d * d;
            }
        }
        sx[ly][lx] = x;
        sy[ly][lx] = y;
    }
    if (c >= kSsimColor0 && ssd) atomicAdd(&ssd_tile, ssd);               // an integer sum: any order gives the same value
    __syncthreads();

    // row pass: the five sums over 7 pixels to the right of (r, col), for every staged row
    for (int i = t; i < kSsimStageH * kSsimTileW; i += kSsimTile) {
        const int r = i / kSsimTileW, col = i % kSsimTileW;
        int32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int k = 0; k < kSsimWin; ++k) {
            const int32_t x = sx[r][col + k], y = sy[r][col + k];
            s0 += x; s1 += y; s2 += x * x; s3 += y * y; s4 += x * y;
        }
        rows[0][r][col] = s0; rows[1][r][col] = s1; rows[2][r][col] = s2; rows[3][r][col] = s3; rows[4][r][col] = s4;
    }
    __syncthreads();

    // column pass and S: thread t owns output pixel (x0 + t % 32, y0 + t / 32) of the cropped image
    const int ox = t % kSsimTileW, oy = t / kSsimTileW;
    double S = 0.0;
    if (x0 + ox < a.width - kSsimPad && y0 + oy < a.height - kSsimPad) {
        int32_t s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            int32_t v = 0;
#pragma unroll
            for (int k = 0; k < kSsimWin; ++k) v += rows[q][oy + k][ox];
            s[q] = v;
        }
        S = ssim_pixel(s[0], s[1], s[2], s[3], s[4]);
    }
    red[t] = S;
    __syncthreads();
    for (int h = kSsimTile / 2; h > 0; h >>= 1) {                         // ssim_fold, one pair per thread
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const size_t ntiles = (size_t)tiles_x * (size_t)tiles_y;
        a.part[((size_t)m * kSsimChannels + (size_t)c) * ntiles + (size_t)tile] = red[0];
        if (c >= kSsimColor0) a.ssd[((size_t)m * 3 + (size_t)(c - kSsimColor0)) * ntiles + (size_t)tile] = (long long)ssd_tile;
    }
}

__global__ __launch_bounds__(64) void ssim_finish_kernel(SsimLaunch a)
{
    const int m = (int)blockIdx.x, t = (int)threadIdx.x;
    const int ntiles = ssim_tiles_x(a.width) * ssim_tiles_y(a.height);
    __shared__ double s_sum[kSsimChannels];
    __shared__ long long ssd[3];
    if (t < kSsimChannels) {
        const bool have = t == 0 || (t < kSsimColor0 ? a.has_normal : a.has_color) != 0;
        s_sum[t] = have ? ssim_sum_in_order(a.part + ((size_t)m * kSsimChannels + (size_t)t) * (size_t)ntiles, ntiles) : 0.0;
    } else if (t < kSsimChannels + 3) {
        const int k = t - kSsimChannels;
        ssd[k] = a.has_color ? ssim_sum_in_order(a.ssd + ((size_t)m * 3 + (size_t)k) * (size_t)ntiles, ntiles) : 0;
    }
    __syncthreads();
    if (t == 0) ssim_combine(s_sum, ssd, a.width, a.height, a.has_normal != 0, a.has_color != 0, a.out + 4 * (size_t)m);
}

// rm_ssim_scores has validated the arguments: sides >= 7, nmethods in [1, kSsimMaxMethods], every buffer sized for them
static hipError_t launch_ssim(const SsimLaunch& a, hipStream_t s)
{
    const size_t npix = (size_t)a.width * (size_t)a.height;
    const unsigned ntiles = (unsigned)(ssim_tiles_x(a.width) * ssim_tiles_y(a.height));
    hipLaunchKernelGGL(ssim_reference_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(ntiles, kSsimChannels, (unsigned)a.nmethods), dim3(kSsimTile), 0, s, a);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)a.nmethods), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace rm

// ---- rm_ssim_scores of the C ABI ------------------------------------------------------------------------------------------
using namespace rm::capi;

namespace {

WsBuf ssim_depth, ssim_normal, ssim_color, ssim_hit;   // the methods' maps, then the reference's
WsBuf ssim_ref, ssim_part, ssim_ssd, ssim_out;         // the reference images, partial sums and scores

int ssim_check_maps(const RmCaptureMaps& c, const RmCaptureMaps& ref, const char* who, int index)
{
    if (!c.depth || !c.hit) return fail(RM_E_BAD_ARG, "%s %d: depth and hit are required", who, index);
    if (!c.normal != !ref.normal) return fail(RM_E_BAD_ARG, "%s %d: normal is NULL on one side only", who, index);
    if (!c.color != !ref.color) return fail(RM_E_BAD_ARG, "%s %d: color is NULL on one side only", who, index);
    return RM_OK;
}

}  // namespace

extern "C" int rm_ssim_scores(int32_t width, int32_t height, const RmCaptureMaps* reference, const RmCaptureMaps* methods,
                              int32_t nmethods, double* out, RmTiming* timing)
{
    if (!reference || !methods || !out) return fail(RM_E_BAD_ARG, "reference, methods or out is NULL");
    if (nmethods <= 0 || nmethods > rm::kSsimMaxMethods)
        return fail(RM_E_BAD_ARG, "nmethods %d outside [1, %d]", nmethods, rm::kSsimMaxMethods);
    if (width < rm::kSsimWin || height < rm::kSsimWin)
        return fail(RM_E_BAD_DIMS, "a %dx%d image holds no %dx%d window", width, height, rm::kSsimWin, rm::kSsimWin);
    if ((long long)width * height > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "image too large");
    int rc = ssim_check_maps(*reference, *reference, "reference", 0);
    for (int m = 0; !rc && m < nmethods; ++m) rc = ssim_check_maps(methods[m], *reference, "method", m);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const hipStream_t s = lib_stream();
    const size_t npix = (size_t)width * (size_t)height, caps = (size_t)nmethods + 1;      // the reference is capture `nmethods`
    const size_t ntiles = (size_t)rm::ssim_tiles_x(width) * (size_t)rm::ssim_tiles_y(height);
    const bool has_normal = reference->normal != nullptr, has_color = reference->color != nullptr;
    if ((rc = ssim_depth.ensure(caps * npix * 4)) || (rc = ssim_hit.ensure(caps * npix)) ||
        (has_normal && (rc = ssim_normal.ensure(caps * npix * 12))) || (has_color && (rc = ssim_color.ensure(caps * npix * 12))) ||
        (rc = ssim_ref.ensure(rm::kSsimChannels * npix)) || (rc = ssim_part.ensure((size_t)nmethods * rm::kSsimChannels * ntiles * 8)) ||
        (rc = ssim_ssd.ensure((size_t)nmethods * 3 * ntiles * 8)) || (rc = ssim_out.ensure((size_t)nmethods * 32)))
        return rc;
    for (size_t m = 0; m < caps; ++m) {
        const RmCaptureMaps& c = m < (size_t)nmethods ? methods[m] : *reference;
        HIP_TRY(hipMemcpyAsync((float*)ssim_depth.p + m * npix, c.depth, npix * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((uint8_t*)ssim_hit.p + m * npix, c.hit, npix, hipMemcpyHostToDevice, s));
        if (has_normal) HIP_TRY(hipMemcpyAsync((float*)ssim_normal.p + m * npix * 3, c.normal, npix * 12, hipMemcpyHostToDevice, s));
        if (has_color) HIP_TRY(hipMemcpyAsync((float*)ssim_color.p + m * npix * 3, c.color, npix * 12, hipMemcpyHostToDevice, s));
    }
    double lo, hi;
    rm::ssim_depth_minmax(reference->depth, reference->hit, npix, &lo, &hi);
    rm::SsimLaunch a;
    a.width = width; a.height = height; a.nmethods = nmethods; a.has_normal = has_normal; a.has_color = has_color;
    a.range = rm::ssim_depth_range(lo, hi);
    a.depth = (const float*)ssim_depth.p; a.hit = (const uint8_t*)ssim_hit.p;
    a.normal = has_normal ? (const float*)ssim_normal.p : nullptr;
    a.color = has_color ? (const float*)ssim_color.p : nullptr;
    a.ref_depth = a.depth + (size_t)nmethods * npix; a.ref_hit = a.hit + (size_t)nmethods * npix;
    a.ref_normal = has_normal ? a.normal + (size_t)nmethods * npix * 3 : nullptr;
    a.ref_color = has_color ? a.color + (size_t)nmethods * npix * 3 : nullptr;
    a.ref_img = (uint8_t*)ssim_ref.p;
    a.part = (double*)ssim_part.p; a.ssd = (long long*)ssim_ssd.p; a.out = (double*)ssim_out.p;
    rc = once_or_timed(e, timing, s, [&] {
        HIP_TRY(rm::launch_ssim(a, s));
        return (int)RM_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, a.out, (size_t)nmethods * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RM_OK;
}
