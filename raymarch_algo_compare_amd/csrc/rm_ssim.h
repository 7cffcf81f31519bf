// rm_ssim.h -- the tertiary tier of capture scoring: SSIM of the depth, normal and colour images of two captures and the
// RMSE of their colour images.  Shared by the gfx950 kernels (rm_ssim.hip), the C ABI (rm_ssim_scores) and the host check
// build (tests/native/ssim_check.cpp): the quantisation, the per-pixel formula and the summation order are written once,
// here, so the host build and the device give the same bits.
//
// Images.  A capture's float32 maps become 8-bit images as the reference's data/capture_io.py makes them (_to_u8: NaN ->
// 0, +inf -> 1, -inf -> 0, x * 255 in binary32, clamped to [0, 255], truncated):
//   depth    1 - clamp((depth - lo) / max(hi - lo, 1e-6), 0, 1) on a hit, 0 on a miss ((lo, hi): the REFERENCE capture's
//            depth range over its hits, (0, 1) without any; near is bright.  The range is NumPy's min / max: one NaN hit
//            depth of the reference makes it (NaN, NaN), and then both depth images are 0 on every hit pixel; a +-inf
//            hit depth is an ordinary bound)
//   normal   n * 0.5 + 0.5 on a hit, 0 on a miss, per component
//   colour   as it is
// Seven channels: 0 depth, 1..3 normal, 4..6 colour.
//
// SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) with the defaults of skimage.metrics.structural_similarity for 8-bit
// input, per channel: over every 7 x 7 window that lies wholly inside the image (the image cropped by 3 on each side,
// so no border rule is ever used), with the window means ux, uy of the two images, the means uxx, uyy, uxy of their
// squares and product, the sample (co)variances v = 49/48 * (u__ - u_ * u_), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2:
//   S = ((2 ux uy + C1) (2 vxy + C2)) / ((ux^2 + uy^2 + C1) (vx + vy + C2))
// and the channel's score is the mean of S.  A three-channel image scores the mean of its channels' scores.  The five
// window sums are integers (at most 49 * 255^2): exact in int32, so S depends on nothing but the window's content.
// colour RMSE = sqrt(mean((x - y)^2)) over all pixels and channels of the two colour images: an exact integer sum.
//
// Summation order (the same on the host and on the device, whatever workgroup runs a tile): the cropped image is cut
// into tiles of kSsimTileW x kSsimTileH output pixels; a tile's S values (row-major, 0.0 where the tile overhangs) are
// folded by halves (ssim_fold: v[i] += v[i + 128], then + 64, ... + 1); the tiles' partial sums are added in tile index
// order (ssim_sum_in_order).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rm_core.h"

namespace rm {

constexpr int kSsimWin = 7;                                // window side
constexpr int kSsimPad = kSsimWin - 1;                     // a tile's halo: 3 on each side
constexpr int kSsimTileW = 32, kSsimTileH = 8;             // output pixels of a tile (one per thread of a workgroup)
constexpr int kSsimTile = kSsimTileW * kSsimTileH;
constexpr int kSsimStageW = kSsimTileW + kSsimPad, kSsimStageH = kSsimTileH + kSsimPad;   // the pixels a tile reads
constexpr int kSsimChannels = 7;                           // depth, normal xyz, colour rgb
constexpr int kSsimColor0 = 4;                             // first colour channel

// ---- quantisation (capture_io.py: _to_u8, depth_to_image, normal_to_image, color_to_image) -----------------------------

RM_HD uint8_t ssim_to_u8(float x)
{
    if (x != x) x = 0.0f;                                  // np.nan_to_num(x, nan=0, posinf=1, neginf=0)
    else if (x == __builtin_inff()) x = 1.0f;
    else if (x == -__builtin_inff()) x = 0.0f;
    float v = x * 255.0f;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);       // np.clip
    return (uint8_t)v;                                     // astype(uint8): truncation
}

// the shared depth normalisation: lo and the floored range, as binary32 (NumPy computes `(depth - lo) / rng` of a
// float32 map in binary32)
struct SsimDepthRange {
    float lo, rng;
};

RM_HD SsimDepthRange ssim_depth_range(double lo, double hi)
{
    const double r = hi - lo;
    SsimDepthRange d;
    d.lo = (float)lo;
    d.rng = (float)(r > 1e-6 ? r : 1e-6);                  // max(hi - lo, 1e-6)
    return d;
}

// (min, max) of a capture's depth over its hits; (0, 1) without a hit.  As NumPy's min / max, a NaN on any hit makes
// both NaN, wherever it sits (`d < a` alone would skip it unless it came first).  ssim_depth_range(NaN, NaN) keeps its
// floor (`NaN > 1e-6` is false) and that does not matter: lo is NaN, so `depth - lo` is NaN on every hit pixel and the
// depth image is 0 there whatever the range is.
inline void ssim_depth_minmax(const float* depth, const uint8_t* hit, size_t n, double* lo, double* hi)
{
    bool any = false, nan = false;
    float a = 0.0f, b = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        if (!hit[i]) continue;
        const float d = depth[i];
        if (d != d) nan = true;
        if (!any) { a = b = d; any = true; }
        else { a = d < a ? d : a; b = d > b ? d : b; }
    }
    if (nan) a = b = __builtin_nanf("");
    *lo = any ? (double)a : 0.0;
    *hi = any ? (double)b : 1.0;
}

RM_HD uint8_t ssim_depth_u8(float depth, bool hit, SsimDepthRange r)
{
    // binary32 quotient, correctly rounded: the binary64 quotient of two binary32 numbers rounds to it (53 >= 2 * 24 + 2)
    float norm = (float)((double)(depth - r.lo) / (double)r.rng);
    norm = norm < 0.0f ? 0.0f : (norm > 1.0f ? 1.0f : norm);      // np.clip: a NaN stays
    return ssim_to_u8(hit ? 1.0f - norm : 0.0f);
}

RM_HD uint8_t ssim_normal_u8(float n, bool hit) { return ssim_to_u8(hit ? n * 0.5f + 0.5f : 0.0f); }

// pixel p of channel c of a capture's images (normal / colour: H x W x 3 interleaved)
RM_HD uint8_t ssim_channel_u8(int c, const float* depth, const float* normal, const float* color, const uint8_t* hit, size_t p,
                              SsimDepthRange r)
{
    if (c == 0) return ssim_depth_u8(depth[p], hit[p] != 0, r);
    if (c < kSsimColor0) return ssim_normal_u8(normal[3 * p + (size_t)(c - 1)], hit[p] != 0);
    return ssim_to_u8(color[3 * p + (size_t)(c - kSsimColor0)]);
}

// ---- the per-pixel formula -----------------------------------------------------------------------------------------------

// S of one window from its five integer sums
RM_HD double ssim_pixel(int32_t sx, int32_t sy, int32_t sxx, int32_t syy, int32_t sxy)
{
    const double n = (double)(kSsimWin * kSsimWin), cov_norm = n / (n - 1.0);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double ux = (double)sx / n, uy = (double)sy / n;
    const double uxx = (double)sxx / n, uyy = (double)syy / n, uxy = (double)sxy / n;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

// ---- the device call (rm_ssim_scores and its launch_ssim, both in rm_ssim.hip) ------------------------------------------

constexpr int kSsimMaxMethods = 65535;                     // a grid's z extent

// Everything in device memory.  The methods' maps lie method after method (depth, hit: W*H each; normal, color: W*H*3);
// part holds nmethods x kSsimChannels x tiles sums of S, ssd nmethods x 3 x tiles sums of squared differences, out
// nmethods x 4 scores.  has_normal / has_color == 0: those maps are NULL and their channels are skipped.
struct SsimLaunch {
    int width, height, nmethods, has_normal, has_color;
    SsimDepthRange range;
    const float *ref_depth, *ref_normal, *ref_color;
    const uint8_t* ref_hit;
    uint8_t* ref_img;                                      // kSsimChannels planes of W*H: the reference's images
    const float *depth, *normal, *color;
    const uint8_t* hit;
    double* part;
    long long* ssd;
    double* out;
};

// ---- tiles and the summation order -------------------------------------------------------------------------------------

RM_HD int ssim_tiles_x(int width) { return (width - kSsimPad + kSsimTileW - 1) / kSsimTileW; }
RM_HD int ssim_tiles_y(int height) { return (height - kSsimPad + kSsimTileH - 1) / kSsimTileH; }

// Which tile adds pixel (lx, ly) of its staged block to the colour image's squared difference: the tile whose output
// block holds it, and the last tile of a row / column for the three pixels the cropping leaves over.
RM_HD bool ssim_owns(int lx, int ly, bool last_x, bool last_y) { return (lx < kSsimTileW || last_x) && (ly < kSsimTileH || last_y); }

// a tile's kSsimTile values folded by halves, on one thread
inline double ssim_fold(double* v)
{
    for (int s = kSsimTile / 2; s > 0; s >>= 1)
        for (int i = 0; i < s; ++i) v[i] += v[i + s];
    return v[0];
}

RM_HD double ssim_sum_in_order(const double* v, int n)
{
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += v[i];
    return s;
}

RM_HD long long ssim_sum_in_order(const long long* v, int n)
{
    long long s = 0;
    for (int i = 0; i < n; ++i) s += v[i];
    return s;
}

// The four scores from the channels' sums of S and the colour channels' sums of squared differences; NaN for the maps
// the captures do not carry.
RM_HD void ssim_combine(const double* s_sum /* kSsimChannels */, const long long* ssd /* 3 */, int width, int height, bool has_normal,
                        bool has_color, double* out /* depth_ssim, normal_ssim, color_ssim, color_rmse */)
{
    const double nan = __builtin_nan("");
    const double windows = (double)((long long)(width - kSsimPad) * (long long)(height - kSsimPad));
    double m[kSsimChannels];
    for (int c = 0; c < kSsimChannels; ++c) m[c] = s_sum[c] / windows;
    out[0] = m[0];
    out[1] = has_normal ? (m[1] + m[2] + m[3]) / 3.0 : nan;
    out[2] = has_color ? (m[4] + m[5] + m[6]) / 3.0 : nan;
    out[3] = has_color ? rm_sqrt((double)(ssd[0] + ssd[1] + ssd[2]) / (double)(3ll * width * height)) : nan;
}

}  // namespace rm
