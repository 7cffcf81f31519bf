// Host-only check build of the SSIM scoring (csrc/rm_ssim.h) -- compiled by g++ for tests ONLY, so the quantisation, the
// per-pixel formula and the summation order the gfx950 kernels are built from can be compared with a plain float64
// restatement, with the reference's images and with the device in a container without a GPU.  Never loaded by the product.
//
// The loops below walk the image as rm_ssim.hip's workgroups do: tile by tile, the tile's 256 values folded by halves,
// the tiles' partial sums added in index order; the colour images' squared differences likewise, each tile adding the
// pixels of its staged block that ssim_owns gives it.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../raymarch_algo_compare_amd/csrc/rm_ssim.h"

using namespace rm;

namespace {

// sum of S over the cropped W x H planes x, y, in the device's order
double plane_sum(const uint8_t* x, const uint8_t* y, int W, int H)
{
    const int tx = ssim_tiles_x(W), ty = ssim_tiles_y(H);
    std::vector<double> part((size_t)tx * ty);
    for (int t = 0; t < tx * ty; ++t) {
        const int x0 = (t % tx) * kSsimTileW, y0 = (t / tx) * kSsimTileH;
        double v[kSsimTile];
        for (int i = 0; i < kSsimTile; ++i) {
            const int ox = x0 + i % kSsimTileW, oy = y0 + i / kSsimTileW;
            v[i] = 0.0;
            if (ox >= W - kSsimPad || oy >= H - kSsimPad) continue;
            int32_t s[5] = { 0, 0, 0, 0, 0 };
            for (int r = 0; r < kSsimWin; ++r)
                for (int c = 0; c < kSsimWin; ++c) {
                    const size_t p = (size_t)(oy + r) * W + (size_t)(ox + c);
                    const int32_t a = x[p], b = y[p];
                    s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
                }
            v[i] = ssim_pixel(s[0], s[1], s[2], s[3], s[4]);
        }
        part[t] = ssim_fold(v);
    }
    return ssim_sum_in_order(part.data(), tx * ty);
}

// sum of squared differences of the W x H planes x, y, walked as the device walks them: every tile goes over its staged
// block (output pixels and halo) and adds the pixels that ssim_owns gives it; the tiles' sums are added in index order
long long plane_ssd(const uint8_t* x, const uint8_t* y, int W, int H)
{
    const int tx = ssim_tiles_x(W), ty = ssim_tiles_y(H);
    std::vector<long long> part((size_t)tx * ty);
    for (int t = 0; t < tx * ty; ++t) {
        const int tix = t % tx, tiy = t / tx, x0 = tix * kSsimTileW, y0 = tiy * kSsimTileH;
        const bool last_x = tix == tx - 1, last_y = tiy == ty - 1;
        long long s = 0;
        for (int ly = 0; ly < kSsimStageH; ++ly)
            for (int lx = 0; lx < kSsimStageW; ++lx) {
                const int ix = x0 + lx, iy = y0 + ly;
                if (ix >= W || iy >= H || !ssim_owns(lx, ly, last_x, last_y)) continue;
                const size_t p = (size_t)iy * W + (size_t)ix;
                const int d = (int)x[p] - (int)y[p];
                s += d * d;
            }
        part[t] = s;
    }
    return ssim_sum_in_order(part.data(), tx * ty);
}

void images(int W, int H, const float* depth, const float* normal, const float* color, const uint8_t* hit, SsimDepthRange r,
            uint8_t* out)
{
    const size_t n = (size_t)W * H;
    for (int c = 0; c < kSsimChannels; ++c) {
        if ((c >= 1 && c < kSsimColor0 && !normal) || (c >= kSsimColor0 && !color)) continue;
        for (size_t p = 0; p < n; ++p) out[(size_t)c * n + p] = ssim_channel_u8(c, depth, normal, color, hit, p, r);
    }
}

}  // namespace

extern "C" {

// (lo, hi) of a capture's depth over its hits
void rms_depth_range(int W, int H, const float* depth, const uint8_t* hit, double* lohi)
{
    ssim_depth_minmax(depth, hit, (size_t)W * H, &lohi[0], &lohi[1]);
}

// the seven planes (W*H each: depth, normal xyz, colour rgb) of a capture's images; a NULL normal / colour leaves its planes
void rms_images(int W, int H, const float* depth, const float* normal, const float* color, const uint8_t* hit, double lo, double hi,
                uint8_t* out)
{
    images(W, H, depth, normal, color, hit, ssim_depth_range(lo, hi), out);
}

// mean S of two W x H planes
double rms_plane_ssim(const uint8_t* x, const uint8_t* y, int W, int H)
{
    return plane_sum(x, y, W, H) / (double)((long long)(W - kSsimPad) * (long long)(H - kSsimPad));
}

// the four scores of a method capture against a reference capture, as rm_ssim_scores gives them
int rms_scores(int W, int H, const float* r_depth, const float* r_normal, const float* r_color, const uint8_t* r_hit, const float* m_depth,
               const float* m_normal, const float* m_color, const uint8_t* m_hit, double* out)
{
    if (W < kSsimWin || H < kSsimWin || !r_normal != !m_normal || !r_color != !m_color) return -1;
    const size_t n = (size_t)W * H;
    double lo, hi;
    ssim_depth_minmax(r_depth, r_hit, n, &lo, &hi);
    const SsimDepthRange r = ssim_depth_range(lo, hi);
    std::vector<uint8_t> x(kSsimChannels * n), y(kSsimChannels * n);
    images(W, H, r_depth, r_normal, r_color, r_hit, r, x.data());
    images(W, H, m_depth, m_normal, m_color, m_hit, r, y.data());
    double s_sum[kSsimChannels] = { 0, 0, 0, 0, 0, 0, 0 };
    long long ssd[3] = { 0, 0, 0 };
    for (int c = 0; c < kSsimChannels; ++c) {
        if ((c >= 1 && c < kSsimColor0 && !r_normal) || (c >= kSsimColor0 && !r_color)) continue;
        s_sum[c] = plane_sum(x.data() + c * n, y.data() + c * n, W, H);
        if (c >= kSsimColor0) ssd[c - kSsimColor0] = plane_ssd(x.data() + c * n, y.data() + c * n, W, H);
    }
    ssim_combine(s_sum, ssd, W, H, r_normal != nullptr, r_color != nullptr, out);
    return 0;
}

}
