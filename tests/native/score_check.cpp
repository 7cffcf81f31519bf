// Host-only check build of the capture scoring (csrc/rm_score.h) -- compiled by g++ for tests ONLY, so the per-pixel values,
// the silhouette band, the rank rules and the summation order the gfx950 kernels are built from can be compared with
// scoring.py and with the device in a container without a GPU.  Never loaded by the product.
//
// The loops below walk the image as rm_score.hip's workgroups do: tile by tile, a tile's 256 values folded by halves, the
// tiles' partial sums added in index order.  A plain sort stands in for the radix select: s[j] is read from the sorted
// keys, and s[j + 1] is taken from it by score_next_rank exactly as the device takes it; rmsc_score answers 2 if that
// is not the sorted sample's next element.
//
// With -DRM_SCORE_CHECK_MAIN the file is a stand-alone program (for a sanitizer build): it reads the cases that
// tests/score_cases.py dumps (dump_cases) and runs rmsc_band and rmsc_score on each.
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../raymarch_algo_compare_amd/csrc/rm_score.h"

using namespace rm;

extern "C" {

// scoring.silhouette_band(hit, k): W*H bytes, 1 in the band
void rmsc_band(int W, int H, int k, const uint8_t* hit, uint8_t* band)
{
    std::vector<uint8_t> edge((size_t)W * H);
    auto flag = [&](int x, int y) { return x < 0 || x >= W || y < 0 || y >= H ? 2 : (int)(hit[(size_t)y * W + x] != 0); };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            edge[(size_t)y * W + x] = score_is_edge(flag(x, y), flag(x - 1, y), flag(x + 1, y), flag(x, y - 1), flag(x, y + 1));
    auto is_edge = [&](int x, int y) { return x >= 0 && x < W && y >= 0 && y < H && edge[(size_t)y * W + x] != 0; };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) band[(size_t)y * W + x] = score_in_band(is_edge, x, y, k);
}

// one method against the reference, as rm_score_captures gives it; 0, or -1 for arguments it would refuse
int rmsc_score(int W, int H, int band_k, const void* r_depth, const void* r_normal, const uint8_t* r_hit, int r_fp64,
               const void* m_depth, const void* m_normal, const uint8_t* m_hit, int m_fp64, ScoreResult* out)
{
    if (W <= 0 || H <= 0 || band_k > kScoreMaxBand || !r_depth || !r_hit || !m_depth || !m_hit || !r_normal != !m_normal) return -1;
    const ScoreMaps r = { r_depth, r_normal, r_hit, r_fp64 }, m = { m_depth, m_normal, m_hit, m_fp64 };
    const bool has_normal = r_normal != nullptr;
    std::vector<uint8_t> band;
    if (band_k >= 0) {
        band.resize((size_t)W * H);
        rmsc_band(W, H, band_k, r_hit, band.data());
    }
    const int tx = score_tiles_x(W), ty = score_tiles_y(H);
    std::vector<double> part[kScoreSums];
    for (auto& p : part) p.resize((size_t)tx * ty);
    int64_t counts[kScoreCounts] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    std::vector<uint64_t> keys[2];
    for (int t = 0; t < tx * ty; ++t) {
        const int x0 = (t % tx) * kSsimTileW, y0 = (t / tx) * kSsimTileH;
        double v[kScoreSums][kSsimTile];
        for (int i = 0; i < kSsimTile; ++i) {
            const int x = x0 + i % kSsimTileW, y = y0 + i / kSsimTileW;
            for (auto& q : v) q[i] = 0.0;
            if (x >= W || y >= H) continue;
            const ScorePixel px = score_pixel(m, r, band_k >= 0 ? band.data() : nullptr, has_normal, (size_t)y * W + x);
            const bool co = px.mine && px.truth, un = px.mine || px.truth;
            counts[SC_METHOD] += px.mine; counts[SC_REFERENCE] += px.truth; counts[SC_CO] += co; counts[SC_UNION] += un;
            counts[SC_CO_CORE] += co && px.core; counts[SC_UNION_CORE] += un && px.core;
            if (!co) continue;
            counts[SC_NAN_DEPTH] += px.gap != px.gap; counts[SC_NAN_ANGLE] += px.angle != px.angle;
            v[0][i] = px.mag; v[1][i] = px.gap * px.gap; v[2][i] = px.gap; v[3][i] = px.angle;
            keys[0].push_back(score_key(px.mag));
            if (has_normal) keys[1].push_back(score_key(px.angle));
        }
        for (int q = 0; q < kScoreSums; ++q) part[q][t] = ssim_fold(v[q]);
    }
    double sums[kScoreSums];
    for (int q = 0; q < kScoreSums; ++q) sums[q] = ssim_sum_in_order(part[q].data(), tx * ty);
    const int64_t n = counts[SC_CO];
    ScoreRanks k;
    int rc = 0;
    for (auto& s : keys) std::sort(s.begin(), s.end());
    for (int s = 0; s < kScoreSelects; ++s) {
        const std::vector<uint64_t>& sorted = keys[s == 2];
        k.lo[s] = k.hi[s] = kScoreNoKey;
        if (sorted.empty()) continue;
        const int64_t j = s == 1 ? score_rank_med(n) : score_rank_p95(n);
        const uint64_t sj = sorted[(size_t)j];
        const auto up = std::upper_bound(sorted.begin(), sorted.end(), sj);
        k.lo[s] = sj;
        k.hi[s] = score_next_rank(sj, j, n, (int64_t)(up - sorted.begin()), up == sorted.end() ? kScoreNoKey : *up);
        if (k.hi[s] != sorted[(size_t)std::min(j + 1, n - 1)]) rc = 2;
    }
    score_combine(counts, sums, k, has_normal, out);
    return rc;
}

}

#if defined(RM_SCORE_CHECK_MAIN)
#include <stdio.h>

// the dump of tests/score_cases.py: per case seven int32 { W, H, band_k, r_fp64, m_fp64, has_normal, 0 }, then the
// reference's depth, normal (if any) and hit, then the method's
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[7];
    int ncases = 0, bad = 0;
    while (fread(h, sizeof h, 1, f) == 1) {
        const size_t n = (size_t)h[0] * (size_t)h[1];
        std::vector<char> buf[6];
        const size_t bytes[6] = { n * (h[3] ? 8 : 4), h[5] ? 3 * n * (h[3] ? 8 : 4) : 0, n, n * (h[4] ? 8 : 4), h[5] ? 3 * n * (h[4] ? 8 : 4) : 0, n };
        for (int i = 0; i < 6; ++i) {
            buf[i].resize(bytes[i]);
            if (bytes[i] && fread(buf[i].data(), 1, bytes[i], f) != bytes[i]) return 3;
        }
        std::vector<uint8_t> band(n);
        if (h[2] >= 0) rmsc_band(h[0], h[1], h[2], (const uint8_t*)buf[2].data(), band.data());
        ScoreResult out;
        const int rc = rmsc_score(h[0], h[1], h[2], buf[0].data(), h[5] ? buf[1].data() : nullptr, (const uint8_t*)buf[2].data(), h[3],
                                  buf[3].data(), h[5] ? buf[4].data() : nullptr, (const uint8_t*)buf[5].data(), h[4], &out);
        bad += rc != 0;
        ++ncases;
    }
    fclose(f);
    printf("%d cases, %d refused or inconsistent\n", ncases, bad);
    return bad ? 1 : 0;
}
#endif
