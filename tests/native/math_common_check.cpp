// Host-only check build of the team forms of the libm restatements with their rare-path tests under the harness's
// control (tests only; tests/test_math_exact_team_common.py).  rm_team_rare (rm_math_trig.h) hands every test to
// RM_TEAM_PATH_FORCE: per site the call goes down the body the lane's own predicate picks (0), the general body (1) or
// the common body (2), and the lane's own predicate is recorded either way, so the test knows which arguments a forced
// common body is entitled to.
#include <stddef.h>
#include <stdint.h>

static int rmt_mode[8];                 // per RM_SITE_*: 0 as the lane decides, 1 general, 2 common
static unsigned rmt_rare_sites;         // bit s: the lane's own predicate at site s was "rare" during the current call
static inline bool rmt_decide(bool lane_rare, int site)
{
    if (lane_rare) rmt_rare_sites |= 1u << site;
    return rmt_mode[site] == 1 ? true : (rmt_mode[site] == 2 ? false : lane_rare);
}
#define RM_TEAM_PATH_FORCE(lane_rare, site) rmt_decide(lane_rare, site)
#include "../../raymarch_algo_compare_amd/csrc/rm_math.h"

extern "C" {
void rmt_force(int site, int mode) { rmt_mode[site] = mode; }
// `rare` (may be null): per argument the sites whose own predicate asked for the general body
void rmt_acos(const double* x, size_t n, double* out, uint8_t* rare)
{
    for (size_t i = 0; i < n; ++i) { rmt_rare_sites = 0; out[i] = rm::rm_acos<true>(x[i]); if (rare) rare[i] = (uint8_t)rmt_rare_sites; }
}
void rmt_atan2(const double* y, const double* x, size_t n, double* out, uint8_t* rare)
{
    for (size_t i = 0; i < n; ++i) { rmt_rare_sites = 0; out[i] = rm::rm_atan2<true>(y[i], x[i]); if (rare) rare[i] = (uint8_t)rmt_rare_sites; }
}
void rmt_sincos(const double* x, size_t n, double* s, double* c, uint8_t* rare)
{
    for (size_t i = 0; i < n; ++i) { rmt_rare_sites = 0; rm::rm_sincos<true>(x[i], &s[i], &c[i]); if (rare) rare[i] = (uint8_t)rmt_rare_sites; }
}
// the root with the wave's sparse flag handed down (rm_pow_half_sparse); guard_failed: the full pow stood in
void rmt_pow_half_sparse(const double* x, size_t n, int sparse, double* out, uint8_t* guard_failed)
{
    for (size_t i = 0; i < n; ++i) {
        out[i] = rm::rm_pow_half_sparse(x[i], sparse != 0);
        if (guard_failed) { bool ok; (void)rm::rm_pow_half_guard(x[i], &ok); guard_failed[i] = !ok; }
    }
}
// the banded team forms (COMMON false: every band behind its own ballot, no entry test; on the host every block runs)
void rmb_acos(const double* x, size_t n, double* out) { for (size_t i = 0; i < n; ++i) out[i] = rm::rm_acos_team<false>(x[i]); }
void rmb_atan2(const double* y, const double* x, size_t n, double* out) { for (size_t i = 0; i < n; ++i) out[i] = rm::rm_atan2_team<false>(y[i], x[i]); }
void rmb_sincos(const double* x, size_t n, double* s, double* c) { for (size_t i = 0; i < n; ++i) rm::rm_sincos_team<false>(x[i], &s[i], &c[i]); }
// the dense forms, as tests/native/math_check.cpp names them
void rmc_acos(const double* x, size_t n, double* out) { for (size_t i = 0; i < n; ++i) out[i] = rm::rm_acos<false>(x[i]); }
void rmc_atan2(const double* y, const double* x, size_t n, double* out) { for (size_t i = 0; i < n; ++i) out[i] = rm::rm_atan2<false>(y[i], x[i]); }
void rmc_sincos(const double* x, size_t n, double* s, double* c) { for (size_t i = 0; i < n; ++i) rm::rm_sincos<false>(x[i], &s[i], &c[i]); }
void rmc_pow_half(const double* x, size_t n, double* out) { for (size_t i = 0; i < n; ++i) out[i] = rm::rm_pow(x[i], 0.5); }
}
