// Host-only check build (tests only): Standard sphere tracing of explicit rays through the Mandelbulb evaluation as a
// TEAM steps it -- begin / trip_part<0..2> + trip_join / trip_last / value, the team forms of the libm restatements and
// the root with the sparse flag on (csrc/rm_kernels.h march_rays_team_kernel) -- reporting for every ray which rare
// bands its evaluations meet and at which evaluation first.  tests/test_gpu_common_path.py lays its waves out from
// this, so that it can assert on the CPU that a wave leaves the common path where the test says it does.
#include <stddef.h>
#include <stdint.h>

static unsigned cp_sites;               // bit s: some rm_team_rare test of site s (RM_SITE_*) asked for the general body
static inline bool cp_decide(bool lane_rare, int site)
{
    if (lane_rare) cp_sites |= 1u << site;
    return lane_rare;
}
#define RM_TEAM_PATH_FORCE(lane_rare, site) cp_decide(lane_rare, site)
#include "../../raymarch_algo_compare_amd/csrc/rm_scenes.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_strategies.h"

using namespace rm;
using Scene = SceneMandelbulb;

// the kinds a ray is classified by: the five test sites, then the bands behind them
enum { K_ACOS = 0, K_SINCOS, K_DO_SIN, K_ATAN2_ENTRY, K_ATAN2_FORM, K_ACOS_TAYLOR, K_ACOS_SQRT, K_SINCOS_R2, K_ATAN2_SERIES,
       K_ATAN2_CASE_I, K_ROOT_GUARD, K_KINDS };

static uint32_t hi(double x) { return (uint32_t)(rm_asuint64(x) >> 32) & 0x7fffffffu; }

static unsigned kinds_of_trip(const Scene::Eval& e)
{
    unsigned k = 0;
    const double c = py_max(-1.0, py_min(1.0, e.z.z / py_max(e.r, 1e-12)));
    if (hi(c) < 0x3fc00000u) k |= 1u << K_ACOS_TAYLOR;
    if (hi(c) >= 0x3fef0000u) k |= 1u << K_ACOS_SQRT;
    const double th8 = rm_acos<false>(c) * 8.0, ph8 = rm_atan2<false>(e.z.y, e.z.x) * 8.0;
    const double angles[2] = { th8, ph8 };
    for (double a : angles)
        if (hi(a) >= 0x3feb6000u && hi(a) < 0x400368fdu) k |= 1u << K_SINCOS_R2;
    bool y_lt_x;
    double u, du;
    rm_atan2_quotient(rm_fabs(e.z.x), rm_fabs(e.z.y), &y_lt_x, &u, &du);
    if (u < 0.0625) k |= 1u << K_ATAN2_SERIES;
    if (e.z.x > 0.0 && y_lt_x) k |= 1u << K_ATAN2_CASE_I;
    return k;
}

static unsigned kind_of_root(vec3 a)
{
    bool safe;
    (void)rm_pow_half_guard(a.x * a.x + a.y * a.y + a.z * a.z, &safe);
    return safe ? 0u : 1u << K_ROOT_GUARD;
}

extern "C" {

int cp_kinds(void) { return K_KINDS; }

// first[K_KINDS * i + k]: the evaluation (0-based) of ray i that first meets kind k, -1 if none does
void cp_march(int max_iterations, double hit_threshold, double max_distance, const double* origins, const double* dirs, size_t n,
              uint8_t* hit, double* t, int32_t* iters, double* fs, int32_t* first)
{
    MarchCfg cfg;
    cfg.hit_threshold = hit_threshold; cfg.max_distance = max_distance; cfg.lipschitz = 1.0;
    cfg.max_iterations = max_iterations; cfg.full = 1;
    cfg.prm = default_strat_params();
    for (size_t i = 0; i < n; ++i) {
        const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
        const vec3 d = normalized(v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
        for (int k = 0; k < K_KINDS; ++k) first[K_KINDS * i + k] = -1;
        StratStandard s;
        bool done = s.start(cfg);
        Scene::Eval ev;
        for (int nev = 0; !done; ++nev) {
            const vec3 p = o + d * s.te;
            cp_sites = 0;
            unsigned kinds = kind_of_root(p);
            bool ready = Scene::begin(ev, p, true);
            for (int trip = 0; !ready; ++trip) {
                if (trip == Scene::kLastTrip) { Scene::trip_last(ev); break; }
                kinds |= kinds_of_trip(ev);
                double st, ct, sp, cp, r7, zr;
                Scene::trip_part<0>(ev, st, ct);
                Scene::trip_part<1>(ev, sp, cp);
                Scene::trip_part<2>(ev, r7, zr);
                ready = Scene::trip_join(ev, st, ct, sp, cp, r7, zr, true);
                if (ev.i < 8) kinds |= kind_of_root(ev.z);
            }
            kinds |= cp_sites;
            for (int k = 0; k < K_KINDS; ++k)
                if (((kinds >> k) & 1u) && first[K_KINDS * i + k] < 0) first[K_KINDS * i + k] = nev;
            done = s.step(Scene::value(ev), cfg);
        }
        hit[i] = (uint8_t)s.res.hit; t[i] = s.res.t; iters[i] = s.res.iters; fs[i] = s.res.final_sdf;
    }
}

}
