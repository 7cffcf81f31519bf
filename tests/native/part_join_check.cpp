// Host-only check build (tests only) of the Mandelbulb's join per part (csrc/rm_scenes.h THE JOIN PER PART): the bail-out
// decision from the squared length (csrc/rm_math_pow.h rm_bail4) next to the compares it stands for, and one SDF
// evaluation as the part-P wave of a team steps it (csrc/rm_kernels.h team_flag_evaluation) next to SceneMandelbulb::sdf.
// Never loaded by the product.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_scenes.h"

using namespace rm;
using Scene = SceneMandelbulb;

// The evaluation of point p as team_flag_evaluation<Scene, SPARSE> runs it for one lane of the part-P wave.  The values of
// the exchange come from where the team takes them: part 1's from this wave when P == 1, everything that reads r from
// `w`, a wave that keeps today's begin and join (parts 0 and 2).  *lockstep is cleared if the two waves ever decide
// differently.
template <int P, bool SPARSE>
static void part_eval(vec3 p, Scene::Eval& e, int32_t* ended, uint8_t* lockstep)
{
    Scene::Eval w;
    double s2 = 0.0, none = 0.0;
    bool ready = Scene::begin_part<P>(e, p, SPARSE, s2);
    bool wready = Scene::begin_part<0>(w, p, SPARSE, none);
    *lockstep = ready == wready;
    *ended = ready ? 0 : -1;                       // 0: ready at begin; 1..7: bail-out in that trip; 8: by the count
    for (int n = 0; n < Scene::kLastTrip && !ready; ++n) {
        double st, ct, sp, cp, r7, zr;
        Scene::trip_part<0, SPARSE>(w, st, ct);
        Scene::trip_part<1, SPARSE>(P == 1 ? e : w, sp, cp);
        Scene::trip_part<2, SPARSE>(w, r7, zr);
        ready = Scene::trip_join_part<P>(e, st, ct, sp, cp, r7, zr, SPARSE, s2);
        wready = Scene::trip_join_part<0>(w, st, ct, sp, cp, r7, zr, SPARSE, none);
        if (ready != wready) *lockstep = 0;
        if (ready) *ended = n + 1;
    }
    if (P == 1) Scene::part1_root(e, SPARSE, s2);
    if (!ready) { Scene::trip_last(e); *ended = 8; }
}

extern "C" {

// decision[i] = rm_bail4(s[i], sparse); band[i] = rm_bail4_band(s[i]); rm_gt / libm_gt: the compares it stands for
void pj_bail4(const double* s, size_t n, int sparse, uint8_t* decision, uint8_t* band, uint8_t* rm_gt, uint8_t* libm_gt)
{
    double (*volatile f)(double, double) = ::pow;
    for (size_t i = 0; i < n; ++i) {
        decision[i] = rm_bail4(s[i], sparse != 0) ? 1 : 0;
        band[i] = rm_bail4_band(s[i]) ? 1 : 0;
        rm_gt[i] = rm_pow(s[i], 0.5) > 4.0 ? 1 : 0;
        libm_gt[i] = f(s[i], 0.5) > 4.0 ? 1 : 0;
    }
}

double pj_band_hi(void) { return kBail4Hi; }

// the part-`part` form of the evaluation at every point: r, dr, i, value(), how it ended, and whether the wave stayed in
// step with one that keeps today's join
void pj_part_eval(int part, int sparse, const double* xyz, size_t n, double* r, double* dr, int32_t* it, double* value, int32_t* ended,
                  uint8_t* lockstep)
{
    for (size_t i = 0; i < n; ++i) {
        const vec3 p = v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        Scene::Eval e;
        if (sparse) {
            if (part == 0) part_eval<0, true>(p, e, &ended[i], &lockstep[i]);
            else if (part == 1) part_eval<1, true>(p, e, &ended[i], &lockstep[i]);
            else part_eval<2, true>(p, e, &ended[i], &lockstep[i]);
        } else {
            if (part == 0) part_eval<0, false>(p, e, &ended[i], &lockstep[i]);
            else if (part == 1) part_eval<1, false>(p, e, &ended[i], &lockstep[i]);
            else part_eval<2, false>(p, e, &ended[i], &lockstep[i]);
        }
        r[i] = e.r; dr[i] = e.dr; it[i] = e.i; value[i] = Scene::value(e);
    }
}

// SceneMandelbulb::sdf's own pieces run to the end: r, dr, i and the value
void pj_sdf(const double* xyz, size_t n, double* r, double* dr, int32_t* it, double* value, double* sdf)
{
    for (size_t i = 0; i < n; ++i) {
        const vec3 p = v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        Scene::Eval e;
        bool done = Scene::begin(e, p);
        for (int k = 0; !done; ++k) {
            if (k == Scene::kLastTrip) { Scene::trip_last(e); break; }
            done = Scene::trip(e);
        }
        r[i] = e.r; dr[i] = e.dr; it[i] = e.i; value[i] = Scene::value(e);
        sdf[i] = Scene::sdf(p);
    }
}

}
