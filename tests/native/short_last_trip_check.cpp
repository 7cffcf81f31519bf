// Host-only check build of SceneMandelbulb (rm_scenes.h) for the short last trip -- compiled by g++ for tests ONLY.
// slt_sdf is the product's sdf() (its eighth trip is trip_last); slt_full runs the same evaluation to completion through
// begin / trip / value, every trip a full pass, and reports the trips it took.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_scenes.h"

using namespace rm;

extern "C" {

void slt_sdf(const double* xyz, size_t n, double* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = SceneMandelbulb::sdf(v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
}

void slt_full(const double* xyz, size_t n, double* out, int32_t* trips, double* r_last)
{
    for (size_t i = 0; i < n; ++i) {
        SceneMandelbulb::Eval e;
        bool done = SceneMandelbulb::begin(e, v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
        while (!done) done = SceneMandelbulb::trip(e);
        out[i] = SceneMandelbulb::value(e);
        trips[i] = SceneMandelbulb::eval_trips(e);
        r_last[i] = e.r;
    }
}

// begin, full trips up to the short one, trip_last: the evaluation as a team runs it; also the trip count it leaves
void slt_stepped(const double* xyz, size_t n, double* out, int32_t* trips)
{
    for (size_t i = 0; i < n; ++i) {
        SceneMandelbulb::Eval e;
        bool done = SceneMandelbulb::begin(e, v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
        for (int k = 0; !done; ++k) {
            if (k == SceneMandelbulb::kLastTrip) { SceneMandelbulb::trip_last(e); done = true; }
            else done = SceneMandelbulb::trip(e);
        }
        out[i] = SceneMandelbulb::value(e);
        trips[i] = SceneMandelbulb::eval_trips(e);
    }
}

}
