// Host-only check build of the launch plan (csrc/rm_launch_plan.h) -- compiled by g++ for tests ONLY, with faked device
// facts, so tests/test_launch_plan.py can pin the launch policy without a GPU.  Never loaded by the product.
#include <stdint.h>
#include <string.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_launch_plan.h"

using namespace rm;

#define PLAN_FIELDS(X)                                                                                                 \
    X(nframes) X(batch) X(march_frame) X(rays) X(tile_h) X(tiles_x) X(tiles_y) X(refill_min) X(interleave) X(mode)    \
    X(park[0]) X(park[1]) X(single) X(fused_reduce) X(tile_order) X(static_order) X(render_grid) X(queue_entry_bytes)  \
    X(team_wgs) X(producer_waves) X(late_team_first) X(early_exit_wgs) X(exit_backlog) X(keep_busy) X(early_trips)     \
    X(early_handover) X(suspend_after2) X(q0_detach) X(q0_first) X(q0_refill_min) X(q0_retry) X(team_retry)            \
    X(team_steal) X(team_prio) X(max_spins) X(pipeline_grid) X(resume_grid) X(resume_refill_min) X(pass_keep_busy)     \
    X(team_pass_grid) X(pass_team[0]) X(pass_team[1])

extern "C" {

// the field names, comma-separated, in the order rmplan writes them (after the refusal flag)
const char* rmplan_fields(void)
{
#define X(f) #f ","
    return PLAN_FIELDS(X);
#undef X
}

// plan_launch with faked device facts: per-CU occupancy of the render kernel (one frame / batch) and of the pipeline
// kernel.  out[0] = 1 when the plan refuses the descriptor, then the fields of rmplan_fields.  asked[0..1]: how often the
// plan asked for the render / pipeline occupancy.
void rmplan(const RmFrameDesc* d, int batch_frames, const RmMarchConfig* configs, int cus, int occ_render, int occ_batch,
            int occ_pipeline, int has_teams, int has_resume_team, int entry_bytes, int64_t* out, int* asked)
{
    DeviceFacts f;
    f.cus = cus;
    f.has_teams = has_teams != 0;
    f.has_resume_team = has_resume_team != 0;
    f.entry_bytes = entry_bytes;
    asked[0] = asked[1] = 0;
    f.per_cu = [&](OccKernel k, int, int, int batch) {
        ++asked[k == OccKernel::pipeline ? 1 : 0];
        return k == OccKernel::pipeline ? occ_pipeline : (batch ? occ_batch : occ_render);
    };
    const LaunchPlan p = plan_launch(*d, f, batch_frames, configs);
    int i = 0;
    out[i++] = p.refuse != nullptr;
#define X(f) out[i++] = (int64_t)p.f;
    PLAN_FIELDS(X)
#undef X
}

}
