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
    X(team_pass_grid) X(pass_team[0]) X(pass_team[1]) X(form)

extern "C" {

// the field names, comma-separated, in the order rmplan writes them (after the refusal flag)
const char* rmplan_fields(void)
{
#define X(f) #f ","
    return PLAN_FIELDS(X);
#undef X
}

// plan_launch with faked device facts: per-CU occupancy of the render kernel (one frame / batch) and of the pipeline
// kernel, and of the split form's producer and team kernels (has_split: the scene has them).  out[0] = 1 when the plan
// refuses the descriptor, then the fields of rmplan_fields.  asked[0..3]: how often the plan asked for the render /
// pipeline / split producers' / split teams' occupancy.
void rmplan(const RmFrameDesc* d, int batch_frames, const RmMarchConfig* configs, int cus, int occ_render, int occ_batch,
            int occ_pipeline, int has_teams, int has_resume_team, int entry_bytes, int64_t* out, int* asked, int has_split,
            int occ_producers, int occ_teams)
{
    DeviceFacts f;
    f.cus = cus;
    f.has_teams = has_teams != 0;
    f.has_resume_team = has_resume_team != 0;
    f.entry_bytes = entry_bytes;
    f.has_split = has_split != 0;
    asked[0] = asked[1] = asked[2] = asked[3] = 0;
    f.per_cu = [&](OccKernel k, int, int, int batch) {
        ++asked[(int)k];
        switch (k) {
            case OccKernel::pipeline: return occ_pipeline;
            case OccKernel::split_producers: return occ_producers;
            case OccKernel::split_teams: return occ_teams;
            default: return batch ? occ_batch : occ_render;
        }
    };
    const LaunchPlan p = plan_launch(*d, f, batch_frames, configs);
    int i = 0;
    out[i++] = p.refuse != nullptr;
#define X(f) out[i++] = (int64_t)p.f;
    PLAN_FIELDS(X)
#undef X
}

// queue_step: out = { bytes to clear, then the key to remember: stride, writer, used }
void rmplan_queue(int prev_stride, int prev_writer, uint64_t prev_used, int writer, int stride, uint64_t need, uint64_t cap_before,
                  uint64_t cap_after, uint64_t* out)
{
    const QueueStep s = queue_step({ prev_stride, prev_writer, (size_t)prev_used }, writer, stride, (size_t)need, (size_t)cap_before, (size_t)cap_after);
    out[0] = s.clear; out[1] = (uint64_t)s.key.stride; out[2] = (uint64_t)s.key.writer; out[3] = s.key.used;
}

int rmplan_fillers(int cus, int64_t nteams) { return team_fillers(cus, nteams); }

// frame_key (10 words) and static_order_key (12 words) of `d`
void rmplan_keys(const RmFrameDesc* d, int tile_h, int nframes, int order, int64_t* dynamic10, int64_t* static12)
{
    long long a[10], b[12];
    frame_key(*d, tile_h, a);
    static_order_key(*d, tile_h, nframes, order, b);
    for (int i = 0; i < 10; ++i) dynamic10[i] = a[i];
    for (int i = 0; i < 12; ++i) static12[i] = b[i];
}

}
