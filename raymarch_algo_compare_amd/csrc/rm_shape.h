// rm_shape.h -- the tile and workgroup shape shared by the kernels (rm_kernels.h, rm_pipeline.h) and the host's launch
// plan (rm_launch_plan.h).  No HIP include: the plan is compiled by the host compiler alone in tests/native/plan_check.cpp.
#pragma once

namespace rm {

constexpr int kTileW = 64;          // one tile row == one wavefront-wide store
constexpr int kWavesPerWG = 4;      // 256-thread workgroups: four waves share one LDS copy of the libm tables

// Workgroup shape of the pipeline kernel (1080p Mandelbulb / Standard figures).  Built: 256-thread
// workgroups, two per compute unit; a team workgroup (three waves, the fourth exits) shares its CU -- and every one of
// its SIMDs -- with a producer workgroup: 9.6-10.0 ms.  Measured and rejected, and no longer in the source:
//  * 512-thread workgroups, one per CU, of which `team_grid` carry one or two teams and nothing else (two teams
//    synchronised through an LDS arrival counter): chains at the speed of an idle CU (13 us per evaluation against
//    17-20 next to producers), but 48-96 such CUs cannot absorb the rays that cross the threshold: 11.1-12.0 ms.
//  * 512-thread workgroups, one per CU, a team workgroup being waves {0,1,2} = the team, wave 4 idle and waves
//    {3,5,6,7} producers, so the team's critical wave has its SIMD to itself: 10.2-10.4 ms -- no better, so what holds
//    the longest rays back next to producers is not the issue slot they share.  The marks (rm_get_pass_ms) say what
//    is: when the producers are done the longest ray still has > 400 of its 464 team evaluations ahead -- it sat in
//    queue 1 behind the burst of rays that cross the threshold while the object's tiles are rendered (90 000 at 48
//    trips, of which 133 run to 512 and nothing tells them apart).
constexpr int kPipeWaves = 4;

}  // namespace rm
