// rm_launch_plan.h -- the launch policy of a frame: how many launches, which budgets, grids, team share, tile order and
// knobs.  One pure function of the frame descriptor and a few device facts; no HIP call, no HIP include.  rm_frame.hip
// performs the plan (buffers, caches, enqueues) and takes the smaller rules at the end of this file -- the parked-ray
// queues' clear, the filler count of a team chain, the keys of the tile-order caches -- from here as well;
// tests/native/plan_check.cpp and tests/test_launch_plan.py pin all of it on the CPU.  Schedules never change results,
// so nothing else would notice a slip here.
//
// Scene ids (registry.py): 0 Sphere, 1 Grazing Plane, 2 Cube, 3 Thin Torus, 4 Cylinder, 5 Near Miss, 6 Hollow Cube,
// 10 Mandelbulb, 12 Pillar Forest, 13 Thin Planes Stack, 14 Sphere Cloud, 15 Bumpy Sphere, 18 Box Lattice,
// 19 Metaballs.  Strategy kernels: 4 Enhanced, 6 Overstep-Bisect, 7 Skipping-Spheres, 8 RevAA, 9 Adaptive-Hybrid,
// 10 Segment.
#pragma once

#include <algorithm>
#include <cstddef>
#include <functional>

#include "../../include/rm_hip.h"
#include "rm_shape.h"

namespace rm {

enum class OccKernel { render, pipeline, split_producers, split_teams };      // the last two: the split form's two kernels

// What the plan needs to know of the device and of the scene's kernels.
struct DeviceFacts {
    int cus = 0;                  // compute units
    bool has_teams = false;       // the scene has a team form (SceneLaunchers.has_teams)
    bool has_resume_team = false; // ... and a team resume kernel (SceneLaunchers.resume_team)
    bool has_split = false;       // ... and the split form of the single launch (SceneLaunchers.pipeline_producers / _teams)
    int entry_bytes = 0;          // one parked-ray queue entry of the strategy (SceneLaunchers.entry_bytes)
    // workgroups per compute unit the kernel reaches (<= 0: unknown); asked only where the plan needs it
    std::function<int(OccKernel kernel, int tile_h, int interleave, int batch)> per_cu;
};

struct LaunchPlan {
    const char* refuse = nullptr;     // set: the descriptor asks for a launch form that does not exist
    int nframes = 1;                  // frames of the launch (a batch of one is still a batch: `batch`)
    bool batch = false;
    int march_frame = -1;             // batches with per-frame configurations: the one the policy looked at
    long long rays = 0;               // rows x width x nframes
    int tile_h = 4, tiles_x = 0, tiles_y = 0;
    int refill_min = 0, interleave = 0;
    int mode = 1;                     // 1 = one launch per pass, 2 = the single launch (rm_pipeline.h)
    int park[2] = { 0, 0 };           // trip budgets of pass 1 / pass 2 (0 = that pass does not park)
    bool single = false;              // park[0] > 0 && mode == 2: the whole frame in ONE pipeline launch
    int fused_reduce = 0;
    int tile_order = 0;               // 1 = longest-first from the previous frame's costs, 2 = centre-out, 3 = natural,
    int static_order = 0;             // 4 = middle rows first; static_order: the library's choice (order 1 without costs)
    int render_grid = 0;              // persistent grid of the render kernel (not single)
    int queue_entry_bytes = 0;        // park[0] > 0: the parked-ray queues' entry stride
    // the single launch
    int team_wgs = 0, producer_waves = 0, late_team_first = 0, early_exit_wgs = 0, exit_backlog = 0, keep_busy = 0;
    int early_trips = 0, early_handover = 0, suspend_after2 = 0;
    int q0_detach = 0, q0_first = 0, q0_refill_min = 0, q0_retry = 0, team_retry = 0, team_steal = 0, team_prio = 0, max_spins = 0;
    int pipeline_grid = 0;
    int form = 0;                     // how the single launch is performed (single_launch_form): 1 fused, 2 split side by side, 3 split in sequence
    // one launch per pass: passes 2 and 3
    int resume_grid = 0, resume_refill_min = 0, pass_keep_busy = 0, team_pass_grid = 0;
    bool pass_team[2] = { false, false };     // the pass runs the team resume kernel
};

// A strategy program (rm_strategy_program.h; ids from RM_STRATEGY_PROGRAM_BASE) has exactly three kernels per scene: the
// render kernel for one frame and for a batch, and the per-ray kernel.
inline int default_tile_order(const RmFrameDesc& d, int nframes);
inline bool is_strategy_program(int strategy_id) { return strategy_id >= RM_STRATEGY_PROGRAM_BASE; }

// THE RULE FOR A STRATEGY PROGRAM: one plain render pass.  No parking levels and no single launch (there is no resume,
// team or pipeline kernel, and the interpreter's registers live in the rendering workgroup's LDS, not in the strategy
// record a queue entry would carry), whole evaluations (no interleaved form), 64x4 tiles, and the library's static tile
// order (the longest-first order keeps per-strategy costs, which must not outlive a program).  The descriptor's
// scheduling fields are ignored rather than refused, so one descriptor serves a compiled strategy and its twin.
inline void plan_strategy_program(const RmFrameDesc& d, LaunchPlan& p)
{
    p.tile_h = 4;
    p.tiles_y = (d.rows + 3) / 4;
    p.interleave = 0;
    p.mode = 1;
    p.park[0] = p.park[1] = 0;
    p.single = false;
    p.fused_reduce = (p.nframes == 1 && d.rows > 0) ? 1 : 0;
    p.refuse = nullptr;
    p.static_order = default_tile_order(d, p.nframes);
    p.tile_order = p.static_order;
    p.queue_entry_bytes = 0;
}

// Workgroups per compute unit of a persistent grid: 2 where the occupancy is unknown, three at most -- the cheap scenes
// fit four, and measured 10-16 % slower with four (Sphere 0.50 -> 0.45 ms, Cube 0.40 -> 0.34) while the long-ray
// scenes are indifferent.
inline int grid_per_cu(int reached) { return reached <= 0 ? 2 : std::min(reached, 3); }

// KEEP BUSY (rm_kernels.h): RmFrameDesc.keep_busy > 0 explicit, 0 the default burst, < 0 off.
inline int resolve_keep_busy(const RmFrameDesc& d) { return d.keep_busy > 0 ? d.keep_busy : (d.keep_busy == 0 ? 256 : 0); }

// Which launch structure a frame with long-ray suspension uses (RmFrameDesc.pipeline; 0 leaves it to the library).
// Measured on Mandelbulb, every strategy, 640x360 ... 5120x2880: the single launch is
// 4-27 % faster than one launch per pass (1080p Standard 11.0-12.4 -> 9.9 ms, Enhanced 9.7 -> 7.9, Hybrid 6.2 ->
// 5.0, 3840x2160 21.4 -> 15.7 ms); at 7680x4320 the frame is throughput-bound and wants every workgroup as a
// producer (52.5 ms without suspension, 59 with the pipeline).  Other scenes keep their measured pass schedules.
inline int pipeline_mode(const RmFrameDesc& d, long long rays, int max_iterations)
{
    if (d.scene_id >= RM_SCENE_PROGRAM_BASE) return 1;      // a scene program has no single-launch form
    if (d.pipeline != 0) return d.pipeline;
    return (d.scene_id == 10 && rays <= 24000000ll && max_iterations > 128) ? 2 : 1;
}

// Trip budgets of pass 1 / pass 2 (0 = that pass does not park).  RmFrameDesc.suspend_after: 0 = library
// default, < 0 = off, > 0 = explicit.
inline void suspend_levels(const RmFrameDesc& d, long long rays, int mode, int max_iterations, int* park)
{
    // Default: on for Mandelbulb launches of up to ~16 M rays -- those are bound by the latency of a few
    // hundred 512-trip rays (1080p: 15.2 -> 11.1 ms at 32 / 128 trips; 3840x2160: 22.8 -> 20.2 and
    // 5120x2880: 30.3 -> 28.4 ms at 48 / 192); larger launches are throughput-bound (7680x4320: 50 ms
    // without, 53-58 with), every other scene's SDF is too cheap for the extra passes to pay, and the
    // strategies whose rays end early or whose loop index restarts (Overstep-Bisect, Skipping-Spheres)
    // measured no faster or slower with it.
    const bool strat_ok = d.strategy_id != 6 && d.strategy_id != 7;
    const bool long_budget = rays <= 16000000ll && max_iterations > 128;
    const bool dflt = d.scene_id == 10 && strat_ok && long_budget;
    // Segment and RevAA evaluate the SDF twice per loop trip: half the trip budgets (Segment 19.7 -> 16.4 ms,
    // RevAA 22.2 -> 19.5 ms at 16 / 64)
    const int two = (d.strategy_id == 10 || d.strategy_id == 8) ? 2 : 1;
    const int d0 = (rays <= 3000000ll ? 32 : 48) / two, d1 = (rays <= 3000000ll ? 128 : 192) / two;
    park[0] = d.suspend_after[0] > 0 ? d.suspend_after[0] : (d.suspend_after[0] == 0 && dflt ? d0 : 0);
    park[1] = d.suspend_after[1] > 0 ? d.suspend_after[1] : (d.suspend_after[1] == 0 && dflt && d.suspend_after[0] == 0 ? d1 : 0);
    // Grazing Plane and Thin Planes Stack: a large share of the frame runs hundreds of trips (whole pixel rows
    // skim the planes; mean 40-68 trips).  Parking at 128 trips turns those rays into dense wavefronts of
    // their own instead of dragging them along with short rays -- lane compaction: 20-45 % faster for every strategy but
    // Skipping-Spheres (Grazing Plane / Segment 2.16 -> 1.22 ms, Thin Planes / Hybrid 2.23 -> 1.49).  No other
    // scene gains (17 scenes x 4 strategies measured).
    if ((d.scene_id == 1 || d.scene_id == 13) && d.strategy_id != 7 && d.suspend_after[0] == 0 && long_budget) park[0] = 128;
    // Sphere Cloud and Bumpy Sphere (unions of 24 / 31 spheres: a pow per sphere and evaluation).  The long rays are
    // parked at 16 trips and finished by TEAMS, each wave taking a third of the sphere list: 3.8 -> 3.0 ms and
    // 6.4 -> 5.0-5.2 ms (Curvature 6.7 -> 5.6, Segment 7.3 -> 5.7).  Not for Adaptive-Hybrid, whose rays end early
    // (2.33 vs 1.88 ms and 3.23 vs 3.10 without).
    if ((d.scene_id == 14 || d.scene_id == 15) && strat_ok && d.strategy_id != 9 && d.suspend_after[0] == 0 && long_budget)
        park[0] = 16 / two;
    // Gyroid (three sincos per evaluation, long skimming rays inside the ball) parked at 24 trips in round 1 (1.88 ->
    // 1.63 ms in natural tile order).  With the centre-out order its long rays start early anyway: parking measured
    // 1.63 vs 1.60 ms without (Adaptive-Hybrid 1.17 vs 1.05), so it no longer parks.
    // Single launch (Mandelbulb): rays are struck from their tile at 16 trips (the tile slot is free again) and handed
    // to the teams at 48; larger frames, and Segment whose trips evaluate twice, at 32 / 64.  Every strategy gains,
    // Overstep-Bisect and Skipping-Spheres included (3.56 -> 3.08 ms, 11.3 -> 10.2 ms).
    if (mode == 2 && d.scene_id == 10 && max_iterations > 128) {
        // (with the previous frame's tile costs the long rays start first: 24 / 56 with 7/16 of the grid as teams measured
        // 7.3-7.5 ms, 32 / 64 7.5-7.6, 16 / 48 8.5)
        const bool small = rays <= 3000000ll && d.strategy_id != 10 && d.tile_order_mode != 1;
        const bool ordered = rays <= 3000000ll && d.strategy_id != 10 && d.tile_order_mode == 1;
        // (a strike at 24 measured the same as 16 over the Mandelbulb's three curated viewpoints x Standard / Enhanced / Adaptive-Hybrid
        // -- sums 28.98 / 21.30 / 17.00 ms against 28.96 / 21.32 / 16.93, profiles/r03/viewpoint_budgets.jsonl)
        // (with the early hand-over of near-surface rays the strike is back at 16: those rays leave the producer as soon as they
        // are struck)
        if (d.suspend_after[0] == 0) park[0] = small ? 16 : (ordered ? 24 : 32);
        if (d.suspend_after[1] == 0 && d.suspend_after[0] == 0) park[1] = small ? 48 : (ordered ? 56 : 64);
    }
    if (park[0] == 0) park[1] = 0;
    if (park[1] > 0 && park[1] <= park[0]) park[1] = 0;
}

// The library's tile order (RmFrameDesc.tile_order_mode = 0).  A frame ends with its longest ray, and that ray starts
// when the order reaches its tile; the registry's cameras look at their object, so handing tiles out from the image
// centre outwards starts the object -- and its grazing / fractal rays -- first.  Measured at 1920x1080, Standard
// (natural -> centre-out): Sphere 0.46 -> 0.40 ms, Cube 0.239 -> 0.219, Menger 0.87 -> 0.74, Near Miss 0.66 -> 0.58,
// Cylinder 0.51 -> 0.39, Hollow Cube 0.35 -> 0.28, Box Lattice 0.52 -> 0.38, Metaballs 1.78 -> 1.47, Mandelbulb single
// launch 10.5 -> 9.7 (16 of 20 scenes gain, 3-27 %); worse where the long rays are NOT in the middle -- planes and
// pillars to the horizon: Grazing Plane 0.58 -> 0.70, Thin Planes Stack 0.92 -> 1.05, Pillar Forest 1.95 -> 2.10 --
// which keep the natural order (Bad Lipschitz Sphere: no difference) -- except that Pillar Forest, whose long rays lie along
// the horizon line in the middle rows, takes the middle-rows-first order (4): Standard 1.76 -> 1.72, Segment 2.24 -> 2.00
// (Grazing Plane 0.58 -> 0.63 and Thin Planes Stack 0.90 -> 0.91 do not gain: their horizon is not the middle row / the
// natural order already reaches it in time).  The permutation is cached per frame shape.  Batches keep the natural
// order (their tiles run frame-major).
inline int default_tile_order(const RmFrameDesc& d, int nframes)
{
    if (nframes > 1) return d.scene_id == 10 ? 2 : 3;     // Mandelbulb sweeps: centre-out within every frame
    // Round 3 held the choice against EVERY curated viewpoint of the reference (viewpoints.py:41-123; 53 cameras at
    // 1920x1080, Standard, profiles/r03/viewpoint_orders.jsonl): centre-out is within 5 % of the best static order for all
    // viewpoints of 15 scenes; the plane scenes want the natural order from every camera (centre-out +15...26 %); Pillar
    // Forest, Thin Torus (ring seen edge-on: -13 %, -8 %, -4 %) and Near Miss (the gap between the spheres: -13 %, -10 %,
    // -4 %) the middle rows first.  Intermediate ellipses (horizontal weight 1/4, 1/2) were measured too: never the best.
    // No single static order is within 5 % everywhere (centre-out: 17 of 53 cameras behind, natural 35, middle rows 29).
    switch (d.scene_id) {
        case 1: case 13: return 3;
        case 3: case 5: case 12: return 4;
        default: return 2;
    }
}

// How the single launch of plan `p` is performed (RmFrameDesc.pipeline_form): 1 = the fused pipeline_kernel, 2 = producers
// and teams as two kernels side by side, 3 = the two kernels one after the other on the caller's stream (tests).
// The split form covers the default schedule -- detach mode, every team resident from the start -- where a producer never
// waits for a team; any other knob set keeps the fused kernel.  Library's choice (0): RM_SPLIT_BY_DEFAULT, and only where
// each of the two kernels reaches at least the workgroups per compute unit the plan's grid counts on (`fused`: what the
// fused kernel reaches, which sized that grid), so that together they occupy no more than the fused grid does.
// Measured (parent, fused default and split default alternating three times on one MI355X, DESIGN.md section 3 "Split single
// launch"): bench.py 270.5-272.5 Mrays/s with the fused kernel, 278.0-278.7 split.
#ifndef RM_SPLIT_BY_DEFAULT
#define RM_SPLIT_BY_DEFAULT 1      // (-DRM_SPLIT_BY_DEFAULT=0: the other default, for a same-box A/B of two libraries)
#endif
inline int single_launch_form(const RmFrameDesc& d, const DeviceFacts& dev, LaunchPlan& p, int fused)
{
    if (d.pipeline_form == 1) return 1;
    const bool covered = dev.has_split && p.team_wgs > 0 && p.suspend_after2 > 0 && p.q0_detach != 0 && p.early_exit_wgs == 0 &&
                         p.late_team_first == p.pipeline_grid;
    if (d.pipeline_form >= 2) {
        if (!covered && !p.refuse)
            p.refuse = d.pipeline_form == 2
                ? "pipeline_form 2: the split form exists for single launches with teams in detach mode without late teams"
                : "pipeline_form 3: the split form exists for single launches with teams in detach mode without late teams";
        return covered ? d.pipeline_form : 1;
    }
    if (!RM_SPLIT_BY_DEFAULT || !covered || p.batch) return 1;
    // Skipping-Spheres and Adaptive-Hybrid keep the fused kernel: same alternation at 1920x1080, fused / split 8.91 / 8.99-9.00 ms
    // and 4.61 / 4.68-4.76 (few of their rays reach the teams; the other nine of the registry gain or stay within the spread)
    if (d.strategy_id == 7 || d.strategy_id == 9) return 1;
    if (fused <= 0) return 1;      // occupancy unknown
    const int per_cu = grid_per_cu(fused);
    return dev.per_cu(OccKernel::split_producers, p.tile_h, p.interleave, 0) >= per_cu &&
           dev.per_cu(OccKernel::split_teams, p.tile_h, p.interleave, 0) >= per_cu ? 2 : 1;
}

// The single launch (rm_pipeline.h): producers + queue-0 consumers + teams side by side.  Fills the single-launch fields.
inline void plan_single_launch(const RmFrameDesc& d, const DeviceFacts& dev, LaunchPlan& p)
{
    const bool teams = dev.has_teams && p.park[1] > 0 && d.resume_mode != 1;
    const int fused = dev.per_cu(OccKernel::pipeline, p.tile_h, p.interleave, p.batch ? 1 : 0);
    const int per_cu = grid_per_cu(fused);
    const long long resident = (long long)dev.cus * per_cu;
    const long long ntiles = (long long)p.tiles_x * p.tiles_y * p.nframes;
    const long long rays = p.rays;
    // producers and teams wait for one another (bounded), so the grid never exceeds what is resident at once
    long long team_wgs = 0;
    if (teams) {
        // Share of the resident workgroups that run as teams (512 resident at 2 per CU).  Measured after the guarded
        // square root made a team's trip shorter (Mandelbulb / Standard, ms per frame by team workgroups):
        //   960x540     128: 8.9   192: 8.4   224: 8.1            1280x720   128: 8.4   192: 8.0   224: 8.1
        //   1920x1080   128: 9.8   160: 9.4   192: 9.4   224: 10.1  (previous frame's costs: 128: 8.5  192: 7.7  240: 7.3-7.5)
        //   2560x1440    64: 11.7   96: 10.8  128: 11.3  192: 11.3   3840x2160  64: 19.2   96: 15.1  128: 15.2  192: 17.9
        //   5120x2880    64: 27.6   96: 24.4  128: 26.2  192: 31.0
        // Small frames are all tail (the chains of the long rays): more teams; large frames are fresh-pixel
        // throughput with a short tail: more producers.
        long long share16 = rays <= 1000000ll ? 7 : (rays <= 3000000ll ? 6 : 3);      // sixteenths of the grid
        // (with keep_busy, over the three curated viewpoints: 1280x720 wants 128-160 teams, not 224 -- Enhanced 17.6 -> 15.6 ms in
        // the sum at 128, Relaxed / Auto-Relaxed / Slope / Curvature 2-5 % at 160, Standard flat; 960x540 and 1920x1080 stay)
        if (rays > 600000ll && rays <= 1000000ll) share16 = d.strategy_id == 4 ? 4 : 5;
        if (d.tile_order_mode == 1 && rays <= 3000000ll) share16 = 7;                      // (15/32 measured 2 % better still)
        if (p.nframes > 1 && rays > 3000000ll) share16 = 4;        // sweeps: 64 x 384^2 viewpoints 29.0 ms (96: 31, 192: 34.6)
        // Strategies whose rays end early hand few rays to the teams: Overstep-Bisect 2.95 / 3.03 / 3.32 ms and
        // Adaptive-Hybrid 4.67 / 4.69 / 4.71 at 96 / 128 / 192 teams (with the previous frame's costs 2.81 vs 3.46
        // and 3.79 vs 4.81 at 128 vs 224; Skipping-Spheres 6.6 vs 6.8).  The other eight gain from the larger share
        // like Standard (Enhanced 7.26 -> 7.1, RevAA 15.1 -> 14.2; ordered: Enhanced 6.3 -> 5.6, RevAA 12.1 -> 10.4).
        if (d.strategy_id == 6 || d.strategy_id == 9) share16 = d.tile_order_mode == 1 ? 4 : 3;
        if (d.strategy_id == 7 && d.tile_order_mode == 1) share16 = 4;
        team_wgs = d.team_grid > 0 ? d.team_grid : std::max<long long>(1, resident * share16 / 16);
        team_wgs = std::min<long long>(team_wgs, std::max<long long>(1, resident / 2));
    }
    // Late teams (rm_pipeline.h): a share of the team workgroups is put behind the resident grid -- their places are held
    // by producers until queue 1 fills.
    long long late = 0;
    const bool detach_mode = d.queue_first == 3 || (d.queue_first == 0 && teams);
    if (teams && detach_mode && d.grid_waves == 0) {
        // measured at 1080p (Mandelbulb / Standard, trace of round 3): with 64 resident + 128 late teams the tile counter
        // runs out at 3.8 instead of 4.6 ms and the last long ray enters queue 1 a millisecond earlier (2.5 vs 3.5 ms),
        // but a producer workgroup only leaves when it would open its next tile (every 1-2 ms per wave in the object's
        // tiles), the late teams arrive at 1.8-2.5 ms and the rays pushed meanwhile wait ~1.3 ms: 9.6 vs 9.8 ms.  Off by
        // default; the demand for teams jumps from 0 to ~140 workgroups within 0.5 ms.
        if (d.late_teams > 0) late = d.late_teams;
    }
    const long long want_pw = d.grid_waves > 0 ? d.grid_waves : resident * kPipeWaves;   // producer waves asked for
    long long pure = (std::min<long long>(want_pw, ntiles) + kPipeWaves - 1) / kPipeWaves;
    pure = std::max<long long>(1, std::min<long long>(pure, resident - team_wgs));
    late = std::min<long long>(late, std::max<long long>(0, pure - 1));      // one producer workgroup at least stays to the end
    // grid = static teams + producers + late teams
    p.team_wgs = (int)team_wgs;
    p.producer_waves = (int)(pure * kPipeWaves);
    p.late_team_first = (int)(team_wgs + pure);
    p.early_exit_wgs = (int)late;
    p.pipeline_grid = (int)(pure + late + team_wgs);
    p.exit_backlog = d.exit_backlog > 0 ? d.exit_backlog : 64;
    // KEEP BUSY (rm_kernels.h): finished producer workgroups stay until the teams are through -- 1080p Mandelbulb / Standard
    // 9.4 -> 8.1 ms, Enhanced 7.0 -> 6.2 (burst 16 ... 2048 alike; fp64, fp32 and integer filler alike; s_sleep in the same
    // place: nothing).  Not with late teams, which need the producers' places.
    p.keep_busy = (teams && late == 0) ? resolve_keep_busy(d) : 0;
    // EARLY HAND-OVER (rm_pipeline.h): struck near-surface rays go to the teams at once.  Over the Mandelbulb's three curated
    // viewpoints at 1080p with the strike at 16: Standard 8.19 / 13.19 / 7.84 -> 7.81 / 13.02 / 7.81 ms, Enhanced 6.33 / 9.18 / 6.30
    // -> 6.34 / 9.06 / 6.38 (sums -2.0 % / -0.1 %; strikes of 8 ... 24 alike, a regular hand-over later than 48 worse)
    // By strategy (default camera, on / off): Relaxed 7.90 / 8.36, Auto-Relaxed 7.92 / 8.19, Slope 6.67 / 7.10, Curvature 7.65 / 8.12,
    // Segment 10.6 / 11.9, Safe-Relaxed 7.75 / 8.08; RevAA and Dense-March alike; the three whose rays end early or whose loop
    // index restarts lose 1-2 % (Overstep-Bisect 3.09 / 3.03, Skipping-Spheres 8.77 / 8.66, Adaptive-Hybrid 4.74 / 4.69): off there.
    // early_trips: how many of the eight fractal iterations make an evaluation "near-surface".  Six, together with a regular
    // hand-over at 64 instead of 48 trips, measured Standard 7.75 / 11.81 / 7.96 ms against 7.85 / 12.88 / 7.77 from the three
    // curated cameras (Auto-Relaxed 7.83 / 11.99 / 7.54 against 8.01 / 12.61 / 7.71; the bench line 266-270 Mrays/s instead of
    // 261-264) -- but twice as many rays go through the queue: 88.9 MB of HBM traffic per frame instead of 58.2, for 1-2 % from
    // the default camera and a loss from the angled one.  The default stays 8 of 8; the knob is there.
    p.early_trips = d.early_trips > 0 ? d.early_trips : 8;
    const bool eh_default = d.strategy_id != 6 && d.strategy_id != 7 && d.strategy_id != 9;
    p.early_handover = (teams && detach_mode)
        ? (d.early_handover > 0 ? d.early_handover : (d.early_handover == 0 && eh_default ? std::max(1, p.park[0]) : 0)) : 0;
    p.suspend_after2 = teams ? p.park[1] : 0;
    // default: with teams, rays below suspend_after[1] never leave their lane (no queue-0 traffic); without
    // teams queue 0 is the lane-compaction queue, parked rays first
    p.q0_detach = detach_mode ? 1 : 0;
    p.q0_first = (d.queue_first == 0 || d.queue_first == 1) ? 1 : 0;
    p.q0_refill_min = d.queue_refill_min > 0 ? d.queue_refill_min : 16;
    p.q0_retry = d.queue_retry > 0 ? d.queue_retry : 16;
    p.team_retry = d.team_retry > 0 ? d.team_retry : 8;      // (with keep_busy: 2: 8.29, 4: 8.19, 8: 7.97, 16: 8.12, 32: 8.33 ms; other strategies flat)
    p.team_steal = (d.team_steal == 0 || d.team_steal == 1) ? 1 : 0;
    p.team_prio = 3;          // 0 / 1 / 3 measured alike (10.0-10.4 ms): what slows a ray next to producers is not the issue slot
    p.max_spins = 50000;      // ~50 ms of polling: only reached when part of the grid is not resident
    p.form = single_launch_form(d, dev, p, fused);
}

// One launch per pass: pass 1 (render) parks rays beyond park[0] trips, pass 2 restarts them all at once and parks those
// beyond park[1], pass 3 finishes the few that remain.
inline void plan_passes(const RmFrameDesc& d, const DeviceFacts& dev, LaunchPlan& p)
{
    p.resume_refill_min = 16;
    // one workgroup per compute unit: measured best for both the dense second pass and the sparse last one
    p.resume_grid = d.resume_grid > 0 ? d.resume_grid : std::min(p.render_grid, dev.cus);
    const bool team = dev.has_resume_team && d.resume_mode != 1;
    // KEEP BUSY (rm_kernels.h): a team pass is followed by as many filler workgroups, which start when its queue is handed out
    p.pass_keep_busy = team ? resolve_keep_busy(d) : 0;
    p.team_pass_grid = p.pass_keep_busy > 0 ? 2 * p.resume_grid : p.resume_grid;
    p.pass_team[0] = team && (p.park[1] == 0 || d.resume_mode == 3);
    p.pass_team[1] = team;
}

// The plan of a launch of descriptor `d`: one frame (batch_frames = 0), or a batch of `batch_frames` frames of d's shape,
// optionally with per-frame march configurations (`configs`, may be null).
inline LaunchPlan plan_launch(const RmFrameDesc& d, const DeviceFacts& dev, int batch_frames = 0, const RmMarchConfig* configs = nullptr)
{
    LaunchPlan p;
    p.batch = batch_frames > 0;
    p.nframes = p.batch ? batch_frames : 1;
    // the launch-wide scheduling policy looks at the largest budget of a batch
    int max_iterations = d.march.max_iterations;
    if (p.batch && configs) {
        p.march_frame = 0;
        for (int f = 1; f < p.nframes; ++f)
            if (configs[f].max_iterations > configs[p.march_frame].max_iterations) p.march_frame = f;
        max_iterations = configs[p.march_frame].max_iterations;
    }
    p.rays = (long long)d.rows * d.width * p.nframes;
    p.tile_h = d.tile_rows ? d.tile_rows : 4;
    p.tiles_x = (d.width + kTileW - 1) / kTileW;
    p.tiles_y = (d.rows + p.tile_h - 1) / p.tile_h;
    // refill batching: ray set-up (~250 instructions) is amortised over the idle lanes it serves.  8 idle lanes is the
    // default (Pillar Forest 1.93 -> 1.69 ms against the 24 used earlier); the scenes whose rays are short -- set-up is a
    // larger share of a ray -- measured better at 16 under the centre-out order (Cube 0.182 -> 0.174 ms, Cylinder
    // 0.366 -> 0.346, Hollow Cube 0.250 -> 0.244, Box Lattice 0.377 -> 0.370, Sphere 0.353 -> 0.345, Metaballs
    // 1.52 -> 1.49, Thin Torus 0.666 -> 0.655), the others not (Menger 0.675 -> 0.702, Pillar Forest 1.70 -> 1.74).
    int refill_default = 8;
    switch (d.scene_id) { case 0: case 2: case 3: case 4: case 6: case 18: case 19: refill_default = 16; break; default: break; }
    p.refill_min = (d.refill_min > 0 && d.refill_min <= 64) ? d.refill_min : refill_default;
    // one trip per turn pays where the trip count varies (Mandelbulb); the one-trip union scenes run whole evaluations
    p.interleave = d.eval_mode == 2 || (d.eval_mode == 0 && d.scene_id == 10);

    // launch structure and trip budgets: the single launch of a scene with teams uses one-row tiles
    p.mode = pipeline_mode(d, p.rays, max_iterations);
    suspend_levels(d, p.rays, p.mode, max_iterations, p.park);
    p.single = p.park[0] > 0 && p.mode == 2;
    // One-pass frames fold their statistics in the render kernel itself (frame_reduce_by_last_workgroup)
    p.fused_reduce = (p.park[0] == 0 && p.nframes == 1 && d.rows > 0) ? 1 : 0;
    if (d.tile_rows == 1 && !(p.single && dev.has_teams))
        p.refuse = "tile_rows = 1 exists for the single launch (pipeline = 2 with suspension) of scenes with a team form";
    if (p.single && dev.has_teams && (d.tile_rows == 1 || (d.tile_rows == 0 && d.tile_order_mode == 1))) {
        // 64x1 tiles: all 64 pixels of a tile start when the tile is opened.  With 64x4 tiles the last pixels of a
        // tile wait in its pixel pool for lanes that rays of 16-48 trips hold (~1 ms each).  Default only with the
        // previous frame's tile costs (tile_order_mode 1: the long rays' tiles are opened first, so their pixels
        // should not queue inside them -- 1080p 9.6 -> 8.5 ms); with a static order 64x4 tiles measured better
        // (9.9 against 10.9 ms: the tile order does not know where the long rays are).
        p.tile_h = 1;
        p.tiles_y = d.rows;
    }
    p.static_order = default_tile_order(d, p.nframes);
    p.tile_order = d.tile_order_mode != 0 ? d.tile_order_mode : p.static_order;
    if (p.park[0] > 0) p.queue_entry_bytes = dev.entry_bytes;
    if (is_strategy_program(d.strategy_id)) plan_strategy_program(d, p);

    if (p.single) {
        plan_single_launch(d, dev, p);
        return p;
    }
    // persistent grid of 4-wave workgroups; every wave pulls tiles on its own.  An explicit grid_waves is capped by one
    // frame's tiles, the occupancy grid by all tiles of the launch.
    const long long frame_tiles = (long long)p.tiles_x * p.tiles_y;
    long long wgs, cap;
    if (d.grid_waves > 0) {
        wgs = (d.grid_waves + kWavesPerWG - 1) / kWavesPerWG;
        cap = (frame_tiles + kWavesPerWG - 1) / kWavesPerWG;
    } else {
        wgs = (long long)dev.cus * grid_per_cu(dev.per_cu(OccKernel::render, p.tile_h, p.interleave, p.batch ? 1 : 0));
        cap = (frame_tiles * p.nframes + kWavesPerWG - 1) / kWavesPerWG;
    }
    p.render_grid = (int)std::max<long long>(1, std::min<long long>(wgs, cap));
    if (p.park[0] > 0) plan_passes(d, dev, p);
    return p;
}

// ---- the smaller rules of a frame's host side ---------------------------------------------------------------------------------

// Who wrote a parked-ray queue last.  A single-launch consumer takes an entry for published when the word at the
// entry's `ready` offset equals the launch's generation tag; a frame with another entry stride (another strategy), or
// one that follows a multi-pass frame (entries without tags), would put those offsets on stale payload words -- old
// output indices, counts, halves of doubles -- that can equal a small tag.  The span a different writer may have
// touched is therefore cleared before a single launch uses the queue.
struct QueueKey {
    int stride = 0;
    int writer = 0;       // 1 = pass per launch, 2 = single launch, 3 = unknown (rm_debug_poison_queues)
    size_t used = 0;      // bytes from the buffer's start that a writer may have touched since the last clear
};
struct QueueStep { size_t clear; QueueKey key; };     // bytes to zero from the buffer's start before the launch; the key to remember

// The queue's step for a launch of `writer` with entries of `stride` bytes that needs `need` bytes of a buffer which
// held cap_before bytes and, grown where that was too little, holds cap_after.
inline QueueStep queue_step(QueueKey prev, int writer, int stride, size_t need, size_t cap_before, size_t cap_after)
{
    size_t clear = 0;
    if (need > cap_before) {
        // fresh memory: no word of it may look like a published entry of a later launch (QEntry.ready)
        clear = need;
        prev.used = 0;
    } else if (writer == 2 && prev.used > 0 && (prev.writer != 2 || prev.stride != stride)) {
        // another layout wrote here: stale payload words now sit at this launch's `ready` offsets
        clear = std::min(prev.used, cap_after);
        prev.used = 0;
    }
    return { clear, { stride, writer, std::max(prev.used, need) } };
}

// rm_march_rays_team: the teams of a few rays are all that runs, so filler workgroups (two per compute unit in all) keep
// the chip at the speed a frame's teams run at (KEEP BUSY, rm_kernels.h).
inline int team_fillers(int cus, long long nteams) { return (int)std::max<long long>(0, 2ll * cus - nteams); }

// The frame shape whose per-tile costs the longest-first order (tile_order 1) may reuse ...
inline void frame_key(const RmFrameDesc& d, int tile_h, long long* k /* 10 words */)
{
    k[0] = d.scene_id; k[1] = d.strategy_id; k[2] = d.width; k[3] = d.height; k[4] = d.row0; k[5] = d.rows;
    k[6] = d.band_rows; k[7] = d.band_stride; k[8] = d.band_offset; k[9] = tile_h;
}

// ... and the one whose static permutation (tile_order 2 and 4) is kept: pure geometry, the same for every scene and strategy.
inline void static_order_key(const RmFrameDesc& d, int tile_h, int nframes, int order, long long* k /* 12 words */)
{
    frame_key(d, tile_h, k);
    k[0] = k[1] = 0;
    k[10] = nframes; k[11] = order;
}

}  // namespace rm
