/*
 * rm_hip.h -- C ABI of librm_hip.so, the MI355X (gfx950) sphere-tracing engine.
 *
 * Drop-in boundary for ONE path of kylegrover/raymarch-algo-compare: the per-ray
 * SDF sphere-tracing frame render.  Each entry point names the reference
 * interface it replaces (paths relative to raymarching_benchmark/).  Plain
 * pointers and sizes only; no C++ or torch types cross this boundary.  Nothing
 * here falls back to a CPU implementation: every call fails with RM_E_NO_DEVICE /
 * RM_E_HIP when no gfx950 device is usable.
 *
 * Ids: scene_id = index in get_all_scenes() (scenes/catalog.py:640-663), 0..19, or the id of a scene program
 *      (rm_scene_program_create: RM_SCENE_PROGRAM_BASE and up);
 *      strategy_id = index in the STRATEGIES dict (strategies/__init__.py:16-28), 0..10.
 * Threading: every entry point may be called from any host thread; calls are serialised by one lock inside the
 * library (one in-flight CALL per device), calls are synchronous unless stated, and frames enqueued on different streams
 * are ordered on the device by an event (they share one workspace).  A `stream` argument must be a hipStream_t of the
 * HIP runtime this library is bound to (rm_runtime_info).  A process can hold two copies of libamdhip64 -- this library
 * loaded before PyTorch, whose wheel bundles its own -- and HIP dereferences whatever handle it is given, so a stream of
 * the other copy corrupts the runtime (round 2's SIGABRT).  While two copies are mapped, only streams made by
 * rm_stream_create are accepted (anything else: RM_E_BAD_ARG, the handle is not touched); with one copy mapped every
 * hipStream_t of the process is that runtime's and is accepted (e.g. a torch stream when torch was imported first).
 * Hosts without a HIP binding of their own take streams from rm_stream_create; rm_shutdown destroys those that are left.
 * One stream of the library's own per session: a single-launch frame in its split form (RmFrameDesc.pipeline_form) runs
 * its team kernel on an internal stream next to the producer kernel on the caller's.  The internal stream starts after
 * what the caller's stream held when the frame was enqueued and the caller's stream continues after it, so events the
 * caller records around a frame cover both kernels and nothing else of the caller's is reordered.  It is created by the
 * first such frame and destroyed by rm_shutdown.
 * Scene programs: the registry of programs has a lock of its own; create / destroy may be called from any thread.
 * Destroying a program while a frame that renders it is still in flight on a stream is the caller's error (the
 * frame reads the program's device copy until it ends): synchronise the stream first.
 */
#ifndef RM_HIP_H
#define RM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_OK 0
#define RM_E_BAD_SCENE (-1)
#define RM_E_BAD_STRATEGY (-2)
#define RM_E_BAD_DIMS (-3)
#define RM_E_NO_DEVICE (-4)
#define RM_E_HIP (-5)
#define RM_E_BAD_ARG (-6)
#define RM_E_RCCL (-7)     /* librccl could not be loaded, or one of its calls failed (text in rm_last_error) */

#define RM_NUM_SCENES 20
#define RM_NUM_STRATEGIES 11
/* Strategy ids [0, RM_NUM_STRATEGIES) are the reference's CPU registry (strategies/__init__.py:16-28).  Two more exist
 * only in its fragment shader (gpu/shaders/strategies.glsl:508-541 safe_relaxed = 11, :559-593 dense_march = 12; shader
 * ids 8 and 9): here they run the shader's control flow on the CPU path's arithmetic (binary64, this camera).  PARITY
 * UNPINNED: no Python statement of them exists and the shader computes in fp32, so nothing of the reference can check
 * them; they are not part of the registry (rm_num_strategies() stays 11, names / CLI "all" unchanged). */
#define RM_NUM_STRATEGY_KERNELS 13
#define RM_HIST_BINS 544 /* iterations histogram bins; counts >= RM_HIST_BINS-1 share the last bin */
#define RM_MAX_TIMED 256

/* The constructor arguments of the reference's strategy classes -- what `STRATEGIES[key](**kwargs)` takes and
 * what its accelerator seam threads through as per-run uniform overrides (gpu/runner.py:108-124, swept by
 * param_grid.py:20-27 / sweep.py:181,222-223) -- plus four constants the CPU march() bodies hold as literals.
 * Defaults (rm_default_strategy_params) are the reference's; with them every result is bit-identical to the
 * registry's no-argument instances.  A strategy reads only its own fields. */
typedef struct RmStrategyParams {
    double omega;                     /* 1.2   RelaxedSphereTracing(omega)                 strategies/relaxed_sphere.py:17 */
    double ar_omega_min;              /* 1.0   AutoRelaxedSphereTracing(omega_min,          strategies/auto_relaxed.py:21-23 */
    double ar_omega_max;              /* 2.0     omega_max, */
    double ar_smoothing;              /* 0.7     smoothing, */
    double ar_growth_rate;            /* 1.05    growth_rate, */
    double ar_decay_rate;             /* 0.7     decay_rate) */
    double beta;                      /* 0.3   SlopeAutoRelaxed(beta)                      strategies/slope_auto_relaxed.py:25 */
    double overstep_min_step;         /* 0.01  OverstepBisectTracing(min_step_factor,       strategies/overstep_bisect.py:18 */
    double hybrid_stuck_step_ratio;   /* 0.001 AdaptiveHybridTracing(stuck_step_ratio,      strategies/adaptive_hybrid.py:17-19 */
    double hybrid_min_step;           /* 0.005   min_step_factor, */
    double margin;                    /* 0.05  SkippingSpheresTracing: the literal `margin` of march() (skipping_spheres.py:30),
                                               uniform `margin` of the GLSL seam (gpu/runner.py:115) */
    double ar_omega_init;             /* 1.2   AutoRelaxedSphereTracing: the literal start value `omega = 1.2` of march() (auto_relaxed.py:41);
                                               the GLSL seam's `omega` uniform drives its auto-relaxed marcher too (param_grid.py:23) */
    int32_t overstep_bisection_steps; /* 16      bisection_steps)                           strategies/overstep_bisect.py:18 */
    int32_t hybrid_stuck_threshold;   /* 5       stuck_threshold)                           strategies/adaptive_hybrid.py:17 */
    int32_t segment_bisection_steps;  /* 8     SegmentTracing: the literal `range(8)` of march()      segment_tracing.py:79 */
    int32_t revaa_bisection_steps;    /* 8     RevAAApproxTracing: the literal `range(8)` of march()  rev_affine.py:70 */
    /* shader-only uniforms (the CPU strategies have no such constant; defaults change no bit of the registry's results) */
    double step_scale;                /* 1.0   `stepScale`: standard() multiplies every step by it (strategies.glsl:24,47 -- the
                                               understep oracle of gpu/groundtruth.py:59-61 uses 0.6), dense_march() too (:570) */
    double dense_min_step;            /* 1e-4  `minStep` as dense_march reads it (strategies.glsl:570; the seam's default is
                                               max(hit_threshold, min_step_fraction * max_distance), gpu/runner.py:117-118) */
} RmStrategyParams;

/* MarchConfig (config.py:19-29) -- the three fields the CPU strategies read -- plus
 * SegmentTracing.lipschitz as wired by run_once (main.py:58-61) and the strategy's constructor arguments.
 * full != 0 also produces MarchResult.final_sdf (costs the reference's tail evaluations).
 * use_params == 0: `params` is ignored and every strategy constant has the reference's default (a zeroed
 * record is therefore a valid default configuration); != 0: `params` is read (fill it with
 * rm_default_strategy_params first and override what the run sweeps). */
typedef struct RmMarchConfig {
    int32_t max_iterations; /* 512   */
    int32_t full;
    double hit_threshold;   /* 1e-4  */
    double max_distance;    /* 100.0 */
    double lipschitz;       /* 1.0   */
    int32_t use_params;
    int32_t reserved;       /* 0 */
    RmStrategyParams params;
} RmMarchConfig;

/* One frame (or a row shard of it).  cam[14] = position, forward, right, up,
 * half_width, half_height exactly as Camera.__init__ computes them (core/camera.py:11-33);
 * rows [row0, row0+rows) of a width x height image are rendered, row 0 = top
 * (core/types.py:90).  Output arrays hold rows*width elements, row-major from row0. */
typedef struct RmFrameDesc {
    int32_t scene_id;
    int32_t strategy_id;
    int32_t width, height;
    int32_t row0, rows;
    double cam[14];
    RmMarchConfig march;
    int32_t tile_rows;   /* 0 = default; rows per 64-pixel-wide wave tile: 4, or 1 for the single launch (pipeline = 2 with
                          * suspension) of scenes with a team form -- default there when tile_order_mode = 1 */
    int32_t refill_min;  /* 0 = default; idle lanes required before a wave refills */
    int32_t grid_waves;  /* 0 = default (fill the device); persistent wavefront count */
    /* Band-cyclic row sharding (multi-GPU load balance): local row y of this slice is image row
     *   row0 + ((y / band_rows) * band_stride + band_offset) * band_rows + y % band_rows.
     * band_rows = 0 (or band_stride <= 1) means contiguous rows.  band_rows must be a multiple of
     * the tile height; `rows` counts LOCAL rows and the mapped rows must stay below `height`. */
    int32_t band_rows;
    int32_t band_stride;
    int32_t band_offset;
    /* Tile scheduling order (results are identical in every mode; only the schedule changes -- a frame ends with its
     * longest ray, and that ray starts when the order reaches its tile).
     *   0  the library's choice: centre-out for one-frame launches of every scene but the three whose geometry runs to
     *      the horizon (Grazing Plane, Thin Planes Stack: natural; Pillar Forest: 4), natural for batches of cheap scenes
     *   1  longest-first using the per-tile cost (max iterations) the previous render of the SAME frame shape left in the
     *      library workspace -- rays that ran long last frame start first; the order of mode 0 when no matching previous frame exists
     *   2  centre-out: a static permutation of the frame shape, cached until the shape changes (the registry's cameras
     *      look at their object, so the object's grazing / fractal rays start first)
     *   3  natural (row-major tiles)
     *   4  middle rows first (centre-out with the horizontal distance weighted 1/16): for geometry that runs to the
     *      horizon, whose long rays lie along the horizon line (the library's choice for Pillar Forest) */
    int32_t tile_order_mode;
    /* Scenes whose SDF is a data-dependent loop (Mandelbulb, catalog.py:266-293).  0 = default
     * (library's choice, currently 2); 1 = a whole SDF evaluation per wave turn; 2 = one trip of the
     * SDF loop per wave turn, lanes advance to their next evaluation independently.  Results are
     * identical in either mode; ignored for every other scene. */
    int32_t eval_mode;
    /* Long-ray suspension.  A frame cannot finish before its longest ray, and that ray only starts
     * when the tile order reaches its pixel.  Pass 1 parks every ray still marching after
     * suspend_after[0] trips of its strategy loop and goes on with fresh pixels; pass 2 restarts all
     * parked rays at once (dense wavefronts of long rays) and parks those beyond suspend_after[1]
     * trips for a last sparse pass.  A parked ray continues from its saved strategy state, so results
     * are identical with or without suspension.  Per entry: 0 = library default, < 0 = off. */
    int32_t suspend_after[2];
    int32_t resume_grid;   /* 0 = default (one per compute unit); workgroups of the resume passes */
    /* How parked rays are finished.  0 = default (2 where the scene has a team form), 1 = one wavefront per
     * 64 rays, 2 = wavefront TEAMS for the last pass: three waves carry the same 64 rays and each evaluates
     * one of the three independent transcendental chains of a Mandelbulb trip (rm_march_rays_team), 3 = teams
     * for both resume passes (measured slower than 2; kept for experiments). */
    int32_t resume_mode;
    /* How the passes of a frame with long-ray suspension are launched.  0 = default (library's choice), 1 = one
     * launch per pass (first pass, resume, last resume), 2 = ONE launch: producer workgroups render fresh tiles,
     * take parked rays out of queue 0 as lanes fall idle and park them again at suspend_after[1] trips in queue 1,
     * which `team_grid` workgroups of wavefront teams consume while the producers are still rendering -- a long ray
     * moves to the next form the moment it crosses a threshold instead of waiting for a kernel boundary.  Identical
     * results in every mode.  The remaining fields tune the single launch (0 = library default):
     *   team_grid        workgroups that run as teams (scenes with a team form; the rest are producers)
     *   queue_first      1 = idle producer lanes take parked rays before fresh pixels, 2 = fresh pixels first,
     *                    3 = queue 0 is not used: at suspend_after[0] trips a ray is struck from its tile (the tile is
     *                    flushed without it) and marches on in its lane until suspend_after[1] (default with teams)
     *   team_steal       1 = teams take queue 0 entries while queue 1 is empty, 2 = never
     *   queue_refill_min idle lanes a producer wave needs before it looks at queue 0
     *   queue_retry      turns between two looks of a producer wave whose lanes stay idle
     *   team_retry       evaluations between two looks of a team that still carries rays
     *   age_priority     accepted and ignored by this build (an experiment: waves raising their issue priority with the
     *                    trip count of their oldest ray measured no gain on any scene and cost the cheap scenes 6-8 %;
     *                    the note above KernelArgs in csrc/rm_kernels.h records it) */
    int32_t pipeline;
    int32_t team_grid;
    int32_t queue_first;
    int32_t team_steal;
    int32_t queue_refill_min;
    int32_t queue_retry;
    int32_t team_retry;
    int32_t age_priority;
    /* Single launch, roles that change while the frame runs (scenes with a team form, queue_first = 0 / 3).  A frame's
     * first milliseconds want every workgroup as a producer -- the last of its long rays is found when the tile order
     * reaches it -- and its tail wants teams.  `late_teams` further team workgroups are put BEHIND the grid that is
     * resident at once: the dispatcher starts one whenever a producer workgroup has left, and up to `late_teams` producer
     * workgroups leave early (stop taking tiles, hand their rays to queue 1) when queue 1 holds `exit_backlog` (default
     * 64) rays more than the teams have taken.  0 = none (measured: no gain at the default sizes, csrc/rm_capi.hip).
     * Results are identical for every setting. */
    int32_t late_teams;
    int32_t exit_backlog;
    /* KEEP BUSY.  The same march loop runs at two speeds on this chip: the full one while most compute units execute
     * vector instructions, and 15-60 % slower when few wavefronts are live (tools/ubench/
     * sparse_share.hip) -- which is exactly the state of a frame whose last long rays are finished by a few team
     * wavefronts.  With keep_busy the workgroups that have run out of work do not leave: they execute `keep_busy`
     * fp32 multiply-adds per lane between two looks at a counter until the teams are through (bounded: 30 ms), and
     * the chains of the long rays run at the full speed (Mandelbulb 1920x1080: 9.4 -> 8.1 ms).  0 = library default
     * (256 in launches that end with teams, off elsewhere: where other workgroups still render tiles the filler only
     * takes their issue slots), < 0 = off, > 0 = explicit burst length.  Results are identical for every setting. */
    int32_t keep_busy;
    /* EARLY HAND-OVER (single launch, scenes with a team form and a per-evaluation cost measure: the Mandelbulb).  A ray that
     * has been struck from its tile and whose last evaluation ran every iteration of the fractal loop -- a near-surface ray,
     * eight producer turns per evaluation -- is handed to the teams at once instead of at suspend_after[1] trips.
     * 0 = library default (on from the strike budget; off for Overstep-Bisect, Skipping-Spheres and Adaptive-Hybrid, which
     * measured 1-2 % slower with it), < 0 = off, > 0 = the earliest trip.  `early_trips`: the iterations an evaluation must
     * have run to count as near-surface (0 = library default: 8 of 8; 1 ... 8 explicit -- 6 with suspend_after = {16, 64} is
     * 1-8 % faster from two of the Mandelbulb's three curated cameras and writes half as much again to HBM).  Results are identical. */
    int32_t early_handover;
    int32_t early_trips;
    /* How the single launch (pipeline = 2) is performed.  0 = library's choice, 1 = fused: one kernel whose workgroups are
     * producers or teams, 2 = split: the producers and the teams are two kernels that run side by side, the producers on the
     * caller's stream and the teams on a stream of the library's own (each kernel gets a register allocation of its own;
     * the caller's stream continues when both have ended), 3 = the two kernels one after the other on the caller's stream
     * (for tests: what a device that does not run them side by side makes of form 2).  Forms 2 and 3 exist for the default
     * schedule -- scenes with a team form, queue_first = 0 / 3, no late teams -- and are refused elsewhere (RM_E_BAD_ARG);
     * ignored by frames that are not single launches.  Results are identical in every form. */
    int32_t pipeline_form;
} RmFrameDesc;

/* Frame reduce computed in-kernel (the integer part of RayMarchStats.compute, core/types.py:77-137). */
typedef struct RmStats {
    uint64_t total_rays;
    uint64_t hit_count;
    uint64_t sum_iters; /* sample_count */
    int32_t iter_max;
    int32_t iter_min;
    uint64_t iter_hist[RM_HIST_BINS];
    uint64_t sum_evals; /* SDF evaluations of all rays (see RmOutputs.evals; in batches only when the evals map is requested) */
} RmStats;

/* in: warmup, repeats (<= RM_MAX_TIMED).  out: per-launch kernel milliseconds measured with
 * hipEvents on the launch stream (cf. gpu/runner.py:139-165, main.py:152-153). */
typedef struct RmTiming {
    int32_t warmup;
    int32_t repeats;
    float ms_median, ms_mean, ms_min, ms_max;
    float ms_each[RM_MAX_TIMED];
} RmTiming;

typedef struct RmDeviceInfo {
    char name[128];
    char arch[64];
    int32_t device_id;
    int32_t compute_units;
    int32_t clock_mhz;
    int32_t wavefront_size;
    uint64_t total_mem_bytes;
} RmDeviceInfo;

/* Select the device and create the library's stream + workspace.  Must be called
 * before anything else; idempotent for the same device. */
int rm_init(int device_id);
void rm_shutdown(void);
/* Thread-local text of the last error on this thread (never NULL). */
const char* rm_last_error(void);
int rm_device_info(RmDeviceInfo* out);
int rm_num_scenes(void);
int rm_num_strategies(void);
/* The reference's defaults (the values its registry's no-argument constructors use); never fails. */
void rm_default_strategy_params(RmStrategyParams* out);

/* SDFScene.sdf (scenes/base.py:29-32) over n points; host pointers, xyz is n x 3. */
int rm_sdf_eval(int scene_id, const double* xyz, size_t n, double* out);

/* MarchStrategy.march (strategies/base.py:25-38) over n explicit rays; host pointers.
 * Directions are normalised as Ray.__init__ does (core/ray.py:11-13). */
int rm_march_rays(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins,
                  const double* dirs, size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf);

/* ---- Scene programs: user-defined CSG scenes, evaluated by an interpreter on the device ---------------------------
 * A program is a postfix list of the reference's scenes/primitives.py functions.  Primitives push a distance computed at
 * the current point; combinators pop two distances (d1 pushed first, d2 second) and push one; distance modifiers replace
 * the top distance; point transforms save the current point and replace it by the transformed point, which the ops up to
 * the matching RM_SOP_POP_POINT read; RM_SOP_POP_POINT restores the saved point.  Evaluation starts at the query point;
 * exactly one distance must be left at the end, and every transform must be matched.  Constants go in f[], in the
 * order of the reference's arguments; a constant the reference computes with a transcendental function is passed
 * already computed (the device evaluates trigonometry for RM_SOP_GYROID only).  `arg` is reserved (0), unused f[] entries too.
 *   op                          f[]                                              primitives.py
 *   RM_SOP_SPHERE               radius                                           :11-12
 *   RM_SOP_BOX                  half_extents x, y, z                             :14-18
 *   RM_SOP_PLANE                normal x, y, z, offset                           :20-21
 *   RM_SOP_CYLINDER             radius, half_height                              :23-28
 *   RM_SOP_TORUS                major_radius, minor_radius                       :30-32
 *   RM_SOP_CAPSULE              a x, y, z, b x, y, z, radius                     :34-39
 *   RM_SOP_CAPPED_TORUS         sc[0] = sin(half angle), sc[1] = cos(half angle), ra, rb     :41-50
 *   RM_SOP_CONE                 cos(angle_rad), sin(angle_rad), height           :53-65
 *   RM_SOP_UNION / SUBTRACT / INTERSECT                 (none)                   :70-77
 *   RM_SOP_SMOOTH_UNION / SMOOTH_SUBTRACT / SMOOTH_INTERSECT   k (non-zero)      :80-92
 *   RM_SOP_TRANSLATE            offset x, y, z                                   :99-100
 *   RM_SOP_REPEAT               spacing x, y, z (an axis with spacing <= 0 is untouched)       :102-108
 *   RM_SOP_POP_POINT            (none)
 *   RM_SOP_ROUND                radius                                           :110-111
 *   RM_SOP_ONION                thickness                                        :113-114
 * Four ops that primitives.py does not have (the catalogue's Bad Lipschitz Sphere, Box Lattice, Menger and Gyroid are
 * written with them; scenes/catalog.py lines on the right).  `py_mod` is Python's float `%`, min / max / abs Python's:
 *   RM_SOP_SCALE                factor (finite, > 0): modifier, d * factor                            :320-321
 *   RM_SOP_LIMITED_REPEAT       spacing x, y, z, limit x, y, z (each limit finite, >= 0): point transform closed by
 *                               RM_SOP_POP_POINT; per axis with spacing c > 0
 *                               x - c * max(-l, min(l, floor(x / c + 0.5))), an axis with spacing <= 0 is untouched   :581-590
 *   RM_SOP_MENGER_CROSS         s (finite, > 0), s * 3.0 (as the caller's multiplication rounds it): primitive, one trip of
 *                               the Menger loop: a = py_mod(p * s, 2.0) - 1.0, r = abs(1.0 - 3.0 * abs(a)) per axis,
 *                               (min(max(r.x, r.y), min(max(r.y, r.z), max(r.z, r.x))) - 1.0) / (s * 3.0)         :221-237
 *   RM_SOP_GYROID               freq, lipschitz (finite, > 0): primitive, with q = freq * p
 *                               (sin(q.x) * cos(q.y) + sin(q.y) * cos(q.z) + sin(q.z) * cos(q.x)) / lipschitz      :510-514
 * Two placement ops, point transforms closed by RM_SOP_POP_POINT like RM_SOP_TRANSLATE (neither is in the reference):
 *   RM_SOP_ROTATE               cx, sx, cy, sy, cz, sz: the cosine and sine of three angles, each pair finite with
 *                               |c * c + s * s - 1| <= 2^-50.  The child solid is turned about the world x axis, then y,
 *                               then z; the point therefore goes the other way round, each step forming its products first
 *                               and then one add or subtract, both from the old pair:
 *                                 z: (x, y) <- (cz * x + sz * y, cz * y - sz * x)
 *                                 y: (z, x) <- (cy * z + sy * x, cy * x - sy * z)
 *                                 x: (y, z) <- (cx * y + sx * z, cx * z - sx * y)
 *                               A pair that is exactly (1, 0) leaves its plane untouched (no arithmetic); a pair of 0 and
 *                               +-1 (a quarter turn) permutes two axes and rounds nothing.
 *   RM_SOP_MIRROR               flag x, y, z, each exactly 0.0 or 1.0: a flagged coordinate becomes its absolute value
 * Both keep a 1-Lipschitz child 1-Lipschitz (a rotation is an isometry, abs is 1-Lipschitz).  A rotated child's value is
 * its distance; a mirror's value is the child's distance only where the child's solid lies on the positive side of every
 * flagged plane (a solid that crosses a mirror plane gives a bound of the distance to its mirrored union, not the distance).
 * One RM_SOP_ROTATE is a full orientation in one of the RM_SCENE_PROGRAM_MAX_POINTS point slots.
 * RM_SOP_GYROID is the one op that evaluates trigonometry on the device: sin and cos are the library's exact restatements
 * of glibc's for |q| < 105414336 (0x1.921fbp+26) and NaN for larger or non-finite arguments, so the op's value is NaN
 * there (the catalogue's Gyroid scene has the same limit).
 * RM_SOP_CAPPED_TORUS (and the catalogue's Capped Torus) is NaN where p.p + ra^2 - 2 ra k rounds below zero: on the centre
 * circle of the tube the terms cancel to +-1 ulp, about one point in six of the circle comes out negative, the reference's
 * `** 0.5` turns complex there and its caller raises TypeError; the library's pow returns NaN for a negative base.
 * Cylinders (RM_SOP_CYLINDER, Cylinder, Pillar Forest): where a `** 2` leaves binary64 (a radial or axial distance of
 * 2^512 = 1.34e154 or more) the reference raises OverflowError; the library returns what libm's pow makes of it, +inf.
 * Every result the reference defines is bit-identical to its functions (binary64, its evaluation order); the edges of that
 * arithmetic are pinned by tests/golden/sdf_edges.npz.
 * Ids of programs start at RM_SCENE_PROGRAM_BASE, increase monotonically and are never reused within a process.  A
 * program id is accepted by every frame entry point (rm_render*, rm_render_device, rm_bench_device, rm_render_batch*,
 * rm_march_rays, rm_sdf_eval, rm_gather_frame*) until it is destroyed; afterwards they return RM_E_BAD_SCENE.  A program
 * scene has no wavefront-team form (rm_march_rays_team: RM_E_BAD_SCENE) and never runs the single-launch pipeline
 * (RmFrameDesc.pipeline is ignored); it takes the library's defaults of a cheap scene.  rm_num_scenes() stays 20. */
#define RM_SCENE_PROGRAM_BASE 1024
#define RM_SCENE_PROGRAM_MAX_OPS 256
#define RM_SCENE_PROGRAM_MAX_VALUES 8   /* value stack depth */
#define RM_SCENE_PROGRAM_MAX_POINTS 4   /* saved points (nested transforms) */
enum {
    RM_SOP_SPHERE = 0, RM_SOP_BOX = 1, RM_SOP_PLANE = 2, RM_SOP_CYLINDER = 3, RM_SOP_TORUS = 4, RM_SOP_CAPSULE = 5,
    RM_SOP_CAPPED_TORUS = 6, RM_SOP_CONE = 7,
    RM_SOP_UNION = 8, RM_SOP_SUBTRACT = 9, RM_SOP_INTERSECT = 10,
    RM_SOP_SMOOTH_UNION = 11, RM_SOP_SMOOTH_SUBTRACT = 12, RM_SOP_SMOOTH_INTERSECT = 13,
    RM_SOP_TRANSLATE = 14, RM_SOP_REPEAT = 15, RM_SOP_POP_POINT = 16,
    RM_SOP_ROUND = 17, RM_SOP_ONION = 18,
    RM_SOP_SCALE = 19, RM_SOP_LIMITED_REPEAT = 20, RM_SOP_MENGER_CROSS = 21, RM_SOP_GYROID = 22,
    RM_SOP_ROTATE = 23, RM_SOP_MIRROR = 24,
    RM_SOP_COUNT = 25
};
typedef struct RmSceneOp {
    int32_t op;       /* RM_SOP_* */
    int32_t arg;      /* reserved: 0 */
    double f[8];      /* constants (table above) */
} RmSceneOp;
/* Validates the program on the host (opcodes, stack depths, length, finite constants; RM_E_BAD_ARG with the reason in
 * rm_last_error) and registers it; needs no device (the device copy is made by the first frame that uses it).
 * `lipschitz` (> 0) is kept with the program for the host's bookkeeping; a frame reads RmMarchConfig.lipschitz. */
int rm_scene_program_create(const RmSceneOp* ops, int32_t nops, double lipschitz, int32_t* scene_id);
/* Frees the program and its device copy; its id is never handed out again.  RM_E_BAD_SCENE for an unknown id. */
int rm_scene_program_destroy(int32_t scene_id);

/* ---- Strategy programs: user-defined marching rules run by an interpreter in the render kernels -------------------------
 * A strategy program is a jump-free register program that runs once per SDF evaluation of a ray (DESIGN.md section 3,
 * "Strategy programs").  Its id is passed wherever a strategy id is (rm_render*, rm_render_outputs, rm_render_device,
 * rm_render_batch*, rm_capture, rm_march_rays); rm_march_rays_team refuses it (RM_E_BAD_STRATEGY).  A frame with a program
 * id is always ONE plain render pass: no parked rays, no single launch, no teams, whole evaluations, the library's
 * static tile order (the descriptor's scheduling fields are ignored).
 *
 * Registers, all binary64, per ray:
 *   s0 .. s15   state: persist between evaluations, all zero when a ray starts.  The machine reads seven after a block:
 *                 s0  t          the ray parameter reported when the ray finishes
 *                 s1  te         where the SDF is evaluated next
 *                 s2  phase      which block consumes that value (0 .. 7; anything else names no block)
 *                 s3  status     0 go on; non-zero finished; exactly 2.0: finished and, when the frame runs with `full`,
 *                                evaluate once more at s0 and report that value as final_sdf (skipped without `full`)
 *                 s4  hit        non-zero = hit
 *                 s5  final_sdf
 *                 s6  iterations converted to int32: NaN -> 0, clamped to [0, INT32_MAX], truncated
 *               s7 .. s15 belong to the program.
 *   t0 .. t15   temporaries: live within one block execution only; a block must write one before it reads it.
 * Operand codes (RmStrategyOp.dst / a / b / c):
 *   0 .. 15 = s0 .. s15, 16 .. 31 = t0 .. t15 (the only valid destinations), then read-only:
 *   RM_STRATEGY_IN_D (the value just evaluated; not in the init block), RM_STRATEGY_IN_TE (where it was evaluated; not in
 *   the init block), RM_STRATEGY_IN_HIT_THRESHOLD, _MAX_DISTANCE, _MAX_ITERATIONS (as a double), _LIPSCHITZ (the frame's
 *   RmMarchConfig; RmStrategyParams is never read), and RM_STRATEGY_LITERAL = the op's own `k` (finite; a program may
 *   hold RM_STRATEGY_PROGRAM_MAX_CONSTANTS distinct literals, compared by their bits).
 * Ops (dst <- ...; unused operands must be 0; comparisons and logic yield 1.0 / 0.0, "true" is "!= 0"):
 *   MOV a | ADD SUB MUL DIV a b (one IEEE operation each, never fused) | NEG ABS SQRT a | PYMAX PYMIN a b (Python's
 *   max(a, b) / min(a, b): a unless b compares strictly greater / less) | LT LE GT GE EQ NE a b | AND OR a b | NOT a |
 *   SELECT a b c (b where a != 0, else c).  There are no jumps: a conditional is a select, and a division whose result
 *   is not selected is harmless (IEEE: inf or NaN, no trap).
 * Blocks: RM_STOP_BLOCK with a = RM_STRATEGY_BLOCK_INIT (-1) or a phase 0 .. 7 opens a block; the ops up to the next
 * marker are its body.  The array starts with a marker, the init block is required and each block may appear once.  The
 * init block runs when a ray starts (it may finish the ray at once); a step runs the block of the ray's phase.
 * Evaluation budget (a safety condition): a ray is force-finished at its (8 * max(max_iterations, 0) + 64)-th evaluation
 * (the count clamped to INT32_MAX) if the program has not finished it by then -- hit 0, t = s0, final_sdf = the value of
 * that evaluation, iterations from s6, no further evaluation.  A program that sets a non-zero status in the block of that
 * very evaluation has finished the ray: its hit, t, final_sdf (s5) and iterations stand, and a status of 2 gets no tail
 * evaluation there.  The compiled strategies stay far below the budget (at most 2 * max_iterations + 40).
 * Ids start at RM_STRATEGY_PROGRAM_BASE, increase monotonically and are never reused within a process; ids in
 * [RM_NUM_STRATEGY_KERNELS, RM_STRATEGY_PROGRAM_BASE) and destroyed or never-created program ids are RM_E_BAD_STRATEGY.
 * rm_num_strategies() stays 11. */
#define RM_STRATEGY_PROGRAM_BASE 1024
#define RM_STRATEGY_PROGRAM_MAX_OPS 256        /* instructions of all blocks together (markers not counted) */
#define RM_STRATEGY_PROGRAM_MAX_CONSTANTS 64
#define RM_STRATEGY_PROGRAM_MAX_STATE 16
#define RM_STRATEGY_PROGRAM_MAX_TEMPS 16
#define RM_STRATEGY_PROGRAM_MAX_PHASES 8
enum {
    RM_STOP_MOV = 0, RM_STOP_ADD = 1, RM_STOP_SUB = 2, RM_STOP_MUL = 3, RM_STOP_DIV = 4, RM_STOP_NEG = 5, RM_STOP_ABS = 6,
    RM_STOP_SQRT = 7, RM_STOP_PYMAX = 8, RM_STOP_PYMIN = 9, RM_STOP_LT = 10, RM_STOP_LE = 11, RM_STOP_GT = 12,
    RM_STOP_GE = 13, RM_STOP_EQ = 14, RM_STOP_NE = 15, RM_STOP_AND = 16, RM_STOP_OR = 17, RM_STOP_NOT = 18,
    RM_STOP_SELECT = 19,
    RM_STOP_COUNT = 20,
    RM_STOP_BLOCK = 32
};
enum {
    RM_STRATEGY_IN_D = 32, RM_STRATEGY_IN_TE = 33, RM_STRATEGY_IN_HIT_THRESHOLD = 34, RM_STRATEGY_IN_MAX_DISTANCE = 35,
    RM_STRATEGY_IN_MAX_ITERATIONS = 36, RM_STRATEGY_IN_LIPSCHITZ = 37,
    RM_STRATEGY_LITERAL = 63,
    RM_STRATEGY_BLOCK_INIT = -1
};
typedef struct RmStrategyOp {
    int32_t op;          /* RM_STOP_* */
    int32_t dst;         /* operand code 0 .. 31 (0 for RM_STOP_BLOCK) */
    int32_t a, b, c;     /* operand codes; RM_STOP_BLOCK: a = RM_STRATEGY_BLOCK_INIT or the phase */
    int32_t reserved;    /* 0 */
    double k;            /* the value RM_STRATEGY_LITERAL operands of this op read; 0 when none does */
} RmStrategyOp;
/* Validates the program on the host (RM_E_BAD_ARG with the reason in rm_last_error: unknown op, operand out of range, a
 * temporary read before its block wrote it, no init block, a phase above 7, a duplicate block, a non-finite literal, too
 * many instructions or literals) and registers it; needs no device. */
int rm_strategy_program_create(const RmStrategyOp* ops, int32_t nops, int32_t* strategy_id);
/* Frees the program and its device copy; its id is never handed out again.  RM_E_BAD_STRATEGY for an unknown id. */
int rm_strategy_program_destroy(int32_t strategy_id);

/* ---- Interval first-hit oracle (gpu/interval_oracle.py, gpu/interval.py) ----------------------------------------------
 * A sound first hit by interval root isolation: each step evaluates an interval extension of the scene's SDF over the
 * box of the ray segment [t, t + h]; lo > 0 proves the segment empty (t += h, h = min(h * growth, h_max); a miss once
 * t > t_max), otherwise h shrinks by half until h <= tol, and the ray hits at t.  A miss after max_steps steps.  Unlike a
 * sampling marcher it cannot tunnel through thin features.  Rounding is to nearest, as in the reference: the enclosure
 * is exact in real arithmetic only.
 * Scenes: the 14 catalogue scenes that are compositions of primitives.py (ids 0-8, 12, 13, 14, 17, 19: the library holds
 * their programs) and every live scene program.  Sphere, Grazing Plane, Cube and Thin Torus are the reference's
 * INTERVAL_SCENES bit for bit.  Any other scene (Mandelbulb, Menger, Gyroid, ...) and a destroyed program: RM_E_BAD_SCENE.
 * The scene and the configuration are checked before the device: RM_E_BAD_SCENE / RM_E_BAD_ARG come without a GPU, every
 * call that passes them returns RM_E_NO_DEVICE without one.  Host pointers; synchronous. */
/* Ceiling of RmIntervalConfig.max_steps: every step is one dependent evaluation of the scene's interval program (2-25 us
 * on the MI355X for the catalogue scenes), so 10x the reference's 20000 bounds one launch to seconds, not hours. */
#define RM_INTERVAL_MAX_STEPS 200000
typedef struct RmIntervalConfig {  /* every field 0 = the reference's constant */
    double t_max;                  /* 100    DEFAULT_T_MAX */
    double tol;                    /* 1e-5   DEFAULT_TOL: a hit once a non-empty probe has h <= tol */
    double h0;                     /* 0.25   _H0: first probe length */
    double growth;                 /* 1.5    _GROWTH: probe growth across empty space (> 1) */
    double h_max;                  /* 10     _HMAX: probe ceiling */
    double normal_eps;             /* 1e-4   _normals_fd's eps */
    double bound_radius;           /* rm_interval_render's prune (_prune_candidates, origin-centred sphere): 0 = the library's
                                    * bound for the scene (SCENE_BOUND: Sphere 1.05, Cube 1.7421, Thin Torus 1.65; none for the
                                    * others), > 0 = this radius, < 0 = no prune */
    int32_t max_steps;             /* 20000  _MAX_ITERS: steps per ray (at most RM_INTERVAL_MAX_STEPS) */
    int32_t reserved;              /* 0 */
} RmIntervalConfig;
/* Negative or non-finite fields, growth <= 1 after defaults, max_steps < 0 or > RM_INTERVAL_MAX_STEPS, reserved != 0:
 * RM_E_BAD_ARG. */

/* 1 when scene_id has an interval extension (a restated catalogue id or a live program), else 0.  Host only. */
int rm_interval_supported(int scene_id);
/* The interval extension over n boxes: lo, hi are n x 3 corners; out_lo / out_hi receive the enclosure per box. */
int rm_interval_sdf_eval(int scene_id, const double* lo, const double* hi, size_t n, double* out_lo, double* out_hi);
/* first_hit over n explicit rays (origins, dirs: n x 3; directions are used as given, first_hit does not normalise).
 * t: first hit, +inf on a miss.  steps (n int32, optional): steps the ray marched.  normals (n x 3, optional): _normals_fd
 * at o + t * d on a hit, 0 on a miss.  cfg may be NULL (all defaults); its bound_radius is not used here. */
int rm_interval_march_rays(int scene_id, const RmIntervalConfig* cfg, const double* origins, const double* dirs,
                           size_t n, double* t, int32_t* steps, double* normals);
/* interval_capture over rows [row0, row0 + rows) of the frame desc describes (scene_id, width, height, row0, rows, cam:
 * the library's camera rays, the ones rm_render marches; every other field is ignored).  Per pixel, row-major from row0:
 * depth (t on a hit, 0 on a miss), hit (0 / 1), normal (3 doubles, optional), steps (optional; 0 for a pruned ray).
 * timing (optional): warmup + repeats timed launches as rm_render. */
int rm_interval_render(const RmFrameDesc* desc, const RmIntervalConfig* cfg, double* depth, uint8_t* hit,
                       double* normal, int32_t* steps, RmTiming* timing);

/* ---- Sound segment tracer (gpu/faithful_offline.py, gpu/interval_autodiff.py) -----------------------------------------
 * The ceiling of the comparison: a Galin-style segment tracer whose Lipschitz bound is not sampled but proven.  Each trip
 * evaluates f at the cursor t (the interval program at a degenerate box) -- a hit when |f| < tol -- and a dual interval
 * (value enclosure + enclosure of the derivative along the ray, csrc/rm_segment.h) over [t, t + h]:
 * K = clip(max |der|, k_min, l_global) bounds |g'| there, so step = min(|f| / K, h) is short of the surface;
 * t += step, h = clip(max(step, |f| / K) * kappa, h_min, h_max); a miss once t > t_max or after `budget` trips.
 * Scenes, errors, stream and timing conventions: exactly as the interval oracle above (the same 14 catalogue scenes and
 * every live scene program; RM_E_BAD_SCENE otherwise).  Sphere, Grazing Plane, Cube and Thin Torus are the reference's
 * COMPONENT_SCENES bit for bit.  l_global is a bound of |grad f| times the length of the direction: the default 1 is
 * right for exact SDFs and unit directions only. */
/* Ceiling of RmSegmentConfig.budget: every trip is two dependent evaluations of the scene's program (the point, then the
 * dual interval over the probe), so 10x the reference's 4096 bounds one launch to seconds like RM_INTERVAL_MAX_STEPS. */
#define RM_SEGMENT_MAX_STEPS 40960
typedef struct RmSegmentConfig {   /* every field 0 = the reference's constant */
    double t_max;                  /* 100    DEFAULT_T_MAX */
    double tol;                    /* 1e-4   _TOL: a hit once |f| < tol at the cursor */
    double h0;                     /* 0.1    _H0: first probe length */
    double kappa;                  /* 1.5    _KAPPA: probe growth */
    double h_min;                  /* 1e-5   _HMIN */
    double h_max;                  /* 10     _HMAX */
    double k_min;                  /* 1e-6   _KMIN: floor of the directional bound K */
    double l_global;               /* 1      the global Lipschitz bound K is clamped to */
    double bound_radius;           /* rm_segment_render's prune, as RmIntervalConfig.bound_radius */
    int32_t budget;                /* 4096   _BUDGET: trips per ray (at most RM_SEGMENT_MAX_STEPS) */
    int32_t reserved;              /* 0 */
} RmSegmentConfig;
/* Negative or non-finite fields, budget < 0 or > RM_SEGMENT_MAX_STEPS, reserved != 0: RM_E_BAD_ARG. */

/* Same answer as rm_interval_supported.  Host only. */
int rm_segment_supported(int scene_id);
/* The dual interval over n ray segments: segs is n x 8 (origin, direction, t0, t1; the direction as given); out is n x 4
 * (val.lo, val.hi, der.lo, der.hi).  val equals rm_interval_sdf_eval of the segment's box bit for bit. */
int rm_segment_sdf_eval(int scene_id, const double* segs, size_t n, double* out);
/* segment_trace over n explicit rays (directions as given).  t: the hit, +inf on a miss.  iters (n int32, optional): trips
 * the ray was active.  cursor (n, optional): the final t.  cfg may be NULL; its bound_radius is not used here. */
int rm_segment_march_rays(int scene_id, const RmSegmentConfig* cfg, const double* origins, const double* dirs,
                          size_t n, double* t, int32_t* iters, double* cursor);
/* faithful_capture over rows [row0, row0 + rows) of the frame desc describes (as rm_interval_render).  Per pixel: depth (t
 * on a hit, 0 on a miss), hit, iters (optional; 0 for a pruned ray), cursor (optional; the final t, 0 for a pruned ray). */
int rm_segment_render(const RmFrameDesc* desc, const RmSegmentConfig* cfg, double* depth, uint8_t* hit,
                      int32_t* iters, double* cursor, RmTiming* timing);

/* ---- Certified first hit (csrc/rm_certify.h) ------------------------------------------------------------------------------
 * An error bar on the interval oracle, per ray: a bracket [t_lo, t_hi] and a status such that, in real arithmetic and for a
 * continuous g(tau) = f(o + tau d),
 *   * [0, t_lo) is proven free of the solid: every sub-segment of it was discharged by a proof, never by "h <= tol";
 *   * t_hi is witnessed: the computed pointwise value (the interval program at a degenerate box) has g(t_hi) < 0 (a
 *     computed 0 is what rounding makes of a tangent contact and witnesses nothing); t_hi = +inf: no witness was found;
 * so the first hit lies in [t_lo, t_hi].  A probe [a, a + h] is proven free when the interval enclosure has lo > 0 (the
 * interval oracle's rule) or when g(a) > K h, K = clip(max |der|, k_min, l_global) the dual-interval bound of |g'| over the
 * probe (the segment tracer's rule, with its caveats: l_global bounds |grad f| times the direction's length, and g must
 * be continuous -- a repeat of a shape that is not even in the repeated coordinate jumps at cell boundaries).  The probe
 * loop is the interval oracle's (h0, growth, h_max); an unproven probe halves, g at its end is looked at, and once a
 * witness b exists the probes stay inside [a, b] and are at most half of it.  Rounding is to nearest.
 *   RM_CERTIFY_MISS  all of [0, t_max] is proven free (or the ray misses the prune's sphere); t_lo = t_hi = +inf
 *   RM_CERTIFY_HIT   witnessed, and t_hi - t_lo <= width; t_lo <= t_max
 *   RM_CERTIFY_OPEN  anything else: no witness (a grazing contact, an enclosure that never clears), an unproven probe
 *                    shrunk to 2^-50 t_lo (four units in the last place), or max_steps probes made.  The bracket reached is
 *                    returned and is as sound as any other.
 * Scenes, errors, stream and timing conventions: exactly as the interval oracle above. */
#define RM_CERTIFY_MISS 0
#define RM_CERTIFY_HIT 1
#define RM_CERTIFY_OPEN 2
typedef struct RmCertifyConfig {   /* every field 0 = its default; the first five as RmIntervalConfig */
    double t_max;                  /* 100 */
    double tol;                    /* 1e-5   the interval oracle's tolerance; checked, but no probe is discharged by it */
    double h0;                     /* 0.25   first probe length */
    double growth;                 /* 1.5    probe growth across proven space (> 1) */
    double h_max;                  /* 10     probe ceiling */
    double bound_radius;           /* rm_certify_render's prune, as RmIntervalConfig.bound_radius */
    double width;                  /* a HIT's bracket is at most this wide; 0 = 1e-10 (1 + t_lo) */
    double l_global;               /* 1      the global Lipschitz bound K is clamped to (RmSegmentConfig.l_global) */
    double k_min;                  /* 1e-6   floor of the directional bound K */
    int32_t max_steps;             /* 20000  probes per ray (at most RM_INTERVAL_MAX_STEPS); a probe is two evaluations */
    int32_t reserved;              /* 0 */
} RmCertifyConfig;
/* Negative or non-finite fields, growth <= 1 after defaults, max_steps < 0 or > RM_INTERVAL_MAX_STEPS, reserved != 0:
 * RM_E_BAD_ARG. */

/* Same answer as rm_segment_supported.  Host only. */
int rm_certify_supported(int scene_id);
/* The bracket of n explicit rays (directions as given).  t_lo, t_hi: n doubles; status: n bytes (RM_CERTIFY_*); steps (n
 * int32, optional): the probes made.  cfg may be NULL; its bound_radius is not used here. */
int rm_certify_march_rays(int scene_id, const RmCertifyConfig* cfg, const double* origins, const double* dirs,
                          size_t n, double* t_lo, double* t_hi, uint8_t* status, int32_t* steps);
/* The brackets of rows [row0, row0 + rows) of the frame desc describes (as rm_interval_render).  Per pixel: t_lo, t_hi,
 * status, steps (optional; 0 for a pruned ray, which is a MISS). */
int rm_certify_render(const RmFrameDesc* desc, const RmCertifyConfig* cfg, double* t_lo, double* t_hi, uint8_t* status,
                      int32_t* steps, RmTiming* timing);

/* ---- Affine range (gpu/affine.py) ----------------------------------------------------------------------------------------
 * The third sound evaluation of a scene over a ray segment: revised affine arithmetic with one noise symbol for the march
 * parameter (csrc/rm_affine.h), and the interval oracle's march with that range plugged in (the reference's march_count).
 * What it measures is tightness: SDF segment evaluations (`steps`) needed against rm_interval_render at the same hit map.
 *   RM_RANGE_AFFINE  the reference's range: range() of the affine form.  Sphere, Grazing Plane, Cube and Thin Torus are
 *                    its COMPONENT_SCENES over AAForm bit for bit.
 *   RM_RANGE_MEET    lo = max(lo_affine, lo_interval), hi = min(hi_affine, hi_interval), the interval half being the
 *                    interval oracle's enclosure of the same segment: sound because both are, per probe at least as tight
 *                    as either, one more walk over the program per probe.
 * Scenes, errors, stream and timing conventions: exactly as the interval oracle above.  The march's constants are
 * RmIntervalConfig's (normal_eps is not used); the mode travels as its own argument, any other value is RM_E_BAD_ARG. */
#define RM_RANGE_AFFINE 1
#define RM_RANGE_MEET 2
/* Same answer as rm_interval_supported.  Host only. */
int rm_affine_supported(int scene_id);
/* The range over n ray segments: segs is n x 8 as in rm_segment_sdf_eval; out_range is n x 2 (lo, hi); out_form (n x 3:
 * x0, x1, e; optional) receives the affine form and must be NULL in RM_RANGE_MEET, whose range is no form's. */
int rm_affine_range_eval(int scene_id, int mode, const double* segs, size_t n, double* out_range, double* out_form);
/* march_count over n explicit rays (directions as given).  t: the hit, +inf on a miss.  steps (n int32, optional): the
 * ray's range evaluations.  cfg may be NULL; its bound_radius is not used here. */
int rm_affine_march_rays(int scene_id, int mode, const RmIntervalConfig* cfg, const double* origins, const double* dirs,
                         size_t n, double* t, int32_t* steps);
/* _capture over rows [row0, row0 + rows) of the frame desc describes (as rm_interval_render, without normals).  Per
 * pixel: depth (t on a hit, 0 on a miss), hit, steps (optional; 0 for a pruned ray).  The sum of steps is the
 * reference's eval count. */
int rm_affine_render(const RmFrameDesc* desc, int mode, const RmIntervalConfig* cfg, double* depth, uint8_t* hit,
                     int32_t* steps, RmTiming* timing);

/* ---- Exact first hit (csrc/rm_exact.h) -----------------------------------------------------------------------------------
 * Closed-form ray / surface intersection of a hard-CSG scene program: no march.  For the ray o + t d (d as given) the set
 * S = { t : f(o + t d) <= 0 } is built from closed per-leaf sets (union, intersection, A with the closure of the complement
 * of B for op_subtract(a, b); round, scale and onion move the level at which a leaf is cut), and the result is the smallest
 * end point t_min < t <= t_max of a maximal interval of S: an entry, the exit when the eye is inside the solid, or a contact
 * of measure zero.  The normal is the outward unit normal of the solid there, `leaf` the index in the program of the
 * primitive whose boundary was hit.
 * Scenes: catalogue ids 0-6, 8 and 14 and every live scene program made of sphere, box, plane, cylinder, torus, capsule,
 * union, subtract, intersect, translate, rotate (the ray is turned into the child's frame, the normal back into the world's)
 * and -- directly over a sphere, plane, torus or capsule -- round, onion and scale.
 * Anything else has no exact form here (rm_exact_supported says why): the smooth combinators, the repeats, the mirror (it
 * folds the ray), cone, capped
 * torus, Menger cross and gyroid; a modifier over a box or a cylinder; and three cases narrower than the op subset suggests --
 * a modifier over the result of a union, subtract or intersect (modifiers are folded into the leaf they follow; write
 * round(union(a, b)) as union(round(a), round(b))), more than three onions over one leaf, and a torus cut at a level where
 * its tube closes the hole (minor radius + level >= major radius).  RM_E_BAD_SCENE, also for a destroyed program.
 * Errors, stream and timing conventions: as the interval oracle above (RM_E_BAD_SCENE / RM_E_BAD_ARG without a GPU). */
typedef struct RmExactConfig {
    double t_min;                  /* roots at or below it are behind / at the eye; 0 = 1e-6 */
    double t_max;                  /* roots above it are misses; 0 = no limit */
    int32_t reserved[2];           /* 0 */
} RmExactConfig;
/* Negative or NaN fields, reserved != 0: RM_E_BAD_ARG. */

/* 1 when scene_id has an exact form, else 0 with the reason in rm_last_error.  Host only. */
int rm_exact_supported(int scene_id);
/* The exact first hit of n explicit rays (origins, dirs: n x 3; directions as given).  t: +inf on a miss.  normals (n x 3,
 * optional): 0 on a miss.  leaf (n int32, optional): -1 on a miss.  cfg may be NULL (all defaults). */
int rm_exact_march_rays(int scene_id, const RmExactConfig* cfg, const double* origins, const double* dirs, size_t n,
                        double* t, double* normals, int32_t* leaf);
/* The same over rows [row0, row0 + rows) of the frame desc describes (as rm_interval_render: the library's camera rays).
 * Per pixel: depth (t on a hit, 0 on a miss), hit (0 / 1), normal (3 doubles, optional), leaf (int32, optional). */
int rm_exact_render(const RmFrameDesc* desc, const RmExactConfig* cfg, double* depth, uint8_t* hit, double* normal,
                    int32_t* leaf, RmTiming* timing);

/* Same contract, evaluated by wavefront TEAMS (scenes whose SDF is a loop of independent
 * transcendental chains -- Mandelbulb: three waves carry the same 64 rays and each evaluates one
 * chain per trip; see rm_kernels.h).  Identical results; RM_E_BAD_SCENE for scenes without a team form. */
int rm_march_rays_team(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins,
                       const double* dirs, size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf);

/* MetricsCollector.benchmark_strategy (metrics/collector.py:19-66): render the frame and
 * copy the maps back.  Host pointers; depth/iters/hit are required (depth is fp32: t if hit
 * else 0, core/types.py:93), the rest optional (NULL):
 *   t_raw      fp64 termination parameter of every ray (MarchResult.t)
 *   final_sdf  fp64 MarchResult.final_sdf (requires desc->march.full)
 *   block_var  (rows/4) x (width/8) int64: 32*sum(x^2) - sum(x)^2 of the iteration counts of each
 *              full 8x4 block (the population variance x 1024 behind warp_divergence_proxy,
 *              core/types.py:125-133); requires row0 % 4 == 0
 * With timing != NULL the kernel is launched warmup + repeats times and timed per launch. */
int rm_render(const RmFrameDesc* desc, float* depth, int32_t* iters, uint8_t* hit, double* t_raw,
              double* final_sdf, int64_t* block_var, RmStats* stats, RmTiming* timing);

/* rm_render with the output pointers in a record, plus one more optional map:
 *   evals   int32 per ray: the number of SDF evaluations its march performed -- what the reference's GLSL
 *           backend counts in g_evals (gpu/shaders/scenes.glsl:10-12).  With march.full = 1 this is the number
 *           of sdf() calls the reference's CPU march() makes for that ray (it also evaluates once more for
 *           final_sdf on a miss and at bisection exits); with full = 0 those final_sdf-only evaluations are skipped.
 * Iterations are not evaluations: Segment, RevAA and Hybrid evaluate more than once per counted iteration. */
typedef struct RmOutputs {
    float* depth;        /* required */
    int32_t* iters;      /* required */
    uint8_t* hit;        /* required */
    double* t_raw;       /* optional, as rm_render */
    double* final_sdf;
    int64_t* block_var;
    int32_t* evals;
} RmOutputs;
int rm_render_outputs(const RmFrameDesc* desc, const RmOutputs* out, RmStats* stats, RmTiming* timing);

/* Same render, outputs left in device memory (caller-owned device pointers, e.g. torch
 * tensors handed to RCCL afterwards).  Asynchronous on `stream` (a hipStream_t, NULL = the
 * library stream).  d_stats: device buffer of rm_stats_device_bytes() bytes or NULL to use
 * the library workspace; decode it with rm_read_stats after synchronising. */
int rm_render_device(const RmFrameDesc* desc, void* d_depth, void* d_iters, void* d_hit, void* d_stats,
                     void* stream);
size_t rm_stats_device_bytes(void);
int rm_read_stats(const void* d_stats, void* stream, RmStats* out);

/* hipEvent-timed loop of rm_render_device on the library stream (device outputs stay resident). */
int rm_bench_device(const RmFrameDesc* desc, void* d_depth, void* d_iters, void* d_hit, RmStats* stats,
                    RmTiming* timing);

/* N frames of one (scene, strategy, frame shape) rendered in ONE launch: the reference's real
 * workload is sweeps of many small frames -- curated viewpoints (viewpoints.py:41-140) and
 * iteration-budget / epsilon levels (sweep.py:96-127) -- and a small frame is bound by the latency
 * of its longest ray, not by throughput.  The tiles of all frames feed one persistent grid (every
 * ray carries its own frame's camera origin and march configuration), so the long-ray tails of the
 * frames overlap and the whole device stays busy.
 *   shape     scene / strategy / width / height / row0 / rows (cam and march of `shape` are ignored)
 *   cams      nframes x 14 doubles (one camera per frame, as RmFrameDesc.cam)
 *   configs   nframes march configs, or NULL to use shape->march for every frame
 *   depth / iters / hit   host arrays of nframes x rows x width elements (frame-major)
 *   stats     nframes RmStats or NULL;  ms_total  device time of the batch launch (hipEvents) or NULL
 *   all configs must share `full`; tile_order_mode must be 0
 * Every frame is bit-identical to what rm_render returns for it alone. */
int rm_render_batch(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                    float* depth, int32_t* iters, uint8_t* hit, RmStats* stats, float* ms_total);

/* Entries each of the two parked-ray queues may hold (device memory: entries x 64..136 bytes, allocated on
 * first use; default 4 Mi, 0 restores it).  A ray that finds the queue full simply marches on where it is,
 * so the capacity bounds memory, never results. */
int rm_set_queue_capacity(int64_t entries);

/* Per-pass device time of the LAST frame launched (rm_render / rm_render_device / ...): a frame is one
 * render pass plus, with long-ray suspension, up to two resume passes (RmFrameDesc.suspend_after).  For a
 * single-launch frame (RmFrameDesc.pipeline = 2) four spans inside the one kernel are returned instead, read
 * from the device clock by the waves themselves: launch -> the tile counter ran out, -> the last producer wave
 * finished its fresh pixels, -> the last producer wave exited, -> the end of the kernel (the teams' tail).
 * rm_set_pass_timing(1) makes every launch record hipEvents between its passes on the launch stream;
 * rm_get_pass_ms synchronises that stream and returns the count and the milliseconds of each pass
 * (ms must hold RM_MAX_PASSES floats). */
#define RM_MAX_PASSES 4
int rm_set_pass_timing(int enable);
int rm_get_pass_ms(void* stream, int32_t* npasses, float* ms);
/* Single-launch frames: milliseconds after launch of the last push into and the last pop out of queue 1, as decoded
 * by the latest rm_get_pass_ms (0 when there was none).  A tuning aid: pop long after push = the teams fell behind. */
int rm_last_queue_marks(float* last_push_ms, float* last_pop_ms);
/* The same for the rays that ended with >= 500 iterations (the frame's longest chains): ms[0], ms[1] = earliest and
 * latest time after launch at which one of them was handed to the teams, ms[2], ms[3] = shortest and longest time one
 * of them then spent with a team. */
int rm_long_ray_marks(float ms[4]);

/* rm_render_batch with an outputs record: depth / iters / hit as above plus the optional frame-major evals map
 * (RmOutputs.evals; t_raw, final_sdf and block_var must be NULL).  With evals, stats[f].sum_evals is filled. */
int rm_render_batch_outputs(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                            const RmOutputs* out, RmStats* stats, float* ms_total);

/* Library-owned device frame buffers for callers without their own allocator. */
int rm_alloc_frame(int32_t width, int32_t rows, void** d_depth, void** d_iters, void** d_hit);
int rm_free_frame(void* d_depth, void* d_iters, void* d_hit);
int rm_copy_frame_to_host(int32_t width, int32_t rows, const void* d_depth, const void* d_iters,
                          const void* d_hit, float* depth, int32_t* iters, uint8_t* hit);

/* ---- BASELINE config 5: one frame row-sharded over the GPUs of a node, one process per GPU ------------------
 * The frame shards with no exchange while it is rendered (rays are independent); its only communication is the
 * final gather of the three maps.  These entry points do that gather from C with RCCL over xGMI -- no PyTorch on the
 * path.  RCCL is loaded on first use (dlopen "librccl.so.1"); the library has no link-time dependency on it.  The
 * environment variable RM_RCCL_LIBRARY, read once at that first load, names the one library to load instead (a particular
 * RCCL build; the tests' loop-back stand-in): if it cannot be loaded or lacks a symbol the call fails with RM_E_RCCL and
 * the message names the path -- the default names are not tried.  Unset or empty: the default names.
 *   rank 0:      rm_comm_unique_id(id);  ship the 128 bytes to the other ranks (any channel: a file, MPI, a socket)
 *   every rank:  rm_init(local device);  rm_comm_init(id, world_size, rank);
 *   per frame:   rm_render_device(shard desc, ...);  rm_gather_frame(...)  -> the whole frame on every rank
 *   at exit:     rm_comm_destroy();
 * Row plan (the same on every rank; raymarch_algo_compare_amd/sharding.py states it in Python): height a multiple of
 * 4 * world_size -> band-cyclic, rank r renders the 4-row bands r, r + N, r + 2N ... (RmFrameDesc.band_rows = 4,
 * band_stride = N, band_offset = r, rows = height / N), so every rank holds the same mix of sky and object rows and
 * no 8x4 divergence block straddles two ranks; otherwise contiguous 4-aligned blocks of rm_shard_rows() rows (the
 * last rank takes the remainder). */
#define RM_COMM_ID_BYTES 128
int rm_comm_unique_id(uint8_t id[RM_COMM_ID_BYTES]);
int rm_comm_init(const uint8_t id[RM_COMM_ID_BYTES], int32_t world_size, int32_t rank);
int rm_comm_destroy(void);
/* Rows per rank of the contiguous plan: ceil(ceil(height / 4) / world_size) * 4. */
int32_t rm_shard_rows(int32_t height, int32_t world_size);
/* All-gather the local shard (RmFrameDesc.rows x width elements per map, device pointers, as rm_render_device left
 * them) from every rank -- three ncclAllGather on `stream` (NULL = the library stream) -- and put the rows in image
 * order: d_full_* hold height x width elements on every rank.  `shard` is the descriptor the shard was rendered
 * with.  Asynchronous on the stream. */
int rm_gather_frame(const RmFrameDesc* shard, const void* d_depth, const void* d_iters, const void* d_hit,
                    void* d_full_depth, void* d_full_iters, void* d_full_hit, void* stream);
/* The same exchange when only ONE rank needs the image (BASELINE config 5 asks for the gathered frame, not for eight
 * copies of it): every other rank sends its shard to `root` (grouped ncclSend / ncclRecv over the direct xGMI links: the
 * root receives 7/8 of the frame, nobody else receives anything).  Contiguous plan: the shards land straight in the image
 * (no second pass over the frame); band-cyclic plan: in a rank-major buffer that one placement pass turns into the image.
 * d_full_* are read on the root only (NULL elsewhere).  Asynchronous on the stream.  Both gather forms: offsets, counts
 * and pairing exercised for N = 2, 3, 4, 8 against a loop-back stand-in on one GPU (tests/test_gpu_loopback_gather.py);
 * never run over real RCCL with N > 1; no scaling figure measured. */
int rm_gather_frame_root(const RmFrameDesc* shard, const void* d_depth, const void* d_iters, const void* d_hit,
                         void* d_full_depth, void* d_full_iters, void* d_full_hit, int32_t root, void* stream);
/* The second half of rm_gather_frame on its own: `d_gathered` holds the shards of all ranks one after the other
 * (rank-major, rows_per_rank x width elements of elem_bytes each, as ncclAllGather leaves them); writes the
 * height x width image.  cyclic != 0: band-cyclic plan with 4-row bands; else contiguous blocks.  Asynchronous. */
int rm_assemble_frame(int32_t world_size, int32_t height, int32_t width, int32_t rows_per_rank, int32_t cyclic,
                      int32_t elem_bytes, const void* d_gathered, void* d_full, void* stream);

/* Which HIP runtime the library's calls resolve to (path of the loaded libamdhip64 and its version numbers).  Needs no
 * device.  Stream handles passed to this library must come from THIS runtime. */
typedef struct RmRuntimeInfo {
    char hip_runtime_path[512];
    int32_t hip_runtime_version;
    int32_t hip_driver_version;
    int32_t hip_runtimes_loaded;     /* copies of libamdhip64 mapped in this process right now (1 is the healthy case) */
    int32_t reserved;
    char other_runtime_path[512];    /* one of the copies that is NOT ours ("" when there is none) */
} RmRuntimeInfo;
int rm_runtime_info(RmRuntimeInfo* out);
/* Streams of the library's own runtime (non-blocking streams on the bound device) for hosts that have no HIP binding:
 * what rm_render_device / rm_gather_frame / rm_read_stats accept as `stream`.  rm_stream_synchronize(NULL) waits for the
 * library stream; it does not hold the library lock while it waits. */
int rm_stream_create(void** stream);
int rm_stream_synchronize(void* stream);
int rm_stream_destroy(void* stream);

/* Test aid: fills both parked-ray queues with the 32-bit word (tag of the next single-launch frame + word_offset) -- the
 * worst stale content a queue can hold -- and marks them as written by an unknown layout, which is what obliges the next
 * single-launch frame to clear them (see State::qkey in csrc/rm_capi.hip).  next_generation (optional) receives that tag. */
int rm_debug_poison_queues(uint32_t word_offset, uint32_t* next_generation);

/* Development trace of single-launch frames (off by default; costs a store per ray and an atomic per ray a team
 * finishes).  After rm_debug_set_trace(1) every single-launch frame records, for each ray a wavefront team finished, eight
 * 32-bit words { output index, iterations, push / pop / end time in 10 ns ticks since launch, SDF evaluations at the pop
 * and at the end, team workgroup | rays alive in the team << 16 } and, per pixel, the device-clock ticks (low 32 bits)
 * at which its ray started and was struck from its tile (0 = never); launch_tick = the same clock at launch.
 * tools/trace_pipeline.py turns this into the time line DESIGN.md section 3 quotes. */
int rm_debug_set_trace(int enable);
int rm_debug_get_trace(uint32_t* records, int64_t max_records, int64_t* nrecords, uint32_t* start_ticks,
                       uint32_t* detach_ticks, int64_t npix, uint32_t* launch_tick);

/* Routines of the device math (csrc/rm_math_*.h) that rm_debug_math_eval evaluates; out0 / out1 per routine.  _U: the
 * wave-uniform band-skipping forms the wavefront teams call; POW_HALF_SPARSE: the guarded square root of waves with at
 * most 16 live lanes (pow for the lanes the guard refuses). */
enum RmMathFn {
    RM_MATH_POW = 0,            /* rm_pow(a, b) */
    RM_MATH_POW2 = 1,           /* rm_pow2(a, 7.0, 8.0): a^7 / a^8 */
    RM_MATH_POW_HALF_DENSE = 2, /* rm_pow_half<false>(a) */
    RM_MATH_POW_HALF_SPARSE = 3,/* rm_pow_half<true>(a) */
    RM_MATH_POW_HALF_GUARD = 4, /* rm_pow_half_guard(a): rounded root / safe flag as 0.0 or 1.0 */
    RM_MATH_SQRT = 5,           /* rm_sqrt(a) */
    RM_MATH_SIN = 6,            /* rm_sin(a) */
    RM_MATH_COS = 7,            /* rm_cos(a) */
    RM_MATH_SINCOS = 8,         /* rm_sincos<false>(a): sin / cos */
    RM_MATH_SINCOS_U = 9,       /* rm_sincos<true>(a): sin / cos */
    RM_MATH_ACOS = 10,          /* rm_acos<false>(a) */
    RM_MATH_ACOS_U = 11,        /* rm_acos<true>(a) */
    RM_MATH_ATAN2 = 12,         /* rm_atan2<false>(a, b) */
    RM_MATH_ATAN2_U = 13,       /* rm_atan2<true>(a, b) */
    RM_MATH_LOG = 14,           /* rm_log(a) */
    RM_MATH_COUNT = 15
};
/* Development / tests: evaluates one RmMathFn routine on the device, one element per live lane, in the render kernels'
 * 256-thread workgroups with the libm tables in LDS.  a, b, out0, out1 are host arrays of n doubles (b is read only by
 * POW and ATAN2*, out1 written only by POW2, POW_HALF_GUARD and SINCOS*; either may be NULL otherwise).  lane_mask selects
 * the live lanes of every wavefront (bit l = lane l): element e goes to the (e mod p)-th live lane of wavefront e / p,
 * p = popcount(lane_mask); the other lanes take part in loading the tables and leave before the routine runs.
 * Synchronous.  RM_E_BAD_ARG for fn out of range, lane_mask == 0 or a NULL buffer the routine needs. */
int rm_debug_math_eval(int32_t fn, const double* a, const double* b, size_t n, uint64_t lane_mask, double* out0, double* out1);

/* Development / tests: the Mandelbulb's bail-out decision from the squared length (csrc/rm_math_pow.h rm_bail4) on the
 * device, laid out over wavefronts as rm_debug_math_eval lays its elements out.  decision[e] = 1.0 where
 * rm_pow(s[e], 0.5) > 4.0 is decided true, else 0.0; band[e] = 1.0 where s[e] lies in the band that takes the root
 * itself (rm_bail4_band), else 0.0.  sparse != 0: with rm_pow_half_sparse's flag on.  Synchronous.  RM_E_BAD_ARG for
 * lane_mask == 0 or a NULL buffer. */
int rm_debug_bail4_eval(const double* s, size_t n, uint64_t lane_mask, int32_t sparse, double* decision, double* band);

/* Store-path probe: writes the 9 B/ray outputs with the render kernel's flush code and no
 * marching, to measure the isolated HBM write bandwidth of the path. */
int rm_bench_store_path(int32_t width, int32_t rows, void* d_depth, void* d_iters, void* d_hit,
                        RmTiming* timing);

/* ---- SSIM and colour-RMSE scoring of captures (csrc/rm_ssim.h) ---------------------------------------------------
 * The tertiary tier of the reference's metrics/scoring.py: the structural similarity (Wang et al. 2004, the defaults of
 * skimage.metrics.structural_similarity: 7 x 7 uniform window, sample covariances, K1 = 0.01, K2 = 0.03, data range 255,
 * the mean over the windows that lie inside the image) of the 8-bit depth, normal and colour images of two captures, and
 * the RMSE of their colour images.  The images are made from the float maps exactly as the reference's
 * data/capture_io.py makes them; the depth images share the reference capture's depth range over its hits.
 *
 * The maps of one width x height capture, row-major HOST arrays: depth (W*H), normal and color (W*H*3, interleaved),
 * hit (W*H, non-zero = hit).  depth and hit are required.  normal, or color, may be NULL in the reference and in every
 * method alike (captures without that map): the matching outputs are NaN.  NULL on one side only is RM_E_BAD_ARG. */
typedef struct RmCaptureMaps {
    const float* depth;
    const float* normal;
    const float* color;
    const uint8_t* hit;
} RmCaptureMaps;
/* Scores `nmethods` captures against one reference in one call; out: nmethods x 4 doubles { depth_ssim, normal_ssim,
 * color_ssim, color_rmse }.  The reference's images are made once.  Window sums are exact integers and every
 * floating-point sum has a fixed order, so the same inputs give the same bits on every run, and a method scores the same
 * alone or in a batch.  `timing` (optional) times the kernels -- reference images, tiles, final sums -- without the
 * copies.  Checked before the device is touched: RM_E_BAD_ARG for a NULL argument or required map, nmethods outside
 * [1, 65535] or a one-sided NULL map; RM_E_BAD_DIMS for a side below 7 (no window fits) or more than 2^31 - 1 pixels. */
int rm_ssim_scores(int32_t width, int32_t height, const RmCaptureMaps* reference, const RmCaptureMaps* methods,
                   int32_t nmethods, double* out, RmTiming* timing);

/* ---- hit-mask, depth and normal scoring of captures (csrc/rm_score.h) ---------------------------------------------
 * The primary and secondary tiers of the reference's metrics/scoring.py and its calibration residual
 * (gpu/oracle_calibration.py), for `nmethods` captures against one reference in one call; csrc/rm_score.h states every
 * definition in full.
 *
 * The maps of one width x height capture, row-major HOST arrays: depth (W*H), normal (W*H*3, interleaved), hit (W*H
 * bytes, non-zero = hit).  depth and normal hold doubles when fp64 != 0, floats otherwise (widened on read, which is
 * exact).  depth and hit are required; normal may be NULL in the reference and in every method alike (the two normal
 * outputs are then NaN), NULL on one side only is RM_E_BAD_ARG. */
typedef struct RmScoreMaps {
    const void* depth;
    const void* normal;
    const uint8_t* hit;
    int32_t fp64;
} RmScoreMaps;
/* One method's result.  With m the method's hit mask and r the reference's:
 *   n_method_hit |m|, n_reference_hit |r|, n_co_hit |m & r|, n_union |m | r|; n_co_hit_core and n_union_core count the
 *   same pixels outside the reference's silhouette band (the pixels within L1 distance band_k of a pixel whose hit flag
 *   differs from an in-image 4-neighbour's: scoring.silhouette_band); n_nan_depth / n_nan_angle count the co-hit pixels
 *   whose depth gap / normal angle is NaN.  Rates (IoU, false hit, false miss) are left to the caller: integer divisions
 *   of these counts.
 *   Over the co-hit pixels, gap = depth - reference depth: depth_mae = mean |gap|, depth_rmse = sqrt(mean gap^2),
 *   depth_signed = mean gap, depth_p95 and depth_med = np.percentile(|gap|, 95) and np.median(|gap|), exact order
 *   statistics under NumPy's interpolation rules; normal_mean_deg and normal_p95_deg likewise of the angle between the
 *   normals in degrees (cosine clamped to [-1, 1], a NaN kept).  All NaN when n_co_hit = 0; a NaN in a sample makes its
 *   percentile and median NaN. */
typedef struct RmScoreResult {
    int64_t n_method_hit, n_reference_hit, n_co_hit, n_union, n_co_hit_core, n_union_core, n_nan_depth, n_nan_angle;
    double depth_mae, depth_rmse, depth_signed, depth_p95, depth_med, normal_mean_deg, normal_p95_deg;
} RmScoreResult;
/* Scores methods[0 .. nmethods) against `reference`; out: nmethods results.  band_k in [0, 8] is the half width of the
 * silhouette band, made once from the reference; a negative band_k means no band (the core counts equal the full
 * counts).  There is no minimum side: 1 x 1 is valid.  Counts are integer sums, every floating-point sum has a fixed
 * order (32 x 8 tiles folded by halves, added in tile order) and the order statistics are exact selections, so the same
 * inputs give the same bits on every run, a method scores the same alone or in a batch, and a host build of
 * csrc/rm_score.h reproduces the result bit for bit.  `timing` (optional) times the kernels without the copies; a timed
 * call returns the same bits.  Checked before the device is touched: RM_E_BAD_ARG for a NULL argument, a NULL depth or
 * hit map, a one-sided NULL normal, nmethods outside [1, 65535] or band_k above 8; RM_E_BAD_DIMS for a non-positive side
 * or more than 2^31 - 1 pixels. */
int rm_score_captures(int32_t width, int32_t height, int32_t band_k, const RmScoreMaps* reference, const RmScoreMaps* methods,
                      int32_t nmethods, RmScoreResult* out, RmTiming* timing);

/* ---- capture on the device: hit normals and shading (csrc/rm_capture.h) ------------------------------------------
 * A capture is a march result plus, per pixel, the tetrahedron normal of the scene at the hit point (four SDF
 * evaluations at p + 0.0005 * k_i) and the shaded colour of the reference's fragment shader (fixed key light, hemisphere
 * ambient, gamma 0.4545; its sky gradient on a miss) -- the maps GPURunner.capture returns.  One kernel computes them in
 * binary64 in a fixed, unfused order from the very camera ray the march kernels shoot and rounds each result to float
 * once: the same inputs give the same bits on every run and on a host build of rm_capture.h.
 *
 * The float maps of the rows [row0, row0 + rows) of a frame, row-major HOST arrays of rows x width elements (geom x4,
 * normal and color x3, interleaved).  hit is required, any other map may be NULL (not computed, not copied):
 *   geom    [hit, iters / max_iterations, t / max_distance, final_sdf] (the divisions in binary64, then rounded)
 *   normal  unit normal on a hit ((0, 0, 0) where the four samples are equal), (0, 0, 0) on a miss
 *   depth   t on a hit, 0 on a miss
 *   color   shaded colour on a hit, background on a miss
 *   evals   SDF evaluations of the march (RmOutputs.evals), as float
 *   hit     0 / 1 */
typedef struct RmCaptureOutputs {
    float* geom;
    float* normal;
    float* depth;
    float* color;
    float* evals;
    uint8_t* hit;        /* required */
} RmCaptureOutputs;
/* Renders `desc` as rm_render_outputs does, then runs the capture kernel on the same stream over the march's device
 * outputs and copies back only the requested maps: one synchronisation, no fp64 map crosses the bus.  hit, depth, evals
 * and geom are the casts of what rm_render_outputs returns for the same desc.  Catalogue scenes and scene programs alike.
 * desc->march.full must be 1 (final_sdf is part of geom) and the slice must not be band-cyclic: RM_E_BAD_ARG.  `timing`
 * (optional) times march + capture kernels without the copies; a timed call returns the same bits.  desc, out and timing
 * are checked before the device is touched. */
int rm_capture(const RmFrameDesc* desc, const RmCaptureOutputs* out, RmStats* stats, RmTiming* timing);

/* The shading pass alone, for frames that already exist on the host (batched sweep frames, segment-tracer frames,
 * anything with a depth and a hit map): `nframes` frames of width x height pixels, frame-major, frame f seen by the
 * camera cams[14 * f .. 14 * f + 14) (RmFrameDesc.cam layout), in ONE launch and one pair of copies.  Exactly one of `t`
 * (fp64 ray parameters) and `depth` (fp32, widened to double) is non-NULL; it is read where hit != 0 only.  Writes normal
 * and color (nframes x height x width x 3 floats each, both required).  A frame gets the same bits alone or in a batch,
 * and rm_shade_frames(t = t_raw) gives rm_capture's normal and color bit for bit.
 * Checked before the device is touched: RM_E_BAD_ARG for a NULL cams / hit / normal / color, both or neither of t and
 * depth, nframes outside [1, 65535], a hit pixel whose depth is not finite or a camera field that is not (a host scan:
 * such a value must not reach the kernel); RM_E_BAD_DIMS for a non-positive side or more than 2^31 - 1 pixels in all;
 * RM_E_BAD_SCENE for an unknown or destroyed scene id. */
int rm_shade_frames(int scene_id, int32_t width, int32_t height, int32_t nframes, const double* cams, const double* t,
                    const float* depth, const uint8_t* hit, float* normal, float* color, RmTiming* timing);

/* ---- discovery features of a (scene, viewpoint) (csrc/rm_features.h) -----------------------------------------------
 * The strategy-independent description the reference's research layer joins sweep rows against (report/features.py):
 * two intrinsic features of the scene's SDF sampled in a box, five view features of a dense-march capture;
 * csrc/rm_features.h states every definition in full.
 *
 * One sample set's intrinsic result: lipschitz_p99 = np.percentile(|grad f|, 99) over the n_finite samples whose central-
 * difference gradient magnitude is finite; slab_median = np.median of the lengths of the n_slabs solid (f < 0) runs along
 * the set's chords -- a length: the caller divides by its box diagonal.  NaN (0x7ff8000000000000) for an empty sample. */
typedef struct RmIntrinsicFeatures {
    double lipschitz_p99, slab_median;
    int64_t n_finite, n_slabs;
} RmIntrinsicFeatures;
/* Generates, evaluates and reduces `nsets` sample sets of scene `scene_id` (a catalogue scene or a scene program) on the
 * device: the six points p +- eps e_axis of each of the n_lip points of a set, the chord_steps samples a + ts[i] * (b - a)
 * of each of its n_chords chords, ONE call of the scene's own point-evaluation kernel over all of them, then gradients,
 * runs of inside samples (one wavefront per chord) and two exact selections per set.  Only the caller's draws go up and
 * only the results come down.  pts, chords, seglen (|b - a| as the caller computed it) and ts are HOST arrays and the
 * caller's data on purpose: the draws are its random generator's and its norm and linspace are not restated here.
 * Optional HOST outputs: gmag_out (nsets x n_lip, NaN = left out of the sample), slab_counts_out (nsets x n_chords runs
 * per chord).  The same inputs give the same bits on every run, a set gives the same bits alone or in a batch, and a host
 * build of csrc/rm_features.h reproduces them from the same SDF values.  `timing` (optional) times the kernels without the
 * copies.  Limits: nsets in [1, 256], n_lip in [0, 65536], n_chords in [0, 4096], chord_steps in [2, 1024]; n_lip == 0 and
 * n_chords == 0 are valid and give NaN and a count of 0.  Checked before the device is touched: RM_E_BAD_ARG for an
 * argument out of range, a lip_eps that is not finite and positive, a NULL required pointer or a seglen element that is
 * NaN or has its sign bit set (a length: +inf is valid; the message names the index); RM_E_BAD_SCENE for an
 * unknown or destroyed scene id. */
int rm_intrinsic_features(int scene_id, int32_t nsets, int32_t n_lip, const double* pts, double lip_eps, int32_t n_chords,
                          const double* chords, const double* seglen, int32_t chord_steps, const double* ts, RmIntrinsicFeatures* out,
                          double* gmag_out, int32_t* slab_counts_out, RmTiming* timing);

/* The maps of one width x height capture as rm_capture writes them, row-major HOST arrays, all required: depth (W*H),
 * normal (W*H*3, interleaved), evals (W*H) as floats; hit (W*H bytes, non-zero = hit).  evals are counts, integers in
 * [0, 2^24]: a NaN or a negative value is read as 0, a value above 2^24 (+inf too) as 2^24, any other is truncated. */
typedef struct RmViewMaps {
    const float* depth;
    const float* normal;
    const float* evals;
    const uint8_t* hit;
} RmViewMaps;
/* One capture's view features.  n_hit; n_grazing: hits with |ray . normal| < 0.20; n_perimeter: hits with a non-hit
 * 4-neighbour (a neighbour beyond the image is a non-hit); sum_evals over the hits.  hit_rate = n_hit / (W * H),
 * grazing_frac = n_grazing / n_hit, silhouette_cplx = n_perimeter / sqrt(n_hit), hardness_mean = sum_evals / n_hit,
 * hardness_cv = population standard deviation of evals over the hits / hardness_mean (0 for a mean of 0); all four 0
 * without a hit.  box_lo / box_hi: per-axis min / max of the hit points origin + depth * ray (+inf / -inf without a hit);
 * an axis over which any hit point's coordinate is NaN is NaN (0x7ff8000000000000) in both. */
typedef struct RmViewFeatures {
    int64_t n_hit, n_grazing, n_perimeter, sum_evals;
    double hit_rate, grazing_frac, silhouette_cplx, hardness_mean, hardness_cv;
    double box_lo[3], box_hi[3];
} RmViewFeatures;
/* The view features of `nviews` captures of width x height pixels in one call, view v seen by the camera
 * cams[14 * v .. 14 * v + 14) (RmFrameDesc.cam layout); each pixel's ray is the one the march kernels shoot.  Counts are
 * integer sums and the one floating-point sum has a fixed order (32 x 8 tiles folded by halves, added in tile order): the
 * same inputs give the same bits on every run, alone or in a batch, and on a host build of csrc/rm_features.h.  `timing`
 * (optional) times the kernels without the copies.  Checked before the device is touched: RM_E_BAD_ARG for a NULL
 * argument or map, nviews outside [1, 65535] or a camera field that is not finite; RM_E_BAD_DIMS for a non-positive side
 * or more than 2^31 - 1 pixels. */
int rm_view_features(int32_t width, int32_t height, int32_t nviews, const double* cams, const RmViewMaps* maps, RmViewFeatures* out,
                     RmTiming* timing);

#ifdef __cplusplus
}
#endif
#endif /* RM_HIP_H */
