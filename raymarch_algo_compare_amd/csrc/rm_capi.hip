// rm_capi.hip -- host side of librm_hip.so: the C ABI declared in include/rm_hip.h.
//
// Owns the device selection, one HIP stream, a grow-only device workspace and the
// (scene, strategy) -> kernel dispatch.  No CPU implementation of the path exists in
// this library: without a usable gfx950 device every entry point returns an error.
//
// The entry points here are the frame path's: frames, batches, streams, the multi-GPU gather, capture and the debug
// trace.  Those of the analysis subsystems sit below their kernels (rm_interval.hip ... rm_math_check.hip) and use this
// file's lock, stream, staging and timing through rm_capi_internal.h.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is loaded with dlopen on first use

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rm_hip.h"
#include "rm_kernels.h"
#include "rm_launch_plan.h"
#include "rm_pipeline.h"
#include "rm_scene_program.h"
#include "rm_capi_internal.h"

static_assert(RM_HIST_BINS == rm::kHistBins, "histogram size mismatch between ABI and kernels");
static_assert(RM_NUM_SCENES == 20 && RM_NUM_STRATEGIES == 11 && RM_NUM_STRATEGY_KERNELS == 13, "registry size");

namespace rm {
#if defined(RM_DEV_STRATEGIES)
// development library (make DEV=1): only some scenes' translation units are linked; the others resolve to null
#define RM_X(id, S) const SceneLaunchers* scene_launchers_##id() __attribute__((weak));
#else
#define RM_X(id, S) const SceneLaunchers* scene_launchers_##id();
#endif
RM_SCENE_LIST(RM_X)
#undef RM_X
#if defined(RM_DEV_STRATEGIES)
const SceneLaunchers* scene_launchers_program() __attribute__((weak));
const SceneLaunchers* scene_launchers_program_ext() __attribute__((weak));
#else
const SceneLaunchers* scene_launchers_program();
const SceneLaunchers* scene_launchers_program_ext();      // ... of programs with an op beyond primitives.py (SceneExtProgram)
#endif

static const SceneLaunchers* scene(int id)
{
    switch (id) {
#if defined(RM_DEV_STRATEGIES)
#define RM_X(id, S) case id: return scene_launchers_##id ? scene_launchers_##id() : nullptr;
#else
#define RM_X(id, S) case id: return scene_launchers_##id();
#endif
        RM_SCENE_LIST(RM_X)
#undef RM_X
    }
    return nullptr;
}
}  // namespace rm

// What the other translation units' entry points use as well (rm_capi_internal.h) is defined in rm::capi; the rest of
// this file's own state and helpers, and its kernels, in the unnamed namespace.
using namespace rm::capi;

static thread_local char g_err[512] = "";

int rm::capi::fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

Buf* rm::capi::g_workspace_bufs = nullptr;   // freed by rm_shutdown

namespace {

void release_all(Buf* owner)
{
    for (Buf* b = owner; b; b = b->next) b->release();
}
Buf* g_comm_bufs = nullptr;        // freed by rm_comm_destroy
struct CommBuf : Buf { CommBuf() : Buf(g_comm_bufs) {} };

// Everything one rm_init .. rm_shutdown life of the library knows, the device buffers aside: rm_shutdown destroys the
// stream and the events and then assigns a fresh Session, so nothing that described freed memory survives it and a
// new field needs no line there.
struct Session {
    bool ready = false;
    int device = -1;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
    bool stats_ready = false;   // the library's statistics buffer was left clean by a fused-reduce frame (launch_frame)
    // shape of the frame whose per-tile costs sit in `tcost` (tile_order_mode 1 needs a match)
    long long cost_key[10] = { -1 };
    bool cost_valid = false;
    hipEvent_t ev[2 * RM_MAX_TIMED];
    bool events = false;
    bool tracing = false;                   // development trace of single-launch frames (rm_debug_set_trace)
    size_t trace_pix = 0;
    unsigned long long trace_t0 = 0;        // low bits irrelevant: the start mark of the traced frame is read back from the stats block
    long long corder_key[12] = { -1 };      // the frame shape whose centre-out tile order sits in `corder`
    bool corder_valid = false;
    // optional per-pass timing of the last frame (rm_set_pass_timing): events around the passes
    bool pass_timing = false;
    hipEvent_t pev[RM_MAX_PASSES + 1];
    bool pev_ready = false;
    int pass_count = 0;
    bool last_was_pipeline = false;                  // rm_get_pass_ms decodes the in-kernel marks of `last_stats`
    const unsigned long long* last_stats = nullptr;
    float long_marks[4] = { 0.f, 0.f, 0.f, 0.f };    // longest rays: earliest / latest push, shortest / longest stay with a team
    float last_push_ms = 0.f, last_pop_ms = 0.f;     // queue-1 marks of the last single-launch frame decoded by rm_get_pass_ms
    uint32_t generation = 0;                         // tag of the queue entries of the latest single-launch frame
    // Who wrote each parked-ray queue last.  A single-launch consumer takes an entry for published when the word at the
    // entry's `ready` offset equals the launch's generation tag; a frame with another entry stride (another strategy), or
    // one that follows a multi-pass frame (entries without tags), would put those offsets on stale payload words -- old
    // output indices, counts, halves of doubles -- that can equal a small tag.  The span a different writer may have
    // touched is therefore cleared before a single launch uses the queue (launch_frame).
    struct QueueKey { int stride = 0; int writer = 0; size_t used = 0; } qkey[rm::kQueues];   // writer: 1 = pass per launch, 2 = single launch, 3 = unknown
    hipEvent_t frame_ev = nullptr;                   // end of the latest frame, on `frame_stream` (frames share one workspace)
    hipStream_t frame_stream = nullptr;
    bool frame_ev_valid = false;
    // The split single launch (rm_pipeline.h): the team kernel runs on a stream of the library's own, next to the producer
    // kernel on the caller's.  Created by the first split frame; split_ev[0] = "the frame's set-up is enqueued" (the side
    // stream waits for it), split_ev[1] = "the team kernel has ended" (the caller's stream waits for it).
    hipStream_t team_stream = nullptr;
    hipEvent_t split_ev[2] = { nullptr, nullptr };
};

// The library's state: the session and the grow-only device workspace.  Only buffers are declared here (anything else
// belongs to Session, where rm_shutdown resets it).
struct State : Session {
    WsBuf stats, depth, iters, hit, traw, fs, bvar, evals, tcost, torder, queue[rm::kQueues];
    WsBuf in[2], out[4];   // staging of the per-point / per-ray calls (Staged)
    WsBuf bstats;   // rm_render_batch: the device frame table
    WsBuf ctl;     // single-launch pipeline: its hot counters, one per 128-byte line
    WsBuf busy;     // rm_march_rays_team: the counter its filler workgroups watch (its own word: a frame in flight owns `ctl`)
    WsBuf trace, trace_start, trace_detach;   // development trace of single-launch frames (rm_debug_set_trace)
    WsBuf ccost, corder;   // single-launch pipeline: the centre-out tile order of the frame shape `corder_key`
    WsBuf cap_out[5], cap_cams;   // rm_capture / rm_shade_frames: geom, normal, depth, color, evals maps; the frames' cameras
} g;

std::mutex g_mu;

}  // namespace

hipStream_t rm::capi::lib_stream() { return g.stream; }
WsBuf (&rm::capi::stage_in)[2] = g.in;
WsBuf (&rm::capi::stage_out)[4] = g.out;

namespace {

// ---- scene programs (rm_scene_program.h) ----------------------------------------------------------------------------
// A registered program: its validated device image on the host, and the device copy the first frame that renders it
// makes (under g_mu; freed by rm_scene_program_destroy and rm_shutdown).
struct Program {
    std::unique_ptr<rm::ProgramImage> img;
    void* dev = nullptr;
    double lipschitz = 1.0;
    bool ext = false;                         // holds RM_SOP_SCALE .. RM_SOP_MIRROR: rendered by SceneExtProgram's kernels
};
std::mutex g_prog_mu;                          // guards g_programs and g_next_program; taken after g_mu where both are held
std::map<int32_t, Program> g_programs;
int32_t g_next_program = RM_SCENE_PROGRAM_BASE;   // ids are never reused: no per-scene cache can outlive its program

const rm::SceneLaunchers* program_launchers(bool ext)
{
#if defined(RM_DEV_STRATEGIES)
    if (ext) return rm::scene_launchers_program_ext ? rm::scene_launchers_program_ext() : nullptr;
    return rm::scene_launchers_program ? rm::scene_launchers_program() : nullptr;
#else
    return ext ? rm::scene_launchers_program_ext() : rm::scene_launchers_program();
#endif
}

}  // namespace

namespace rm::capi {

bool program_exists(int id, bool* ext)
{
    std::lock_guard<std::mutex> lk(g_prog_mu);
    auto it = g_programs.find(id);
    if (it == g_programs.end()) return false;
    if (ext) *ext = it->second.ext;
    return true;
}

bool with_program_image(int id, const std::function<void(const ProgramImage&)>& look)
{
    std::lock_guard<std::mutex> lk(g_prog_mu);
    auto it = g_programs.find(id);
    if (it == g_programs.end()) return false;
    look(*it->second.img);
    return true;
}

// The kernels of scene `id` (a catalogue scene or a program; check_scene has accepted the id): a program that holds an
// op beyond primitives.py (RM_SOP_SCALE .. RM_SOP_MIRROR) has its own instantiation of the interpreter
// (looked up by id again rather than carried out of check_scene through plan_for / launch_frame; the program cannot
// vanish in between: the caller holds g_mu, which rm_scene_program_destroy takes first)
static const rm::SceneLaunchers* launchers(int id)
{
    if (!is_program_id(id)) return rm::scene(id);
    bool ext = false;
    (void)program_exists(id, &ext);
    return program_launchers(ext);
}

SdfEval sdf_eval_of(int id) { return launchers(id)->sdf_eval; }

int no_such_program(int id) { return fail(RM_E_BAD_SCENE, "scene program %d does not exist (never created, or destroyed)", id); }

int check_scene(int id)
{
    if (is_program_id(id)) {
        bool ext = false;
        if (!program_exists(id, &ext)) return no_such_program(id);
        if (!program_launchers(ext)) return fail(RM_E_BAD_SCENE, "the scene-program kernels are not built into this (development) library");
        return RM_OK;
    }
    if (id < 0 || id >= RM_NUM_SCENES) return fail(RM_E_BAD_SCENE, "scene_id %d out of range", id);
    if (!rm::scene(id)) return fail(RM_E_BAD_SCENE, "scene %d is not built into this (development) library", id);
    return RM_OK;
}

// The launch data of scene `id` (KernelArgs.scene_data; under g_mu with the device selected): a program's device image,
// copied by its first frame; nullptr for a catalogue scene.
int scene_data(int id, const void** data)
{
    *data = nullptr;
    if (!is_program_id(id)) return RM_OK;
    std::lock_guard<std::mutex> lk(g_prog_mu);
    auto it = g_programs.find(id);
    if (it == g_programs.end()) return no_such_program(id);
    Program& p = it->second;
    if (!p.dev) {
        void* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(rm::ProgramImage)));
        const hipError_t e = hipMemcpy(dev, p.img.get(), sizeof(rm::ProgramImage), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return fail(RM_E_HIP, "scene program %d: copy to the device failed: %s", id, hipGetErrorString(e));
        }
        p.dev = dev;
    }
    *data = p.dev;
    return RM_OK;
}

}  // namespace rm::capi

namespace {

constexpr size_t kStatsBlockBytes = sizeof(unsigned long long) * rm::kStatsWords;   // the canonical block (what the host reads)
constexpr size_t kStatsBytes = kStatsBlockBytes * rm::kStatsBlocks;                 // + the partial blocks (device buffer size)

int check_ready()
{
    if (!g.ready) return fail(RM_E_NO_DEVICE, "rm_init() has not succeeded: no gfx950 device bound");
    return RM_OK;
}

// A caller's hipStream_t must belong to the HIP runtime this library is bound to.  A process can hold two copies of
// libamdhip64 (librm_hip.so loaded before PyTorch, whose wheel bundles its own runtime under the file name
// libamdhip64.so: the loader does not match it with the already loaded SONAME libamdhip64.so.7); a stream made by the
// other copy is a pointer into a foreign runtime's heap, and HIP 7.2 dereferences whatever it is handed (measured on the
// MI355X box: hipStreamGetFlags on a pointer that is no stream faults instead of returning an error), so a handle cannot be
// validated by asking the runtime.  What CAN be known without touching the handle: streams this library made itself
// (rm_stream_create) are ours; and while only ONE libamdhip64 is mapped in the process, every hipStream_t there is must
// be that runtime's.  With two copies mapped a handle we did not make is refused.
struct HipCopies { int count; char other[256]; const void* mine; };
int count_hip_runtimes_cb(struct dl_phdr_info* info, size_t, void* data)
{
    HipCopies* c = (HipCopies*)data;
    const char* name = info->dlpi_name ? info->dlpi_name : "";
    const char* base = strrchr(name, '/');
    base = base ? base + 1 : name;
    if (strncmp(base, "libamdhip64.so", 14) != 0) return 0;
    ++c->count;
    // is this the copy our own calls resolve to?  (its load segments contain the function's address)
    bool ours = false;
    for (int i = 0; i < info->dlpi_phnum; ++i) {
        const ElfW(Phdr)& ph = info->dlpi_phdr[i];
        if (ph.p_type != PT_LOAD) continue;
        const char* lo = (const char*)info->dlpi_addr + ph.p_vaddr;
        if ((const char*)c->mine >= lo && (const char*)c->mine < lo + ph.p_memsz) ours = true;
    }
    if (!ours) snprintf(c->other, sizeof c->other, "%s", name);
    return 0;
}
HipCopies hip_runtimes_loaded()
{
    HipCopies c;
    memset(&c, 0, sizeof c);
    c.mine = reinterpret_cast<const void*>(&hipStreamCreateWithFlags);
    dl_iterate_phdr(count_hip_runtimes_cb, &c);
    return c;
}
std::vector<void*> g_own_streams, g_seen_streams;      // guarded by g_mu
int check_stream(void* stream)
{
    if (!stream) return RM_OK;
    for (void* p : g_own_streams) if (p == stream) return RM_OK;
    for (void* p : g_seen_streams) if (p == stream) return RM_OK;
    const HipCopies c = hip_runtimes_loaded();
    if (c.count > 1)
        return fail(RM_E_BAD_ARG, "stream %p was not made by rm_stream_create, and this process holds %d copies of the HIP runtime "
                                  "(also %s): a stream of another copy cannot be used here.  Create the stream with rm_stream_create, or "
                                  "load the other runtime's owner (e.g. import torch) BEFORE this library so both share one runtime "
                                  "(rm_runtime_info)", stream, c.count, c.other);
    if (g_seen_streams.size() < 4096) g_seen_streams.push_back(stream);
    return RM_OK;
}

int select_device()
{
    HIP_TRY(hipSetDevice(g.device));
    return RM_OK;
}

}  // namespace

namespace rm::capi {

// (g_mu, check_ready, select_device, in that order; read_stats and shard_open ask for an Entry as well)
Entry::Entry() : lk_(g_mu), rc_(check_ready())
{
    if (!rc_) rc_ = select_device();
    if (rc_) lk_.unlock();
}

int Entry::stream(void* users, hipStream_t* s) const
{
    if (int rc = check_stream(users)) return rc;
    *s = users ? (hipStream_t)users : g.stream;
    return RM_OK;
}

// The rows [row0, row0 + rows) of a width x height frame; a band-cyclic slice (check_desc) has its own test of the last row.
int check_slice(const RmFrameDesc* d, bool band_cyclic)
{
    if (d->width <= 0 || d->height <= 0 || d->row0 < 0 || d->rows < 0 || (!band_cyclic && d->row0 + d->rows > d->height))
        return fail(RM_E_BAD_DIMS, "bad frame slice: %dx%d rows [%d,%d)", d->width, d->height, d->row0, d->row0 + d->rows);
    if ((long long)d->width * d->height > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "frame too large");
    return RM_OK;
}

// The camera record of 14 doubles as the kernels take it.
rm::CameraParams camera_of(const double* cam14)
{
    rm::CameraParams c;
    for (int i = 0; i < 14; ++i) c.v[i] = cam14[i];
    return c;
}

}  // namespace rm::capi

namespace {

int check_desc(const RmFrameDesc* d)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    if (int rc = check_scene(d->scene_id)) return rc;
    if (d->strategy_id < 0 || d->strategy_id >= RM_NUM_STRATEGY_KERNELS)
        return fail(RM_E_BAD_STRATEGY, "strategy_id %d out of range", d->strategy_id);
    if (int rc = check_slice(d, d->band_rows > 0 && d->band_stride > 1)) return rc;
    if (d->tile_rows != 0 && d->tile_rows != 4 && d->tile_rows != 1) return fail(RM_E_BAD_ARG, "tile_rows must be 0, 4 or 1");
    if (d->tile_order_mode < 0 || d->tile_order_mode > 4) return fail(RM_E_BAD_ARG, "tile_order_mode must be 0 .. 4");
    if (d->eval_mode < 0 || d->eval_mode > 2) return fail(RM_E_BAD_ARG, "eval_mode must be 0, 1 or 2");
    if (d->resume_mode < 0 || d->resume_mode > 3) return fail(RM_E_BAD_ARG, "resume_mode must be 0..3");
    if (d->resume_grid < 0) return fail(RM_E_BAD_ARG, "negative resume_grid");
    if (d->pipeline < 0 || d->pipeline > 2) return fail(RM_E_BAD_ARG, "pipeline must be 0, 1 or 2");
    if (d->pipeline_form < 0 || d->pipeline_form > 3) return fail(RM_E_BAD_ARG, "pipeline_form must be 0 .. 3");
    if (d->team_grid < 0 || d->queue_first < 0 || d->queue_first > 3 || d->team_steal < 0 || d->team_steal > 2 ||
        d->queue_refill_min < 0 || d->queue_refill_min > 64 || d->queue_retry < 0 || d->team_retry < 0 || d->age_priority < 0)
        return fail(RM_E_BAD_ARG, "bad single-launch tuning field");
    if (d->exit_backlog < 0 || d->late_teams > 65536) return fail(RM_E_BAD_ARG, "bad late-team field");
    if (d->keep_busy > (1 << 20)) return fail(RM_E_BAD_ARG, "keep_busy out of range");
    if (d->early_handover > (1 << 20)) return fail(RM_E_BAD_ARG, "early_handover out of range");
    if (d->early_trips < 0 || d->early_trips > 64) return fail(RM_E_BAD_ARG, "early_trips out of range");
    if (d->band_rows < 0 || d->band_stride < 0 || d->band_offset < 0) return fail(RM_E_BAD_ARG, "negative band parameter");
    if (d->band_rows > 0 && d->band_stride > 1) {
        const int th = d->tile_rows ? d->tile_rows : 4;
        if (d->band_rows % th) return fail(RM_E_BAD_ARG, "band_rows must be a multiple of the tile height %d", th);
        if (d->band_offset >= d->band_stride) return fail(RM_E_BAD_ARG, "band_offset must be < band_stride");
        if (d->rows > 0) {
            const long long y = d->rows - 1;
            const long long last = d->row0 + ((y / d->band_rows) * d->band_stride + d->band_offset) * d->band_rows + y % d->band_rows;
            if (last >= d->height) return fail(RM_E_BAD_DIMS, "band-cyclic slice maps row %lld beyond height %d", last, d->height);
        }
    }
    return RM_OK;
}

rm::MarchCfg to_cfg(const RmMarchConfig& m)
{
    rm::MarchCfg c;
    c.hit_threshold = m.hit_threshold;
    c.max_distance = m.max_distance;
    c.lipschitz = m.lipschitz;
    c.max_iterations = m.max_iterations;
    c.full = m.full ? 1 : 0;
    c.prm = rm::default_strat_params();
    if (m.use_params) {
        static_assert(sizeof(RmStrategyParams) == sizeof(rm::StratParams), "RmStrategyParams and rm::StratParams must match");
        memcpy(&c.prm, &m.params, sizeof c.prm);
    }
    return c;
}

// The launch plan of `d` (rm_launch_plan.h) with this device's and this scene's facts.
rm::LaunchPlan plan_for(const RmFrameDesc* d, int batch_frames = 0, const RmMarchConfig* configs = nullptr)
{
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    const int strategy = d->strategy_id;
    rm::DeviceFacts f;
    f.cus = g.prop.multiProcessorCount;
    f.has_teams = sc->has_teams;
    f.has_resume_team = sc->resume_team != nullptr;
    f.entry_bytes = sc->entry_bytes(strategy);
    f.per_cu = [sc, strategy](rm::OccKernel k, int /*tile_h: both queries answer for 64x4 tiles*/, int interleave, int batch) {
        int n = 0;
        const hipError_t e = k == rm::OccKernel::pipeline ? sc->occupancy_pipeline(strategy, interleave, batch, &n)
                                                          : sc->occupancy(strategy, interleave, batch, &n);
        return e == hipSuccess ? n : 0;
    };
    return rm::plan_launch(*d, f, batch_frames, configs);
}

// Kernel arguments of one frame of `d` (a batch sets frames / nframes / full / evals itself): pointers and plan fields.
int make_args(const RmFrameDesc* d, const rm::LaunchPlan& p, float* depth, int32_t* iters, uint8_t* hit, double* traw, double* fs,
              long long* bvar, unsigned long long* stats, rm::KernelArgs* a)
{
    memset(a, 0, sizeof *a);
    if (int rc = scene_data(d->scene_id, &a->scene_data)) return rc;
    a->single.cam = camera_of(d->cam);
    a->single.cfg = to_cfg(d->march);
    a->frames = nullptr;
    a->nframes = 1;
    a->full = d->march.full ? 1 : 0;
    a->width = d->width; a->height = d->height; a->row0 = d->row0; a->rows = d->rows;
    a->tiles_x = p.tiles_x;
    a->tiles_y = p.tiles_y;
    a->tiles_per_frame = a->tiles_x * a->tiles_y;
    a->tile_h = p.tile_h;
    a->refill_min = p.refill_min;
    a->hist_bins = rm::kHistBins;
    a->interleave = p.interleave;
    a->age_prio = d->age_priority > 0 ? d->age_priority : 0;
    if (d->band_rows > 0 && d->band_stride > 1) {
        a->band_rows = d->band_rows; a->band_stride = d->band_stride; a->band_offset = d->band_offset;
    }
    a->depth = depth; a->iters = iters; a->hit = hit; a->t_raw = traw; a->final_sdf = fs;
    a->block_var = bvar; a->stats = stats;
    a->fused_reduce = p.fused_reduce;
    if (p.park[0] > 0) {
        a->suspend_after = p.park[0];
        a->suspend_queue = 0;
    }
    if (p.single) {
        a->team_wgs = p.team_wgs;
        a->producer_waves = p.producer_waves;
        a->late_team_first = p.late_team_first;
        a->early_exit_wgs = p.early_exit_wgs;
        a->exit_backlog = p.exit_backlog;
        a->keep_busy = p.keep_busy;
        a->early_trips = p.early_trips;
        a->early_handover = p.early_handover;
        a->suspend_after2 = p.suspend_after2;
        a->q0_detach = p.q0_detach;
        a->q0_first = p.q0_first;
        a->q0_refill_min = p.q0_refill_min;
        a->q0_retry = p.q0_retry;
        a->team_retry = p.team_retry;
        a->team_steal = p.team_steal;
        a->max_spins = p.max_spins;
        a->team_prio = p.team_prio;
    }
    return RM_OK;
}

// Longest-first tile order from last frame's per-tile cost: a counting sort by descending cost
// (one workgroup; ties keep no particular order -- the order only affects the schedule).
__global__ __launch_bounds__(1024) void order_tiles_kernel(const int32_t* __restrict__ cost, int32_t* __restrict__ order, int n)
{
    constexpr int BINS = 1024;
    __shared__ int hist[BINS];
    for (int b = threadIdx.x; b < BINS; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[min(max(cost[i], 0), BINS - 1)], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int b = BINS - 1; b >= 0; --b) { const int c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int pos = atomicAdd(&hist[min(max(cost[i], 0), BINS - 1)], 1);
        order[pos] = i;
    }
}

// Static priorities: tiles nearer the image centre (where the camera looks) get a higher cost.  xweight = 1: centre-out
// (a disc grows from the middle); xweight < 1 flattens the disc into an ellipse -- at 1/16 the middle ROWS go first, centre
// columns leading: where the geometry runs to the horizon (planes, pillar grids) the long rays lie along the horizon line.
__global__ void center_cost_kernel(int32_t* __restrict__ cost, int tiles_x, int tiles_y, int nframes, int tile_h, int width, int height,
                                   int row0, int band_rows, int band_stride, int band_offset, float xweight)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles_x * tiles_y * nframes) return;
    const int tf = t % (tiles_x * tiles_y);               // tile ids run frame-major: every frame of a batch centre-out
    const int tx = tf % tiles_x, ty = tf / tiles_x;
    const int y0 = ty * tile_h;
    const int gy = band_rows > 0 ? row0 + ((y0 / band_rows) * band_stride + band_offset) * band_rows + (y0 % band_rows) : row0 + y0;
    const float cx = (tx * 64 + 32 - 0.5f * width) / (0.5f * height);      // both axes in units of half the image height
    const float cy = (gy + 0.5f * tile_h - 0.5f * height) / (0.5f * height);
    const float r = sqrtf(xweight * cx * cx + cy * cy);
    cost[t] = max(0, 1023 - (int)(r * 256.0f));
}

// 8x4-block variance numerators 32*sum(x^2) - sum(x)^2 of the finished iteration map (core/types.py:125-133),
// one thread per full block: used instead of the in-flush reduction when rays were parked (their
// pixels are not in the tile when it is flushed).
__global__ void block_var_kernel(const int32_t* __restrict__ iters, int width, int rows, int nframes,
                                 long long* __restrict__ out)
{
    const int bw = width >> 3, bh = rows >> 2;
    const long long n = (long long)bw * bh * nframes;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int f = (int)(b / ((long long)bw * bh));
    const int r = (int)(b - (long long)f * bw * bh);
    const int by = r / bw, bx = r - by * bw;
    const int32_t* p = iters + (size_t)f * (size_t)rows * (size_t)width + (size_t)(by * 4) * (size_t)width + (size_t)(bx * 8);
    long long S = 0, Q = 0;
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const long long v = p[(size_t)y * (size_t)width + x];
            S += v; Q += v * v;
        }
    out[b] = 32 * Q - S * S;
}

// Sum the partial stats blocks into the canonical block 0 (totals: add; iter_max and the complemented iter_min: max).
__global__ void stats_reduce_kernel(unsigned long long* __restrict__ stats)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;      // word index within a block
    if (w >= rm::kStatsWords || w == 0 || (w >= 6 && w < 10) || (w > 10 && w < rm::kStatsHead)) return;   // counters live in block 0 only
    unsigned long long acc = 0;
    const bool is_max = (w == 3 || w == 4);
    for (int p = 1; p <= rm::kStatsParts; ++p) {
        const unsigned long long v = stats[(size_t)p * rm::kStatsWords + w];
        acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
    stats[w] = acc;
}

constexpr long long kQueueCapMax = 1ll << 22;   // default entries per suspended-ray queue (a full queue leaves rays in place)
long long g_queue_cap = kQueueCapMax;           // rm_set_queue_capacity

void frame_key(const RmFrameDesc* d, int tile_h, long long* k)
{
    k[0] = d->scene_id; k[1] = d->strategy_id; k[2] = d->width; k[3] = d->height; k[4] = d->row0; k[5] = d->rows;
    k[6] = d->band_rows; k[7] = d->band_stride; k[8] = d->band_offset; k[9] = tile_h;
}

int launch_frame(const RmFrameDesc* d, const rm::LaunchPlan& p, rm::KernelArgs a, hipStream_t s);

// One frame: (optional) longest-first tile order from the previous frame's costs, stats reset, render.
int launch(const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, hipStream_t s)
{
    // The parked-ray queues, tile costs / orders, the control block and the pass events are ONE workspace: frames
    // are serialised on the device.  A frame enqueued on another stream than the previous one first waits for it
    // (callers may still overlap their own copies and other kernels with a frame).
    if (g.frame_ev_valid && g.frame_stream != s) HIP_TRY(hipStreamWaitEvent(s, g.frame_ev, 0));
    const int rc_frame = launch_frame(d, p, a, s);
    if (rc_frame) return rc_frame;
    if (!g.frame_ev_valid) {
        HIP_TRY(hipEventCreateWithFlags(&g.frame_ev, hipEventDisableTiming));
        g.frame_ev_valid = true;
    }
    HIP_TRY(hipEventRecord(g.frame_ev, s));
    g.frame_stream = s;
    return RM_OK;
}

// How the single launch of plan `p` is performed (RmFrameDesc.pipeline_form): 1 = the fused pipeline_kernel, 2 = producers
// and teams as two kernels side by side, 3 = the two kernels one after the other on the caller's stream (tests).
// The split form covers the default schedule -- detach mode, every team resident from the start -- where a producer never
// waits for a team; any other knob set keeps the fused kernel.  Library's choice (0): kSplitByDefault, and only where
// each of the two kernels reaches at least the workgroups per compute unit the plan's grid counts on, so that together
// they occupy no more than the fused grid does.
// Measured (parent, fused default and split default alternating three times on one MI355X, DESIGN.md section 3 "Split single
// launch"): bench.py 270.5-272.5 Mrays/s with the fused kernel, 278.0-278.7 split.
#ifndef RM_SPLIT_BY_DEFAULT
#define RM_SPLIT_BY_DEFAULT 1      // (-DRM_SPLIT_BY_DEFAULT=0: the other default, for a same-box A/B of two libraries)
#endif
constexpr bool kSplitByDefault = RM_SPLIT_BY_DEFAULT != 0;
int single_launch_form(const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, const rm::SceneLaunchers* sc, int* form)
{
    *form = 1;
    if (d->pipeline_form == 1) return RM_OK;
    const bool covered = sc->pipeline_teams && sc->pipeline_producers && p.team_wgs > 0 && p.suspend_after2 > 0 && p.q0_detach != 0 &&
                         p.early_exit_wgs == 0 && p.late_team_first == p.pipeline_grid;
    if (d->pipeline_form >= 2) {
        if (!covered)
            return fail(RM_E_BAD_ARG, "pipeline_form %d: the split form exists for single launches with teams in detach mode without late teams", d->pipeline_form);
        *form = d->pipeline_form;
        return RM_OK;
    }
    if (!kSplitByDefault || !covered || a.frames) return RM_OK;
    // Skipping-Spheres and Adaptive-Hybrid keep the fused kernel: same alternation at 1920x1080, fused / split 8.91 / 8.99-9.00 ms
    // and 4.61 / 4.68-4.76 (few of their rays reach the teams; the other nine of the registry gain or stay within the spread)
    if (d->strategy_id == 7 || d->strategy_id == 9) return RM_OK;
    int fused = 0, producers = 0, teams = 0;
    if (sc->occupancy_pipeline(d->strategy_id, a.interleave, 0, &fused) != hipSuccess ||
        sc->occupancy_split(d->strategy_id, a.tile_h, a.interleave, 0, &producers, &teams) != hipSuccess)
        return RM_OK;
    const int per_cu = rm::grid_per_cu(fused);
    if (producers >= per_cu && teams >= per_cu) *form = 2;
    return RM_OK;
}

// Performs the plan `p` (rm_launch_plan.h) of one launch: workspace, caches and enqueues in the order it dictates.
int launch_frame(const RmFrameDesc* d, const rm::LaunchPlan& p, rm::KernelArgs a, hipStream_t s)
{
    a.raw_outputs = (a.t_raw || a.final_sdf || a.evals) ? 1 : 0;
    // A fused-reduce frame leaves the statistics buffer zeroed where the next frame needs it: no reduce launch, and --
    // for the library's own buffer, which nobody else writes -- no memset either.  A caller's buffer is always cleared
    // (its contents are not ours to trust).
    const bool own_stats = a.stats == (unsigned long long*)g.stats.p;
    if (!(own_stats && g.stats_ready)) HIP_TRY(hipMemsetAsync(a.stats, 0, kStatsBytes, s));
    if (own_stats) g.stats_ready = a.fused_reduce != 0;
    if (d->rows == 0) return RM_OK;
    if (p.refuse) return fail(RM_E_BAD_ARG, "%s", p.refuse);
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    const int ntiles = a.tiles_per_frame * a.nframes;
    int order = p.tile_order;
    if (order == 1) {
        int rc;
        if ((rc = g.tcost.ensure((size_t)ntiles * 4)) || (rc = g.torder.ensure((size_t)ntiles * 4))) return rc;
        long long key[10];
        frame_key(d, p.tile_h, key);
        if (g.cost_valid && memcmp(key, g.cost_key, sizeof key) == 0) {
            hipLaunchKernelGGL(order_tiles_kernel, dim3(1), dim3(1024), 0, s, (const int32_t*)g.tcost.p,
                               (int32_t*)g.torder.p, ntiles);
            HIP_TRY(hipGetLastError());
            a.tile_order = (const int32_t*)g.torder.p;
        }
        a.tile_cost = (int32_t*)g.tcost.p;      // this frame's costs feed the next frame's order
        memcpy(g.cost_key, key, sizeof key);
        g.cost_valid = true;
        if (!a.tile_order) order = p.static_order;    // no costs yet: the first frame takes the static order
    }
    if (order == 2 || order == 4) {
        // A static permutation of the frame shape, computed once and kept until the shape changes: no extra launch per frame.
        long long key[12];
        frame_key(d, p.tile_h, key);
        key[0] = key[1] = 0;                    // pure geometry: the same permutation for every scene and strategy
        key[10] = a.nframes; key[11] = order;
        int rc2;
        if ((rc2 = g.corder.ensure((size_t)ntiles * 4))) return rc2;
        if (!g.corder_valid || memcmp(key, g.corder_key, sizeof key) != 0) {
            if ((rc2 = g.ccost.ensure((size_t)ntiles * 4))) return rc2;
            hipLaunchKernelGGL(center_cost_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, s, (int32_t*)g.ccost.p, a.tiles_x,
                               a.tiles_y, a.nframes, p.tile_h, a.width, a.height, a.row0, a.band_rows, a.band_stride, a.band_offset,
                               order == 4 ? 1.0f / 16.0f : 1.0f);
            hipLaunchKernelGGL(order_tiles_kernel, dim3(1), dim3(1024), 0, s, (const int32_t*)g.ccost.p, (int32_t*)g.corder.p, ntiles);
            HIP_TRY(hipGetLastError());
            memcpy(g.corder_key, key, sizeof key);
            g.corder_valid = true;
        }
        a.tile_order = (const int32_t*)g.corder.p;
    }
    // long-ray suspension: the queues of the parked rays
    long long* const block_var = a.block_var;
    if (p.park[0] > 0) {
        const long long total = (long long)a.rows * a.width * a.nframes;
        const long long cap = std::min<long long>(total, g_queue_cap);
        const int stride = p.queue_entry_bytes;
        int rc;
        for (int q = 0; q < (p.park[1] > 0 ? 2 : 1); ++q) {
            const size_t need = (size_t)cap * (size_t)stride;
            State::QueueKey& key = g.qkey[q];
            if (need > g.queue[q].cap) {
                if ((rc = g.queue[q].ensure(need))) return rc;
                // fresh memory: no word of it may look like a published entry of a later launch (QEntry.ready)
                HIP_TRY(hipMemsetAsync(g.queue[q].p, 0, need, s));
                key.used = 0;
            }
            const int writer = p.single ? 2 : 1;
            if (writer == 2 && key.used > 0 && (key.writer != 2 || key.stride != stride)) {
                // another layout wrote here: stale payload words now sit at this launch's `ready` offsets
                HIP_TRY(hipMemsetAsync(g.queue[q].p, 0, std::min(key.used, g.queue[q].cap), s));
                key.used = 0;
            }
            key.writer = writer;
            key.stride = stride;
            key.used = std::max(key.used, need);
            a.queue[q] = (unsigned char*)g.queue[q].p;
        }
        a.queue_cap = (int32_t)cap;
        a.queue_stride = stride;
        a.block_var = nullptr;      // parked pixels are missing at flush time: reduced from the finished map below
    }
    const bool pt = g.pass_timing && g.pev_ready;
    g.pass_count = 0;
    g.last_was_pipeline = false;
    if (pt) HIP_TRY(hipEventRecord(g.pev[0], s));
    if (p.single) {
        // ---- the whole frame in ONE launch (rm_pipeline.h): producers + queue-0 consumers + teams side by side
        {
            int rc2;
            if ((rc2 = g.ctl.ensure(sizeof(unsigned long long) * rm::kCtlWords))) return rc2;
            HIP_TRY(hipMemsetAsync(g.ctl.p, 0, sizeof(unsigned long long) * rm::kCtlWords, s));
            a.ctl = (unsigned long long*)g.ctl.p;
        }
        if (++g.generation == 0) g.generation = 1;
        a.generation = g.generation;
        a.marks = (g.pass_timing || g.tracing) ? 1 : 0;      // device-clock marks only when somebody will read them (rm_get_pass_ms)
        if (g.tracing) {
            constexpr size_t kTraceRecords = 1u << 20;
            const size_t npix = (size_t)a.rows * a.width * a.nframes;
            int rc3;
            if ((rc3 = g.trace.ensure((8 + 8 * kTraceRecords) * 4)) || (rc3 = g.trace_start.ensure(npix * 4)) ||
                (rc3 = g.trace_detach.ensure(npix * 4)))
                return rc3;
            HIP_TRY(hipMemsetAsync(g.trace.p, 0, 32, s));
            HIP_TRY(hipMemsetAsync(g.trace_start.p, 0, npix * 4, s));
            HIP_TRY(hipMemsetAsync(g.trace_detach.p, 0, npix * 4, s));
            a.trace = (uint32_t*)g.trace.p;
            a.trace_cap = (uint32_t)kTraceRecords;
            a.trace_start = (uint32_t*)g.trace_start.p;
            a.trace_detach = (uint32_t*)g.trace_detach.p;
            g.trace_pix = npix;
        }
        if (a.tile_cost) HIP_TRY(hipMemsetAsync(a.tile_cost, 0, (size_t)ntiles * 4, s));   // resumed rays may report before the tile flush
        int form = 1;
        if (int rcf = single_launch_form(d, p, a, sc, &form)) return rcf;
        if (form == 1) {
            HIP_TRY(sc->pipeline(d->strategy_id, a, p.pipeline_grid, s));
        } else {
            // PRODUCERS FIRST: they never wait for a team, so whatever the device makes of the two kernels -- side by side, or
            // the teams only once the producers have left -- the frame is correct and ends.  A team that starts before any
            // producer polls (bounded) until the producer waves have reported their exit.
            const int producer_wgs = p.pipeline_grid - p.team_wgs;
            hipStream_t ts = s;
            if (form == 2) {
                if (!g.team_stream) {
                    HIP_TRY(hipStreamCreateWithFlags(&g.team_stream, hipStreamNonBlocking));
                    for (auto& e : g.split_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                }
                ts = g.team_stream;
                HIP_TRY(hipEventRecord(g.split_ev[0], s));            // control block, queues and statistics are reset
                HIP_TRY(hipStreamWaitEvent(ts, g.split_ev[0], 0));
            }
            HIP_TRY(sc->pipeline_producers(d->strategy_id, a, producer_wgs, s));
            HIP_TRY(sc->pipeline_teams(d->strategy_id, a, p.team_wgs, ts));
            if (form == 2) {
                // the caller's stream goes on when both kernels have ended: its events and the statistics fold cover the teams
                HIP_TRY(hipEventRecord(g.split_ev[1], ts));
                HIP_TRY(hipStreamWaitEvent(s, g.split_ev[1], 0));
            }
        }
        if (pt) HIP_TRY(hipEventRecord(g.pev[++g.pass_count], s));
        g.last_was_pipeline = true;
        g.last_stats = a.stats;
    } else {
        HIP_TRY(sc->render(d->strategy_id, a, p.render_grid, s));
        if (pt) HIP_TRY(hipEventRecord(g.pev[++g.pass_count], s));
    }
    if (p.park[0] > 0 && !p.single) {
        // passes 2 and 3: the parked rays of queue 0, then those parked again in queue 1
        rm::KernelArgs b = a;
        b.suspend_after = p.park[1];
        b.suspend_queue = 1;
        b.refill_min = p.resume_refill_min;
        b.team_wgs = p.resume_grid;
        b.keep_busy = p.pass_keep_busy;
        if (p.pass_team[0])
            HIP_TRY(sc->resume_team(d->strategy_id, 0, b, p.team_pass_grid, s));
        else
            HIP_TRY(sc->resume(d->strategy_id, 0, b, p.resume_grid, s));
        if (pt) HIP_TRY(hipEventRecord(g.pev[++g.pass_count], s));
        if (p.park[1] > 0) {
            b.suspend_after = 0;
            b.interleave = 0;       // a sparse pass of very long rays is latency-bound: whole evaluations per turn
            if (p.pass_team[1])
                HIP_TRY(sc->resume_team(d->strategy_id, 1, b, p.team_pass_grid, s));
            else
                HIP_TRY(sc->resume(d->strategy_id, 1, b, p.resume_grid, s));
            if (pt) HIP_TRY(hipEventRecord(g.pev[++g.pass_count], s));
        }
    }
    if (p.park[0] > 0 && block_var) {
        const long long nb = (long long)(a.width >> 3) * (a.rows >> 2) * a.nframes;
        if (nb > 0) {
            hipLaunchKernelGGL(block_var_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, a.iters, a.width,
                               a.rows, a.nframes, block_var);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!a.fused_reduce) {
        hipLaunchKernelGGL(stats_reduce_kernel, dim3((rm::kStatsWords + 255) / 256), dim3(256), 0, s, a.stats);
        HIP_TRY(hipGetLastError());
    }
    return RM_OK;
}

// a single-launch frame whose queue protocol ran into one of its wait bounds (rm_pipeline.h) reports it here
int check_pipeline_error(const unsigned long long* w)
{
    if (w[rm::kWError] != 0)
        return fail(RM_E_HIP, "single-launch pipeline: a wait of the queue protocol hit its bound (code %llu); results are incomplete", w[rm::kWError]);
    return RM_OK;
}

void decode_stats(const unsigned long long* w, RmStats* out)
{
    out->hit_count = w[1];
    out->sum_iters = w[2];
    out->iter_max = (int32_t)w[3];
    out->total_rays = w[5];
    out->sum_evals = w[10];
    out->iter_min = w[5] ? (int32_t)(0x7fffffffull - w[4]) : 0;
    for (int b = 0; b < RM_HIST_BINS; ++b) out->iter_hist[b] = w[rm::kStatsHead + b];
}

void summarise(RmTiming* t)
{
    const int n = t->repeats;
    if (n <= 0) { t->ms_median = t->ms_mean = t->ms_min = t->ms_max = 0.f; return; }
    std::vector<float> v(t->ms_each, t->ms_each + n);
    std::sort(v.begin(), v.end());
    t->ms_min = v.front(); t->ms_max = v.back();
    t->ms_median = (n & 1) ? v[n / 2] : 0.5f * (v[n / 2 - 1] + v[n / 2]);
    double sum = 0; for (float x : v) sum += x;
    t->ms_mean = (float)(sum / n);
}

int ensure_events()
{
    if (g.events) return RM_OK;
    for (auto& e : g.ev) HIP_TRY(hipEventCreate(&e));
    g.events = true;
    return RM_OK;
}

}  // namespace

int rm::capi::check_timing(const RmTiming* t)
{
    if (t->repeats < 1 || t->repeats > RM_MAX_TIMED || t->warmup < 0)
        return fail(RM_E_BAD_ARG, "timing: repeats must be 1..%d, warmup >= 0", RM_MAX_TIMED);
    return RM_OK;
}

// Runs `once` (one enqueue on `s`, returning an RM_ code) warmup + repeats times, each timed run bracketed by events
// on `s`; waits for the stream and fills ms_each and the summary of `t`.
int rm::capi::timed(const Entry&, RmTiming* t, hipStream_t s, const std::function<int()>& once)
{
    int rc = check_timing(t);
    if (rc || (rc = ensure_events())) return rc;
    for (int i = 0; i < t->warmup; ++i)
        if ((rc = once())) return rc;
    for (int i = 0; i < t->repeats; ++i) {
        HIP_TRY(hipEventRecord(g.ev[2 * i], s));
        if ((rc = once())) return rc;
        HIP_TRY(hipEventRecord(g.ev[2 * i + 1], s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < t->repeats; ++i) HIP_TRY(hipEventElapsedTime(&t->ms_each[i], g.ev[2 * i], g.ev[2 * i + 1]));
    summarise(t);
    return RM_OK;
}

namespace {

// The events of timed() bracket one whole frame: stats reset, optional tile ordering, render kernel.
int timed_launches(const Entry& e, const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, RmTiming* t)
{
    return timed(e, t, g.stream, [&] { return launch(d, p, a, g.stream); });
}

// The canonical statistics block at `dev`, read once `s` has run dry: the pipeline's error word, then the counters.
int read_stats(const Entry&, const void* dev, hipStream_t s, RmStats* out)
{
    unsigned long long w[rm::kStatsWords];
    HIP_TRY(hipMemcpyAsync(w, dev, kStatsBlockBytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_pipeline_error(w)) return rc;
    if (out) decode_stats(w, out);
    return RM_OK;
}

// ---- RCCL, loaded on first use ------------------------------------------------------------
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    ncclComm_t comm = nullptr;
    int world = 0, rank = -1;
    CommBuf gather[3], pad[3];  // all-gather landing buffers (rank-major) and padded send buffers of a short last shard
} R;

int rccl_load()
{
    if (R.handle) return RM_OK;
    // RM_RCCL_LIBRARY (read once, on the first load): the one library to use -- a particular RCCL build, or the tests'
    // loop-back stand-in.  A named library that cannot be loaded is an error, never a reason to try the default names.
    static const std::string named = [] { const char* v = getenv("RM_RCCL_LIBRARY"); return std::string(v ? v : ""); }();
    void* h = nullptr;
    if (!named.empty()) {
        h = dlopen(named.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(RM_E_RCCL, "RM_RCCL_LIBRARY=%s could not be loaded: %s", named.c_str(), dlerror());
    } else {
        for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return fail(RM_E_RCCL, "librccl.so.1 could not be loaded: %s", dlerror());
    }
    const char* const where = named.empty() ? "librccl" : named.c_str();
#define RM_SYM(field, sym)                                                                     \
    R.field = reinterpret_cast<decltype(R.field)>(dlsym(h, #sym));                              \
    if (!R.field) { dlclose(h); return fail(RM_E_RCCL, "%s lacks %s", where, #sym); }
    RM_SYM(GetUniqueId, ncclGetUniqueId)
    RM_SYM(CommInitRank, ncclCommInitRank)
    RM_SYM(CommDestroy, ncclCommDestroy)
    RM_SYM(AllGather, ncclAllGather)
    RM_SYM(Send, ncclSend)
    RM_SYM(Recv, ncclRecv)
    RM_SYM(GroupStart, ncclGroupStart)
    RM_SYM(GroupEnd, ncclGroupEnd)
    RM_SYM(GetErrorString, ncclGetErrorString)
#undef RM_SYM
    R.handle = h;
    return RM_OK;
}

#define RCCL_TRY(expr)                                                                         \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess)                                                                 \
            return fail(RM_E_RCCL, "%s failed: %s (%s:%d)", #expr, R.GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

// Rows of the gathered shards (rank-major) -> image order.  One thread per 16-byte (or 1-byte) piece of a row.
template <class T>
__global__ void assemble_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int world, int height, long long row_elems,
                                     int rows_per_rank, int cyclic)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= row_elems) return;
    const int y = blockIdx.y;                          // image row
    int r, local;
    if (cyclic) {
        const int band = y >> 2;                       // 4-row bands dealt round-robin
        r = band % world;
        local = (band / world) * 4 + (y & 3);
    } else {
        r = y / rows_per_rank;
        local = y - r * rows_per_rank;
    }
    dst[(long long)y * row_elems + i] = src[((long long)r * rows_per_rank + local) * row_elems + i];
}

int assemble(int world, int height, int width, int rows_per_rank, int cyclic, int elem_bytes, const void* src, void* dst, hipStream_t s)
{
    const long long row_bytes = (long long)width * elem_bytes;
    if (height <= 0 || row_bytes <= 0) return RM_OK;
    const bool vec = (row_bytes % 16 == 0) && ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0);
    if (vec) {
        const long long n = row_bytes / 16;
        hipLaunchKernelGGL((assemble_rows_kernel<uint4>), dim3((unsigned)((n + 255) / 256), (unsigned)height), dim3(256), 0, s,
                           (const uint4*)src, (uint4*)dst, world, height, n, rows_per_rank, cyclic);
    } else {
        hipLaunchKernelGGL((assemble_rows_kernel<unsigned char>), dim3((unsigned)((row_bytes + 255) / 256), (unsigned)height), dim3(256), 0, s,
                           (const unsigned char*)src, (unsigned char*)dst, world, height, row_bytes, rows_per_rank, cyclic);
    }
    HIP_TRY(hipGetLastError());
    return RM_OK;
}

// ---- store-path probe: the flush of render_kernel without the march --------------------
__global__ __launch_bounds__(64) void store_path_kernel(float* depth, int32_t* iters, uint8_t* hit, int width,
                                                        int rows, int tiles_x, int ntiles)
{
    constexpr int TILE_H = 4;
    __shared__ float s_depth[64 * TILE_H];
    __shared__ int32_t s_iters[64 * TILE_H];
    __shared__ uint8_t s_hit[64 * TILE_H];
    const int lane = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * 64, y0 = (tile / tiles_x) * TILE_H;
        for (int r = 0; r < TILE_H; ++r) {
            s_depth[r * 64 + lane] = (float)(tile + r);
            s_iters[r * 64 + lane] = tile ^ lane;
            s_hit[r * 64 + lane] = (uint8_t)((tile + lane) & 1);
        }
        __syncthreads();
        const int gx = x0 + lane;
        for (int r = 0; r < TILE_H; ++r)
            if (gx < width && y0 + r < rows) {
                const size_t gi = (size_t)(y0 + r) * width + gx;
                depth[gi] = s_depth[r * 64 + lane];
                iters[gi] = s_iters[r * 64 + lane];
                hit[gi] = s_hit[r * 64 + lane];
            }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

const char* rm_last_error(void) { return g_err; }
int rm_num_scenes(void) { return RM_NUM_SCENES; }

int rm_scene_program_create(const RmSceneOp* ops, int32_t nops, double lipschitz, int32_t* scene_id)
{
    if (!scene_id) return fail(RM_E_BAD_ARG, "scene_id is NULL");
    if (!(lipschitz > 0.0) || !(lipschitz - lipschitz == 0.0)) return fail(RM_E_BAD_ARG, "lipschitz must be finite and > 0");
    std::unique_ptr<rm::ProgramImage> img(new rm::ProgramImage());
    char why[256];
    if (!rm::program_encode(ops, nops, img.get(), why, sizeof why)) return fail(RM_E_BAD_ARG, "scene program: %s", why);
    std::lock_guard<std::mutex> lk(g_prog_mu);
    if (g_next_program == INT32_MAX) return fail(RM_E_BAD_ARG, "scene program ids exhausted");
    const int32_t id = g_next_program++;
    Program& p = g_programs[id];
    p.ext = rm::program_has_ext(*img);
    p.img = std::move(img);
    p.lipschitz = lipschitz;
    *scene_id = id;
    return RM_OK;
}

int rm_scene_program_destroy(int32_t scene_id)
{
    std::lock_guard<std::mutex> lk(g_mu);       // no call of this library is enqueueing a frame of the program meanwhile
    void* dev = nullptr;
    {
        std::lock_guard<std::mutex> lp(g_prog_mu);
        auto it = g_programs.find(scene_id);
        if (it == g_programs.end()) return no_such_program(scene_id);
        dev = it->second.dev;
        g_programs.erase(it);
    }
    if (dev) {
        if (g.ready) (void)hipSetDevice(g.device);
        HIP_TRY(hipFree(dev));
    }
    return RM_OK;
}
int rm_num_strategies(void) { return RM_NUM_STRATEGIES; }

void rm_default_strategy_params(RmStrategyParams* out)
{
    if (!out) return;
    const rm::StratParams p = rm::default_strat_params();
    memcpy(out, &p, sizeof *out);
}
size_t rm_stats_device_bytes(void) { return kStatsBytes; }

int rm_init(int device_id)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g.ready && g.device == device_id) return RM_OK;
    if (g.ready) return fail(RM_E_BAD_ARG, "already initialised on device %d; call rm_shutdown() first", g.device);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(RM_E_NO_DEVICE, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(RM_E_NO_DEVICE, "device %d out of range (have %d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    HIP_TRY(hipGetDeviceProperties(&g.prop, device_id));
    if (strncmp(g.prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RM_E_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device_id, g.prop.gcnArchName);
    HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    int rc = g.stats.ensure(kStatsBytes);
    if (rc) return rc;
    g.device = device_id;
    g.ready = true;
    return RM_OK;
}

void rm_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g.ready) return;
    (void)hipSetDevice(g.device);
    (void)hipStreamSynchronize(g.stream);
    if (g.team_stream) {
        (void)hipStreamSynchronize(g.team_stream);
        for (auto& e : g.split_ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(g.team_stream);
    }
    // streams handed out by rm_stream_create belong to this session: run them dry, destroy and forget them
    for (void* s : g_own_streams) {
        (void)hipStreamSynchronize((hipStream_t)s);
        (void)hipStreamDestroy((hipStream_t)s);
    }
    g_own_streams.clear();
    g_seen_streams.clear();
    release_all(g_workspace_bufs);
    if (g.frame_ev_valid) (void)hipEventDestroy(g.frame_ev);
    if (g.events) for (auto& e : g.ev) (void)hipEventDestroy(e);
    if (g.pev_ready) for (auto& e : g.pev) (void)hipEventDestroy(e);
    {
        // programs stay registered; their device copies are made again by the next frame after rm_init
        std::lock_guard<std::mutex> lp(g_prog_mu);
        for (auto& kv : g_programs)
            if (kv.second.dev) {
                (void)hipFree(kv.second.dev);
                kv.second.dev = nullptr;
            }
    }
    (void)hipStreamDestroy(g.stream);
    static_cast<Session&>(g) = Session();       // not ready, no device, and nothing remembered about what was just freed
}

int rm_device_info(RmDeviceInfo* out)
{
    int rc = check_ready();
    if (rc) return rc;
    if (!out) return fail(RM_E_BAD_ARG, "out is NULL");
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", g.prop.name);
    snprintf(out->arch, sizeof out->arch, "%s", g.prop.gcnArchName);
    out->device_id = g.device;
    out->compute_units = g.prop.multiProcessorCount;
    out->clock_mhz = g.prop.clockRate / 1000;
    out->wavefront_size = g.prop.warpSize;
    out->total_mem_bytes = g.prop.totalGlobalMem;
    return RM_OK;
}

int rm_sdf_eval(int scene_id, const double* xyz, size_t n, double* out)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_scene(scene_id))) return rc;
    if (n == 0) return RM_OK;
    if (!xyz || !out) return fail(RM_E_BAD_ARG, "NULL buffer");
    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    Staged st(e);
    const double* d_xyz = st.in(g.in[0], xyz, n * 24);
    double* d_out = st.out(g.out[0], out, n * 8);
    if ((rc = st.begin())) return rc;
    HIP_TRY(launchers(scene_id)->sdf_eval(d_xyz, n, d_out, data, g.stream));
    return st.finish();
}

static int march_rays_impl(bool team, int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins,
                           const double* dirs, size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_scene(scene_id))) return rc;
    if (strategy_id < 0 || strategy_id >= RM_NUM_STRATEGY_KERNELS)
        return fail(RM_E_BAD_STRATEGY, "strategy_id %d out of range", strategy_id);
    if (!cfg) return fail(RM_E_BAD_ARG, "cfg is NULL");
    if (team && !launchers(scene_id)->march_rays_team) return fail(RM_E_BAD_SCENE, "scene %d has no wavefront-team form", scene_id);
    if (n == 0) return RM_OK;
    if (!origins || !dirs || !hit || !t || !iters || !final_sdf) return fail(RM_E_BAD_ARG, "NULL buffer");
    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    Staged st(e);
    const double* d_origins = st.in(g.in[0], origins, n * 24);
    const double* d_dirs = st.in(g.in[1], dirs, n * 24);
    uint8_t* d_hit = st.out(g.out[0], hit, n);
    double* d_t = st.out(g.out[1], t, n * 8);
    int32_t* d_iters = st.out(g.out[2], iters, n * 4);
    double* d_fs = st.out(g.out[3], final_sdf, n * 8);
    if ((rc = st.begin())) return rc;
    rm::MarchCfg c = to_cfg(*cfg);
    c.full = 1;   // per-ray API always returns final_sdf, like MarchResult
    if (team) {
        // the teams of a few rays are all that runs: filler workgroups (two per compute unit in all) keep the chip at the
        // speed a frame's teams run at (KEEP BUSY, rm_kernels.h) -- rm_march_rays_team is how bench.py measures a chain
        if ((rc = g.busy.ensure(128))) return rc;
        HIP_TRY(hipMemsetAsync(g.busy.p, 0, sizeof(unsigned long long), g.stream));
        const long long nteams = (long long)((n + 63) / 64);
        const int fillers = (int)std::max<long long>(0, 2ll * g.prop.multiProcessorCount - nteams);
        HIP_TRY(launchers(scene_id)->march_rays_team(strategy_id, c, d_origins, d_dirs, n, d_hit, d_t, d_iters, d_fs,
                                                     (unsigned long long*)g.busy.p, fillers, g.stream));
    } else {
        HIP_TRY(launchers(scene_id)->march_rays(strategy_id, c, d_origins, d_dirs, n, d_hit, d_t, d_iters, d_fs, data, g.stream));
    }
    return st.finish();
}

int rm_march_rays(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins, const double* dirs,
                  size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    return march_rays_impl(false, scene_id, strategy_id, cfg, origins, dirs, n, hit, t, iters, final_sdf);
}

int rm_march_rays_team(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins, const double* dirs,
                       size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    return march_rays_impl(true, scene_id, strategy_id, cfg, origins, dirs, n, hit, t, iters, final_sdf);
}

int rm_render_outputs(const RmFrameDesc* d, const RmOutputs* o, RmStats* stats, RmTiming* timing)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!o || !o->depth || !o->iters || !o->hit) return fail(RM_E_BAD_ARG, "depth, iters and hit are required");
    if (o->final_sdf && !d->march.full) return fail(RM_E_BAD_ARG, "final_sdf requires march.full = 1");
    if (o->block_var && (d->row0 % 4) != 0) return fail(RM_E_BAD_ARG, "block_var requires row0 %% 4 == 0");
    const size_t n = (size_t)d->rows * (size_t)d->width;
    const size_t nblk = (size_t)(d->rows / 4) * (size_t)(d->width / 8);
    Staged st(e);
    float* d_depth = st.out(g.depth, o->depth, n * 4, 16);
    int32_t* d_iters = st.out(g.iters, o->iters, n * 4, 16);
    uint8_t* d_hit = st.out(g.hit, o->hit, n, 16);
    double* d_traw = st.out(g.traw, o->t_raw, n * 8, 16);
    double* d_fs = st.out(g.fs, o->final_sdf, n * 8, 16);
    long long* d_bvar = (long long*)st.out(g.bvar, o->block_var, nblk * 8, 16);
    int32_t* d_evals = st.out(g.evals, o->evals, n * 4, 16);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, d_depth, d_iters, d_hit, d_traw, d_fs, d_bvar, (unsigned long long*)g.stats.p, &a))) return rc;
    a.evals = d_evals;
    if ((rc = timing ? timed_launches(e, d, p, a, timing) : launch(d, p, a, g.stream))) return rc;
    if ((rc = st.download())) return rc;
    return read_stats(e, g.stats.p, g.stream, stats);
}

int rm_render(const RmFrameDesc* d, float* depth, int32_t* iters, uint8_t* hit, double* t_raw, double* final_sdf,
              int64_t* block_var, RmStats* stats, RmTiming* timing)
{
    RmOutputs o;
    memset(&o, 0, sizeof o);
    o.depth = depth; o.iters = iters; o.hit = hit; o.t_raw = t_raw; o.final_sdf = final_sdf; o.block_var = block_var;
    return rm_render_outputs(d, &o, stats, timing);
}

int rm_render_device(const RmFrameDesc* d, void* d_depth, void* d_iters, void* d_hit, void* d_stats, void* stream)
{
    Entry e;                                  // the enqueue touches the shared workspace (queues, tile order, pass events)
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit) return fail(RM_E_BAD_ARG, "device output pointers are required");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, (float*)d_depth, (int32_t*)d_iters, (uint8_t*)d_hit, nullptr, nullptr, nullptr,
                        (unsigned long long*)(d_stats ? d_stats : g.stats.p), &a)))
        return rc;
    return launch(d, p, a, s);
}

int rm_read_stats(const void* d_stats, void* stream, RmStats* out)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!out) return fail(RM_E_BAD_ARG, "out is NULL");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    return read_stats(e, d_stats ? d_stats : g.stats.p, s, out);
}

int rm_bench_device(const RmFrameDesc* d, void* d_depth, void* d_iters, void* d_hit, RmStats* stats, RmTiming* timing)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit || !timing) return fail(RM_E_BAD_ARG, "device outputs and timing are required");
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, (float*)d_depth, (int32_t*)d_iters, (uint8_t*)d_hit, nullptr, nullptr, nullptr,
                        (unsigned long long*)g.stats.p, &a)))
        return rc;
    if ((rc = timed_launches(e, d, p, a, timing))) return rc;
    return stats ? read_stats(e, g.stats.p, g.stream, stats) : RM_OK;
}

int rm_render_batch_outputs(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                            const RmOutputs* o, RmStats* stats, float* ms_total)
{
    if (!o) return fail(RM_E_BAD_ARG, "outputs record is NULL");
    if (o->t_raw || o->final_sdf || o->block_var) return fail(RM_E_BAD_ARG, "batches return depth, iters, hit and evals only");
    float* const depth = o->depth;
    int32_t* const iters = o->iters;
    uint8_t* const hit = o->hit;
    int32_t* const evals = o->evals;
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(shape))) return rc;
    if (nframes < 0 || (nframes > 0 && (!cams || !depth || !iters || !hit))) return fail(RM_E_BAD_ARG, "bad batch arguments");
    if (shape->tile_order_mode != 0) return fail(RM_E_BAD_ARG, "tile_order_mode is not supported for batches");
    if (nframes == 0) return RM_OK;
    const int full = configs ? (configs[0].full ? 1 : 0) : (shape->march.full ? 1 : 0);
    for (int f = 0; configs && f < nframes; ++f)
        if ((configs[f].full ? 1 : 0) != full) return fail(RM_E_BAD_ARG, "all frames of a batch must share march.full");
    const size_t n = (size_t)shape->rows * (size_t)shape->width;          // elements per frame
    const size_t total = n * (size_t)nframes;
    if (total > (size_t)1 << 31) return fail(RM_E_BAD_DIMS, "batch too large");
    if ((rc = ensure_events())) return rc;
    // the frame table: one camera + march configuration per frame
    std::vector<rm::FrameParams> fp((size_t)nframes);
    for (int f = 0; f < nframes; ++f) {
        fp[f].cam = camera_of(cams + (size_t)f * 14);
        fp[f].cfg = to_cfg(configs ? configs[f] : shape->march);
    }
    Staged st(e);
    float* d_depth = st.out(g.depth, depth, total * 4, 16);
    int32_t* d_iters = st.out(g.iters, iters, total * 4, 16);
    uint8_t* d_hit = st.out(g.hit, hit, total, 16);
    int32_t* d_evals = st.out(g.evals, evals, total * 4, 16);
    const rm::FrameParams* d_frames = st.in(g.bstats, fp.data(), sizeof(rm::FrameParams) * (size_t)nframes);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(shape, nframes, configs);
    RmFrameDesc d = *shape;
    if (p.march_frame >= 0) d.march = configs[p.march_frame];      // (KernelArgs.single: the configuration the plan looked at)
    rm::KernelArgs a;
    if ((rc = make_args(&d, p, d_depth, d_iters, d_hit, nullptr, nullptr, nullptr, (unsigned long long*)g.stats.p, &a))) return rc;
    a.frames = d_frames;
    a.nframes = nframes;
    a.full = full;
    a.evals = d_evals;
    HIP_TRY(hipEventRecord(g.ev[0], g.stream));
    if ((rc = launch(&d, p, a, g.stream))) return rc;
    HIP_TRY(hipEventRecord(g.ev[1], g.stream));
    if ((rc = st.download())) return rc;
    unsigned long long whead[rm::kStatsHead];
    HIP_TRY(hipMemcpyAsync(whead, g.stats.p, sizeof whead, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (g.last_was_pipeline && (rc = check_pipeline_error(whead))) return rc;      // a wait bound hit: the maps are incomplete
    if (ms_total) HIP_TRY(hipEventElapsedTime(ms_total, g.ev[0], g.ev[1]));
    if (stats) {
        // per-frame integer reduce of the returned maps (the in-kernel block aggregates the whole batch)
        for (int f = 0; f < nframes; ++f) {
            RmStats& st = stats[f];
            memset(&st, 0, sizeof st);
            st.total_rays = n;
            st.iter_min = n ? 0x7fffffff : 0;
            const int32_t* it = iters + (size_t)f * n;
            const uint8_t* h = hit + (size_t)f * n;
            for (size_t i = 0; i < n; ++i) {
                st.hit_count += h[i];
                st.sum_iters += (uint64_t)it[i];
                st.iter_max = std::max(st.iter_max, it[i]);
                st.iter_min = std::min(st.iter_min, it[i]);
                st.iter_hist[std::min<int32_t>(std::max<int32_t>(it[i], 0), RM_HIST_BINS - 1)] += 1;
            }
            if (evals)
                for (size_t i = 0; i < n; ++i) st.sum_evals += (uint64_t)evals[(size_t)f * n + i];
        }
    }
    return RM_OK;
}

int32_t rm_shard_rows(int32_t height, int32_t world_size)
{
    if (height <= 0 || world_size <= 0) return 0;
    const int nblk = (height + 3) / 4;
    return ((nblk + world_size - 1) / world_size) * 4;
}

int rm_comm_unique_id(uint8_t id[RM_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == RM_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id) return fail(RM_E_BAD_ARG, "id is NULL");
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId u;
    RCCL_TRY(R.GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return RM_OK;
}

int rm_comm_init(const uint8_t id[RM_COMM_ID_BYTES], int32_t world_size, int32_t rank)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!id || world_size < 1 || rank < 0 || rank >= world_size) return fail(RM_E_BAD_ARG, "bad communicator arguments");
    if ((rc = rccl_load())) return rc;
    if (R.comm) return fail(RM_E_BAD_ARG, "a communicator exists already; call rm_comm_destroy() first");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCL_TRY(R.CommInitRank(&R.comm, world_size, u, rank));
    R.world = world_size;
    R.rank = rank;
    return RM_OK;
}

int rm_comm_destroy(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!R.comm) return RM_OK;
    if (g.ready) {
        (void)hipSetDevice(g.device);
        (void)hipDeviceSynchronize();
    }
    const ncclResult_t r = R.CommDestroy(R.comm);
    R.comm = nullptr;
    R.world = 0; R.rank = -1;
    release_all(g_comm_bufs);
    if (r != ncclSuccess) return fail(RM_E_RCCL, "ncclCommDestroy failed: %s", R.GetErrorString(r));
    return RM_OK;
}

int rm_assemble_frame(int32_t world_size, int32_t height, int32_t width, int32_t rows_per_rank, int32_t cyclic, int32_t elem_bytes,
                      const void* d_gathered, void* d_full, void* stream)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (world_size < 1 || height < 0 || width <= 0 || rows_per_rank < 0 || (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) ||
        !d_gathered || !d_full)
        return fail(RM_E_BAD_ARG, "bad assemble arguments");
    if (cyclic && (height % (4 * world_size) != 0 || rows_per_rank != height / world_size))
        return fail(RM_E_BAD_DIMS, "band-cyclic plan needs height %% (4 * world_size) == 0 and rows_per_rank == height / world_size");
    if (!cyclic && (long long)rows_per_rank * world_size < height) return fail(RM_E_BAD_DIMS, "the shards do not cover the frame");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    return assemble(world_size, height, width, rows_per_rank, cyclic ? 1 : 0, elem_bytes, d_gathered, d_full, s);
}

// What rm_gather_frame and rm_gather_frame_root share: this rank's three maps, where they go, and the plan the shard
// descriptor must follow on this communicator -- rows every rank contributes to the collective (`per`), cyclic or not.
static const int kMapBytes[3] = { 4, 4, 1 };   // bytes per pixel of depth, iters, hit
struct Shard {
    hipStream_t s;
    int N, H, W, per;
    bool cyclic, is_root;
    const void* src[3];
    void* dst[3];
    size_t bytes(int k, long long rows) const { return (size_t)rows * W * kMapBytes[k]; }
};

static int shard_plan(const RmFrameDesc* d, Shard* sh)
{
    const int N = R.world, H = d->height;
    sh->cyclic = d->band_rows > 0 && d->band_stride > 1;
    if (sh->cyclic) {
        if (d->band_rows != 4 || d->band_stride != N || d->band_offset != R.rank || d->row0 != 0 || H % (4 * N) != 0 || d->rows != H / N)
            return fail(RM_E_BAD_DIMS, "band-cyclic shard does not match the communicator (4-row bands, stride = world size %d, "
                                       "offset = rank %d, rows = height / world size)", N, R.rank);
        sh->per = d->rows;
    } else {
        sh->per = N == 1 ? H : rm_shard_rows(H, N);
        const int r0 = std::min(R.rank * sh->per, H), r1 = std::min((R.rank + 1) * sh->per, H);
        if (d->row0 != r0 || d->rows != r1 - r0)
            return fail(RM_E_BAD_DIMS, "contiguous shard of rank %d must be rows [%d, %d)", R.rank, r0, r1);
    }
    return RM_OK;
}

// After the descriptor and the shard pointers have been checked: the communicator, the root (`root` only counts with
// to_root; without it every rank receives the frame), the stream, the plan.
static int shard_open(const Entry& e, const RmFrameDesc* d, const void* d_depth, const void* d_iters, const void* d_hit, void* d_full_depth,
                      void* d_full_iters, void* d_full_hit, bool to_root, int root, void* stream, Shard* sh)
{
    if (!R.comm) return fail(RM_E_RCCL, "no communicator: call rm_comm_init() first");
    *sh = Shard{ nullptr, R.world, d->height, d->width, 0, false, true, { d_depth, d_iters, d_hit }, { d_full_depth, d_full_iters, d_full_hit } };
    if (to_root) {
        if (root < 0 || root >= R.world) return fail(RM_E_BAD_ARG, "root %d outside the communicator of %d", root, R.world);
        sh->is_root = R.rank == root;
        if (sh->is_root && (!d_full_depth || !d_full_iters || !d_full_hit)) return fail(RM_E_BAD_ARG, "the root needs the three full-frame buffers");
    }
    if (int rc = e.stream(stream, &sh->s)) return rc;
    return shard_plan(d, sh);
}

int rm_gather_frame(const RmFrameDesc* d, const void* d_depth, const void* d_iters, const void* d_hit, void* d_full_depth,
                    void* d_full_iters, void* d_full_hit, void* stream)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit || !d_full_depth || !d_full_iters || !d_full_hit) return fail(RM_E_BAD_ARG, "NULL buffer");
    Shard sh;
    if ((rc = shard_open(e, d, d_depth, d_iters, d_hit, d_full_depth, d_full_iters, d_full_hit, false, 0, stream, &sh))) return rc;
    const void* send[3];
    for (int k = 0; k < 3; ++k) {
        const size_t shard_bytes = sh.bytes(k, sh.per);
        if ((rc = R.gather[k].ensure(shard_bytes * (size_t)sh.N + 16))) return rc;
        send[k] = sh.src[k];
        if (d->rows < sh.per) {                     // short last shard of a contiguous plan: pad the send buffer
            if ((rc = R.pad[k].ensure(shard_bytes + 16))) return rc;
            HIP_TRY(hipMemsetAsync(R.pad[k].p, 0, shard_bytes, sh.s));
            if (d->rows > 0) HIP_TRY(hipMemcpyAsync(R.pad[k].p, sh.src[k], sh.bytes(k, d->rows), hipMemcpyDeviceToDevice, sh.s));
            send[k] = R.pad[k].p;
        }
    }
    // the frame's only exchange: three all-gathers in one group (direct xGMI links between the GPUs of a node)
    RCCL_TRY(R.GroupStart());
    for (int k = 0; k < 3; ++k) {
        const ncclResult_t r = R.AllGather(send[k], R.gather[k].p, sh.bytes(k, sh.per), ncclUint8, R.comm, sh.s);
        if (r != ncclSuccess) {
            (void)R.GroupEnd();
            return fail(RM_E_RCCL, "ncclAllGather failed: %s", R.GetErrorString(r));
        }
    }
    RCCL_TRY(R.GroupEnd());
    for (int k = 0; k < 3; ++k)
        if ((rc = assemble(sh.N, sh.H, sh.W, sh.per, sh.cyclic ? 1 : 0, kMapBytes[k], R.gather[k].p, sh.dst[k], sh.s))) return rc;
    return RM_OK;
}

int rm_gather_frame_root(const RmFrameDesc* d, const void* d_depth, const void* d_iters, const void* d_hit, void* d_full_depth,
                         void* d_full_iters, void* d_full_hit, int32_t root, void* stream)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit) return fail(RM_E_BAD_ARG, "NULL shard buffer");
    Shard sh;
    if ((rc = shard_open(e, d, d_depth, d_iters, d_hit, d_full_depth, d_full_iters, d_full_hit, true, root, stream, &sh))) return rc;
    const int N = sh.N, H = sh.H, per = sh.per;
    auto rows_of = [&](int r) { return sh.cyclic ? per : std::max(0, std::min((r + 1) * per, H) - std::min(r * per, H)); };
    // Where rank r's rows land on the root: contiguous plan -> straight into the image (its rows are one block there: no
    // second pass over the frame); band-cyclic plan -> slot r of a rank-major landing buffer, placed by ONE pass of
    // assemble_rows_kernel afterwards (receiving every 4-row band into place would be H / (4 N) x 3 x (N - 1)
    // point-to-point operations per frame: 2835 at 7680x4320 on 8 ranks).
    if (sh.is_root && sh.cyclic)
        for (int k = 0; k < 3; ++k)
            if ((rc = R.gather[k].ensure(sh.bytes(k, per) * (size_t)N + 16))) return rc;
    // (The min() below is a guard only: slot() is reached for ranks with rows_of(r) > 0, i.e. r * per < H, so it never
    // clamps under the present callers and no test can tell it from r * per.)
    auto slot = [&](int k, int r) -> char* {
        return sh.cyclic ? (char*)R.gather[k].p + sh.bytes(k, (long long)r * per) : (char*)sh.dst[k] + sh.bytes(k, std::min(r * per, H));
    };
    RCCL_TRY(R.GroupStart());
    ncclResult_t err = ncclSuccess;
    for (int k = 0; k < 3 && err == ncclSuccess; ++k) {
        if (!sh.is_root) {
            if (d->rows > 0) err = R.Send(sh.src[k], sh.bytes(k, d->rows), ncclUint8, root, R.comm, sh.s);
        } else {
            for (int r = 0; r < N && err == ncclSuccess; ++r)
                if (r != root && rows_of(r) > 0) err = R.Recv(slot(k, r), sh.bytes(k, rows_of(r)), ncclUint8, r, R.comm, sh.s);
        }
    }
    if (err != ncclSuccess) {
        (void)R.GroupEnd();
        return fail(RM_E_RCCL, "ncclSend / ncclRecv failed: %s", R.GetErrorString(err));
    }
    RCCL_TRY(R.GroupEnd());
    if (sh.is_root) {
        for (int k = 0; k < 3; ++k)
            if (d->rows > 0 && slot(k, root) != (const char*)sh.src[k])
                HIP_TRY(hipMemcpyAsync(slot(k, root), sh.src[k], sh.bytes(k, d->rows), hipMemcpyDeviceToDevice, sh.s));
        if (sh.cyclic)
            for (int k = 0; k < 3; ++k)
                if ((rc = assemble(N, H, sh.W, per, 1, kMapBytes[k], R.gather[k].p, sh.dst[k], sh.s))) return rc;
    }
    return RM_OK;
}

int rm_set_queue_capacity(int64_t entries)
{
    if (entries < 0) return fail(RM_E_BAD_ARG, "negative queue capacity");
    std::lock_guard<std::mutex> lk(g_mu);
    g_queue_cap = entries == 0 ? kQueueCapMax : std::min<long long>(entries, 1ll << 30);
    return RM_OK;
}

int rm_set_pass_timing(int enable)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (enable && !g.pev_ready) {
        for (auto& e : g.pev) HIP_TRY(hipEventCreate(&e));
        g.pev_ready = true;
    }
    g.pass_timing = enable != 0;
    g.pass_count = 0;
    return RM_OK;
}

int rm_get_pass_ms(void* stream, int32_t* npasses, float* ms)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!npasses || !ms) return fail(RM_E_BAD_ARG, "NULL output");
    if (!g.pass_timing || !g.pev_ready) return fail(RM_E_BAD_ARG, "pass timing is off (rm_set_pass_timing)");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    *npasses = g.pass_count;
    for (int i = 0; i < g.pass_count; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], g.pev[i], g.pev[i + 1]));
    if (g.last_was_pipeline && g.pass_count == 1 && g.last_stats) {
        // one kernel: split its time at the marks its waves left in the stats block (100 MHz device clock)
        unsigned long long w[rm::kStatsHead];
        HIP_TRY(hipMemcpyAsync(w, g.last_stats, sizeof w, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const unsigned long long start = ~w[rm::kWMarkStart], tiles = ~w[rm::kWMarkTiles];
        if (w[rm::kWMarkStart] != 0 && w[rm::kWMarkTiles] != 0 && tiles >= start && w[rm::kWMarkFresh] >= tiles &&
            w[rm::kWMarkProd] >= w[rm::kWMarkFresh]) {
            const float total = ms[0];
            const float t_tiles = (float)((double)(tiles - start) * 1e-5);
            const float fresh = (float)((double)(w[rm::kWMarkFresh] - start) * 1e-5);
            const float prod = (float)((double)(w[rm::kWMarkProd] - start) * 1e-5);
            ms[0] = t_tiles; ms[1] = fresh - t_tiles; ms[2] = prod - fresh; ms[3] = std::max(0.f, total - prod);
            *npasses = 4;
            // times of the last push into / pop out of queue 1 since launch, for tools (rm_last_queue_marks)
            g.last_push_ms = w[rm::kWMarkPush] >= start ? (float)((double)(w[rm::kWMarkPush] - start) * 1e-5) : 0.f;
            g.last_pop_ms = w[rm::kWMarkPop] >= start ? (float)((double)(w[rm::kWMarkPop] - start) * 1e-5) : 0.f;
            g.long_marks[0] = w[rm::kWLongPushMin] ? (float)((double)(~w[rm::kWLongPushMin]) * 1e-5) : 0.f;
            g.long_marks[1] = (float)((double)w[rm::kWLongPushMax] * 1e-5);
            g.long_marks[2] = w[rm::kWLongTeamMin] ? (float)((double)(~w[rm::kWLongTeamMin]) * 1e-5) : 0.f;
            g.long_marks[3] = (float)((double)w[rm::kWLongTeamMax] * 1e-5);
        }
    }
    return RM_OK;
}

int rm_last_queue_marks(float* last_push_ms, float* last_pop_ms)
{
    if (!last_push_ms || !last_pop_ms) return fail(RM_E_BAD_ARG, "NULL output");
    std::lock_guard<std::mutex> lk(g_mu);
    *last_push_ms = g.last_push_ms;
    *last_pop_ms = g.last_pop_ms;
    return RM_OK;
}

int rm_long_ray_marks(float ms[4])
{
    if (!ms) return fail(RM_E_BAD_ARG, "NULL output");
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < 4; ++i) ms[i] = g.long_marks[i];
    return RM_OK;
}

int rm_render_batch(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                    float* depth, int32_t* iters, uint8_t* hit, RmStats* stats, float* ms_total)
{
    RmOutputs o;
    memset(&o, 0, sizeof o);
    o.depth = depth; o.iters = iters; o.hit = hit;
    return rm_render_batch_outputs(shape, nframes, cams, configs, &o, stats, ms_total);
}

int rm_alloc_frame(int32_t width, int32_t rows, void** d_depth, void** d_iters, void** d_hit)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (width <= 0 || rows <= 0 || !d_depth || !d_iters || !d_hit) return fail(RM_E_BAD_ARG, "bad arguments");
    const size_t n = (size_t)width * rows;
    HIP_TRY(hipMalloc(d_depth, n * 4));
    HIP_TRY(hipMalloc(d_iters, n * 4));
    HIP_TRY(hipMalloc(d_hit, n));
    return RM_OK;
}

int rm_free_frame(void* d_depth, void* d_iters, void* d_hit)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (d_depth) HIP_TRY(hipFree(d_depth));
    if (d_iters) HIP_TRY(hipFree(d_iters));
    if (d_hit) HIP_TRY(hipFree(d_hit));
    return RM_OK;
}

int rm_copy_frame_to_host(int32_t width, int32_t rows, const void* d_depth, const void* d_iters, const void* d_hit,
                          float* depth, int32_t* iters, uint8_t* hit)
{
    Entry e;
    if (e.rc()) return e.rc();
    const size_t n = (size_t)width * rows;
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (depth) HIP_TRY(hipMemcpy(depth, d_depth, n * 4, hipMemcpyDeviceToHost));
    if (iters) HIP_TRY(hipMemcpy(iters, d_iters, n * 4, hipMemcpyDeviceToHost));
    if (hit) HIP_TRY(hipMemcpy(hit, d_hit, n, hipMemcpyDeviceToHost));
    return RM_OK;
}

int rm_debug_poison_queues(uint32_t word_offset, uint32_t* next_generation)
{
    Entry e;
    if (e.rc()) return e.rc();
    HIP_TRY(hipStreamSynchronize(g.stream));
    uint32_t next = g.generation + 1u;
    if (next == 0) next = 1;
    const uint32_t word = next + word_offset;
    for (int q = 0; q < rm::kQueues; ++q) {
        if (!g.queue[q].p || g.queue[q].cap == 0) continue;
        HIP_TRY(hipMemsetD32((hipDeviceptr_t)g.queue[q].p, (int)word, g.queue[q].cap / 4));
        g.qkey[q].writer = 3;                 // somebody else's layout: the next single launch must clear what it will poll
        g.qkey[q].used = g.queue[q].cap;
    }
    HIP_TRY(hipDeviceSynchronize());
    if (next_generation) *next_generation = next;
    return RM_OK;
}

int rm_debug_set_trace(int enable)
{
    Entry e;
    if (e.rc()) return e.rc();
    g.tracing = enable != 0;
    return RM_OK;
}

int rm_debug_get_trace(uint32_t* records, int64_t max_records, int64_t* nrecords, uint32_t* start_ticks, uint32_t* detach_ticks,
                       int64_t npix, uint32_t* launch_tick)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (!nrecords) return fail(RM_E_BAD_ARG, "nrecords is NULL");
    HIP_TRY(hipDeviceSynchronize());
    if (!g.trace.p || !g.last_stats) return fail(RM_E_BAD_ARG, "no traced single-launch frame (rm_debug_set_trace, then render)");
    uint32_t head[8];
    HIP_TRY(hipMemcpy(head, g.trace.p, sizeof head, hipMemcpyDeviceToHost));
    const int64_t n = std::min<int64_t>(head[0], 1 << 20);
    *nrecords = n;
    if (records && max_records > 0)
        HIP_TRY(hipMemcpy(records, (const uint32_t*)g.trace.p + 8, (size_t)std::min<int64_t>(n, max_records) * 32, hipMemcpyDeviceToHost));
    const size_t np = std::min<size_t>((size_t)std::max<int64_t>(npix, 0), g.trace_pix);
    if (start_ticks && np) HIP_TRY(hipMemcpy(start_ticks, g.trace_start.p, np * 4, hipMemcpyDeviceToHost));
    if (detach_ticks && np) HIP_TRY(hipMemcpy(detach_ticks, g.trace_detach.p, np * 4, hipMemcpyDeviceToHost));
    if (launch_tick) {
        unsigned long long w[rm::kStatsHead];
        HIP_TRY(hipMemcpy(w, g.last_stats, sizeof w, hipMemcpyDeviceToHost));
        *launch_tick = (uint32_t)(~w[rm::kWMarkStart]);
    }
    return RM_OK;
}

int rm_runtime_info(RmRuntimeInfo* out)
{
    if (!out) return fail(RM_E_BAD_ARG, "out is NULL");
    memset(out, 0, sizeof *out);
    // the address our own calls resolve to (a GOT entry in position-independent code), then the object that holds it
    Dl_info info;
    memset(&info, 0, sizeof info);
    void* const fn = reinterpret_cast<void*>(&hipStreamCreateWithFlags);
    if (dladdr(fn, &info) && info.dli_fname) snprintf(out->hip_runtime_path, sizeof out->hip_runtime_path, "%s", info.dli_fname);
    const HipCopies c = hip_runtimes_loaded();
    out->hip_runtimes_loaded = c.count;
    snprintf(out->other_runtime_path, sizeof out->other_runtime_path, "%s", c.other);
    int v = 0;
    if (hipRuntimeGetVersion(&v) == hipSuccess) out->hip_runtime_version = v;
    v = 0;
    if (hipDriverGetVersion(&v) == hipSuccess) out->hip_driver_version = v;
    return RM_OK;
}

int rm_stream_create(void** stream)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (!stream) return fail(RM_E_BAD_ARG, "stream is NULL");
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    g_own_streams.push_back((void*)s);
    *stream = (void*)s;
    return RM_OK;
}

int rm_stream_synchronize(void* stream)
{
    hipStream_t s;
    {
        Entry e;
        int rc = e.rc();
        if (rc || (rc = e.stream(stream, &s))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));      // outside the lock: other threads may enqueue while this one waits
    return RM_OK;
}

int rm_stream_destroy(void* stream)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!stream) return RM_OK;
    if ((rc = check_stream(stream))) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (g.frame_ev_valid && g.frame_stream == (hipStream_t)stream) g.frame_stream = nullptr;   // its last frame has completed
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    g_own_streams.erase(std::remove(g_own_streams.begin(), g_own_streams.end(), stream), g_own_streams.end());
    g_seen_streams.erase(std::remove(g_seen_streams.begin(), g_seen_streams.end(), stream), g_seen_streams.end());
    return RM_OK;
}

int rm_bench_store_path(int32_t width, int32_t rows, void* d_depth, void* d_iters, void* d_hit, RmTiming* t)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (width <= 0 || rows <= 0 || !d_depth || !d_iters || !d_hit || !t) return fail(RM_E_BAD_ARG, "bad arguments");
    const int tiles_x = (width + 63) / 64, tiles_y = (rows + 3) / 4;
    const int ntiles = tiles_x * tiles_y;
    const int grid = std::min(ntiles, g.prop.multiProcessorCount * 32);
    return timed(e, t, g.stream, [&] {
        hipLaunchKernelGGL(store_path_kernel, dim3(grid), dim3(64), 0, g.stream, (float*)d_depth, (int32_t*)d_iters,
                           (uint8_t*)d_hit, width, rows, tiles_x, ntiles);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
}

// ---- capture on the device: hit normals and shading (rm_capture.h, capture_kernel) ------------------------------------

int rm_capture(const RmFrameDesc* d, const RmCaptureOutputs* o, RmStats* stats, RmTiming* timing)
{
    if (!d || !o) return fail(RM_E_BAD_ARG, "desc or out is NULL");
    if (!o->hit) return fail(RM_E_BAD_ARG, "hit is required");
    if (!d->march.full) return fail(RM_E_BAD_ARG, "rm_capture requires march.full = 1 (final_sdf is part of geom)");
    if (d->band_rows > 0 && d->band_stride > 1) return fail(RM_E_BAD_ARG, "rm_capture takes no band-cyclic slice");
    int rc = check_desc(d);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const size_t n = (size_t)d->rows * (size_t)d->width;
    // the march's outputs stay in the workspace; only the float maps the caller asked for (and hit) are staged back
    Staged st(e);
    float* d_depth = st.scratch<float>(g.depth, n * 4, 16);
    int32_t* d_iters = st.scratch<int32_t>(g.iters, n * 4, 16);
    double* d_traw = st.scratch<double>(g.traw, n * 8, 16);
    double* d_fs = st.scratch<double>(g.fs, n * 8, 16);
    int32_t* d_evals = st.scratch<int32_t>(g.evals, n * 4, 16);
    uint8_t* d_hit = st.out(g.hit, o->hit, n, 16);
    rm::CaptureArgs c;
    memset(&c, 0, sizeof c);
    c.geom = st.out(g.cap_out[0], o->geom, n * 16);
    c.normal = st.out(g.cap_out[1], o->normal, n * 12);
    c.depth = st.out(g.cap_out[2], o->depth, n * 4);
    c.color = st.out(g.cap_out[3], o->color, n * 12);
    c.evals_f = st.out(g.cap_out[4], o->evals, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, d_depth, d_iters, d_hit, d_traw, d_fs, nullptr, (unsigned long long*)g.stats.p, &a))) return rc;
    a.evals = d_evals;
    c.cam = a.single.cam;
    c.width = d->width; c.height = d->height; c.row0 = d->row0; c.rows = d->rows;
    c.max_iterations = d->march.max_iterations; c.max_distance = d->march.max_distance;
    c.hit = d_hit; c.t = a.t_raw; c.iters = a.iters; c.final_sdf = a.final_sdf; c.evals = a.evals;
    c.scene_data = a.scene_data;
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    rc = once_or_timed(e, timing, g.stream, [&] {
        if (int rc1 = launch(d, p, a, g.stream)) return rc1;
        HIP_TRY(sc->capture(c, 1, g.stream));
        return (int)RM_OK;
    });
    if (rc || (rc = st.download())) return rc;
    return read_stats(e, g.stats.p, g.stream, stats);
}

int rm_shade_frames(int scene_id, int32_t width, int32_t height, int32_t nframes, const double* cams, const double* t,
                    const float* depth, const uint8_t* hit, float* normal, float* color, RmTiming* timing)
{
    if (!cams || !hit || !normal || !color) return fail(RM_E_BAD_ARG, "cams, hit, normal or color is NULL");
    if (!t == !depth) return fail(RM_E_BAD_ARG, "exactly one of t and depth must be given");
    if (nframes < 1 || nframes > 65535) return fail(RM_E_BAD_ARG, "nframes %d outside [1, 65535]", nframes);
    if (width <= 0 || height <= 0) return fail(RM_E_BAD_DIMS, "bad frame shape %dx%d", width, height);
    if ((long long)width * height * nframes > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "frames too large");
    int rc = check_scene(scene_id);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    const size_t npix = (size_t)width * (size_t)height, n = npix * (size_t)nframes;
    for (size_t i = 0; i < n; ++i) {      // the libm restatements are unclaimed for NaN arguments
        if (!hit[i]) continue;
        const double v = t ? t[i] : (double)depth[i];
        if (!(v - v == 0.0))
            return fail(RM_E_BAD_ARG, "frame %zu, pixel %zu: the depth of a hit is not finite", i / npix, i % npix);
    }
    for (size_t i = 0; i < (size_t)nframes * 14; ++i)
        if (!(cams[i] - cams[i] == 0.0)) return fail(RM_E_BAD_ARG, "camera %zu: field %zu is not finite", i / 14, i % 14);
    Entry e;
    if ((rc = e.rc())) return rc;

    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    Staged st(e);
    rm::CaptureArgs c;
    memset(&c, 0, sizeof c);
    static_assert(sizeof(rm::CameraParams) == 14 * sizeof(double), "cams is an array of CameraParams");
    c.cams = (const rm::CameraParams*)st.in(g.cap_cams, cams, (size_t)nframes * sizeof(rm::CameraParams));
    if (t) c.t = st.in(g.in[0], t, n * 8);
    else c.depth_in = st.in(g.in[0], depth, n * 4);
    c.hit = st.in(g.in[1], hit, n);
    c.normal = st.out(g.cap_out[1], normal, n * 12);
    c.color = st.out(g.cap_out[3], color, n * 12);
    if ((rc = st.begin())) return rc;
    c.width = width; c.height = height; c.row0 = 0; c.rows = height;
    c.max_iterations = 1; c.max_distance = 1.0;
    c.scene_data = data;
    const rm::SceneLaunchers* const sc = launchers(scene_id);
    rc = once_or_timed(e, timing, g.stream, [&] {
        HIP_TRY(sc->capture(c, nframes, g.stream));
        return (int)RM_OK;
    });
    if (rc) return rc;
    return st.finish();
}

}  // extern "C"
