// rm_capi.hip -- host side of librm_hip.so: the C ABI declared in include/rm_hip.h.
//
// Owns the device selection, one HIP stream, a grow-only device workspace and the
// (scene, strategy) -> kernel dispatch.  No CPU implementation of the path exists in
// this library: without a usable gfx950 device every entry point returns an error.
//
// What is here is the library's core: the error text, the scene dispatch table and the program registry, the lock
// and the Entry that every call takes, init and shutdown, the streams, timed(), and the frame buffers handed to callers.
// Everything else sits below its kernels and reaches the core through rm_capi_internal.h: the march's host side -- frames,
// batches, rays, capture, pass timing and the debug trace -- in rm_frame.hip, the RCCL exchange in rm_gather.hip, the
// analysis subsystems in rm_interval.hip ... rm_math_check.hip.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <link.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/rm_hip.h"
#include "rm_kernels.h"
#include "rm_scene_program.h"
#include "rm_capi_internal.h"

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
// this file's own state and helpers in the unnamed namespace.
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

Buf* rm::capi::g_workspace_bufs = nullptr;                  // freed by rm_shutdown
SessionItem* rm::capi::SessionItem::head = nullptr;         // ended by rm_shutdown

namespace {

// The device the library is bound to between rm_init and rm_shutdown, which assigns a fresh Session.
struct Session {
    bool ready = false;
    int device = -1;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
} g;

WsBuf g_in[2], g_out[4];      // staging of the per-point / per-ray calls (Staged)
std::mutex g_mu;

}  // namespace

hipStream_t rm::capi::lib_stream() { return g.stream; }
const hipDeviceProp_t& rm::capi::device_prop() { return g.prop; }
WsBuf (&rm::capi::stage_in)[2] = g_in;
WsBuf (&rm::capi::stage_out)[4] = g_out;

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
const rm::SceneLaunchers* launchers(int id)
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
// The streams of this session (guarded by g_mu): those handed out by rm_stream_create, which rm_shutdown runs dry,
// destroys and forgets, and the callers' own that check_stream has accepted.
struct Streams final : SessionItem {
    std::vector<void*> own, seen;
    void end() override
    {
        for (void* s : own) {
            (void)hipStreamSynchronize((hipStream_t)s);
            (void)hipStreamDestroy((hipStream_t)s);
        }
        own.clear();
        seen.clear();
    }
} g_streams;
int check_stream(void* stream)
{
    if (!stream) return RM_OK;
    for (void* p : g_streams.own) if (p == stream) return RM_OK;
    for (void* p : g_streams.seen) if (p == stream) return RM_OK;
    const HipCopies c = hip_runtimes_loaded();
    if (c.count > 1)
        return fail(RM_E_BAD_ARG, "stream %p was not made by rm_stream_create, and this process holds %d copies of the HIP runtime "
                                  "(also %s): a stream of another copy cannot be used here.  Create the stream with rm_stream_create, or "
                                  "load the other runtime's owner (e.g. import torch) BEFORE this library so both share one runtime "
                                  "(rm_runtime_info)", stream, c.count, c.other);
    if (g_streams.seen.size() < 4096) g_streams.seen.push_back(stream);
    return RM_OK;
}

int select_device()
{
    HIP_TRY(hipSetDevice(g.device));
    return RM_OK;
}

}  // namespace

namespace rm::capi {

Lock::Lock() : lk_(g_mu) {}
bool Lock::select_device() const { return g.ready && hipSetDevice(g.device) == hipSuccess; }

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

Events<2 * RM_MAX_TIMED> g_ev;      // timed(): a pair around every timed run

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
    if (rc || (rc = g_ev.ensure())) return rc;
    for (int i = 0; i < t->warmup; ++i)
        if ((rc = once())) return rc;
    for (int i = 0; i < t->repeats; ++i) {
        HIP_TRY(hipEventRecord(g_ev[2 * i], s));
        if ((rc = once())) return rc;
        HIP_TRY(hipEventRecord(g_ev[2 * i + 1], s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < t->repeats; ++i) HIP_TRY(hipEventElapsedTime(&t->ms_each[i], g_ev[2 * i], g_ev[2 * i + 1]));
    summarise(t);
    return RM_OK;
}

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
    g.device = device_id;
    g.ready = true;
    return RM_OK;
}

void rm_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g.ready) return;
    (void)hipSetDevice(g.device);
    // Every stream runs dry first -- the library's, its side streams, the callers' -- so the walks below may end events,
    // streams and buffers in any order (freeing the first workspace buffer would wait for the device anyway).
    (void)hipDeviceSynchronize();
    for (SessionItem* i = SessionItem::head; i; i = i->next) i->end();
    for (Buf* b = g_workspace_bufs; b; b = b->next) b->release();
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
    g = Session();       // not ready, no device
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

int rm_alloc_frame(int32_t width, int32_t rows, void** d_depth, void** d_iters, void** d_hit)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (width <= 0 || rows <= 0 || !d_depth || !d_iters || !d_hit) return fail(RM_E_BAD_ARG, "bad arguments");
    const size_t n = (size_t)width * rows;
    void** const out[3] = { d_depth, d_iters, d_hit };
    const size_t bytes[3] = { n * 4, n * 4, n };
    for (int k = 0; k < 3; ++k) {
        const hipError_t err = hipMalloc(out[k], bytes[k]);
        if (err == hipSuccess) continue;
        for (int j = 0; j < k; ++j) {           // nothing of a frame that cannot be had is kept
            (void)hipFree(*out[j]);
            *out[j] = nullptr;
        }
        return fail(RM_E_HIP, "hipMalloc(%zu) failed: %s", bytes[k], hipGetErrorString(err));
    }
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
    g_streams.own.push_back((void*)s);
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
    frame_stream_destroyed((hipStream_t)stream);
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    for (auto* v : { &g_streams.own, &g_streams.seen }) v->erase(std::remove(v->begin(), v->end(), stream), v->end());
    return RM_OK;
}

}  // extern "C"
