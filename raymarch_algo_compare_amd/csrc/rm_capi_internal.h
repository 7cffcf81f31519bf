// rm_capi_internal.h -- what the entry points of the C ABI (include/rm_hip.h) share.  Host only.
//
// The entry points of a subsystem sit below its kernels -- the march's host side in rm_frame.hip, the RCCL exchange in
// rm_gather.hip, the analysis calls in rm_interval.hip ... rm_math_check.hip -- and reach the library's lock, device,
// stream, staging and timing through this header.  rm_capi.hip defines what is declared here, except check_desc and
// frame_stream_destroyed (rm_frame.hip) and the interval oracle's part at the end (rm_interval.hip), and keeps the
// session to itself.  What a unit makes or remembers for one rm_init .. rm_shutdown life it declares as a SessionItem
// next to the code that uses it; rm_shutdown walks those, as it walks the workspace buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <optional>

#include "../../include/rm_hip.h"

namespace rm {

struct CameraParams; struct IntervalParams; struct ProgramImage; struct SceneLaunchers;

namespace capi {

int fail(int code, const char* fmt, ...);      // sets the calling thread's rm_last_error() text, returns `code`

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::rm::capi::fail(RM_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// A grow-only device buffer.  Every Buf links itself into its owner's list when it is constructed, so "free all the
// device memory this owner holds" is a walk of that list (release_all): a new buffer needs no second edit anywhere.
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf* const next;
    explicit Buf(Buf*& owner) : next(owner) { owner = this; }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return RM_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(RM_E_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        cap = bytes;
        return RM_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

// The workspace's list, freed by rm_shutdown.  The head is a constant-initialised pointer, so a WsBuf constructed during
// any translation unit's dynamic initialisation links itself into a valid list: a subsystem declares its buffers as
// file-local WsBuf objects next to the entry point that uses them, and rm_shutdown's walk frees them with the rest.
extern Buf* g_workspace_bufs;
struct WsBuf : Buf { WsBuf() : Buf(g_workspace_bufs) {} };

// What belongs to one rm_init .. rm_shutdown life of the library, the device memory aside: events and streams made on
// first use, and host state that describes the session.  Like a Buf, every item links itself into a constant-initialised
// list when it is constructed, and rm_shutdown ends them all in one walk (the device selected and run dry, in no
// particular order): a unit that adds one needs no edit outside itself.
struct SessionItem {
    SessionItem* const next;
    SessionItem() : next(head) { head = this; }
    SessionItem(const SessionItem&) = delete;
    SessionItem& operator=(const SessionItem&) = delete;
    virtual void end() = 0;      // destroy what was made, forget what was remembered
    static SessionItem* head;     // constant-initialised: valid during any translation unit's dynamic initialisation
protected:
    ~SessionItem() = default;
};

// N events, created together by the first ensure().
template <int N>
struct Events final : SessionItem {
    hipEvent_t e[N] = {};
    const unsigned flags;
    bool made = false;
    explicit Events(unsigned flags_ = hipEventDefault) : flags(flags_) {}
    hipEvent_t operator[](int i) const { return e[i]; }
    int ensure()
    {
        if (made) return RM_OK;
        for (auto& x : e)
            if (!x) HIP_TRY(hipEventCreateWithFlags(&x, flags));
        made = true;
        return RM_OK;
    }
    void end() override
    {
        for (auto& x : e)
            if (x) { (void)hipEventDestroy(x); x = nullptr; }
        made = false;
    }
};

// A non-blocking stream of the library's own, created by the first ensure().
struct SideStream final : SessionItem {
    hipStream_t s = nullptr;
    int ensure()
    {
        if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return RM_OK;
    }
    void end() override
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};

// Host state of the session: the members of T start again from their initialisers, so a new member needs no line.
template <class T>
struct PerSession final : SessionItem, T {
    void end() override { static_cast<T&>(*this) = T(); }
};

hipStream_t lib_stream();                            // the library's own stream (valid while an Entry's rc() is RM_OK)
const hipDeviceProp_t& device_prop();                // ... and the device's properties
extern WsBuf (&stage_in)[2], (&stage_out)[4];        // staging of the per-point / per-ray calls (Staged)

// An entry point's way to the workspace and the device.  Constructing one takes the library's lock, refuses a library
// without a device (RM_E_NO_DEVICE) and selects the device, in that order; while rc() is RM_OK the lock is held until the
// Entry goes out of scope.  Whatever enqueues on the workspace (Staged, once_or_timed, interval_program) asks for an
// Entry, so it cannot be reached without the lock held and the device selected.
class Entry {
public:
    Entry();
    int rc() const { return rc_; }
    // The stream a call enqueues on: the caller's (checked) or, for NULL, the library's own.
    int stream(void* users, hipStream_t* s) const;

private:
    std::unique_lock<std::mutex> lk_;
    int rc_;
};

// The lock alone, for the calls that touch the library's state without a device.
class Lock {
public:
    Lock();
    bool select_device() const;      // false: the library has no device (nothing selected)

private:
    std::lock_guard<std::mutex> lk_;
};

// The staging of a call that takes host arrays and returns host arrays: inputs and outputs are declared with the
// workspace buffer that carries them (every `ensure` happens here, before anything is enqueued; scratch() sizes a
// buffer that is not copied), begin() reports an allocation failure or enqueues the uploads, download() enqueues the
// copies back in declaration order and finish() waits for them.  A NULL host output is an optional one the caller did
// not ask for: nothing is allocated or copied and its device pointer is NULL.  Everything runs on the library's stream.
class Staged {
public:
    explicit Staged(const Entry&) {}
    template <class T>
    const T* in(Buf& b, const T* host, size_t bytes)
    {
        return (const T*)add(b, const_cast<T*>(host), bytes, 0, true);
    }
    template <class T>
    T* out(Buf& b, T* host, size_t bytes, size_t slack = 0)
    {
        return host ? (T*)add(b, host, bytes, slack, false) : nullptr;
    }
    // a buffer the call's kernels hand to each other: sized here like every other one, never copied
    template <class T>
    T* scratch(Buf& b, size_t bytes, size_t slack = 0)
    {
        if (rc_ || (rc_ = b.ensure(bytes + slack))) return nullptr;
        return (T*)b.p;
    }
    int begin()
    {
        if (rc_) return rc_;
        for (int i = 0; i < n_; ++i)
            if (v_[i].upload) HIP_TRY(hipMemcpyAsync(v_[i].dev, v_[i].host, v_[i].bytes, hipMemcpyHostToDevice, lib_stream()));
        return RM_OK;
    }
    int download()
    {
        for (int i = 0; i < n_; ++i)
            if (!v_[i].upload && v_[i].bytes) HIP_TRY(hipMemcpyAsync(v_[i].host, v_[i].dev, v_[i].bytes, hipMemcpyDeviceToHost, lib_stream()));
        return RM_OK;
    }
    int finish()
    {
        if (int rc = download()) return rc;
        HIP_TRY(hipStreamSynchronize(lib_stream()));
        return RM_OK;
    }

private:
    void* add(Buf& b, void* host, size_t bytes, size_t slack, bool upload)
    {
        if (rc_) return nullptr;
        if (n_ == kMax) { rc_ = fail(RM_E_BAD_ARG, "more than %d staged arrays", kMax); return nullptr; }
        if ((rc_ = b.ensure(bytes + slack))) return nullptr;
        v_[n_++] = { host, b.p, bytes, upload };
        return b.p;
    }
    static constexpr int kMax = 8;
    struct Array { void* host; void* dev; size_t bytes; bool upload; } v_[kMax];
    int n_ = 0, rc_ = RM_OK;
};

int check_timing(const RmTiming* t);
// `once` (one enqueue on `s`, returning an RM_ code) warmup + repeats times, every timed run bracketed by events on `s`:
// waits for the stream and fills ms_each and the summary of `t`.  once_or_timed: `once` alone when no timing was asked for.
int timed(const Entry&, RmTiming* t, hipStream_t s, const std::function<int()>& once);
inline int once_or_timed(const Entry& e, RmTiming* t, hipStream_t s, const std::function<int()>& once) { return t ? timed(e, t, s, once) : once(); }

int check_slice(const RmFrameDesc* d, bool band_cyclic);
int check_desc(const RmFrameDesc* d);               // every field of a frame descriptor (rm_frame.hip)
void frame_stream_destroyed(hipStream_t s);          // rm_stream_destroy tells the frame engine, which remembers the latest frame's stream
int check_scene(int id);
int scene_data(int id, const void** data);
// The sdf_eval launcher of scene `id` (check_scene has accepted it; under the lock).  Not its whole SceneLaunchers:
// rm_kernels.h puts the libm tables of the kernels compiled after it into LDS, which rm_features.hip's do not fill.
// The kernels of scene `id` (check_scene has accepted it; under the lock), for the units that include rm_kernels.h.
const SceneLaunchers* launchers(int id);
using SdfEval = hipError_t (*)(const double* xyz, size_t n, double* out, const void* scene_data, hipStream_t s);
SdfEval sdf_eval_of(int id);
inline bool is_program_id(int id) { return id >= RM_SCENE_PROGRAM_BASE; }
bool program_exists(int id, bool* ext = nullptr);
int no_such_program(int id);
// Calls `look` with the host image of the registered program `id` while the registry's lock is held (the image must
// not be kept); false when no such program exists.
bool with_program_image(int id, const std::function<void(const ProgramImage&)>& look);
CameraParams camera_of(const double* cam14);
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- rm_interval.hip: the scenes, the march constants and the call head that the five sound tracers share -----------------
const ProgramImage* interval_catalogue_image(int id);
int interval_check_scene(int id);
int interval_params(int id, const RmIntervalConfig* cfg, IntervalParams* P);
int interval_program(const Entry&, int id, const void** prog);

// The common head of the rm_interval_* / rm_segment_* calls, in the order every one of them checks: the scene, the
// call's configuration (`resolve`, an RM_ code), for a render its slice `d` and `timing`, then the Entry, nothing to do
// for n == 0, the required buffers (`have`, else `missing` is the error) and the device image of the program.  After
// RM_OK `prog` is NULL exactly when n == 0.
struct SoundCall {
    std::optional<Entry> e;
    const void* prog = nullptr;
    template <class Resolve>
    int open(int scene_id, Resolve resolve, const RmFrameDesc* d, const RmTiming* timing, size_t n, bool have, const char* missing)
    {
        int rc = interval_check_scene(scene_id);
        if (rc || (rc = resolve())) return rc;
        if (d && (rc = check_slice(d, false))) return rc;       // not check_desc: most of its fields mean nothing here
        if (timing && (rc = check_timing(timing))) return rc;
        e.emplace();
        if ((rc = e->rc()) || n == 0) return rc;
        if (!have) return fail(RM_E_BAD_ARG, "%s", missing);
        return interval_program(*e, scene_id, &prog);
    }
};

inline int no_config() { return RM_OK; }

}  // namespace capi
}  // namespace rm
