// rm_gather.hip -- the frame exchange between the GPUs of a run: RCCL, loaded on first use, the kernel that puts the
// gathered shards' rows into image order, and the entry points of the C ABI (include/rm_hip.h) rm_shard_rows, rm_comm_*,
// rm_assemble_frame and rm_gather_frame*.  Lock, device and streams come from rm_capi.hip through rm_capi_internal.h.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is loaded with dlopen on first use

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/rm_hip.h"
#include "rm_capi_internal.h"

using namespace rm::capi;

namespace {

Buf* g_comm_bufs = nullptr;        // freed with the communicator
struct CommBuf : Buf { CommBuf() : Buf(g_comm_bufs) {} };

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
    // the session's communicator: closed by rm_comm_destroy, and by rm_shutdown where the caller did not
    struct Comm final : SessionItem {
        ncclComm_t comm = nullptr;
        int world = 0, rank = -1;
        ncclResult_t close();
        void end() override { (void)close(); }
    };
    CommBuf gather[3], pad[3];  // all-gather landing buffers (rank-major) and padded send buffers of a short last shard
} R;
Rccl::Comm g_comm;

ncclResult_t Rccl::Comm::close()
{
    if (!comm) return ncclSuccess;
    const ncclResult_t r = R.CommDestroy(comm);
    comm = nullptr;
    world = 0; rank = -1;
    for (Buf* b = g_comm_bufs; b; b = b->next) b->release();
    return r;
}

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

}  // namespace

extern "C" {

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
    Lock lk;
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
    if (g_comm.comm) return fail(RM_E_BAD_ARG, "a communicator exists already; call rm_comm_destroy() first");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCL_TRY(R.CommInitRank(&g_comm.comm, world_size, u, rank));
    g_comm.world = world_size;
    g_comm.rank = rank;
    return RM_OK;
}

int rm_comm_destroy(void)
{
    Lock lk;
    if (!g_comm.comm) return RM_OK;
    if (lk.select_device()) (void)hipDeviceSynchronize();
    const ncclResult_t r = g_comm.close();
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
    const int N = g_comm.world, H = d->height;
    sh->cyclic = d->band_rows > 0 && d->band_stride > 1;
    if (sh->cyclic) {
        if (d->band_rows != 4 || d->band_stride != N || d->band_offset != g_comm.rank || d->row0 != 0 || H % (4 * N) != 0 || d->rows != H / N)
            return fail(RM_E_BAD_DIMS, "band-cyclic shard does not match the communicator (4-row bands, stride = world size %d, "
                                       "offset = rank %d, rows = height / world size)", N, g_comm.rank);
        sh->per = d->rows;
    } else {
        sh->per = N == 1 ? H : rm_shard_rows(H, N);
        const int r0 = std::min(g_comm.rank * sh->per, H), r1 = std::min((g_comm.rank + 1) * sh->per, H);
        if (d->row0 != r0 || d->rows != r1 - r0)
            return fail(RM_E_BAD_DIMS, "contiguous shard of rank %d must be rows [%d, %d)", g_comm.rank, r0, r1);
    }
    return RM_OK;
}

// After the descriptor and the shard pointers have been checked: the communicator, the root (`root` only counts with
// to_root; without it every rank receives the frame), the stream, the plan.
static int shard_open(const Entry& e, const RmFrameDesc* d, const void* d_depth, const void* d_iters, const void* d_hit, void* d_full_depth,
                      void* d_full_iters, void* d_full_hit, bool to_root, int root, void* stream, Shard* sh)
{
    if (!g_comm.comm) return fail(RM_E_RCCL, "no communicator: call rm_comm_init() first");
    *sh = Shard{ nullptr, g_comm.world, d->height, d->width, 0, false, true, { d_depth, d_iters, d_hit }, { d_full_depth, d_full_iters, d_full_hit } };
    if (to_root) {
        if (root < 0 || root >= g_comm.world) return fail(RM_E_BAD_ARG, "root %d outside the communicator of %d", root, g_comm.world);
        sh->is_root = g_comm.rank == root;
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
        const ncclResult_t r = R.AllGather(send[k], R.gather[k].p, sh.bytes(k, sh.per), ncclUint8, g_comm.comm, sh.s);
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
            if (d->rows > 0) err = R.Send(sh.src[k], sh.bytes(k, d->rows), ncclUint8, root, g_comm.comm, sh.s);
        } else {
            for (int r = 0; r < N && err == ncclSuccess; ++r)
                if (r != root && rows_of(r) > 0) err = R.Recv(slot(k, r), sh.bytes(k, rows_of(r)), ncclUint8, r, g_comm.comm, sh.s);
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

}  // extern "C"
