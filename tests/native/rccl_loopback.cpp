// A loop-back stand-in for the nine RCCL symbols librm_hip.so resolves (rm_gather.hip, rccl_load), so that the N > 1
// paths of rm_gather_frame / rm_gather_frame_root run on ONE GPU: one process drives the ranks one after another, each
// with its own rm_comm_init .. rm_comm_destroy.  Named to the library with RM_RCCL_LIBRARY.  Plain C++: host calls of
// the HIP runtime only, no kernels.  tests/test_gpu_loopback_gather.py and tests/test_loopback_host.py build it.
//
// The state is process-wide and outlives ncclCommDestroy:
//   ncclSend      copies the buffer into a parked device allocation, appended to the FIFO (source rank, peer);
//   ncclRecv      pops the head of the FIFO (peer, this rank); an empty FIFO or another byte count is ncclInvalidUsage
//                 with a recorded reason -- it never waits, so a send / receive disagreement that would deadlock real
//                 RCCL is a failed assertion here;
//   ncclAllGather deposits a copy of the send buffer in mailbox (epoch, call index within the group, this rank) and
//                 fills slot r of the receive buffer from mailbox (epoch, index, r), or with the byte 0xA5 where no
//                 rank r has deposited yet; deposits of one index that differ in size are ncclInvalidUsage.
// Data calls outside ncclGroupStart / ncclGroupEnd, a peer outside the world or equal to the caller, and any type but
// ncclUint8 are ncclInvalidUsage: that is all the library uses.
//
// What this cannot show: transport, xGMI, RCCL's own alignment or ordering behaviour, concurrency between ranks.
#include <rccl/rccl.h>
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>

namespace {

struct FakeComm { int world, rank; };
struct Parked { void* dev; size_t n; };

std::mutex mu;
std::map<std::pair<int, int>, std::deque<Parked>> fifo;       // (source rank, destination rank) -> sends not yet received
std::map<std::tuple<int, int, int>, Parked> mailbox;          // (epoch, all-gather index in its group, rank) -> deposit
int group_depth = 0, gather_index = 0, epoch = 0;
unsigned long long counts[6];                                 // calls and bytes of Send, Recv, AllGather
char reason[512] = "";

ncclResult_t refuse(ncclResult_t code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(reason, sizeof reason, fmt, ap);
    va_end(ap);
    return code;
}

#define LB_HIP(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return refuse(ncclUnhandledCudaError, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// a device copy of [src, src + n) made on `stream` and complete on return (the caller reuses its buffer)
ncclResult_t park(const void* src, size_t n, hipStream_t stream, Parked* out)
{
    void* dev = nullptr;
    LB_HIP(hipMalloc(&dev, n ? n : 1));
    hipError_t e = n ? hipMemcpyAsync(dev, src, n, hipMemcpyDeviceToDevice, stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return refuse(ncclUnhandledCudaError, "copy of %zu bytes failed: %s", n, hipGetErrorString(e));
    }
    *out = Parked{ dev, n };
    return ncclSuccess;
}

ncclResult_t usage(const char* call, const void* buf, ncclDataType_t type, ncclComm_t comm, const FakeComm** c)
{
    if (!comm) return refuse(ncclInvalidUsage, "%s: no communicator", call);
    *c = reinterpret_cast<const FakeComm*>(comm);
    if (group_depth <= 0) return refuse(ncclInvalidUsage, "%s on rank %d outside ncclGroupStart / ncclGroupEnd", call, (*c)->rank);
    if (type != ncclUint8) return refuse(ncclInvalidUsage, "%s on rank %d: type %d, not ncclUint8", call, (*c)->rank, (int)type);
    if (!buf) return refuse(ncclInvalidUsage, "%s on rank %d: NULL buffer", call, (*c)->rank);
    return ncclSuccess;
}

ncclResult_t check_peer(const char* call, const FakeComm* c, int peer)
{
    if (peer < 0 || peer >= c->world) return refuse(ncclInvalidUsage, "%s on rank %d: peer %d outside the world of %d", call, c->rank, peer, c->world);
    if (peer == c->rank) return refuse(ncclInvalidUsage, "%s on rank %d: peer %d is the caller", call, c->rank, peer);
    return ncclSuccess;
}

void free_all()
{
    for (auto& kv : fifo)
        for (auto& p : kv.second) (void)hipFree(p.dev);
    for (auto& kv : mailbox) (void)hipFree(kv.second.dev);
    fifo.clear();
    mailbox.clear();
}

}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    if (!id) return ncclInvalidArgument;
    for (int i = 0; i < NCCL_UNIQUE_ID_BYTES; ++i) id->internal[i] = (char)(0x40 + i % 59);
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId, int rank)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return refuse(ncclInvalidArgument, "ncclCommInitRank(%d ranks, rank %d)", nranks, rank);
    *comm = reinterpret_cast<ncclComm_t>(new FakeComm{ nranks, rank });
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    delete reinterpret_cast<FakeComm*>(comm);
    return ncclSuccess;
}

ncclResult_t ncclGroupStart()
{
    std::lock_guard<std::mutex> lk(mu);
    if (group_depth++ == 0) gather_index = 0;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    std::lock_guard<std::mutex> lk(mu);
    if (group_depth <= 0) return refuse(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
    --group_depth;
    return ncclSuccess;
}

ncclResult_t ncclSend(const void* buf, size_t n, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu);
    const FakeComm* c = nullptr;
    ncclResult_t r = usage("ncclSend", buf, type, comm, &c);
    if (r != ncclSuccess || (r = check_peer("ncclSend", c, peer)) != ncclSuccess) return r;
    Parked p;
    if ((r = park(buf, n, stream, &p)) != ncclSuccess) return r;
    fifo[{ c->rank, peer }].push_back(p);
    counts[0] += 1;
    counts[1] += n;
    return ncclSuccess;
}

ncclResult_t ncclRecv(void* buf, size_t n, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu);
    const FakeComm* c = nullptr;
    ncclResult_t r = usage("ncclRecv", buf, type, comm, &c);
    if (r != ncclSuccess || (r = check_peer("ncclRecv", c, peer)) != ncclSuccess) return r;
    auto it = fifo.find({ peer, c->rank });
    if (it == fifo.end() || it->second.empty())
        return refuse(ncclInvalidUsage, "ncclRecv on rank %d: peer %d has sent nothing (real RCCL would wait for ever)", c->rank, peer);
    const Parked p = it->second.front();
    if (p.n != n)
        return refuse(ncclInvalidUsage, "ncclRecv on rank %d: count mismatch, %zu bytes expected from peer %d, which sent %zu", c->rank, n, peer, p.n);
    it->second.pop_front();
    hipError_t e = n ? hipMemcpyAsync(buf, p.dev, n, hipMemcpyDeviceToDevice, stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(p.dev);
    if (e != hipSuccess) return refuse(ncclUnhandledCudaError, "copy of %zu bytes failed: %s", n, hipGetErrorString(e));
    counts[2] += 1;
    counts[3] += n;
    return ncclSuccess;
}

ncclResult_t ncclAllGather(const void* send, void* recv, size_t n, ncclDataType_t type, ncclComm_t comm, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu);
    const FakeComm* c = nullptr;
    ncclResult_t r = usage("ncclAllGather", send, type, comm, &c);
    if (r != ncclSuccess) return r;
    if (!recv) return refuse(ncclInvalidUsage, "ncclAllGather on rank %d: NULL receive buffer", c->rank);
    const int index = gather_index++;
    for (int q = 0; q < c->world; ++q) {
        auto it = mailbox.find({ epoch, index, q });
        if (it != mailbox.end() && it->second.n != n)
            return refuse(ncclInvalidUsage, "ncclAllGather %d on rank %d: count mismatch, %zu bytes here, rank %d deposited %zu", index,
                          c->rank, n, q, it->second.n);
    }
    Parked p;
    if ((r = park(send, n, stream, &p)) != ncclSuccess) return r;
    Parked& mine = mailbox[{ epoch, index, c->rank }];
    if (mine.dev) (void)hipFree(mine.dev);
    mine = p;
    for (int q = 0; q < c->world && n; ++q) {
        char* slot = static_cast<char*>(recv) + (size_t)q * n;
        auto it = mailbox.find({ epoch, index, q });
        if (it != mailbox.end())
            LB_HIP(hipMemcpyAsync(slot, it->second.dev, n, hipMemcpyDeviceToDevice, stream));
        else
            LB_HIP(hipMemsetAsync(slot, 0xA5, n, stream));
    }
    LB_HIP(hipStreamSynchronize(stream));
    counts[4] += 1;
    counts[5] += n;
    return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled HIP error (loop-back stand-in)";
    case ncclInvalidArgument: return "invalid argument (loop-back stand-in)";
    case ncclInvalidUsage: return "invalid usage (loop-back stand-in: lb_last_reason() says which)";
    default: return "error (loop-back stand-in)";
    }
}

// ---- for the tests only -------------------------------------------------------------------------------------

// Free everything parked or deposited; clear the counters, the reason, the epoch and an unbalanced group.
void lb_reset(void)
{
    std::lock_guard<std::mutex> lk(mu);
    free_all();
    memset(counts, 0, sizeof counts);
    reason[0] = 0;
    group_depth = gather_index = epoch = 0;
}

// Sends that were never received.
int lb_pending(void)
{
    std::lock_guard<std::mutex> lk(mu);
    size_t n = 0;
    for (auto& kv : fifo) n += kv.second.size();
    return (int)n;
}

const char* lb_last_reason(void) { return reason; }

// hipMemset: the tests poison device buffers with it (the C ABI of the library has no host-to-device copy).
int lb_fill(void* d, size_t n, int byte)
{
    hipError_t e = hipMemset(d, byte, n);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

// out[0..5]: calls and bytes of ncclSend, of ncclRecv, of ncclAllGather (its send count) that succeeded since lb_reset.
void lb_counts(unsigned long long out[6])
{
    std::lock_guard<std::mutex> lk(mu);
    memcpy(out, counts, sizeof counts);
}

// What rank `rank` handed to all-gather `index` of its group in epoch `e`, copied to the host: its size, or -1 when there
// is no such deposit or it is larger than `cap`.  The padded send buffer of a short shard is seen nowhere else: the
// placement never reads the pad.
long long lb_peek(int e, int index, int rank, void* host, size_t cap)
{
    std::lock_guard<std::mutex> lk(mu);
    auto it = mailbox.find({ e, index, rank });
    if (it == mailbox.end() || it->second.n > cap) return -1;
    if (hipMemcpy(host, it->second.dev, it->second.n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long long)it->second.n;
}

// The all-gather mailboxes are keyed by this number too, so that the deposits of several frames of different sizes can
// be made before the one rank that stays open gathers them in turn (0 after lb_reset).
void lb_epoch(int e)
{
    std::lock_guard<std::mutex> lk(mu);
    epoch = e;
}

}  // extern "C"
