// rm_strategy_program.h -- user-defined marching strategies: a jump-free register program (RmStrategyOp, include/rm_hip.h),
// validated and encoded on the host (strategy_encode), run once per SDF evaluation by an interpreter with the contract of
// the structs of rm_strategies.h (StratProgram: start / step / res), so it drops into render_kernel and march_rays_kernel
// as they stand and march_one<Scene, StratProgram> compiles for the host as well.
//
// Where things live on the device.  The launch passes the device copy of its StrategyImage (KernelArgs.strategy_data);
// the kernel's prologue copies it into LDS next to the libm tables and a scene program's image (rm_load_strategy_data,
// rm_kernels.h).  Every instruction word is read at a wave-uniform address and moved to a scalar register
// (readfirstlane): opcode dispatch and operand selection are scalar branches.  The 16 state registers and 16 temporaries
// of a ray are one LDS array indexed [register][thread] -- the register number is wave-uniform, so an access is one
// ds_read_b64 / ds_write_b64 at a uniform row and the lane's own column, free of bank conflicts; no private array is
// indexed at run time and nothing goes to scratch.  The array is the kernel's dynamic LDS, sized by the launch for the
// workgroup it starts (sp_register_bytes: 64 KiB for render_kernel's 256 threads, 16 KiB for march_rays_kernel's 64).
// The strategy record itself (what a lane keeps in VGPRs between two evaluations) is te, the phase, the evaluation
// count and the result.  A lane owns its column for the life of the
// kernel, so the state survives lane refill and start() zeroes it for the next ray.
//
// No jumps: a block is a straight line, conditionals are selects, so a block's cost is its length and a wave runs a
// block once for all its lanes in that phase.  A step runs the block of each phase some lane of the wave is in (a
// wave-uniform test skips the others) with the other lanes masked off.
//
// The evaluation budget (sp_budget) bounds every ray whatever the program does: see include/rm_hip.h.
#pragma once

#include "../../include/rm_hip.h"
#include "rm_strategies.h"

#include <stdio.h>
#include <string.h>

namespace rm {

constexpr int kSpMaxOps = RM_STRATEGY_PROGRAM_MAX_OPS;
constexpr int kSpMaxConst = RM_STRATEGY_PROGRAM_MAX_CONSTANTS;
constexpr int kSpRegs = RM_STRATEGY_PROGRAM_MAX_STATE + RM_STRATEGY_PROGRAM_MAX_TEMPS;      // s0..s15, t0..t15
constexpr int kSpBlocks = 1 + RM_STRATEGY_PROGRAM_MAX_PHASES;                               // init, phase 0..7
constexpr int kSpConstBase = 64;       // encoded operand of constant i: kSpConstBase + i
// dynamic LDS a launch of `threads` threads per workgroup must pass: the rays' registers, [kSpRegs][threads] doubles
constexpr size_t sp_register_bytes(int threads) { return (size_t)kSpRegs * (size_t)threads * sizeof(double); }

// The device image of a program (what a launch's strategy_data points to).  code[i]: bits 0-4 opcode, 5-9 destination
// register, 10-16 / 17-23 / 24-30 operands a / b / c: 0..31 a register, RM_STRATEGY_IN_* an input, kSpConstBase + i
// constant i.  block[b] = first | end << 16 of block b's instructions (0 = init, 1 + phase; an absent block is empty).
struct StrategyImage {
    int32_t nops, nconst;
    uint32_t block[kSpBlocks];
    uint32_t pad;
    uint32_t code[kSpMaxOps];
    double k[kSpMaxConst];
};

struct SpWord {
    uint32_t w;
    RM_HD int op() const { return (int)(w & 31u); }
    RM_HD int dst() const { return (int)((w >> 5) & 31u); }
    RM_HD int a() const { return (int)((w >> 10) & 127u); }
    RM_HD int b() const { return (int)((w >> 17) & 127u); }
    RM_HD int c() const { return (int)((w >> 24) & 127u); }
};

// operands each opcode reads
RM_HD int sp_op_args(int op)
{
    switch (op) {
        case RM_STOP_MOV: case RM_STOP_NEG: case RM_STOP_ABS: case RM_STOP_SQRT: case RM_STOP_NOT: return 1;
        case RM_STOP_SELECT: return 3;
        default: return 2;
    }
}

// One instruction.  `op` is wave-uniform on the device: the switch is a scalar branch.  One IEEE operation each
// (-ffp-contract=off as everywhere); "true" is "!= 0", so a NaN condition counts as true.
RM_HD double sp_apply(int op, double a, double b, double c)
{
    switch (op) {
        case RM_STOP_MOV: return a;
        case RM_STOP_ADD: return a + b;
        case RM_STOP_SUB: return a - b;
        case RM_STOP_MUL: return a * b;
        case RM_STOP_DIV: return a / b;
        case RM_STOP_NEG: return -a;
        case RM_STOP_ABS: return rm_fabs(a);
        case RM_STOP_SQRT: return rm_sqrt(a);
        case RM_STOP_PYMAX: return py_max(a, b);
        case RM_STOP_PYMIN: return py_min(a, b);
        case RM_STOP_LT: return a < b ? 1.0 : 0.0;
        case RM_STOP_LE: return a <= b ? 1.0 : 0.0;
        case RM_STOP_GT: return a > b ? 1.0 : 0.0;
        case RM_STOP_GE: return a >= b ? 1.0 : 0.0;
        case RM_STOP_EQ: return a == b ? 1.0 : 0.0;
        case RM_STOP_NE: return a != b ? 1.0 : 0.0;
        case RM_STOP_AND: return (a != 0.0 && b != 0.0) ? 1.0 : 0.0;
        case RM_STOP_OR: return (a != 0.0 || b != 0.0) ? 1.0 : 0.0;
        case RM_STOP_NOT: return a == 0.0 ? 1.0 : 0.0;
        default: return a != 0.0 ? b : c;      // RM_STOP_SELECT
    }
}

// s6 as MarchResult.iterations: NaN -> 0, clamped to [0, INT32_MAX], truncated
RM_HD int32_t sp_iterations(double x)
{
    if (!(x > 0.0)) return 0;
    if (x >= 2147483647.0) return 2147483647;
    return (int32_t)x;
}

// s2 as a block number: 1 + phase, or kSpBlocks (no block) for anything that is no phase
RM_HD int sp_phase_block(double x) { return (x >= 0.0 && x < (double)RM_STRATEGY_PROGRAM_MAX_PHASES) ? 1 + (int)x : kSpBlocks; }

// THE EVALUATION BUDGET: a ray is force-finished at this evaluation if its program has not finished it (a program can
// never keep a wave alive).  The compiled strategies need at most 2 * max_iterations + 40 evaluations.  Clamped to
// INT32_MAX, so the 32-bit count of a ray's evaluations reaches it before it could overflow.
RM_HD int32_t sp_budget(const MarchCfg& c)
{
    const long long b = 8ll * (long long)(c.max_iterations > 0 ? c.max_iterations : 0) + 64ll;
    return b < 2147483647ll ? (int32_t)b : 2147483647;
}

#if defined(__HIP_DEVICE_COMPILE__)
// the program of the launch and the rays' registers, filled by StratProgram::load / start (used only by its kernels)
extern __shared__ double rm_s_sp_reg[];      // [kSpRegs][blockDim.x]: the launch's dynamic LDS (sp_register_bytes)
__shared__ uint32_t rm_s_sp_code[kSpMaxOps];
__shared__ double rm_s_sp_k[kSpMaxConst];
__shared__ uint32_t rm_s_sp_block[kSpBlocks];
struct SpMachine {
    __device__ __forceinline__ uint32_t block(int b) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)rm_s_sp_block[b]); }
    __device__ __forceinline__ uint32_t word(int i) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)rm_s_sp_code[i]); }
    __device__ __forceinline__ double k(int i) const { return rm_s_sp_k[i]; }
    __device__ __forceinline__ double reg(int i) const { return rm_s_sp_reg[i * (int)blockDim.x + (int)threadIdx.x]; }
    __device__ __forceinline__ void set(int i, double x) { rm_s_sp_reg[i * (int)blockDim.x + (int)threadIdx.x] = x; }
    // does any lane that is executing here want it? (wave-uniform)
    static __device__ __forceinline__ bool any(bool x) { return __ballot(x) != 0; }
};
#else
// host builds (tests/native): the program StratProgram runs on this thread
inline thread_local const StrategyImage* rm_host_strategy = nullptr;
struct SpMachine {
    double r[kSpRegs];
    uint32_t block(int b) const { return rm_host_strategy ? rm_host_strategy->block[b] : 0u; }
    uint32_t word(int i) const { return rm_host_strategy->code[i]; }
    double k(int i) const { return rm_host_strategy->k[i]; }
    double reg(int i) const { return r[i]; }
    void set(int i, double x) { r[i] = x; }
    static bool any(bool x) { return x; }
};
#endif

// The interpreter as a strategy.  The members the kernels read are StratBase's: te, i (the parking test; a program
// frame never parks and i stays 0) and res.
struct StratProgram {
    static constexpr bool kLaunchData = true;
    double te;
    int32_t i;
    int32_t blk;        // block of the lane's phase (1 + phase; kSpBlocks: none)
    int32_t nev;        // evaluations this ray has consumed (the budget's count)
    int32_t tail;       // the next value is the `full` frame's final_sdf (status 2)
    Result res;
    SpMachine m;

#if defined(__HIP_DEVICE_COMPILE__)
    // prologue of a kernel (all threads of the workgroup; the barrier follows in rm_load_tables).  The bounds are
    // strategy_encode's; the clamps only keep a corrupt image inside the LDS arrays.
    static __device__ __forceinline__ void load(const void* data)
    {
        const StrategyImage* img = static_cast<const StrategyImage*>(data);
        const int n = min(max(img->nops, 0), kSpMaxOps), nk = min(max(img->nconst, 0), kSpMaxConst);
        for (int j = threadIdx.x; j < n; j += blockDim.x) rm_s_sp_code[j] = img->code[j];
        for (int j = threadIdx.x; j < nk; j += blockDim.x) rm_s_sp_k[j] = img->k[j];
        for (int j = threadIdx.x; j < kSpBlocks; j += blockDim.x) {
            const uint32_t b = img->block[j];
            const uint32_t first = min(b & 0xffffu, (uint32_t)n), end = min(b >> 16, (uint32_t)n);
            rm_s_sp_block[j] = first | end << 16;
        }
    }
#elif defined(__HIPCC__)
    static __device__ void load(const void*) {}      // (hipcc's host pass; the device pass has the body above)
#endif

    RM_HD double operand(int code, double d, double te_in, const MarchCfg& c) const
    {
        if (code < kSpRegs) return m.reg(code);
        if (code >= kSpConstBase) return m.k(code - kSpConstBase);
        switch (code) {
            case RM_STRATEGY_IN_D: return d;
            case RM_STRATEGY_IN_TE: return te_in;
            case RM_STRATEGY_IN_HIT_THRESHOLD: return c.hit_threshold;
            case RM_STRATEGY_IN_MAX_DISTANCE: return c.max_distance;
            case RM_STRATEGY_IN_MAX_ITERATIONS: return (double)c.max_iterations;
            default: return c.lipschitz;
        }
    }

    // the instructions of block b, for the lanes that call
    RM_HD void run_block(int b, double d, double te_in, const MarchCfg& c)
    {
        const uint32_t range = m.block(b);
        const int end = (int)(range >> 16);
        for (int pc = (int)(range & 0xffffu); pc < end; ++pc) {
            const SpWord w{ m.word(pc) };
            const int op = w.op(), n = sp_op_args(op);
            const double a = operand(w.a(), d, te_in, c);
            const double b2 = n >= 2 ? operand(w.b(), d, te_in, c) : 0.0;
            const double c3 = n >= 3 ? operand(w.c(), d, te_in, c) : 0.0;
            m.set(w.dst(), sp_apply(op, a, b2, c3));
        }
    }

    // what the machine reads after a block
    RM_HD bool after_block(const MarchCfg& c)
    {
        const double status = m.reg(3);
        if (status == 0.0) {
            te = m.reg(1);
            blk = sp_phase_block(m.reg(2));
            return false;
        }
        res.hit = m.reg(4) != 0.0 ? 1 : 0;
        res.t = m.reg(0);
        res.final_sdf = m.reg(5);
        res.iters = sp_iterations(m.reg(6));
        if (status == 2.0 && c.full) { te = res.t; tail = 1; return false; }
        return true;
    }

    RM_HD bool start(const MarchCfg& c)
    {
        for (int j = 0; j < RM_STRATEGY_PROGRAM_MAX_STATE; ++j) m.set(j, 0.0);
        te = 0.0; i = 0; blk = kSpBlocks; nev = 0; tail = 0;
        run_block(0, 0.0, 0.0, c);
        return after_block(c);
    }

    RM_HD bool step(double d, const MarchCfg& c)
    {
        ++nev;
        bool done;
        if (tail) {
            res.final_sdf = d;
            done = true;
        } else {
            const double te_in = te;
            for (int b = 1; b < kSpBlocks; ++b) {
                if (!SpMachine::any(blk == b)) continue;      // no lane of the wave is in this phase
                if (blk == b) run_block(b, d, te_in, c);
            }
            done = after_block(c);
        }
        if (!done && nev >= sp_budget(c)) {                   // THE EVALUATION BUDGET
            // A program that finished the ray in this very step (status 2 of a `full` frame, which only waits for its tail
            // evaluation) has finished it "by then": its result stands, with s5 as final_sdf and without the tail.
            if (!tail) { res.hit = 0; res.t = m.reg(0); res.final_sdf = d; res.iters = sp_iterations(m.reg(6)); }
            done = true;
        }
        return done;
    }
};

// (host code) Validates a program and writes its device image.  false with the reason in `why`: see rm_strategy_program_create.
inline bool strategy_encode(const RmStrategyOp* ops, int32_t nops, StrategyImage* img, char* why, size_t why_len)
{
    if (!ops) return snprintf(why, why_len, "ops is NULL"), false;
    if (nops <= 0) return snprintf(why, why_len, "program length %d: a program needs an init block", nops), false;
    if (nops > kSpMaxOps + kSpBlocks) return snprintf(why, why_len, "too many instructions: more than %d", kSpMaxOps), false;
    memset(img, 0, sizeof *img);
    bool have[kSpBlocks] = {};
    int cur = -1, n = 0, nk = 0;      // block being filled (-1: none yet), instructions and constants so far
    uint32_t written = 0;             // temporaries the current block has written
    for (int i = 0; i < nops; ++i) {
        const RmStrategyOp& o = ops[i];
        if (o.reserved != 0) return snprintf(why, why_len, "op %d: reserved field is %d, must be 0", i, o.reserved), false;
        if (o.op == RM_STOP_BLOCK) {
            if (o.a != RM_STRATEGY_BLOCK_INIT && (o.a < 0 || o.a >= RM_STRATEGY_PROGRAM_MAX_PHASES))
                return snprintf(why, why_len, "op %d: phase %d above %d", i, o.a, RM_STRATEGY_PROGRAM_MAX_PHASES - 1), false;
            if (o.dst != 0 || o.b != 0 || o.c != 0) return snprintf(why, why_len, "op %d: unused field of a block marker must be 0", i), false;
            if (cur >= 0) img->block[cur] |= (uint32_t)n << 16;
            cur = o.a + 1;
            if (have[cur]) {
                if (cur == 0) return snprintf(why, why_len, "op %d: duplicate init block", i), false;
                return snprintf(why, why_len, "op %d: duplicate block of phase %d", i, o.a), false;
            }
            have[cur] = true;
            img->block[cur] = (uint32_t)n;
            written = 0;
            continue;
        }
        if (o.op < 0 || o.op >= RM_STOP_COUNT) return snprintf(why, why_len, "op %d: unknown opcode %d", i, o.op), false;
        if (cur < 0) return snprintf(why, why_len, "op %d: instruction before the first block marker", i), false;
        if (n >= kSpMaxOps) return snprintf(why, why_len, "too many instructions: more than %d", kSpMaxOps), false;
        if (o.dst < 0 || o.dst >= kSpRegs) return snprintf(why, why_len, "op %d: destination %d out of range", i, o.dst), false;
        const int na = sp_op_args(o.op);
        const int32_t src[3] = { o.a, o.b, o.c };
        uint32_t enc[3] = { 0, 0, 0 };
        bool literal = false;
        for (int j = 0; j < 3; ++j) {
            const int32_t s = src[j];
            if (j >= na) {
                if (s != 0) return snprintf(why, why_len, "op %d: unused operand %c must be 0", i, 'a' + j), false;
                continue;
            }
            if (s == RM_STRATEGY_LITERAL) { literal = true; continue; }
            if (s < 0 || s > RM_STRATEGY_IN_LIPSCHITZ) return snprintf(why, why_len, "op %d: operand %c = %d out of range", i, 'a' + j, s), false;
            if (cur == 0 && (s == RM_STRATEGY_IN_D || s == RM_STRATEGY_IN_TE))
                return snprintf(why, why_len, "op %d: the init block has no evaluated value to read", i), false;
            if (s >= RM_STRATEGY_PROGRAM_MAX_STATE && s < kSpRegs && !(written & (1u << (s - RM_STRATEGY_PROGRAM_MAX_STATE))))
                return snprintf(why, why_len, "op %d: temporary t%d read before it is written in its block", i, s - RM_STRATEGY_PROGRAM_MAX_STATE), false;
            enc[j] = (uint32_t)s;
        }
        if (literal) {
            if (!(o.k - o.k == 0.0)) return snprintf(why, why_len, "op %d: constant is not finite", i), false;
            int at = -1;
            for (int q = 0; q < nk && at < 0; ++q)
                if (memcmp(&img->k[q], &o.k, sizeof o.k) == 0) at = q;
            if (at < 0) {
                if (nk >= kSpMaxConst) return snprintf(why, why_len, "op %d: too many constants: more than %d", i, kSpMaxConst), false;
                img->k[nk] = o.k;
                at = nk++;
            }
            for (int j = 0; j < na; ++j)
                if (src[j] == RM_STRATEGY_LITERAL) enc[j] = (uint32_t)(kSpConstBase + at);
        } else if (o.k != 0.0 || o.k != o.k) {
            return snprintf(why, why_len, "op %d: k must be 0 when no operand is RM_STRATEGY_LITERAL", i), false;
        }
        if (o.dst >= RM_STRATEGY_PROGRAM_MAX_STATE) written |= 1u << (o.dst - RM_STRATEGY_PROGRAM_MAX_STATE);
        img->code[n++] = (uint32_t)o.op | (uint32_t)o.dst << 5 | enc[0] << 10 | enc[1] << 17 | enc[2] << 24;
    }
    if (cur >= 0) img->block[cur] |= (uint32_t)n << 16;
    if (!have[0]) return snprintf(why, why_len, "no init block"), false;
    img->nops = n;
    img->nconst = nk;
    return true;
}

#if defined(__HIPCC__)
struct KernelArgs;
// Per-scene launch table of the interpreter's kernels, filled by rm_strategy_tu.hip (one object per scene).
struct StrategyProgramLaunchers {
    hipError_t (*render)(const KernelArgs& a, int grid, hipStream_t s);                          // 64x4 tiles, whole evaluations
    hipError_t (*occupancy)(int batch, int* blocks_per_cu);                                      // of render
    hipError_t (*march_rays)(const MarchCfg& cfg, const double* o, const double* d, size_t n, uint8_t* hit, double* t,
                             int32_t* iters, double* fs, const void* scene_data, const void* strategy_data, hipStream_t s);
};
#endif

}  // namespace rm
