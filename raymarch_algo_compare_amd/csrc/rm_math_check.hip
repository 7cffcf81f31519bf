// rm_math_check.hip -- the device math on its own, for tests (rm_debug_math_eval, include/rm_hip.h).
//
// One kernel per RmMathFn routine.  Built like every other object of the library (the same HIPFLAGS, through
// hipcc_peephole.sh) and with the libm tables in the LDS mirrors rm_load_tables() fills, so the code under test is the
// code the render kernels run: clang's amdgcn lowering of sqrt / division / ldexp, the re-encoded selects, the mirrors'
// strides -- none of which the host build of the same headers (tests/test_math_exact.py) sees.
//
// Shape of a launch: 256-thread workgroups (kWavesPerWG waves, as the render kernels).  Every thread helps to fill the
// mirrors (the copy loops stride over threadIdx.x); only then do the lanes outside `lane_mask` and the lanes past n
// leave, so the ballots of the wave-uniform forms (rm_band_needed<true>, rm_pow_half<true>) see exactly the live lanes.
#include "rm_kernels.h"
#include "../../include/rm_hip.h"
#include "rm_capi_internal.h"

namespace rm {

struct MathCheckTables;   // a tag that loads every table (Mandelbulb's set)
template <> struct SceneTables<MathCheckTables> { static constexpr unsigned value = TB_POW | TB_SINCOS | TB_ACOS | TB_ATAN | TB_LOG; };

template <int FN>
__device__ __forceinline__ void math_check_eval(double a, double b, double* o0, double* o1)
{
    if constexpr (FN == RM_MATH_POW) *o0 = rm_pow(a, b);
    else if constexpr (FN == RM_MATH_POW2) rm_pow2(a, 7.0, 8.0, o0, o1);      // the Mandelbulb call (power - 1, power)
    else if constexpr (FN == RM_MATH_POW_HALF_DENSE) *o0 = rm_pow_half<false>(a);
    else if constexpr (FN == RM_MATH_POW_HALF_SPARSE) *o0 = rm_pow_half<true>(a);
    else if constexpr (FN == RM_MATH_POW_HALF_GUARD) {
        bool safe;
        *o0 = rm_pow_half_guard(a, &safe);
        *o1 = safe ? 1.0 : 0.0;
    }
    else if constexpr (FN == RM_MATH_SQRT) *o0 = rm_sqrt(a);
    else if constexpr (FN == RM_MATH_SIN) *o0 = rm_sin(a);
    else if constexpr (FN == RM_MATH_COS) *o0 = rm_cos(a);
    else if constexpr (FN == RM_MATH_SINCOS) rm_sincos<false>(a, o0, o1);
    else if constexpr (FN == RM_MATH_SINCOS_U) rm_sincos<true>(a, o0, o1);
    else if constexpr (FN == RM_MATH_ACOS) *o0 = rm_acos<false>(a);
    else if constexpr (FN == RM_MATH_ACOS_U) *o0 = rm_acos<true>(a);
    else if constexpr (FN == RM_MATH_ATAN2) *o0 = rm_atan2<false>(a, b);
    else if constexpr (FN == RM_MATH_ATAN2_U) *o0 = rm_atan2<true>(a, b);
    else if constexpr (FN == RM_MATH_LOG) *o0 = rm_log(a);
    else static_assert(FN < 0, "unknown RmMathFn");
}

// Every mirror is filled with NaN before rm_load_tables() runs.  LDS keeps what the previous workgroup on the compute unit
// left -- the same tables, written to the same places by the same code -- so a row the loader failed to write would
// otherwise still read correct values.
__device__ __forceinline__ void poison_tables()
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double q = __builtin_nan("");
    for (int i = threadIdx.x; i < 128 * kPowLogStride; i += blockDim.x) rm_s_pow_log_tab[i] = q;
    for (int i = threadIdx.x; i < 128 * kExpStride; i += blockDim.x) rm_s_exp_tab[i] = 0x7ff8000000000000ull;
    for (int i = threadIdx.x; i < 128 * kLogStride; i += blockDim.x) rm_s_log_tab[i] = q;
    for (int i = threadIdx.x; i < 110 * kSinCosStride; i += blockDim.x) rm_s_sincostab[i] = q;
    for (int i = threadIdx.x; i < 2808; i += blockDim.x) rm_s_asncs[i] = q;
    for (int i = threadIdx.x; i < 128; i += blockDim.x) rm_s_inroot[i] = q;
    for (int i = threadIdx.x; i < 1687; i += blockDim.x) rm_s_cij[i] = q;
    __syncthreads();
#endif
}

// element e -> wave e / live, its (e % live)-th live lane
template <int FN>
__global__ __launch_bounds__(64 * kWavesPerWG) void math_check_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                     size_t n, uint64_t lane_mask, int live,
                                                                     double* __restrict__ out0, double* __restrict__ out1)
{
    poison_tables();
    rm_load_tables<MathCheckTables>();                 // all 256 threads, ends with the barrier
    const unsigned lane = threadIdx.x & 63u;
    if (!((lane_mask >> lane) & 1ull)) return;
    const size_t wave = (size_t)blockIdx.x * kWavesPerWG + threadIdx.x / 64u;
    const size_t e = wave * (size_t)live + (size_t)__popcll(lane_mask & ((1ull << lane) - 1ull));
    if (e >= n) return;
    double o0 = 0.0, o1 = 0.0;
    math_check_eval<FN>(a[e], b ? b[e] : 0.0, &o0, &o1);
    out0[e] = o0;
    if (out1) out1[e] = o1;
}

template <int FN>
static hipError_t launch_math(const double* a, const double* b, size_t n, uint64_t lane_mask, double* out0, double* out1,
                              hipStream_t s)
{
    const int live = __builtin_popcountll(lane_mask);
    const size_t waves = (n + live - 1) / live;
    const size_t grid = (waves + kWavesPerWG - 1) / kWavesPerWG;
    hipLaunchKernelGGL((math_check_kernel<FN>), dim3((unsigned)grid), dim3(64 * kWavesPerWG), 0, s, a, b, n, lane_mask, live,
                       out0, out1);
    return hipGetLastError();
}

// rm_debug_math_eval has checked fn, lane_mask != 0, n > 0 and the buffers the routine uses
static hipError_t launch_math_check(int fn, const double* a, const double* b, size_t n, uint64_t lane_mask, double* out0, double* out1,
                             hipStream_t s)
{
    switch (fn) {
#define RM_X(F) case F: return launch_math<F>(a, b, n, lane_mask, out0, out1, s);
        RM_X(RM_MATH_POW) RM_X(RM_MATH_POW2) RM_X(RM_MATH_POW_HALF_DENSE) RM_X(RM_MATH_POW_HALF_SPARSE)
        RM_X(RM_MATH_POW_HALF_GUARD) RM_X(RM_MATH_SQRT) RM_X(RM_MATH_SIN) RM_X(RM_MATH_COS) RM_X(RM_MATH_SINCOS)
        RM_X(RM_MATH_SINCOS_U) RM_X(RM_MATH_ACOS) RM_X(RM_MATH_ACOS_U) RM_X(RM_MATH_ATAN2) RM_X(RM_MATH_ATAN2_U)
        RM_X(RM_MATH_LOG)
#undef RM_X
    }
    return hipErrorInvalidValue;
}

// rm_bail4 (rm_math_pow.h), the Mandelbulb's bail-out decision from the squared length, behind an entry point of its own
// (rm_debug_bail4_eval): the same launch shape and element layout as math_check_kernel, the sparse flag of the root behind
// its band as a template argument, as the team loops hold it.  decision / band: 1.0 or 0.0.
template <bool SPARSE>
__global__ __launch_bounds__(64 * kWavesPerWG) void bail4_check_kernel(const double* __restrict__ s, size_t n, uint64_t lane_mask, int live,
                                                                      double* __restrict__ decision, double* __restrict__ band)
{
    poison_tables();
    rm_load_tables<MathCheckTables>();                 // all 256 threads, ends with the barrier
    const unsigned lane = threadIdx.x & 63u;
    if (!((lane_mask >> lane) & 1ull)) return;
    const size_t wave = (size_t)blockIdx.x * kWavesPerWG + threadIdx.x / 64u;
    const size_t e = wave * (size_t)live + (size_t)__popcll(lane_mask & ((1ull << lane) - 1ull));
    if (e >= n) return;
    const double x = s[e];
    decision[e] = rm_bail4(x, SPARSE) ? 1.0 : 0.0;
    band[e] = rm_bail4_band(x) ? 1.0 : 0.0;
}

// rm_debug_bail4_eval has checked lane_mask != 0, n > 0 and the buffers
static hipError_t launch_bail4_check(bool sparse, const double* s, size_t n, uint64_t lane_mask, double* decision, double* band, hipStream_t st)
{
    const int live = __builtin_popcountll(lane_mask);
    const size_t waves = (n + live - 1) / live;
    const dim3 grid((unsigned)((waves + kWavesPerWG - 1) / kWavesPerWG)), block(64 * kWavesPerWG);
    if (sparse) hipLaunchKernelGGL((bail4_check_kernel<true>), grid, block, 0, st, s, n, lane_mask, live, decision, band);
    else hipLaunchKernelGGL((bail4_check_kernel<false>), grid, block, 0, st, s, n, lane_mask, live, decision, band);
    return hipGetLastError();
}

}  // namespace rm

// ---- rm_debug_math_eval and rm_debug_bail4_eval of the C ABI ---------------------------------------------------------------
using namespace rm::capi;

extern "C" {

int rm_debug_math_eval(int32_t fn, const double* a, const double* b, size_t n, uint64_t lane_mask, double* out0, double* out1)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (fn < 0 || fn >= RM_MATH_COUNT) return fail(RM_E_BAD_ARG, "fn %d out of range [0, %d)", (int)fn, (int)RM_MATH_COUNT);
    if (lane_mask == 0) return fail(RM_E_BAD_ARG, "lane_mask is 0: no live lane");
    const bool two_in = fn == RM_MATH_POW || fn == RM_MATH_ATAN2 || fn == RM_MATH_ATAN2_U;
    const bool two_out = fn == RM_MATH_POW2 || fn == RM_MATH_POW_HALF_GUARD || fn == RM_MATH_SINCOS || fn == RM_MATH_SINCOS_U;
    if (n == 0) return RM_OK;
    if (!a || !out0 || (two_in && !b) || (two_out && !out1)) return fail(RM_E_BAD_ARG, "NULL buffer");
    Staged st(e);
    const double* d_a = st.in(stage_in[0], a, n * 8);
    const double* d_b = two_in ? st.in(stage_in[1], b, n * 8) : nullptr;
    double* d_out0 = st.out(stage_out[0], out0, n * 8);
    double* d_out1 = st.out(stage_out[1], two_out ? out1 : nullptr, n * 8);
    if ((rc = st.begin())) return rc;
    HIP_TRY(rm::launch_math_check(fn, d_a, d_b, n, lane_mask, d_out0, d_out1, lib_stream()));
    return st.finish();
}

int rm_debug_bail4_eval(const double* s, size_t n, uint64_t lane_mask, int32_t sparse, double* decision, double* band)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (lane_mask == 0) return fail(RM_E_BAD_ARG, "lane_mask is 0: no live lane");
    if (n == 0) return RM_OK;
    if (!s || !decision || !band) return fail(RM_E_BAD_ARG, "NULL buffer");
    Staged st(e);
    const double* d_s = st.in(stage_in[0], s, n * 8);
    double* d_out0 = st.out(stage_out[0], decision, n * 8);
    double* d_out1 = st.out(stage_out[1], band, n * 8);
    if ((rc = st.begin())) return rc;
    HIP_TRY(rm::launch_bail4_check(sparse != 0, d_s, n, lane_mask, d_out0, d_out1, lib_stream()));
    return st.finish();
}

}  // extern "C"
