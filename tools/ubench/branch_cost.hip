// Micro-benchmark (developer tool): what a wave-uniform branch costs a wavefront that is alone on its SIMD with ONE live
// lane, in steady state -- the case of a ray marching alone in its team (rm_math_trig.h "wave-uniform band skipping").
// Every variant is one dependent fp64 chain (4 fma up front; every iteration depends on the one before), followed by
//   0  nothing                                                                    (the chain alone)
//   1  compare on the chain's value, branch TAKEN over a block of 14 fma          (a skipped ballot-guarded block)
//   2  the same compare, branch NOT taken, the 14 fma run by fall-through         (the layout of a common path)
//   3  the 14 fma with no compare and no branch                                   (what 2 is measured against)
//   4  branch TAKEN over the block on a scalar set before the loop                (no vector-to-scalar wait)
//   5  branch NOT taken on that scalar, the block runs
// written in assembly so that the layout is the one named.  skip = (1) - (0), fall-through = (2) - (3),
// early scalar = (4) - (0) and (5) - (3).  Prints shader ticks (s_memtime) and wall time (s_memrealtime, 100 MHz).
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/branch_cost.hip -o tools/ubench/branch_cost.exe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define RM_FMA4 "v_fma_f64 %0, %0, %1, %2\n v_fma_f64 %0, %0, %1, %2\n v_fma_f64 %0, %0, %1, %2\n v_fma_f64 %0, %0, %1, %2\n"
#define RM_FMA14 RM_FMA4 RM_FMA4 RM_FMA4 "v_fma_f64 %0, %0, %1, %2\n v_fma_f64 %0, %0, %1, %2\n"

template <int WHAT>
__global__ __launch_bounds__(64) void k(int live, int n, int flag, double* out, long long* cyc)
{
    const int lane = (int)threadIdx.x;
    double acc = 1.0 + lane;
    const double half = 0.5, one = 1.0, thr = -1.0;       // acc stays in (1, 65]: `acc < thr` is false in every lane
    const int sflag = __builtin_amdgcn_readfirstlane(flag);   // 0: decided before the loop
    const long long t0 = __builtin_amdgcn_s_memtime();
    const long long r0 = __builtin_amdgcn_s_memrealtime();
    if (lane < live) {
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            asm volatile(RM_FMA4 : "+v"(acc) : "v"(half), "v"(one));
            if constexpr (WHAT == 1) {
                asm volatile("v_cmp_lt_f64 vcc, %0, %3\n s_cbranch_vccz 1f\n" RM_FMA14 "1:\n" : "+v"(acc) : "v"(half), "v"(one), "v"(thr) : "vcc");
            } else if constexpr (WHAT == 2) {
                asm volatile("v_cmp_lt_f64 vcc, %0, %3\n s_cbranch_vccnz 1f\n" RM_FMA14 "1:\n" : "+v"(acc) : "v"(half), "v"(one), "v"(thr) : "vcc");
            } else if constexpr (WHAT == 3) {
                asm volatile(RM_FMA14 : "+v"(acc) : "v"(half), "v"(one));
            } else if constexpr (WHAT == 4) {
                asm volatile("s_cmp_eq_u32 %3, 0\n s_cbranch_scc1 1f\n" RM_FMA14 "1:\n" : "+v"(acc) : "v"(half), "v"(one), "s"(sflag) : "scc");
            } else if constexpr (WHAT == 5) {
                asm volatile("s_cmp_lg_u32 %3, 0\n s_cbranch_scc1 1f\n" RM_FMA14 "1:\n" : "+v"(acc) : "v"(half), "v"(one), "s"(sflag) : "scc");
            }
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    const long long r1 = __builtin_amdgcn_s_memrealtime();
    out[lane] = acc;
    if (lane == 0) { cyc[0] = t1 - t0; cyc[1] = r1 - r0; }
}

template <int WHAT>
double run(const char* name, int live, double* out, long long* cyc)
{
    const int n = 200000;
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((k<WHAT>), dim3(1), dim3(64), 0, 0, live, n, 0, out, cyc);
    long long h[2] = { 0, 0 };
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, cyc, 16, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: failed\n", name); exit(1); }
    printf("%-52s live lanes %2d: %7.2f shader ticks = %6.2f ns per iteration\n", name, live, (double)h[0] / n, (double)h[1] * 10.0 / n);
    return (double)h[0] / n;
}

int main()
{
    double* out; long long* cyc;
    if (hipMalloc(&out, 64 * 8) != hipSuccess || hipMalloc(&cyc, 16) != hipSuccess) { printf("no device memory\n"); return 1; }
    for (int live : { 1, 64 }) {
        const double c0 = run<0>("0 chain alone", live, out, cyc);
        const double c1 = run<1>("1 compare, branch taken over 14 fma", live, out, cyc);
        const double c2 = run<2>("2 compare, branch not taken, 14 fma fall through", live, out, cyc);
        const double c3 = run<3>("3 14 fma, no branch", live, out, cyc);
        const double c4 = run<4>("4 early scalar, branch taken over 14 fma", live, out, cyc);
        const double c5 = run<5>("5 early scalar, branch not taken, 14 fma", live, out, cyc);
        printf("live %2d: skipped block %.1f, fall-through branch %.1f, early scalar taken %.1f / not taken %.1f, the block itself %.1f ticks\n",
               live, c1 - c0, c2 - c3, c4 - c0, c5 - c3, c3 - c0);
    }
    (void)hipFree(out); (void)hipFree(cyc);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
