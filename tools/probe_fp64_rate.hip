// probe_fp64_rate.hip — issue rate of v_add_f64 / v_mul_f64 on the device (the bound tools/snp_kinship_line.py divides by).
// Every lane runs 8 independent dependency chains of alternating double multiplies and adds (no FMA: -ffp-contract=off and
// __dmul_rn / __dadd_rn), enough waves to fill every SIMD several times; the rate is compared with
// CUs x 4 SIMDs x 16 lanes x clock, i.e. one fp64 add or multiply per lane and clock.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/probe_fp64_rate.hip -o tools/bin/probe_fp64_rate
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CK(x)                                                                             \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                       \
            exit(1);                                                                      \
        }                                                                                 \
    } while (0)

__global__ void __launch_bounds__(256) fp64_chains(double* out, int iters, double m, double a) {
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = 1.0 + 1e-3 * (threadIdx.x + k);
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = __dadd_rn(__dmul_rn(x[k], m), a);
    }
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += x[k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    int clock_khz = 0;
    CK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0));
    const int cus = prop.multiProcessorCount;
    const int blocks = cus * 4 * 8 / 4;  // 8 waves per SIMD
    const int iters = 20000;
    double* d = nullptr;
    CK(hipMalloc(&d, (size_t)blocks * 256 * sizeof(double)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(fp64_chains, dim3(blocks), dim3(256), 0, 0, d, 100, 0.999999, 1e-9);  // warm-up
    CK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(fp64_chains, dim3(blocks), dim3(256), 0, 0, d, iters, 0.999999, 1e-9);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double ops = (double)blocks * 256 * iters * 8 * 2;  // one multiply and one add per chain step
    const double rate = ops / (best * 1e-3);
    const double peak = (double)cus * 4 * 16 * clock_khz * 1e3;
    printf("{\"cus\": %d, \"clock_mhz\": %.0f, \"best_ms\": %.3f, \"fp64_ops_per_s\": %.4g, \"lane_clock_peak\": %.4g, \"share\": %.3f}\n", cus,
           clock_khz / 1e3, best, rate, peak, rate / peak);
    CK(hipFree(d));
    return 0;
}
