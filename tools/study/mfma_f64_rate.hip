// Study (not product code): the rate of v_mfma_f64_16x16x4_f64 on this part, the yardstick of the covariate
// projection kernel (covar_project_kernel: 6 M N q fp64 flop).  A bare loop of independent MFMAs on operands held in
// registers (no memory traffic), `chains` accumulators per wave, `waves` waves per SIMD on every CU.
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate tools/study/mfma_f64_rate.hip && ./mfma_f64_rate [iters]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int CHAINS>
__global__ void __launch_bounds__(256) rate_kernel(int iters, double* out) {
    const int lane = threadIdx.x & 63;
    const double a = (lane & 3) == 0 ? 1.0 : 0.0, b = 1.0 + 1e-3 * lane;
    f64x4 acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    if (s == -1.0) out[0] = s;  // (keeps the loop)
}

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                          \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

template <int CHAINS>
int measure(int iters, int wgs_per_cu, int n_cu, double* out) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const dim3 grid(n_cu * wgs_per_cu), block(256);  // 4 waves per workgroup: one per SIMD
    hipLaunchKernelGGL((rate_kernel<CHAINS>), grid, block, 0, 0, iters / 16, out);  // warm-up
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((rate_kernel<CHAINS>), grid, block, 0, 0, iters, out);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best;
    }
    const double flop = 2.0 * 16 * 16 * 4 * (double)CHAINS * iters * 4.0 * n_cu * wgs_per_cu;
    std::printf("{\"chains\": %d, \"waves_per_simd\": %d, \"ms\": %.3f, \"tflops_f64\": %.2f}\n", CHAINS, wgs_per_cu,
                best, flop / (best * 1e-3) / 1e12);
    return 0;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 20000;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    double* out = nullptr;
    CHECK(hipMalloc(&out, sizeof(double)));
    std::printf("{\"device\": \"%s\", \"cus\": %d, \"clock_mhz\": %d}\n", prop.name, prop.multiProcessorCount,
                prop.clockRate / 1000);
    int rc = 0;
    rc |= measure<4>(iters, 1, prop.multiProcessorCount, out);
    rc |= measure<8>(iters, 1, prop.multiProcessorCount, out);
    rc |= measure<8>(iters, 2, prop.multiProcessorCount, out);
    rc |= measure<4>(iters, 4, prop.multiProcessorCount, out);
    rc |= measure<8>(iters, 4, prop.multiProcessorCount, out);
    rc |= measure<4>(iters, 8, prop.multiProcessorCount, out);
    (void)hipFree(out);
    return rc;
}
