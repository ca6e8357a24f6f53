// fp64 arithmetic rate of the chip, measured: v_fma_f64 (VALU) and v_mfma_f64_16x16x4_f64 (matrix core), each as many
// independent dependency chains per wave as it takes to cover the latency, over a grid that fills every CU.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/fp64_rate.hip -o tools/ubench/fp64_rate && tools/ubench/fp64_rate
// Prints one JSON line: TFLOP/s of each (2 FLOP per FMA; 16 x 16 x 4 x 2 per MFMA).  Used by DESIGN.md s5.6 to choose the
// accumulation of the ALS kernel (als.hip), and the denominator of the fp64 fraction in profiles/wrmf_bench.json.
#include <hip/hip_runtime.h>

#include <cstdio>

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kIters = 4096;
constexpr int kChains = 8;

__global__ __launch_bounds__(256) void fma_kernel(double *out, double x, double y) {
    double a[kChains];
#pragma unroll
    for (int k = 0; k < kChains; ++k) a[k] = threadIdx.x + k;
    for (int it = 0; it < kIters; ++it)
#pragma unroll
        for (int k = 0; k < kChains; ++k) a[k] = fma(a[k], x, y);
    double s = 0;
#pragma unroll
    for (int k = 0; k < kChains; ++k) s += a[k];
    if (s == 12345.678) out[0] = s;         // never true; keeps the chains alive
}

__global__ __launch_bounds__(256) void mfma_kernel(double *out, double x, double y) {
    f64x4 c[kChains];
#pragma unroll
    for (int k = 0; k < kChains; ++k) c[k] = f64x4{0.0 + k, 1.0, 2.0, 3.0};
    const double a = x + threadIdx.x, b = y;
    for (int it = 0; it < kIters; ++it)
#pragma unroll
        for (int k = 0; k < kChains; ++k) c[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[k], 0, 0, 0);
    double s = 0;
#pragma unroll
    for (int k = 0; k < kChains; ++k) s += c[k][0] + c[k][1] + c[k][2] + c[k][3];
    if (s == 12345.678) out[0] = s;
}

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

int main() {
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    double *out;
    CK(hipMalloc(&out, 8));
    const int blocks = p.multiProcessorCount * 8;      // 8 waves per SIMD's worth of 256-thread blocks
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    double best_fma = 1e30, best_mfma = 1e30;
    for (int rep = 0; rep < 6; ++rep) {
        float ms;
        CK(hipEventRecord(e0));
        fma_kernel<<<blocks, 256>>>(out, 1.0000001, 1e-9);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) best_fma = ms < best_fma ? ms : best_fma;
        CK(hipEventRecord(e0));
        mfma_kernel<<<blocks, 256>>>(out, 1e-3, 1e-3);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) best_mfma = ms < best_mfma ? ms : best_mfma;
    }
    const double threads = (double)blocks * 256, waves = threads / 64;
    const double fma_flop = threads * kIters * kChains * 2.0;
    const double mfma_flop = waves * kIters * kChains * 16.0 * 16.0 * 4.0 * 2.0;
    printf("{\"device\": \"%s\", \"cu\": %d, \"fma_f64_tflops\": %.2f, \"mfma_f64_16x16x4_tflops\": %.2f, \"fma_ms\": %.4f, \"mfma_ms\": %.4f}\n",
           p.gcnArchName, p.multiProcessorCount, fma_flop / best_fma * 1e-9, mfma_flop / best_mfma * 1e-9, best_fma, best_mfma);
    return 0;
}
