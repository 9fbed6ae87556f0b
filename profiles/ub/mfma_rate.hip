// Attainable MFMA rate of the box the convolutions are priced against: every wave issues `iters` x 4 independent MFMAs back to back, no
// memory, at 1, 2 and 4 waves per SIMD, short and long runs (clock behaviour under sustained matrix load).  First v_mfma_f32_32x32x2_f32
// (the fp32 engine's instruction; read the figure against the 157.3 TF that bench_avatar.py takes from the microarchitecture guide), then
// v_mfma_f32_32x32x16_bf16 (the rate a three-term bf16 split of the fp32 operands runs on).  The two kernels lived in csrc/ag_conv.hip as
// ag_debug_mfma_rate / ag_debug_mfma_rate_bf16 up to commit 7a3cbce, driven by profiles/mfma_peak.py (record: profiles/r01p_mfma_peak.txt).
// build: hipcc --offload-arch=gfx950 -O3 -o mfma_rate mfma_rate.hip
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(256) mfma_rate_kernel(int iters, float* out)
{
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
    float a = 1.0f + threadIdx.x * 1e-6f, b = 0.5f;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
    }
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) v += acc[i][r];
    if (v == 12345.678f) out[0] = v;     // keep the chain alive
}

__global__ void __launch_bounds__(256) mfma_rate_bf16_kernel(int iters, float* out)
{
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
    bf16x8 a, b;
#pragma unroll
    for (int i = 0; i < 8; i++) { a[i] = (__bf16)(1.0f + (threadIdx.x & 7) * 0.125f); b[i] = (__bf16)0.5f; }
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i], 0, 0, 0);
    }
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) v += acc[i][r];
    if (v == 12345.678f) out[0] = v;
}

// one timed launch after a short one of the same grid; k = the MFMA's K (FLOPs per MFMA = 32 * 32 * k * 2)
template <typename Kernel>
static void run(Kernel kernel, int waves_per_simd, int iters, int k, bool third, float* out)
{
    const int blocks = 256 * waves_per_simd;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, 100, out);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, iters, out);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    const double flops = (double)blocks * 4 * iters * 4 * (32.0 * 32 * k * 2);
    printf("%d waves/SIMD, %6d iters: %8.3f ms  %7.1f TFLOP/s", waves_per_simd, iters, ms, flops / ms / 1e9);
    if (third) printf("  (/3 = %6.1f fp32-equivalent)", flops / ms / 3e9);
    printf("\n");
}

int main()
{
    float* out = nullptr;
    if (hipMalloc(&out, 64) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    const int waves[3] = { 1, 2, 4 }, iters_f32[3] = { 2000, 20000, 200000 }, iters_bf16[2] = { 20000, 200000 };
    printf("v_mfma_f32_32x32x2_f32:\n");
    for (int w : waves)
        for (int it : iters_f32) run(mfma_rate_kernel, w, it, 2, false, out);
    printf("v_mfma_f32_32x32x16_bf16 (the instruction a bf16 split of the fp32 operands would run on):\n");
    for (int w : waves)
        for (int it : iters_bf16) run(mfma_rate_bf16_kernel, w, it, 16, true, out);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { fprintf(stderr, "%s\n", hipGetErrorString(e)); return 1; }
    (void)hipFree(out);
    return 0;
}
