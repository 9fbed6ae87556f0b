// The reverse pass of the template renderer's compositing and LaplaceDensity with its gradient (include/ag_ray_march_grad.h).
//
// The composite backward is the forward's shape: one wavefront per ray, one lane per sample of a 64-chunk, the product scan and T of
// ag_ray_scan.h, then ONE reverse scan of affine pairs across the lanes for B.  Nothing is divided by f = 1 - alpha + 1e-10, which is
// 1e-10 at a saturated sample.  All three kernels are memory bound and hold no LDS, no atomics and no scratch.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states every result as individually rounded fp32 operations.
#include <math.h>

#include "ag_common.h"
#include "ag_mlp_tile.h"
#include "ag_ray_scan.h"
#include "../../include/ag_ray_march_grad.h"

namespace ag {
namespace {

constexpr int kThreads = ray::kRayThreads;
constexpr int kGroups = AG_LAPLACE_GROUPS_PER_WAVE;
constexpr long long kMaxElements = 1ll << 33;

// ---- composite backward -------------------------------------------------------------------------------------------------------------
// Every loop count and every branch around a cross-lane move is uniform over the wavefront.
__global__ void __launch_bounds__(kThreads) ray_composite_backward_kernel(const float* __restrict__ density, const float* __restrict__ color,
                                                                          const float* __restrict__ z_vals, long long R, int S, int white_bkgd,
                                                                          const float* __restrict__ g_rgb, const float* __restrict__ g_acc,
                                                                          const float* __restrict__ g_depth, const float* __restrict__ g_w,
                                                                          float* __restrict__ grad_density, float* __restrict__ grad_color)
{
    const long long ray = (long long)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (ray >= R) return;                           // a whole wavefront; there is no barrier in this kernel
    const int lane = threadIdx.x & 63;
    const long long row = ray * S;
    const int chunks = (S + kWave - 1) / kWave;
    if (!g_rgb && !g_acc && !g_depth && !g_w) {     // no upstream gradient: zeros, from this launch
        for (int s = lane; s < S; s += kWave) {
            if (grad_density) grad_density[row + s] = 0.f;
            if (grad_color) { grad_color[3 * (row + s)] = 0.f; grad_color[3 * (row + s) + 1] = 0.f; grad_color[3 * (row + s) + 2] = 0.f; }
        }
        return;
    }
    const float G0 = g_rgb ? g_rgb[3 * ray] : 0.f, G1 = g_rgb ? g_rgb[3 * ray + 1] : 0.f, G2 = g_rgb ? g_rgb[3 * ray + 2] : 0.f;
    float Ga = g_acc ? g_acc[ray] : 0.f;
    if (white_bkgd) Ga = Ga - ((G0 + G1) + G2);
    const float Gd = g_depth ? g_depth[ray] : 0.f;

    // the forward carry of chunk k in lane k (1 for a single chunk)
    float carries = 1.f;
    if (chunks > 1) {
        float carry = 1.f;
        for (int k = 0; k < chunks - 1; ++k) {      // chunks 0 .. chunks - 2 are full
            float z;
            const int s = k * kWave + lane;
            const float dist = ray::sample_dist(z_vals, row, s, S, z);
            const float alpha = 1.f - expf(-density[row + s] * dist);
            const float p = ray::product_scan((1.f - alpha) + 1e-10f, lane);
            carry = ray::next_carry(p, carry);
            if (lane == k + 1) carries = carry;
        }
    }

    float b_in = 0.f;                               // B of the chunk's last position
    for (int k = chunks - 1; k >= 0; --k) {
        const int s = k * kWave + lane;
        const bool valid = s < S;
        float alpha = 0.f, f = 1.f, z = 0.f, dist = 0.f, e = 1.f;
        if (valid) {
            dist = ray::sample_dist(z_vals, row, s, S, z);
            e = expf(-density[row + s] * dist);
            alpha = 1.f - e;
            f = (1.f - alpha) + 1e-10f;
        }
        const float p = ray::product_scan(f, lane);
        const float T = ray::transmittance(p, __shfl(carries, k, 64), lane);
        const float w = alpha * T;                  // the forward's weight
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (valid && color) { c0 = color[3 * (row + s)]; c1 = color[3 * (row + s) + 1]; c2 = color[3 * (row + s) + 2]; }
        const float gw = valid && g_w ? g_w[row + s] : 0.f;
        const float g = G0 * c0 + G1 * c1 + G2 * c2 + Ga + Gd * z + gw;
        // Q_l = M_l o .. o M_63 as (A, C)
        float A = f, C = alpha * g;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const float Ao = __shfl_down(A, o, 64), Co = __shfl_down(C, o, 64);
            if (lane + o < kWave) { C = A * Co + C; A = A * Ao; }
        }
        const float An = __shfl_down(A, 1, 64), Cn = __shfl_down(C, 1, 64);
        const float B = lane == kWave - 1 ? b_in : An * b_in + Cn;
        b_in = __shfl(A, 0, 64) * b_in + __shfl(C, 0, 64);
        if (valid) {
            if (grad_density) grad_density[row + s] = T * (g - B) * dist * e;
            if (grad_color) { grad_color[3 * (row + s)] = w * G0; grad_color[3 * (row + s) + 1] = w * G1; grad_color[3 * (row + s) + 2] = w * G2; }
        }
    }
}

// ---- LaplaceDensity -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) laplace_density_kernel(const float* __restrict__ sdf, long long N, const float* __restrict__ beta,
                                                                   float* __restrict__ density)
{
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const float b = fabsf(beta[0]) + 1e-4f;
    density[n] = mlp::sdf_density(-sdf[n], b, 1.0f / b);
}

// A wavefront owns kGroups consecutive groups of 64 elements; its float64 partial goes to partials[wave].
__global__ void __launch_bounds__(kThreads) laplace_density_backward_kernel(const float* __restrict__ sdf, const float* __restrict__ g_density, long long N,
                                                                            const float* __restrict__ beta, float* __restrict__ grad_sdf,
                                                                            double* __restrict__ partials)
{
    const long long wave = (long long)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long first = wave * (kGroups * kWave);
    if (first >= N) return;                         // a whole wavefront
    const float b = fabsf(beta[0]) + 1e-4f;
    const float inv = 1.0f / b;
    // all of the wavefront's loads first, eight groups in flight (measured: the same 113 us at 16.7 M elements as loading group by
    // group, so load latency is not what bounds it; what does has not been measured)
    float sv[kGroups], gv[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const long long n = first + j * kWave + lane;
        sv[j] = n < N ? sdf[n] : 0.f;
        gv[j] = n < N ? g_density[n] : 0.f;
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const long long n = first + j * kWave + lane;
        float term = 0.f;
        if (n < N) {
            const float v = -sv[j], g = gv[j];
            const float sgn = v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
            const float av = fabsf(v);
            const float ex = expf(-av / b);
            if (grad_sdf) grad_sdf[n] = g * ((sgn * sgn * ex) / ((2.0f * b) * b));
            const float dens = mlp::sdf_density(v, b, inv);
            term = g * (-dens / b + (((inv * 0.5f) * sgn) * ex) * av / (b * b));
        }
        if (partials) sum = sum + (double)wave_sum(term);      // uniform: partials is a kernel argument
    }
    if (partials && lane == 0) partials[wave] = sum;
}

// One wavefront: 64 consecutive runs of the W partials, then the 64 run sums, all float64 in index order.
__global__ void __launch_bounds__(kWave) laplace_beta_fold_kernel(const double* __restrict__ partials, long long W, const float* __restrict__ beta,
                                                                 float* __restrict__ grad_beta)
{
    const int lane = threadIdx.x;
    const long long run = (W + kWave - 1) / kWave;
    const long long lo = lane * run, hi = lo + run < W ? lo + run : W;
    double sum = 0.0;
    for (long long i = lo; i < hi; ++i) sum = sum + partials[i];
    double total = 0.0;
    for (int l = 0; l < kWave; ++l) total = total + __shfl(sum, l, 64);
    if (lane == 0) {
        const float bt = beta[0];
        const float sgn = bt > 0.0f ? 1.0f : (bt < 0.0f ? -1.0f : 0.0f);
        grad_beta[0] = W == 0 ? 0.f : sgn * (float)total;
    }
}

}  // namespace
}  // namespace ag

using namespace ag;

extern "C" int ag_ray_composite_backward(const float* density, const float* color, const float* z_vals, int64_t R, int32_t S, int32_t white_bkgd,
                                         const float* g_rgb_map, const float* g_acc_map, const float* g_depth_map, const float* g_weights,
                                         float* grad_density, float* grad_color, void* stream)
{
    if (ray::bad_counts("ray composite backward", (long long)R, S)) return AG_ERR_INVALID_ARGUMENT;
    if ((color == nullptr) != (g_rgb_map == nullptr)) { set_error("ray composite backward: color and g_rgb_map go together"); return AG_ERR_INVALID_ARGUMENT; }
    if (grad_color && !color) { set_error("ray composite backward: grad_color needs color and g_rgb_map"); return AG_ERR_INVALID_ARGUMENT; }
    if (!grad_density && !grad_color) { set_error("ray composite backward: neither grad_density nor grad_color is asked for"); return AG_ERR_INVALID_ARGUMENT; }
    if (R == 0) return AG_OK;
    if (!density || !z_vals) { set_error("null pointer in ag_ray_composite_backward"); return AG_ERR_INVALID_ARGUMENT; }
    const int per = kThreads / kWave;
    hipLaunchKernelGGL(ray_composite_backward_kernel, dim3((unsigned)(((long long)R + per - 1) / per)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), density, color, z_vals, (long long)R, (int)S, (int)white_bkgd, g_rgb_map, g_acc_map, g_depth_map,
                       g_weights, grad_density, grad_color);
    return check_hip(hipGetLastError(), "ray_composite_backward_kernel");
}

extern "C" int ag_laplace_density(const float* sdf, int64_t N, const float* beta, float* density, void* stream)
{
    if (N < 0 || N > kMaxElements) { set_error("laplace density: N = %lld is outside 0 .. 2^33", (long long)N); return AG_ERR_INVALID_ARGUMENT; }
    if (N == 0) return AG_OK;
    if (!sdf || !beta || !density) { set_error("null pointer in ag_laplace_density"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(laplace_density_kernel, dim3((unsigned)(((long long)N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), sdf, (long long)N, beta, density);
    return check_hip(hipGetLastError(), "laplace_density_kernel");
}

extern "C" size_t ag_laplace_density_backward_workspace_bytes(int64_t N)
{
    const long long per = (long long)kGroups * kWave;
    const long long waves = N > 0 ? ((long long)N + per - 1) / per : 0;
    return sizeof(double) * (size_t)(waves > 1 ? waves : 1);
}

extern "C" int ag_laplace_density_backward(const float* sdf, const float* g_density, int64_t N, const float* beta, float* grad_sdf, float* grad_beta,
                                           void* workspace, void* stream)
{
    if (N < 0 || N > kMaxElements) { set_error("laplace density backward: N = %lld is outside 0 .. 2^33", (long long)N); return AG_ERR_INVALID_ARGUMENT; }
    if (!grad_sdf && !grad_beta) { set_error("laplace density backward: neither grad_sdf nor grad_beta is asked for"); return AG_ERR_INVALID_ARGUMENT; }
    if (!beta) { set_error("laplace density backward: beta is null"); return AG_ERR_INVALID_ARGUMENT; }
    if (grad_beta && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7))) {
        set_error("laplace density backward: grad_beta needs an 8-byte aligned workspace");
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (N > 0 && (!sdf || !g_density)) { set_error("null pointer in ag_laplace_density_backward"); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long per = (long long)kGroups * kWave;
    const long long waves = ((long long)N + per - 1) / per;
    double* partials = grad_beta ? reinterpret_cast<double*>(workspace) : nullptr;
    if (N > 0) {
        const int wpb = kThreads / kWave;
        hipLaunchKernelGGL(laplace_density_backward_kernel, dim3((unsigned)((waves + wpb - 1) / wpb)), dim3(kThreads), 0, s, sdf, g_density, (long long)N,
                           beta, grad_sdf, partials);
        if (int rc = check_hip(hipGetLastError(), "laplace_density_backward_kernel")) return rc;
    }
    if (grad_beta) {
        hipLaunchKernelGGL(laplace_beta_fold_kernel, dim3(1), dim3(kWave), 0, s, partials, waves, beta, grad_beta);
        return check_hip(hipGetLastError(), "laplace_beta_fold_kernel");
    }
    return AG_OK;
}
