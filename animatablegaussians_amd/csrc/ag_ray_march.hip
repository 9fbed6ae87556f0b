// The template stage's ray renderer (include/ag_ray_march.h): near / far of rays against balls around the posed body's vertices, sample
// placement along the rays, alpha compositing.  The field between the last two is ag_template_field.hip.
//
// near_far is compute bound (R x V ball tests, about 40 VALU operations each) and has to fill the chip with 1024 rays (a training
// step) as well as with a million (an image): a ray belongs to a group of G lanes, G chosen from R, and the group's lanes split the
// vertices.  Minimum and maximum are exact, so G never shows in the result.  sample and composite are memory bound: one thread per
// sample with LDS-staged contiguous rows out; one wavefront per ray with one lane per sample, a cross-lane product scan and
// butterfly sums.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states every result as individually rounded fp32 operations, which
// is what the test oracle's float32 restatement (numpy has no FMA) evaluates.
#include <math.h>

#include "ag_common.h"
#include "ag_ray_scan.h"
#include "../../include/ag_ray_march.h"

namespace ag {
namespace {

using ray::bad_counts;

constexpr int kThreads = 256;
constexpr int kVertexTile = 1024;                  // vertices per LDS tile: 12 KiB
constexpr long long kFillLanes = 256ll * 1024;     // lanes that fill the chip: 256 CUs x 4 SIMDs x 4 waves x 64

// ---- near / far ---------------------------------------------------------------------------------------------------------------------
// Lane `sub` of ray `ray`'s group tests vertices sub, sub + G, .. of every tile.  Lanes of one group read consecutive vertices (a stride
// of 3 dwords: no bank is hit twice by 32 lanes), lanes of different groups with the same `sub` read the same address (a broadcast).
// No lane leaves before the last barrier: lanes past R compute on ray R - 1 and do not write.
__global__ void __launch_bounds__(kThreads) ray_near_far_kernel(const float* __restrict__ vertices, int V, const float* __restrict__ ray_o,
                                                                const float* __restrict__ ray_d, long long R, int log2_g, float radius,
                                                                const float* __restrict__ fb_near, const float* __restrict__ fb_far,
                                                                float* __restrict__ near, float* __restrict__ far, uint8_t* __restrict__ hit)
{
    __shared__ float s_v[kVertexTile * 3];
    const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long ray = lane >> log2_g;
    const int G = 1 << log2_g, sub = (int)(lane & (G - 1));
    const long long r = ray < R ? ray : R - 1;
    const float o0 = ray_o[3 * r], o1 = ray_o[3 * r + 1], o2 = ray_o[3 * r + 2];
    const float d0 = ray_d[3 * r], d1 = ray_d[3 * r + 1], d2 = ray_d[3 * r + 2];
    const float a = d0 * d0 + d1 * d1 + d2 * d2;
    const float a4 = 4.f * a;
    const float r2 = radius * radius;
    float lo = INFINITY, hi = -INFINITY;           // folded numerators -b - sqrt(disc) and -b + sqrt(disc)
    int any = 0;
    for (int v0 = 0; v0 < V; v0 += kVertexTile) {
        const int n = min(kVertexTile, V - v0);
        __syncthreads();                            // the previous tile has been read
        for (int i = threadIdx.x; i < 3 * n; i += kThreads) s_v[i] = vertices[3ll * v0 + i];
        __syncthreads();
        for (int j = sub; j < n; j += G) {
            const float x0 = o0 - s_v[3 * j], x1 = o1 - s_v[3 * j + 1], x2 = o2 - s_v[3 * j + 2];
            const float b = 2.f * (d0 * x0 + d1 * x1 + d2 * x2);
            const float c = x0 * x0 + x1 * x1 + x2 * x2 - r2;
            const float disc = b * b - a4 * c;
            if (!((double)disc < 1e-8)) {
                const float s = sqrtf(disc);
                lo = fminf(lo, -b - s);
                hi = fmaxf(hi, -b + s);
                any = 1;
            }
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {          // groups are aligned to G lanes of one wavefront
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        any |= __shfl_xor(any, o, 64);
    }
    if (sub == 0 && ray < R) {
        // x -> x / (2 a) is monotone for the fixed positive 2 a under correct rounding: dividing the folded numerators gives the bits
        // of the minimum / maximum of the per-vertex quotients the header defines
        const float a2 = 2.f * a;
        near[ray] = any ? lo / a2 : (fb_near ? fb_near[ray] : 0.f);
        far[ray] = any ? hi / a2 : (fb_far ? fb_far[ray] : 0.f);
        hit[ray] = (uint8_t)any;
    }
}

// ---- sample placement ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float z_of(float near, float far, float t) { return near * (1.f - t) + far * t; }

// One thread per (ray, sample).  The three coordinates of a thread's point are 12 bytes apart from its neighbour's: the workgroup's
// 768 floats go through LDS and leave as three contiguous rows of 256.  No thread leaves before the barriers.
__global__ void __launch_bounds__(kThreads) ray_sample_kernel(const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                              const float* __restrict__ near, const float* __restrict__ far, long long total, int S,
                                                              const float* __restrict__ t, const float* __restrict__ u, const uint8_t* __restrict__ mask,
                                                              float* __restrict__ z_vals, float* __restrict__ pts, float* __restrict__ viewdirs)
{
    __shared__ float s_p[kThreads * 3];
    const long long base = (long long)blockIdx.x * kThreads;
    const long long i = base + threadIdx.x;
    const bool live = i < total;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f;
    if (live) {
        const long long r = (long long)((unsigned)i / (unsigned)S);      // i < 2^31 (bad_counts)
        const int s = (int)(i - r * S);
        const float nr = near[r], fr = far[r];
        float z = z_of(nr, fr, t[s]);
        if (u && (!mask || mask[r])) {
            const float lower = s == 0 ? z : .5f * (z + z_of(nr, fr, t[s - 1]));
            const float upper = s == S - 1 ? z : .5f * (z_of(nr, fr, t[s + 1]) + z);
            z = lower + (upper - lower) * u[i];
        }
        z_vals[i] = z;
        const float d0 = ray_d[3 * r], d1 = ray_d[3 * r + 1], d2 = ray_d[3 * r + 2];
        p0 = ray_o[3 * r] + d0 * z;
        p1 = ray_o[3 * r + 1] + d1 * z;
        p2 = ray_o[3 * r + 2] + d2 * z;
        if (viewdirs) {
            const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
            w0 = d0 / len; w1 = d1 / len; w2 = d2 / len;
        }
    }
    const long long floats = 3 * (total - base < kThreads ? total - base : (long long)kThreads);   // of this workgroup
    s_p[3 * threadIdx.x] = p0; s_p[3 * threadIdx.x + 1] = p1; s_p[3 * threadIdx.x + 2] = p2;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = k * kThreads + threadIdx.x;
        if (e < floats) pts[3 * base + e] = s_p[e];
    }
    if (viewdirs) {                                 // uniform over the workgroup
        __syncthreads();
        s_p[3 * threadIdx.x] = w0; s_p[3 * threadIdx.x + 1] = w1; s_p[3 * threadIdx.x + 2] = w2;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = k * kThreads + threadIdx.x;
            if (e < floats) viewdirs[3 * base + e] = s_p[e];
        }
    }
}

// ---- compositing ----------------------------------------------------------------------------------------------------------------------
// One wavefront per ray, four rays per workgroup; lane l of chunk k is sample 64 k + l.  The order of the product scan and of the
// sums is the header's, stated once in ag_ray_scan.h for this kernel and the backward.  The loop count is uniform over the wavefront, so every lane takes part in every cross-lane move.
__global__ void __launch_bounds__(kThreads) ray_composite_kernel(const float* __restrict__ density, const float* __restrict__ color,
                                                                 const float* __restrict__ z_vals, long long R, int S, int white_bkgd,
                                                                 float* __restrict__ rgb_map, float* __restrict__ acc_map, float* __restrict__ depth_map,
                                                                 float* __restrict__ disp_map, float* __restrict__ weights)
{
    const long long ray = (long long)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (ray >= R) return;                           // a whole wavefront; there is no barrier in this kernel
    const int lane = threadIdx.x & 63;
    const long long row = ray * S;
    float carry = 1.f, rgb0 = 0.f, rgb1 = 0.f, rgb2 = 0.f, acc = 0.f, depth = 0.f;
    for (int s0 = 0; s0 < S; s0 += kWave) {
        const int s = s0 + lane;
        const bool valid = s < S;
        float alpha = 0.f, f = 1.f, z = 0.f;
        if (valid) {
            const float dist = ray::sample_dist(z_vals, row, s, S, z);
            alpha = 1.f - expf(-density[row + s] * dist);
            f = (1.f - alpha) + 1e-10f;
        }
        const float p = ray::product_scan(f, lane);
        const float T = ray::transmittance(p, carry, lane);
        const float w = alpha * T;                  // 0 past S - 1
        carry = ray::next_carry(p, carry);
        if (valid && weights) weights[row + s] = w;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (valid && color) { c0 = color[3 * (row + s)]; c1 = color[3 * (row + s) + 1]; c2 = color[3 * (row + s) + 2]; }
        const float t0 = wave_sum(w * c0), t1 = wave_sum(w * c1), t2 = wave_sum(w * c2);
        const float ta = wave_sum(w), td = wave_sum(w * z);
        if (s0 == 0) { rgb0 = t0; rgb1 = t1; rgb2 = t2; acc = ta; depth = td; }
        else { rgb0 = rgb0 + t0; rgb1 = rgb1 + t1; rgb2 = rgb2 + t2; acc = acc + ta; depth = depth + td; }
    }
    if (lane == 0) {
        if (rgb_map) {
            const float bg = white_bkgd ? 1.f - acc : 0.f;
            rgb_map[3 * ray] = white_bkgd ? rgb0 + bg : rgb0;
            rgb_map[3 * ray + 1] = white_bkgd ? rgb1 + bg : rgb1;
            rgb_map[3 * ray + 2] = white_bkgd ? rgb2 + bg : rgb2;
        }
        acc_map[ray] = acc;
        if (depth_map) depth_map[ray] = depth;
        if (disp_map) {
            const float q = depth / acc;
            disp_map[ray] = 1.f / (q <= 1e-10f ? 1e-10f : q);     // NaN stays NaN (torch.max)
        }
    }
}

}  // namespace
}  // namespace ag

using namespace ag;

extern "C" int ag_ray_near_far(const float* vertices, int32_t V, const float* ray_o, const float* ray_d, int64_t R, float radius,
                               const float* fallback_near, const float* fallback_far, float* near, float* far, uint8_t* hit, void* stream)
{
    if (V < 1 || R < 0) { set_error("ray near/far: bad sizes V = %d, R = %lld", V, (long long)R); return AG_ERR_INVALID_ARGUMENT; }
    if (R > (1ll << 31)) { set_error("ray near/far: R = %lld rays exceed one launch (2^31)", (long long)R); return AG_ERR_INVALID_ARGUMENT; }
    if (!(radius > 0.f && radius < INFINITY)) { set_error("ray near/far: radius %g must be finite and positive", (double)radius); return AG_ERR_INVALID_ARGUMENT; }
    if ((fallback_near == nullptr) != (fallback_far == nullptr)) {
        set_error("ray near/far: fallback_near and fallback_far go together");
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (R == 0) return AG_OK;
    if (!vertices || !ray_o || !ray_d || !near || !far || !hit) { set_error("null pointer in ag_ray_near_far"); return AG_ERR_INVALID_ARGUMENT; }
    int log2_g = 0;                                 // G = 64 up to 4096 rays, 1 from 262 144
    while (log2_g < 6 && ((long long)R << log2_g) < kFillLanes) ++log2_g;
    const long long blocks = (((long long)R << log2_g) + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(ray_near_far_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), vertices, (int)V, ray_o,
                       ray_d, (long long)R, log2_g, radius, fallback_near, fallback_far, near, far, hit);
    return check_hip(hipGetLastError(), "ray_near_far_kernel");
}

extern "C" int ag_ray_sample(const float* ray_o, const float* ray_d, const float* near, const float* far, int64_t R, const float* t, int32_t S,
                             const float* u, const uint8_t* perturb_mask, float* z_vals, float* pts, float* viewdirs, void* stream)
{
    if (bad_counts("ray sample", (long long)R, S)) return AG_ERR_INVALID_ARGUMENT;
    if (perturb_mask && !u) { set_error("ray sample: a perturb_mask without u"); return AG_ERR_INVALID_ARGUMENT; }
    if (R == 0) return AG_OK;
    if (!ray_o || !ray_d || !near || !far || !t || !z_vals || !pts) { set_error("null pointer in ag_ray_sample"); return AG_ERR_INVALID_ARGUMENT; }
    const long long total = (long long)R * S;
    hipLaunchKernelGGL(ray_sample_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       ray_o, ray_d, near, far, total, (int)S, t, u, perturb_mask, z_vals, pts, viewdirs);
    return check_hip(hipGetLastError(), "ray_sample_kernel");
}

extern "C" int ag_ray_composite(const float* density, const float* color, const float* z_vals, int64_t R, int32_t S, int32_t white_bkgd, float* rgb_map,
                                float* acc_map, float* depth_map, float* disp_map, float* weights, void* stream)
{
    if (bad_counts("ray composite", (long long)R, S)) return AG_ERR_INVALID_ARGUMENT;
    if ((color == nullptr) != (rgb_map == nullptr)) { set_error("ray composite: color and rgb_map go together"); return AG_ERR_INVALID_ARGUMENT; }
    if (R == 0) return AG_OK;
    if (!density || !z_vals || !acc_map) { set_error("null pointer in ag_ray_composite"); return AG_ERR_INVALID_ARGUMENT; }
    const int per = kThreads / kWave;
    hipLaunchKernelGGL(ray_composite_kernel, dim3((unsigned)(((long long)R + per - 1) / per)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       density, color, z_vals, (long long)R, (int)S, (int)white_bkgd, rgb_map, acc_map, depth_map, disp_map, weights);
    return check_hip(hipGetLastError(), "ray_composite_kernel");
}
