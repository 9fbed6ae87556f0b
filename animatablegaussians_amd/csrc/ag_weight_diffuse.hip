// Harmonic extension of the fixed nodes' values through a channel-last [X, Y, Z, C] grid by matrix-free conjugate gradients
// (include/ag_weight_diffuse.h): WeightVolume.diffuse, the project's own `diff_weight_volume`.  Init-time, memory bound.
//
// Mapping: a LANE owns a CHANNEL.  With CP = min(C, 64) channels per pass and G = 64 / CP nodes side by side, lane l of a wave works
// on node (base + l / CP), channel (c0 + l % CP): one wave instruction reads G whole rows, 4 CP G contiguous bytes (220 of 256 at
// C = 55), and a lane's running sum belongs to one channel from the first node to the last, which is what makes the per-channel
// dot products cheap: no cross-lane step per node, one LDS exchange per workgroup at the end.  (One lane per flat element would
// coalesce the last 14 % but turns every lane's channel over every step.)  C > 64 is walked in passes of 64 channels; C = 1 packs
// 64 nodes into a wave.  A wave takes runs of 64 nodes of one z-row, 14 KB contiguous at C = 55, dealt round-robin over at most
// 2048 workgroups of 4 waves; the stencil needs two 32-bit divisions per run, none per node.
//
// Three passes per iteration, each followed by nothing or by a one-wave-per-channel finishing kernel:
//   1  ap = A p, partial sums of p . ap         reads p (the six neighbours come from cache: +-1 row, +-Z rows, +-Y Z rows), writes ap
//      finish: alpha = rr / (p . ap)
//   2  x += alpha p, r -= alpha ap, partial sums of r . r          reads x, r, p, ap, writes x, r
//      finish: beta = rr' / rr, rr = rr'
//   3  p = r + beta p                                              reads r, p, writes p
// Algorithmic traffic: 2 + 6 + 3 = 11 volume passes per iteration, 5.07 GB at 128^3 x 55.  Fusing 3 into the next 1 would need a
// second p (the neighbours must see the old one) to save one pass of eleven; not done.
// p, r, ap and x are zero on fixed nodes, so the stencil reads neighbours unmasked and needs only its own node's mask byte, and
// passes 2 and 3 need no mask at all.
//
// Sums: per lane over its nodes in ascending order, then thread c adds the workgroup's 4 G lanes of channel c from LDS in a fixed
// order, then the finishing kernel's lane l adds partial sums l, l + 64, ... and the wave folds by halves.  No atomics anywhere.
// A neighbour outside the grid is read as the node itself: (u - u) = 0 drops it without a branch, for finite values.
//
// Resources (hipcc, gfx950; profiles/kernel_resources.py prints them): 48 to 68 VGPRs, 96 in pass 2 (four nodes of four vectors in flight: 5 waves
// per SIMD), no scratch; 1 KB of LDS in the kernels that sum.  Compiled WITHOUT fp contraction (build.sh EXACT): the header states rounded fp32 operations.
#include "ag_common.h"
#include "../../include/ag_weight_diffuse.h"

#define AG_WD_FN __host__ __device__ inline

namespace ag {
namespace wdiff {

constexpr int kSeg = 64;          // nodes per run
constexpr int kMaxBlocks = 2048;  // workgroups per launch, rows of the partial-sum table
constexpr int kThreads = 256;

struct DiffArgs {
    int X, Y, Z, C;
    int CP, G;            // channels per pass, nodes side by side in a wave
    unsigned segs;        // runs per z-row
    float wx, wy, wz;
    long long nodes;
};

// thread t < CP of a workgroup adds the 4 G lanes that hold channel c0 + t, in wave then node order
AG_WD_FN float block_sum_thread(const DiffArgs& a, const float* s_part, int t)
{
    float s = 0.f;
    for (int w = 0; w < kThreads / 64; ++w)
        for (int g = 0; g < a.G; ++g) s = s + s_part[w * 64 + g * a.CP + t];
    return s;
}

// Everything thread `tid` of workgroup `block` does for the channel pass c0 of out = A in; returns its share of in . out
template <bool DOT>
AG_WD_FN float stencil_thread(const DiffArgs& a, unsigned items, unsigned block, unsigned blocks, int tid, int c0, const float* __restrict__ in,
                              const uint8_t* __restrict__ fixed, float* __restrict__ out)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = lane / a.CP, cl = lane - sub * a.CP;
    const long long sz = a.C, sy = (long long)a.Z * a.C, sx = (long long)a.Y * sy;
    const int c = c0 + cl;
    const bool ok = sub < a.G && c < a.C;
    float acc = 0.f;
    for (unsigned t = block * (kThreads / 64) + wave; t < items; t += blocks * (kThreads / 64)) {
        const unsigned row = t / a.segs, seg = t - row * a.segs;
        const int i = (int)(row / (unsigned)a.Y), j = (int)row - i * a.Y;
        const int k0 = (int)seg * kSeg, k1 = k0 + kSeg < a.Z ? k0 + kSeg : a.Z;
        const long long xl = i > 0 ? sx : 0, xh = i < a.X - 1 ? sx : 0, yl = j > 0 ? sy : 0, yh = j < a.Y - 1 ? sy : 0;
        const long long row_node = (long long)row * a.Z;
#pragma unroll 2
        for (int k = k0 + sub; ok && k < k1; k += a.G) {
            const long long node = row_node + k;
            const long long e = node * a.C + c;
            const long long zl = k > 0 ? sz : 0, zh = k < a.Z - 1 ? sz : 0;
            const float u = in[e];
            const float dx = (u - in[e - xl]) + (u - in[e + xh]);
            const float dy = (u - in[e - yl]) + (u - in[e + yh]);
            const float dz = (u - in[e - zl]) + (u - in[e + zh]);
            float v = (a.wx * dx + a.wy * dy) + a.wz * dz;
            if (fixed[node]) v = 0.f;
            out[e] = v;
            if (DOT) acc = acc + u * v;
        }
    }
    return acc;
}

enum { M_MASK = 0, M_INIT = 1, M_XR = 2, M_P = 3 };

// Everything thread `tid` of workgroup `block` does for the channel pass c0 of
//   M_MASK  x = fixed ? t : 0                           (u0, parked in x)
//   M_INIT  r = p = 0 - ap, x = 0, its share of r . r
//   M_XR    x += alpha p, r -= alpha ap, its share of r . r
//   M_P     p = r + beta p
// Four nodes' loads are issued before the first of their stores: x and r are read and written through one pointer each, and a
// store in between would hold the later loads back.
template <int MODE>
AG_WD_FN float vector_thread(const DiffArgs& a, unsigned items, unsigned block, unsigned blocks, int tid, int c0, const float* __restrict__ t_in,
                             const uint8_t* __restrict__ fixed, float* __restrict__ x, float* __restrict__ r, float* __restrict__ p,
                             const float* __restrict__ ap, const float* __restrict__ coef)
{
    constexpr int U = 4;
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = lane / a.CP, cl = lane - sub * a.CP;
    const int c = c0 + cl;
    const bool ok = sub < a.G && c < a.C;
    float acc = 0.f;
    float k = 0.f;
    if ((MODE == M_XR || MODE == M_P) && ok) k = coef[c];
    for (unsigned t = block * (kThreads / 64) + wave; t < items; t += blocks * (kThreads / 64)) {
        const long long n0 = (long long)t * kSeg;
        const long long n1 = n0 + kSeg < a.nodes ? n0 + kSeg : a.nodes;
        for (long long nb = n0 + sub; ok && nb < n1; nb += (long long)U * a.G) {
            float v0[U], v1[U], v2[U], v3[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long n = nb + (long long)u * a.G;
                v0[u] = v1[u] = v2[u] = v3[u] = 0.f;
                if (n < n1) {
                    const long long e = n * a.C + c;
                    if (MODE == M_MASK) { v0[u] = t_in[e]; v1[u] = fixed[n] ? 1.f : 0.f; }
                    if (MODE == M_INIT) v0[u] = ap[e];
                    if (MODE == M_XR) { v0[u] = x[e]; v1[u] = r[e]; v2[u] = p[e]; v3[u] = ap[e]; }
                    if (MODE == M_P) { v0[u] = r[e]; v1[u] = p[e]; }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long n = nb + (long long)u * a.G;
                if (n < n1) {
                    const long long e = n * a.C + c;
                    if (MODE == M_MASK) x[e] = v1[u] != 0.f ? v0[u] : 0.f;
                    if (MODE == M_INIT) {
                        const float b = 0.f - v0[u];
                        r[e] = b; p[e] = b; x[e] = 0.f;
                        acc = acc + b * b;
                    }
                    if (MODE == M_XR) {
                        const float rn = v1[u] - k * v3[u];
                        x[e] = v0[u] + k * v2[u];
                        r[e] = rn;
                        acc = acc + rn * rn;
                    }
                    if (MODE == M_P) p[e] = v0[u] + k * v1[u];
                }
            }
        }
    }
    return acc;
}

#ifndef AG_WEIGHT_DIFFUSE_HOST_ONLY
__device__ __forceinline__ void block_sum(const DiffArgs& a, float* s_part, float acc, int c0, float* __restrict__ partial)
{
    s_part[threadIdx.x] = acc;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < a.CP && c0 + t < a.C) partial[(long long)blockIdx.x * a.C + c0 + t] = block_sum_thread(a, s_part, t);
    __syncthreads();
}

// out = A in; DOT: also the workgroup's partial sums of in . out
template <bool DOT>
__global__ void __launch_bounds__(kThreads) stencil_kernel(DiffArgs a, unsigned items, const float* __restrict__ in, const uint8_t* __restrict__ fixed,
                                                           float* __restrict__ out, float* __restrict__ partial)
{
    __shared__ float s_part[kThreads];
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const float acc = stencil_thread<DOT>(a, items, blockIdx.x, gridDim.x, threadIdx.x, c0, in, fixed, out);
        if (DOT) block_sum(a, s_part, acc, c0, partial);
    }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) vector_kernel(DiffArgs a, unsigned items, const float* __restrict__ t_in, const uint8_t* __restrict__ fixed,
                                                          float* __restrict__ x, float* __restrict__ r, float* __restrict__ p, const float* __restrict__ ap,
                                                          const float* __restrict__ coef, float* __restrict__ partial)
{
    __shared__ float s_part[kThreads];
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const float acc = vector_thread<MODE>(a, items, blockIdx.x, gridDim.x, threadIdx.x, c0, t_in, fixed, x, r, p, ap, coef);
        if (MODE == M_INIT || MODE == M_XR) block_sum(a, s_part, acc, c0, partial);
    }
}

#endif  // AG_WEIGHT_DIFFUSE_HOST_ONLY

enum { F_INIT = 0, F_ALPHA = 1, F_BETA = 2 };

// lane l of the finishing wave of channel c adds the workgroups' partial sums l, l + 64, ...
AG_WD_FN float finish_lane_sum(const float* __restrict__ partial, int nb, int C, int c, int lane)
{
    float s = 0.f;
    for (int b = lane; b < nb; b += 64) s = s + partial[(long long)b * C + c];
    return s;
}

// what lane 0 does with the channel's sum s
//   F_INIT   bb = rr = s
//   F_ALPHA  alpha = s > 0 ? rr / s : 0                  (s = p . ap)
//   F_BETA   beta = rr > 0 ? s / rr : 0, rr = s          (s = r . r)
AG_WD_FN void finish_write(int mode, float s, int c, float* __restrict__ rr, float* __restrict__ bb, float* __restrict__ alpha, float* __restrict__ beta)
{
    if (mode == F_INIT) { bb[c] = s; rr[c] = s; }
    if (mode == F_ALPHA) alpha[c] = s > 0.f ? rr[c] / s : 0.f;
    if (mode == F_BETA) { const float old = rr[c]; beta[c] = old > 0.f ? s / old : 0.f; rr[c] = s; }
}

#ifndef AG_WEIGHT_DIFFUSE_HOST_ONLY
// One wave per channel; the 64 lane sums fold by halves (lane l takes lane l + 32, then l + 16, ...).
__global__ void __launch_bounds__(64) finish_kernel(int mode, const float* __restrict__ partial, int nb, int C, float* __restrict__ rr, float* __restrict__ bb,
                                                    float* __restrict__ alpha, float* __restrict__ beta)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    float s = finish_lane_sum(partial, nb, C, c, lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o, 64);
    if (lane == 0) finish_write(mode, s, c, rr, bb, alpha, beta);
}
#endif  // AG_WEIGHT_DIFFUSE_HOST_ONLY

struct Plan {
    DiffArgs a;
    unsigned stencil_items, vector_items;
    int stencil_blocks, vector_blocks;
};

int make_plan(const char* what, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* w, Plan& pl)
{
    if (X < 2 || Y < 2 || Z < 2) { set_error("%s: every resolution must be at least 2, got %d x %d x %d", what, X, Y, Z); return AG_ERR_INVALID_ARGUMENT; }
    if (C < 1) { set_error("%s: bad channel count C = %d", what, C); return AG_ERR_INVALID_ARGUMENT; }
    const long long nodes = (long long)X * Y * Z;
    if (nodes >= 0x7fffffffll) { set_error("%s: %lld nodes exceed 2^31 - 1", what, nodes); return AG_ERR_INVALID_ARGUMENT; }
    DiffArgs& a = pl.a;
    a.X = X; a.Y = Y; a.Z = Z; a.C = C;
    a.CP = C < 64 ? C : 64;
    a.G = 64 / a.CP;
    a.segs = (unsigned)((Z + kSeg - 1) / kSeg);
    a.nodes = nodes;
    a.wx = a.wy = a.wz = 1.f;
    if (w) {
        for (int d = 0; d < 3; ++d)
            if (!(w[d] > 0.f && w[d] <= 1.f)) { set_error("%s: weight %d = %g is not in (0, 1]", what, d, (double)w[d]); return AG_ERR_INVALID_ARGUMENT; }
        a.wx = w[0]; a.wy = w[1]; a.wz = w[2];
    }
    pl.stencil_items = (unsigned)X * (unsigned)Y * a.segs;                 // <= nodes < 2^31
    pl.vector_items = (unsigned)((nodes + kSeg - 1) / kSeg);
    const unsigned per = kThreads / 64;
    pl.stencil_blocks = (int)((pl.stencil_items + per - 1) / per < (unsigned)kMaxBlocks ? (pl.stencil_items + per - 1) / per : kMaxBlocks);
    pl.vector_blocks = (int)((pl.vector_items + per - 1) / per < (unsigned)kMaxBlocks ? (pl.vector_items + per - 1) / per : kMaxBlocks);
    return AG_OK;
}

size_t workspace_bytes(int C) { return (size_t)(kMaxBlocks + 2) * (size_t)C * sizeof(float) + 256; }

struct Work { float *partial, *alpha, *beta; };

Work carve(void* workspace, int C)
{
    Work k;
    k.partial = reinterpret_cast<float*>(aligned_base(workspace));
    k.alpha = k.partial + (size_t)kMaxBlocks * C;
    k.beta = k.alpha + C;
    return k;
}

}  // namespace wdiff
}  // namespace ag

#ifndef AG_WEIGHT_DIFFUSE_HOST_ONLY
using namespace ag;
using namespace ag::wdiff;

extern "C" size_t ag_weight_diffuse_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t C)
{
    if (X < 2 || Y < 2 || Z < 2 || C < 1 || (long long)X * Y * Z >= 0x7fffffffll) return 0;
    return workspace_bytes(C);
}

extern "C" int ag_weight_diffuse_apply(const float* in, const uint8_t* fixed, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* w, float* out,
                                       void* stream)
{
    Plan pl;
    if (!w) { set_error("null pointer in ag_weight_diffuse_apply"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = make_plan("weight diffuse apply", X, Y, Z, C, w, pl)) return rc;
    if (!in || !fixed || !out) { set_error("null pointer in ag_weight_diffuse_apply"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(stencil_kernel<false>, dim3(pl.stencil_blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), pl.a, pl.stencil_items,
                       in, fixed, out, (float*)nullptr);
    return check_hip(hipGetLastError(), "weight_diffuse stencil_kernel");
}

extern "C" int ag_weight_diffuse_init(const float* target, const uint8_t* fixed, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* w, float* x,
                                      float* r, float* p, float* ap, void* workspace, size_t workspace_bytes_given, float* bb, float* rr, void* stream)
{
    Plan pl;
    if (!w) { set_error("null pointer in ag_weight_diffuse_init"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = make_plan("weight diffuse init", X, Y, Z, C, w, pl)) return rc;
    if (!target || !fixed || !x || !r || !p || !ap || !workspace || !bb || !rr) { set_error("null pointer in ag_weight_diffuse_init"); return AG_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes_given < workspace_bytes(C)) {
        set_error("weight diffuse init: workspace of %zu bytes, %zu needed", workspace_bytes_given, workspace_bytes(C));
        return AG_ERR_INVALID_ARGUMENT;
    }
    const Work k = carve(workspace, C);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float* none = nullptr;
    hipLaunchKernelGGL(vector_kernel<M_MASK>, dim3(pl.vector_blocks), dim3(kThreads), 0, s, pl.a, pl.vector_items, target, fixed, x, r, p, none, none, k.partial);
    hipLaunchKernelGGL(stencil_kernel<false>, dim3(pl.stencil_blocks), dim3(kThreads), 0, s, pl.a, pl.stencil_items, (const float*)x, fixed, ap, k.partial);
    hipLaunchKernelGGL(vector_kernel<M_INIT>, dim3(pl.vector_blocks), dim3(kThreads), 0, s, pl.a, pl.vector_items, none, fixed, x, r, p, (const float*)ap, none,
                       k.partial);
    hipLaunchKernelGGL(finish_kernel, dim3(C), dim3(64), 0, s, (int)F_INIT, (const float*)k.partial, pl.vector_blocks, (int)C, rr, bb, k.alpha, k.beta);
    return check_hip(hipGetLastError(), "weight_diffuse init");
}

extern "C" int ag_weight_diffuse_iterate(const uint8_t* fixed, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* w, int32_t n, float* x, float* r,
                                         float* p, float* ap, void* workspace, size_t workspace_bytes_given, float* rr, void* stream)
{
    Plan pl;
    if (!w) { set_error("null pointer in ag_weight_diffuse_iterate"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = make_plan("weight diffuse iterate", X, Y, Z, C, w, pl)) return rc;
    if (n < 0) { set_error("weight diffuse iterate: n = %d iterations", n); return AG_ERR_INVALID_ARGUMENT; }
    if (!fixed || !x || !r || !p || !ap || !workspace || !rr) { set_error("null pointer in ag_weight_diffuse_iterate"); return AG_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes_given < workspace_bytes(C)) {
        set_error("weight diffuse iterate: workspace of %zu bytes, %zu needed", workspace_bytes_given, workspace_bytes(C));
        return AG_ERR_INVALID_ARGUMENT;
    }
    const Work k = carve(workspace, C);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float* none = nullptr;
    float* nobb = nullptr;
    for (int it = 0; it < n; ++it) {
        hipLaunchKernelGGL(stencil_kernel<true>, dim3(pl.stencil_blocks), dim3(kThreads), 0, s, pl.a, pl.stencil_items, (const float*)p, fixed, ap, k.partial);
        hipLaunchKernelGGL(finish_kernel, dim3(C), dim3(64), 0, s, (int)F_ALPHA, (const float*)k.partial, pl.stencil_blocks, (int)C, rr, nobb, k.alpha, k.beta);
        hipLaunchKernelGGL(vector_kernel<M_XR>, dim3(pl.vector_blocks), dim3(kThreads), 0, s, pl.a, pl.vector_items, none, fixed, x, r, p, (const float*)ap,
                           (const float*)k.alpha, k.partial);
        hipLaunchKernelGGL(finish_kernel, dim3(C), dim3(64), 0, s, (int)F_BETA, (const float*)k.partial, pl.vector_blocks, (int)C, rr, nobb, k.alpha, k.beta);
        hipLaunchKernelGGL(vector_kernel<M_P>, dim3(pl.vector_blocks), dim3(kThreads), 0, s, pl.a, pl.vector_items, none, fixed, x, r, p, none,
                           (const float*)k.beta, k.partial);
    }
    return check_hip(hipGetLastError(), "weight_diffuse iterate");
}
#endif  // AG_WEIGHT_DIFFUSE_HOST_ONLY
