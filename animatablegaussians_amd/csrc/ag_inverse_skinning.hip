// Inverse skinning (include/ag_inverse_skinning.h): the Sobel gradient of the blend-weight volume, the initial guess from the inverse
// of the blended joint matrix, and the damped Newton iteration of the reference's root_finding.cu.
//
// Shape of the root finder.  The reference gives every thread one point and keeps the joint matrices, the weight row and the gradient
// row in per-thread arrays (about 900 floats of local memory).  Here a GROUP OF 16 LANES (one DPP row) serves one point:
//   * a volume row is contiguous in j, so lane l takes j = l, l + 16, ... and the group reads each of the 27 rows around the node in
//     64-byte segments (one thread per point would read them with a stride of 4 J bytes between lanes);
//   * the 24 sums (blended matrix 12, J2 9, forward point 3) are streamed over j in registers and folded across the row with four DPP
//     row rotations each (8, 4, 2, 1): fp32 addition commutes, so every lane ends with the bits of the header's tree and all 16 lanes
//     take the 3 x 3 step redundantly, keeping xc in registers; nothing goes through LDS between iterations;
//   * a workgroup (256 threads = 16 groups, 4 rounds = 64 points) serves points of ONE batch, so that batch's matrices (top three rows,
//     12 J floats, at most 6 KB) are staged in LDS once per workgroup.
// A group is wholly active or wholly inactive (the point's mask, the tail of the batch), so a DPP read never meets a lane that is off.
// Latency bound by design: ten dependent iterations of (node -> 27 row reads -> fold -> step) per point; many groups per CU hide it.
//
// What one lane does is a host-callable function, so profiles/ub/inverse_skinning_host_walk.hip runs every lane of every group on the
// CPU under the host sanitizers.  Compiled WITHOUT fp contraction (build.sh EXACT): the header states rounded fp32 operations.
#include "ag_common.h"
#include "../../include/ag_inverse_skinning.h"

#define AG_IS_FN __host__ __device__ __forceinline__

namespace ag {
namespace invskin {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                      // lanes per point: one DPP row
constexpr int kGroups = kThreads / kGroup;      // points per round
constexpr int kRounds = 4;
constexpr int kPointsPerBlock = kGroups * kRounds;
constexpr int kMaxJ = 128;

struct VolArgs {
    int X, Y, Z, J;
    float k[3];             // 1 / (32 * spacing_d)
    float lo[3], len[3];    // bounds[0], bounds[1] - bounds[0]
    float lambda;
    int iterations;
    long long N;            // points per batch
};

// the header's Sobel expression at (x, y, z), channel j.  Every read is unconditional: a neighbour outside the grid is read from `zero`
// (the address of one 0.f) instead, so validity costs an address select and nothing per value.
// The three x planes are a LOOP, not unrolled: unrolled, the compiler keeps the 26 neighbour addresses and their validity masks live
// across the channel loop of the root finder (167 VGPRs and 64 spilled SGPRs at J = 55); plane by plane it holds 9.  s(0) is kept for
// out_0; e and r are needed only in the sums ((.(0) + 2 .(1)) + .(2)), which the loop forms in that order (the first term is copied,
// not added to a zero).
AG_IS_FN void sobel_node(const VolArgs& a, const float* __restrict__ vol, const float* __restrict__ zero, int x, int y, int z, int j, float g[3])
{
    const long long sz = a.J, sy = (long long)a.Z * a.J, sx = (long long)a.Y * sy;
    const float* centre = vol + ((((long long)x * a.Y + y) * a.Z + z) * a.J + j);
    // bit 3 db + dc: neighbour (db, dc) of a plane lies in the grid (one register; nine masks would live in eighteen SGPRs)
    const unsigned my = (y > 0 ? 1u : 0u) | 2u | (y + 1 < a.Y ? 4u : 0u), mz = (z > 0 ? 1u : 0u) | 2u | (z + 1 < a.Z ? 4u : 0u);
    const unsigned in_yz = ((my & 1u) ? mz : 0u) | (mz << 3) | ((my & 4u) ? mz << 6 : 0u);
    float s0 = 0.f, s2 = 0.f, es = 0.f, rs = 0.f;
#pragma unroll 1
    for (int da = 0; da < 3; ++da) {
        const unsigned in = (da == 0 ? x > 0 : (da == 1 || x + 1 < a.X)) ? in_yz : 0u;
        const float* plane = centre + (da - 1) * sx;
        float t[3], q[3];
#pragma unroll
        for (int db = 0; db < 3; ++db) {
            float v[3];
#pragma unroll
            for (int dc = 0; dc < 3; ++dc) v[dc] = *(((in >> (3 * db + dc)) & 1u) ? plane + ((db - 1) * sy + (dc - 1) * sz) : zero);
            t[db] = (v[0] + 2.f * v[1]) + v[2];             // t(1, 1), the only user of the centre, is itself never used
            q[db] = v[2] - v[0];
        }
        const float s = (t[0] + 2.f * t[1]) + t[2];         // s(1) is never used
        const float e = t[2] - t[0];
        const float r = (q[0] + 2.f * q[1]) + q[2];
        if (da == 0) { s0 = s; es = e; rs = r; }
        else if (da == 1) { es = es + 2.f * e; rs = rs + 2.f * r; }
        else { s2 = s; es = es + e; rs = rs + r; }
    }
    g[0] = (s2 - s0) * a.k[0];
    g[1] = es * a.k[1];
    g[2] = rs * a.k[2];
}

AG_IS_FN int axis_node(float p, float lo, float len, int R)
{
    float u = (p - lo) / len;
    u = fmaxf(fminf(u, 1.f), 0.f);                  // fminf(NaN, 1) = 1: always a node of the grid
    return (int)roundf((float)(R - 1) * u);
}

// d, the adjugate and inv = adj * (1.f / d) of the header; m is row-major with `stride` floats per row
AG_IS_FN void inverse3(const float* m, int stride, float inv[9])
{
    const float m00 = m[0], m01 = m[1], m02 = m[2];
    const float m10 = m[stride], m11 = m[stride + 1], m12 = m[stride + 2];
    const float m20 = m[2 * stride], m21 = m[2 * stride + 1], m22 = m[2 * stride + 2];
    const float d = m00 * m11 * m22 - m00 * m12 * m21 - m01 * m10 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20;
    const float rd = 1.f / d;
    inv[0] = (m11 * m22 - m12 * m21) * rd;
    inv[1] = -(m01 * m22 - m02 * m21) * rd;
    inv[2] = (m01 * m12 - m02 * m11) * rd;
    inv[3] = -(m10 * m22 - m12 * m20) * rd;
    inv[4] = (m00 * m22 - m02 * m20) * rd;
    inv[5] = -(m00 * m12 - m02 * m10) * rd;
    inv[6] = (m10 * m21 - m11 * m20) * rd;
    inv[7] = -(m00 * m21 - m01 * m20) * rd;
    inv[8] = (m00 * m11 - m01 * m10) * rd;
}

// acc: m[12] (rows of 4), j2[9], f[3] of one lane at the node of xc; mats: [J, 12], the batch's top three rows
template <bool PRE>
AG_IS_FN void lane_partial(const VolArgs& a, const float* __restrict__ vol, const float* __restrict__ grad, const float* __restrict__ zero, const float* mats, const float xc[3], int lane,
                           float acc[24])
{
    const int nx = axis_node(xc[0], a.lo[0], a.len[0], a.X);
    const int ny = axis_node(xc[1], a.lo[1], a.len[1], a.Y);
    const int nz = axis_node(xc[2], a.lo[2], a.len[2], a.Z);
    const long long node = ((long long)nx * a.Y + ny) * a.Z + nz;
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0.f;
    for (int j = lane; j < a.J; j += kGroup) {
        const float w = vol[node * a.J + j];
        float g[3];
        if (PRE) {
            const float* gp = grad + (node * a.J + j) * 3;
            g[0] = gp[0]; g[1] = gp[1]; g[2] = gp[2];
        } else {
            sobel_node(a, vol, zero, nx, ny, nz, j, g);
        }
        const float* A = mats + 12 * j;
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = acc[i] + w * A[i];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float s = ((A[4 * r] * xc[0] + A[4 * r + 1] * xc[1]) + A[4 * r + 2] * xc[2]) + A[4 * r + 3];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[12 + 3 * r + c] = acc[12 + 3 * r + c] + s * g[c];
            acc[21 + r] = acc[21 + r] + w * s;
        }
    }
}

// the step from the folded sums
AG_IS_FN void newton_step(const VolArgs& a, const float acc[24], const float xt[3], float xc[3])
{
    float jac[9], inv[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) jac[3 * r + c] = acc[4 * r + c] + acc[12 + 3 * r + c] * a.lambda;
    inverse3(jac, 3, inv);
    const float d0 = acc[21] - xt[0], d1 = acc[22] - xt[1], d2 = acc[23] - xt[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float up = (inv[3 * r] * d0 + inv[3 * r + 1] * d1) + inv[3 * r + 2] * d2;
        up = fmaxf(fminf(up, 0.01f), -0.01f);       // a NaN becomes +0.01
        xc[r] = xc[r] - up;
    }
}

// one point of ag_inverse_skinning_init; mats: [J, 12]
AG_IS_FN void init_point(int J, const float* __restrict__ w, const float* mats, const float p[3], const float n[3], float out_p[3], float out_n[3])
{
    float m[12], inv[9];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = 0.f;
    for (int j = 0; j < J; ++j) {
        const float wj = w[j];
        const float* A = mats + 12 * j;
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = m[i] + wj * A[i];
    }
    inverse3(m, 4, inv);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float s = -((inv[3 * r] * m[3] + inv[3 * r + 1] * m[7]) + inv[3 * r + 2] * m[11]);
        out_p[r] = ((inv[3 * r] * p[0] + inv[3 * r + 1] * p[1]) + inv[3 * r + 2] * p[2]) + s;
        out_n[r] = (inv[3 * r] * n[0] + inv[3 * r + 1] * n[1]) + inv[3 * r + 2] * n[2];
    }
}

#ifndef AG_INVERSE_SKINNING_HOST_ONLY
__device__ float g_zero = 0.f;           // what a neighbour outside the grid reads; never written (not const: a constant-space address
                                         // beside global ones would turn the selected reads into flat loads)

template <int CTRL>
__device__ __forceinline__ float row_read(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// v + the value 8, then 4, 2, 1 lanes round the 16-lane row: the header's tree in every lane
__device__ __forceinline__ float row_fold(float v)
{
    v = v + row_read<0x128>(v);         // row_ror:8
    v = v + row_read<0x124>(v);         // row_ror:4
    v = v + row_read<0x122>(v);         // row_ror:2
    v = v + row_read<0x121>(v);         // row_ror:1
    return v;
}

__device__ __forceinline__ void stage_matrices(float* s_mats, const float* __restrict__ jnt_mats, int J)
{
    for (int i = threadIdx.x; i < 12 * J; i += blockDim.x) s_mats[i] = jnt_mats[(i / 12) * 16 + i % 12];
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads) gradient_kernel(VolArgs a, long long total, const float* __restrict__ vol, float* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total) return;
    const long long node = (long long)((unsigned long long)t / (unsigned)a.J);
    const int j = (int)(t - node * a.J);
    const long long xy = node / a.Z;
    const int z = (int)(node - xy * a.Z), y = (int)(xy % a.Y), x = (int)(xy / a.Y);
    float g[3];
    sobel_node(a, vol, &g_zero, x, y, z, j, g);
    out[3 * t] = g[0];
    out[3 * t + 1] = g[1];
    out[3 * t + 2] = g[2];
}

__global__ void __launch_bounds__(kThreads) init_kernel(long long N, int J, const float* __restrict__ points, const float* __restrict__ weights,
                                                        const float* __restrict__ jnt_mats, const float* __restrict__ normals,
                                                        float* __restrict__ out_points, float* __restrict__ out_normals)
{
    __shared__ float s_mats[12 * kMaxJ];
    const long long b = blockIdx.y;
    stage_matrices(s_mats, jnt_mats + b * J * 16, J);
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const long long i = b * N + n;
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    float nn[3] = {0.f, 0.f, 0.f}, op[3], on[3];
    if (normals) { nn[0] = normals[3 * i]; nn[1] = normals[3 * i + 1]; nn[2] = normals[3 * i + 2]; }
    init_point(J, weights + i * J, s_mats, p, nn, op, on);
    out_points[3 * i] = op[0]; out_points[3 * i + 1] = op[1]; out_points[3 * i + 2] = op[2];
    if (normals) { out_normals[3 * i] = on[0]; out_normals[3 * i + 1] = on[1]; out_normals[3 * i + 2] = on[2]; }
}

template <bool PRE>
__global__ void __launch_bounds__(kThreads) root_find_kernel(VolArgs a, const float* __restrict__ vol, const float* __restrict__ grad,
                                                             const float* __restrict__ xt_all, const float* xc_init, const float* __restrict__ jnt_mats,
                                                             const uint8_t* __restrict__ active, float* xc_out)
{
    __shared__ float s_mats[12 * kMaxJ];
    const long long b = blockIdx.y;
    stage_matrices(s_mats, jnt_mats + b * a.J * 16, a.J);
    const int group = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    for (int round = 0; round < kRounds; ++round) {
        const long long n = (long long)blockIdx.x * kPointsPerBlock + round * kGroups + group;
        if (n >= a.N) break;                                            // the same in all 16 lanes of the group
        const long long i = b * a.N + n;
        float xc[3] = {xc_init[3 * i], xc_init[3 * i + 1], xc_init[3 * i + 2]};
        if (!active || active[i]) {
            const float xt[3] = {xt_all[3 * i], xt_all[3 * i + 1], xt_all[3 * i + 2]};
            for (int it = 0; it < a.iterations; ++it) {
                float acc[24];
                lane_partial<PRE>(a, vol, grad, &g_zero, s_mats, xc, lane, acc);
#pragma unroll
                for (int k = 0; k < 24; ++k) acc[k] = row_fold(acc[k]);
                newton_step(a, acc, xt, xc);
            }
        }
        if (lane == 0) { xc_out[3 * i] = xc[0]; xc_out[3 * i + 1] = xc[1]; xc_out[3 * i + 2] = xc[2]; }
    }
}
#endif  // AG_INVERSE_SKINNING_HOST_ONLY

inline int check_volume(const char* what, int X, int Y, int Z, int J)
{
    if (X < 2 || Y < 2 || Z < 2) { set_error("%s: every resolution must be at least 2, got %d x %d x %d", what, X, Y, Z); return AG_ERR_INVALID_ARGUMENT; }
    if (J < 1 || J > kMaxJ) { set_error("%s: J = %d is outside 1 .. %d", what, J, kMaxJ); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

inline int set_spacing(const char* what, const float* spacing, VolArgs& a)
{
    if (!spacing) { set_error("%s: spacing is NULL", what); return AG_ERR_INVALID_ARGUMENT; }
    for (int d = 0; d < 3; ++d) {
        if (!(spacing[d] > 0.f) || !(spacing[d] < 3e38f)) { set_error("%s: spacing[%d] = %g is not finite and positive", what, d, (double)spacing[d]); return AG_ERR_INVALID_ARGUMENT; }
        a.k[d] = 1.f / (32.f * spacing[d]);
    }
    return AG_OK;
}

// the launch-independent part of ag_inverse_skinning_root_find: every refusal, and the arguments of the kernel
inline int make_root_args(int X, int Y, int Z, int J, const float* bounds, const float* spacing, int B, long long N, float lambda, int iterations, VolArgs& a)
{
    if (int rc = check_volume("inverse skinning root_find", X, Y, Z, J)) return rc;
    if (N < 0 || iterations < 0 || B < 0 || B > 65535) {
        set_error("inverse skinning root_find: bad sizes B = %d, N = %lld, iterations = %d", B, N, iterations);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (N > 0x7fffffffll * kPointsPerBlock) { set_error("inverse skinning root_find: N = %lld exceeds one launch", N); return AG_ERR_INVALID_ARGUMENT; }
    if (!bounds) { set_error("inverse skinning root_find: bounds is NULL"); return AG_ERR_INVALID_ARGUMENT; }
    a.X = X; a.Y = Y; a.Z = Z; a.J = J;
    if (int rc = set_spacing("inverse skinning root_find", spacing, a)) return rc;
    for (int d = 0; d < 3; ++d) { a.lo[d] = bounds[d]; a.len[d] = bounds[3 + d] - bounds[d]; }
    a.lambda = lambda;
    a.iterations = iterations;
    a.N = N;
    return AG_OK;
}

}  // namespace invskin
}  // namespace ag

#ifndef AG_INVERSE_SKINNING_HOST_ONLY
using namespace ag;
using namespace ag::invskin;

extern "C" int ag_weight_volume_gradient(const float* volume, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* spacing, float* out, void* stream)
{
    if (int rc = check_volume("weight volume gradient", X, Y, Z, C)) return rc;
    VolArgs a = {};
    a.X = X; a.Y = Y; a.Z = Z; a.J = C;
    if (int rc = set_spacing("weight volume gradient", spacing, a)) return rc;
    if (!volume || !out) { set_error("null pointer in ag_weight_volume_gradient"); return AG_ERR_INVALID_ARGUMENT; }
    const long long total = (long long)X * Y * Z * C;
    if (total > 0x7fffffffll * kThreads) { set_error("weight volume gradient: %lld elements exceed one launch", total); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(gradient_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a, total,
                       volume, out);
    return check_hip(hipGetLastError(), "gradient_kernel");
}

extern "C" int ag_inverse_skinning_init(const float* points, const float* weights, const float* jnt_mats, const float* normals, float* out_points,
                                        float* out_normals, int32_t B, int64_t N, int32_t J, void* stream)
{
    if (J < 1 || J > kMaxJ) { set_error("inverse skinning init: J = %d is outside 1 .. %d", J, kMaxJ); return AG_ERR_INVALID_ARGUMENT; }
    if (N < 0 || B < 0 || B > 65535 || N > 0x7fffffffll * kThreads) {
        set_error("inverse skinning init: bad sizes B = %d, N = %lld", B, (long long)N);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if ((normals == nullptr) != (out_normals == nullptr)) { set_error("inverse skinning init: normals and out_normals go together"); return AG_ERR_INVALID_ARGUMENT; }
    if (N == 0 || B == 0) return AG_OK;
    if (!points || !weights || !jnt_mats || !out_points) { set_error("null pointer in ag_inverse_skinning_init"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       (long long)N, (int)J, points, weights, jnt_mats, normals, out_points, out_normals);
    return check_hip(hipGetLastError(), "init_kernel");
}

extern "C" int ag_inverse_skinning_root_find(const float* volume, const float* grad, int32_t X, int32_t Y, int32_t Z, int32_t J, const float* bounds,
                                             const float* spacing, const float* xt, const float* xc_init, const float* jnt_mats, const uint8_t* active,
                                             float* xc_out, int32_t B, int64_t N, float lambda, int32_t iterations, void* stream)
{
    VolArgs a = {};
    if (int rc = make_root_args(X, Y, Z, J, bounds, spacing, B, (long long)N, lambda, iterations, a)) return rc;
    if (N == 0 || B == 0) return AG_OK;
    if (!volume || !xt || !xc_init || !jnt_mats || !xc_out) { set_error("null pointer in ag_inverse_skinning_root_find"); return AG_ERR_INVALID_ARGUMENT; }
    const dim3 grid((unsigned)((N + kPointsPerBlock - 1) / kPointsPerBlock), (unsigned)B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (grad) hipLaunchKernelGGL(root_find_kernel<true>, grid, dim3(kThreads), 0, s, a, volume, grad, xt, xc_init, jnt_mats, active, xc_out);
    else hipLaunchKernelGGL(root_find_kernel<false>, grid, dim3(kThreads), 0, s, a, volume, grad, xt, xc_init, jnt_mats, active, xc_out);
    return check_hip(hipGetLastError(), "root_find_kernel");
}
#endif  // AG_INVERSE_SKINNING_HOST_ONLY
