// SMPL-X body-model forward for B poses of one subject (gfx950).  See include/ag_smplx.h for the reference lines each
// stage follows.  All of it is HBM / latency bound and tiny next to the render path -- the point of having it on the
// device is that `cano2live_jnt_mats` is produced where it is consumed (no CPU data-loader stage, no upload) and that the
// three model evaluations a data item needs (live, canonical, live without root) read the 61-MB pose-corrective basis
// once.  Three launches per call:
//   shape_kernel   v_shaped = v_template + shapedirs . components           thread per (pose, coordinate)
//   chain_kernel   rest joints, Rodrigues, pose features, kinematic chain, A  one wave per pose, level-synchronous over the tree
//                  (rest joints = J_regressor . v_shaped is linear in the components: J_regressor . v_template and
//                  J_regressor . shapedirs are folded once per model by ag_smplx_prepare -> 60 FMAs per joint instead of a
//                  10475-long reduction per joint and pose)
//   skin_kernel    pose_offsets = features . posedirs (the 61 MB stream), v_posed, T = W . A, vertices
//                  workgroup = 32 vertices x 8 slices of the 486 features; lanes along coordinates (256-B segments)
// The backward of the kinematic chain is one launch (chain_backward_kernel); the backward of the vertex path (key points, skinning,
// the two bases transposed) is the block of kernels after it, ahead of the host functions.  What a forward kernel and its backward must
// agree on bit for bit is stated once: RodriguesHead, chain_forward (the chain itself), inverse4.
#include <type_traits>

#include "ag_common.h"
#include "../../include/ag_smplx.h"

namespace ag {

constexpr int kMaxJoints = 64;
constexpr int kSkinVerts = 32;                 // vertices per workgroup of skin_kernel
constexpr int kSkinCoords = 3 * kSkinVerts;    // 96 coordinates = 384 B of every posedirs row
constexpr int kSkinSlices = 8;                 // the feature loop is dealt over 8 slices
constexpr int kSkinThreads = kSkinCoords * kSkinSlices;   // 768

__global__ void __launch_bounds__(256) smplx_shape_kernel(float* __restrict__ v_shaped, const float* __restrict__ v_template,
                                                         const float* __restrict__ shapedirs, const float* __restrict__ comps,
                                                         int n_coord, int NB)
{
    extern __shared__ float s_comp[];
    const int b = blockIdx.y;
    for (int l = threadIdx.x; l < NB; l += 256) s_comp[l] = comps[(size_t)b * NB + l];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_coord) return;
    const float* row = shapedirs + (size_t)i * NB;
    float acc = 0.f;
    for (int l = 0; l < NB; ++l) acc = fmaf(s_comp[l], row[l], acc);
    v_shaped[(size_t)b * n_coord + i] = v_template[i] + acc;
}

// out[(j * 3 + c) * out_stride + b] = sum_v J_regressor[j][v] * src[(3 v + c) * src_stride + b]   (once per model: folds
// the regressor into v_template (stride 1, one column) and into every column of shapedirs (stride NB, NB columns))
__global__ void __launch_bounds__(256) smplx_joints_kernel(float* __restrict__ out, const float* __restrict__ J_regressor,
                                                          const float* __restrict__ src, int V, int src_stride, int out_stride)
{
    __shared__ float s_part[4][3];
    const int j = blockIdx.x, b = blockIdx.y;
    const float* reg = J_regressor + (size_t)j * V;
    const float* vs = src + b;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float w = reg[v];
        a0 = fmaf(w, vs[(size_t)(3 * v + 0) * src_stride], a0);
        a1 = fmaf(w, vs[(size_t)(3 * v + 1) * src_stride], a1);
        a2 = fmaf(w, vs[(size_t)(3 * v + 2) * src_stride], a2);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_part[wave][0] = a0; s_part[wave][1] = a1; s_part[wave][2] = a2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        out[(size_t)(j * 3 + c) * out_stride + b] = (s_part[0][c] + s_part[1][c]) + (s_part[2][c] + s_part[3][c]);
    }
}

struct Affine {   // [R | t], last row (0 0 0 1) implied
    float r[9], t[3];
};

// lbs.py:299-330, what rodrigues() and its backward both start from: R = I + s K + c1 K K with angle = |rv + 1e-8|, K = skew(rv / angle),
// s = sin(angle), c1 = 1 - cos(angle).  The `+ 1e-8` goes into the norm only (e), the direction divides the untouched vector by it.
struct RodriguesHead {
    float e[3], angle, s, co, c1, K[9];
    __device__ __forceinline__ explicit RodriguesHead(const float* rv)
    {
        for (int c = 0; c < 3; ++c) e[c] = rv[c] + 1e-8f;
        angle = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        const float rx = rv[0] / angle, ry = rv[1] / angle, rz = rv[2] / angle;
        s = sinf(angle), co = cosf(angle), c1 = 1.f - co;
        const float k[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
        for (int i = 0; i < 9; ++i) K[i] = k[i];
    }
};

__device__ __forceinline__ void rodrigues(const float* rv, float* R)
{
    const RodriguesHead h(rv);
    const float s = h.s, c1 = h.c1;
    const float* K = h.K;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float kk = 0.f;
            for (int k = 0; k < 3; ++k) kk = fmaf(K[3 * r + k], K[3 * k + c], kk);
            R[3 * r + c] = (r == c ? 1.f : 0.f) + s * K[3 * r + c] + c1 * kk;
        }
}

// The kinematic chain of one pose, by the one wave of its workgroup (lane = joint): what smplx_chain_kernel writes out and what
// smplx_chain_backward_kernel recomputes, in one place so that the two agree bit for bit.
struct alignas(16) ChainShared {    // in LDS.  16: an Affine is three 16-byte accesses
    Affine glob[kMaxJoints];        // global transforms: G_j = G_parent [R_j | t_j]
    float rest[kMaxJoints][3];      // rest joints
    int par[kMaxJoints];
    int maxdepth;
};

struct ChainLane {                  // what a joint's lane keeps in registers
    Affine loc;                     // [R_j | t_j], t_j = rest_j - rest_parent
    float rest[3];
    int parent, depth;              // depth: steps to the root
    int maxdepth;                   // of the whole tree (uniform)
};

// Fills `sh` (complete on return) and returns the lane's own values; lanes j >= J return rest = 0, parent = -1, depth = 0.  Every lane of
// the workgroup must call it.
__device__ __forceinline__ ChainLane chain_forward(ChainShared& sh, const float* __restrict__ full_pose, const float* __restrict__ comps,
                                                   const float* __restrict__ joint_template, const float* __restrict__ joint_dirs,
                                                   const int* __restrict__ parents, int b, int J, int NB)
{
    const int j = threadIdx.x;
    const bool on = j < J;
    Affine loc;
    float rest[3] = {0.f, 0.f, 0.f};
    int parent = -1, depth = 0;
    if (j == 0) sh.maxdepth = 0;
    __syncthreads();
    if (on) {
        // lbs.py:208-212 with the regressor folded: J_regressor . (v_template + dirs . comps) = joint_template + joint_dirs . comps
        for (int c = 0; c < 3; ++c) {
            const float* d = joint_dirs + (size_t)(3 * j + c) * NB;
            float acc = 0.f;
            for (int l = 0; l < NB; ++l) acc = fmaf(d[l], comps[(size_t)b * NB + l], acc);
            rest[c] = joint_template[3 * j + c] + acc;
            sh.rest[j][c] = rest[c];
        }
        parent = parents[j];
        sh.par[j] = parent;
    }
    __syncthreads();
    if (on) {
        rodrigues(full_pose + ((size_t)b * J + j) * 3, loc.r);
        for (int c = 0; c < 3; ++c) loc.t[c] = parent >= 0 ? rest[c] - sh.rest[parent][c] : rest[c];
        for (int p = parent; p >= 0; p = sh.par[p]) ++depth;
        atomicMax(&sh.maxdepth, depth);
        if (depth == 0) sh.glob[j] = loc;
    }
    __syncthreads();
    const int maxdepth = sh.maxdepth;
    // lbs.py:389-395: transform_chain[i] = transform_chain[parents[i]] @ transforms_mat[i], one tree level per step
    for (int d = 1; d <= maxdepth; ++d) {
        if (on && depth == d) {
            const Affine& P = sh.glob[parent];
            Affine g;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c)
                    g.r[3 * r + c] = fmaf(P.r[3 * r + 2], loc.r[6 + c], fmaf(P.r[3 * r + 1], loc.r[3 + c], P.r[3 * r] * loc.r[c]));
                g.t[r] = fmaf(P.r[3 * r + 2], loc.t[2], fmaf(P.r[3 * r + 1], loc.t[1], P.r[3 * r] * loc.t[0])) + P.t[r];
            }
            sh.glob[j] = g;
        }
        __syncthreads();
    }
    return {loc, {rest[0], rest[1], rest[2]}, parent, depth, maxdepth};
}

__global__ void __launch_bounds__(64) smplx_chain_kernel(float* __restrict__ A_out, float* __restrict__ A_skin,
                                                        float* __restrict__ joints_out, float* __restrict__ pose_feature,
                                                        const float* __restrict__ full_pose, const float* __restrict__ comps,
                                                        const float* __restrict__ joint_template, const float* __restrict__ joint_dirs,
                                                        const int* __restrict__ parents, const float* __restrict__ transl, int J, int NB)
{
    __shared__ ChainShared sh;
    const int b = blockIdx.x, j = threadIdx.x;
    const ChainLane me = chain_forward(sh, full_pose, comps, joint_template, joint_dirs, parents, b, J, NB);
    if (j >= J) return;
    if (j >= 1) {       // lbs.py:221
        float* pf = pose_feature + (size_t)b * 9 * (J - 1) + 9 * (j - 1);
        for (int k = 0; k < 9; ++k) pf[k] = me.loc.r[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
    const Affine g = sh.glob[j];
    float* Aj = A_out + ((size_t)b * J + j) * 16;
    float* As = A_skin + ((size_t)b * J + j) * 12;
    for (int r = 0; r < 3; ++r) {
        // lbs.py:402-403: rel = T - pad(T @ [J; 0]) -> translation column minus R . J_rest
        const float rj = fmaf(g.r[3 * r + 2], me.rest[2], fmaf(g.r[3 * r + 1], me.rest[1], g.r[3 * r] * me.rest[0]));
        const float tr = transl ? transl[3 * b + r] : 0.f;
        for (int c = 0; c < 3; ++c) Aj[4 * r + c] = As[4 * r + c] = g.r[3 * r + c];
        As[4 * r + 3] = g.t[r] - rj;                     // what the skinning uses (lbs.py:241)
        // body_models.py:1272-1275: joints += transl; A[:, :, :3, 3] += transl -- AFTER the skinning used the un-translated A
        Aj[4 * r + 3] = transl ? (g.t[r] - rj) + tr : g.t[r] - rj;
        joints_out[((size_t)b * J + j) * 3 + r] = transl ? g.t[r] + tr : g.t[r];
    }
    Aj[12] = 0.f; Aj[13] = 0.f; Aj[14] = 0.f; Aj[15] = 1.f;
}

template <int NBATCH>
__global__ void __launch_bounds__(kSkinThreads) smplx_skin_kernel(float* __restrict__ vertices, const float* __restrict__ posedirs,
                                                                 const float* __restrict__ pose_feature,
                                                                 const float* __restrict__ v_shaped, const float* __restrict__ A,
                                                                 const float* __restrict__ lbs_weights,
                                                                 const float* __restrict__ transl, float* __restrict__ v_posed_out,
                                                                 int V, int J, int P)
{
    extern __shared__ float smem[];
    float* s_feat = smem;                                   // [NBATCH][P]
    float* s_A = s_feat + NBATCH * P;                       // [NBATCH][J][12]
    float* s_part = s_A + NBATCH * J * 12;                  // [kSkinSlices][NBATCH][kSkinCoords]
    float* s_vp = s_part + kSkinSlices * NBATCH * kSkinCoords;   // [NBATCH][kSkinCoords]
    const int tid = threadIdx.x;
    const int n_coord = 3 * V;
    for (int i = tid; i < NBATCH * P; i += kSkinThreads) s_feat[i] = pose_feature[i];
    for (int i = tid; i < NBATCH * J * 12; i += kSkinThreads) s_A[i] = A[i];     // the un-translated affine rows (chain_kernel)
    __syncthreads();

    const int cx = tid % kSkinCoords, slice = tid / kSkinCoords;
    const int coord = blockIdx.x * kSkinCoords + cx;
    const bool live = coord < n_coord;
    float acc[NBATCH];
    for (int b = 0; b < NBATCH; ++b) acc[b] = 0.f;
    if (live) {
        const float* col = posedirs + coord;
        int p = slice;
        // four rows in flight per thread (the loop is latency bound: 61 MB over ~330 workgroups)
        for (; p + 3 * kSkinSlices < P; p += 4 * kSkinSlices) {
            const float d0 = col[(size_t)p * n_coord];
            const float d1 = col[(size_t)(p + kSkinSlices) * n_coord];
            const float d2 = col[(size_t)(p + 2 * kSkinSlices) * n_coord];
            const float d3 = col[(size_t)(p + 3 * kSkinSlices) * n_coord];
            for (int b = 0; b < NBATCH; ++b) {
                const float* f = s_feat + b * P + p;
                acc[b] = fmaf(f[3 * kSkinSlices], d3, fmaf(f[2 * kSkinSlices], d2, fmaf(f[kSkinSlices], d1, fmaf(f[0], d0, acc[b]))));
            }
        }
        for (; p < P; p += kSkinSlices) {
            const float d0 = col[(size_t)p * n_coord];
            for (int b = 0; b < NBATCH; ++b) acc[b] = fmaf(s_feat[b * P + p], d0, acc[b]);
        }
    }
    for (int b = 0; b < NBATCH; ++b) s_part[(slice * NBATCH + b) * kSkinCoords + cx] = acc[b];
    __syncthreads();

    const bool worker = tid < NBATCH * kSkinCoords;
    const int wb = tid / kSkinCoords;      // pose handled by this thread in the tail (cx is unchanged)
    if (worker && live) {
        float off = 0.f;
        for (int s = 0; s < kSkinSlices; ++s) off += s_part[(s * NBATCH + wb) * kSkinCoords + cx];
        const float vp = off + v_shaped[(size_t)wb * n_coord + coord];                  // lbs.py:233
        s_vp[wb * kSkinCoords + cx] = vp;
        if (v_posed_out) v_posed_out[(size_t)wb * n_coord + coord] = vp;                // kept for ag_smplx_vertex_backward
    }
    __syncthreads();
    if (worker && live) {
        const int lv = cx / 3, c = cx % 3;
        const float* w = lbs_weights + (size_t)(blockIdx.x * kSkinVerts + lv) * J;
        const float* Ab = s_A + wb * J * 12 + 4 * c;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        for (int j = 0; j < J; ++j) {       // lbs.py:241-242: row c of T = W @ A
            const float wj = w[j];
            t0 = fmaf(wj, Ab[12 * j + 0], t0);
            t1 = fmaf(wj, Ab[12 * j + 1], t1);
            t2 = fmaf(wj, Ab[12 * j + 2], t2);
            t3 = fmaf(wj, Ab[12 * j + 3], t3);
        }
        const float* vp = s_vp + wb * kSkinCoords + 3 * lv;
        // the reference skins with the un-translated A and adds transl to the vertices afterwards (body_models.py:1274)
        float out = fmaf(t2, vp[2], fmaf(t1, vp[1], t0 * vp[0])) + t3;
        if (transl) out += transl[3 * wb + c];
        vertices[(size_t)wb * n_coord + coord] = out;
    }
}

__global__ void __launch_bounds__(64) smplx_keypoints_kernel(float* __restrict__ out, const float* __restrict__ vertices,
                                                            const int* __restrict__ idx, const float* __restrict__ w, int V, int K)
{
    const int i = blockIdx.x * 64 + threadIdx.x;   // (k, c)
    const int b = blockIdx.y;
    if (i >= 3 * K) return;
    const int k = i / 3, c = i % 3;
    const float* vb = vertices + (size_t)b * V * 3;
    float acc = 0.f;
    for (int t = 0; t < 3; ++t) acc = fmaf(w[3 * k + t], vb[3 * idx[3 * k + t] + c], acc);
    out[((size_t)b * K + k) * 3 + c] = acc;
}

// general 4x4 inverse through the 2x2 minors of the top and bottom row pairs (adjugate / determinant)
__device__ __forceinline__ void inverse4(const float* m, float* inv)
{
    const float s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    const float s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    const float c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    const float c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    const float det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const float id = 1.f / det;
    inv[0] = (m[5] * c5 - m[6] * c4 + m[7] * c3) * id;
    inv[1] = (-m[1] * c5 + m[2] * c4 - m[3] * c3) * id;
    inv[2] = (m[13] * s5 - m[14] * s4 + m[15] * s3) * id;
    inv[3] = (-m[9] * s5 + m[10] * s4 - m[11] * s3) * id;
    inv[4] = (-m[4] * c5 + m[6] * c2 - m[7] * c1) * id;
    inv[5] = (m[0] * c5 - m[2] * c2 + m[3] * c1) * id;
    inv[6] = (-m[12] * s5 + m[14] * s2 - m[15] * s1) * id;
    inv[7] = (m[8] * s5 - m[10] * s2 + m[11] * s1) * id;
    inv[8] = (m[4] * c4 - m[5] * c2 + m[7] * c0) * id;
    inv[9] = (-m[0] * c4 + m[1] * c2 - m[3] * c0) * id;
    inv[10] = (m[12] * s4 - m[13] * s2 + m[15] * s0) * id;
    inv[11] = (-m[8] * s4 + m[9] * s2 - m[11] * s0) * id;
    inv[12] = (-m[4] * c3 + m[5] * c1 - m[6] * c0) * id;
    inv[13] = (m[0] * c3 - m[1] * c1 + m[2] * c0) * id;
    inv[14] = (-m[12] * s3 + m[13] * s1 - m[14] * s0) * id;
    inv[15] = (m[8] * s3 - m[9] * s1 + m[10] * s0) * id;
}

__global__ void __launch_bounds__(64) mat4_mul_inverse_kernel(float* __restrict__ out, const float* __restrict__ a,
                                                             const float* __restrict__ bm, int n, int b_batch)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float inv[16];
    inverse4(bm + (size_t)(i % b_batch) * 16, inv);
    const float* ai = a + (size_t)i * 16;
    float* oi = out + (size_t)i * 16;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            float acc = 0.f;
            for (int k = 0; k < 4; ++k) acc = fmaf(ai[4 * r + k], inv[4 * k + c], acc);
            oi[4 * r + c] = acc;
        }
}

// Backward of rodrigues().  dR [9] -> drv [3].  The eps keeps the zero pose's gradient finite, as in the reference (its torch autograd of
// the same expression).
__device__ __forceinline__ void rodrigues_backward(const float* rv, const float* dR, float* drv)
{
    const RodriguesHead h(rv);
    const float angle = h.angle, s = h.s, co = h.co, c1 = h.c1;
    const float *e = h.e, *K = h.K;
    float ds = 0.f, dc1 = 0.f, dK[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float kk = 0.f, t = 0.f;
            for (int k = 0; k < 3; ++k) {
                kk = fmaf(K[3 * r + k], K[3 * k + c], kk);
                t += dR[3 * r + k] * K[3 * c + k] + K[3 * k + r] * dR[3 * k + c];     // (dR K^T + K^T dR)[r][c]
            }
            ds += dR[3 * r + c] * K[3 * r + c];
            dc1 += dR[3 * r + c] * kk;
            dK[3 * r + c] = s * dR[3 * r + c] + c1 * t;
        }
    const float da[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    // axis = rv / angle;  angle = |e|
    const float dangle = ds * co + dc1 * s - (da[0] * rv[0] + da[1] * rv[1] + da[2] * rv[2]) / (angle * angle);
    for (int c = 0; c < 3; ++c) drv[c] = da[c] / angle + dangle * e[c] / angle;
}

// Reverse of smplx_chain_kernel, one wave per pose: recomputes the rest joints, the local transforms and the global chain (chain_forward),
// then walks the tree levels from the deepest to the root.  A parent gathers its children's contributions in ascending joint order, so the
// result does not depend on scheduling.  Inputs dA [B][J][4][4] (row 3 unused) and djoints [B][J][3], either may be NULL.
// Outputs: dpose [B][J][3]; dtransl [B][3] (NULL: skipped); dcomps [B][NB] through the folded joint_dirs (NULL: skipped).
// EXT (ag_smplx_backward_full) adds what the vertex path hands over, each NULL or present: dAs [B][J][12] on the un-translated matrices
// the skinning read (joins dA everywhere except in dtransl), dfeat [B][J-1][9] on the local rotations R[1:] (joins dR ahead of the
// Rodrigues backward), dtr_add [B][3] and dcomps_add [B][NB] (added to the two outputs last).  EXT = false is the kernel as it was.
template <bool EXT>
__global__ void __launch_bounds__(64) smplx_chain_backward_kernel(float* __restrict__ dpose, float* __restrict__ dtransl,
                                                                 float* __restrict__ dcomps, const float* __restrict__ dA,
                                                                 const float* __restrict__ djoints, const float* __restrict__ full_pose,
                                                                 const float* __restrict__ comps, const float* __restrict__ joint_template,
                                                                 const float* __restrict__ joint_dirs, const int* __restrict__ parents,
                                                                 int J, int NB, const float* __restrict__ dAs, const float* __restrict__ dfeat,
                                                                 const float* __restrict__ dtr_add, const float* __restrict__ dcomps_add)
{
    __shared__ ChainShared sh;
    __shared__ float s_cr[kMaxJoints][9];     // a joint's contribution to its parent's dL/d(global rotation)
    __shared__ float s_ct[kMaxJoints][3];     // ... to its parent's dL/d(global translation)
    __shared__ float s_dt[kMaxJoints][3];     // dL/d(local translation) = dL/d(rest_j - rest_parent)
    __shared__ float s_drest[kMaxJoints][3];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool on = j < J;
    const ChainLane me = chain_forward(sh, full_pose, comps, joint_template, joint_dirs, parents, b, J, NB);

    // ---- direct gradients: A_j[:3, :3] = Gr_j;  A_j[:3, 3] = Gt_j - Gr_j rest_j (+ transl);  joints_j = Gt_j (+ transl) ----
    float dGr[9], dGt[3], drest[3] = {0.f, 0.f, 0.f};
    if (on) {
        const float* a = dA ? dA + ((size_t)b * J + j) * 16 : nullptr;
        const float* dj = djoints ? djoints + ((size_t)b * J + j) * 3 : nullptr;
        const Affine& g = sh.glob[j];
        const float* as = EXT && dAs ? dAs + ((size_t)b * J + j) * 12 : nullptr;
        float dtr[3];     // the part of dGt that transl sees: dAs belongs to the matrices before transl was added
        for (int r = 0; r < 3; ++r) {
            float dcol = a ? a[4 * r + 3] : 0.f;
            dtr[r] = dcol + (dj ? dj[r] : 0.f);
            if (EXT && as) dcol += as[4 * r + 3];
            dGt[r] = dcol + (dj ? dj[r] : 0.f);
            for (int c = 0; c < 3; ++c) {
                float da = a ? a[4 * r + c] : 0.f;
                if (EXT && as) da += as[4 * r + c];
                dGr[3 * r + c] = da - dcol * me.rest[c];
                drest[c] -= g.r[3 * r + c] * dcol;
            }
        }
        for (int r = 0; r < 3; ++r) s_ct[j][r] = EXT ? dtr[r] : dGt[r];      // read by the dtransl sum only; the level loop rewrites it
    }
    __syncthreads();
    if (dtransl && j < 3) {           // body_models.py:1272-1275: transl is added to every A_j[:3, 3] and every joint
        float acc = 0.f;
        for (int k = 0; k < J; ++k) acc += s_ct[k][j];
        if (EXT && dtr_add) acc += dtr_add[3 * b + j];
        dtransl[3 * b + j] = acc;
    }
    __syncthreads();

    // ---- the chain in reverse, one tree level per step ----
    for (int d = me.maxdepth; d >= 0; --d) {
        if (on && me.depth == d) {
            // Gr_j = Gr_p R_j,  Gt_j = Gr_p t_j + Gt_p   (root: Gr_0 = R_0, Gt_0 = t_0)
            float dR[9], dt[3];
            if (me.parent >= 0) {
                const Affine& P = sh.glob[me.parent];
                for (int k = 0; k < 3; ++k) {
                    for (int c = 0; c < 3; ++c)
                        dR[3 * k + c] = P.r[k] * dGr[c] + P.r[3 + k] * dGr[3 + c] + P.r[6 + k] * dGr[6 + c];
                    dt[k] = P.r[k] * dGt[0] + P.r[3 + k] * dGt[1] + P.r[6 + k] * dGt[2];
                }
                for (int r = 0; r < 3; ++r) {
                    for (int k = 0; k < 3; ++k)
                        s_cr[j][3 * r + k] = dGr[3 * r] * me.loc.r[3 * k] + dGr[3 * r + 1] * me.loc.r[3 * k + 1] +
                                             dGr[3 * r + 2] * me.loc.r[3 * k + 2] + dGt[r] * me.loc.t[k];
                    s_ct[j][r] = dGt[r];
                }
            } else {
                for (int k = 0; k < 9; ++k) dR[k] = dGr[k];
                for (int k = 0; k < 3; ++k) dt[k] = dGt[k];
            }
            for (int k = 0; k < 3; ++k) s_dt[j][k] = dt[k];
            if (EXT && dfeat && j >= 1)       // lbs.py:221: pose_feature = R[1:] - I
                for (int k = 0; k < 9; ++k) dR[k] += dfeat[(size_t)b * 9 * (J - 1) + 9 * (j - 1) + k];
            rodrigues_backward(full_pose + ((size_t)b * J + j) * 3, dR, dpose + ((size_t)b * J + j) * 3);
        }
        __syncthreads();
        if (on && me.depth == d - 1) {
            for (int c = j + 1; c < J; ++c)
                if (sh.par[c] == j) {
                    for (int k = 0; k < 9; ++k) dGr[k] += s_cr[c][k];
                    for (int k = 0; k < 3; ++k) dGt[k] += s_ct[c][k];
                }
        }
        __syncthreads();
    }

    // ---- rest joints: t_j = rest_j - rest_parent;  rest_j = joint_template_j + joint_dirs_j . comps ----
    if (on) {
        for (int k = 0; k < 3; ++k) drest[k] += s_dt[j][k];
        for (int c = j + 1; c < J; ++c)
            if (sh.par[c] == j)
                for (int k = 0; k < 3; ++k) drest[k] -= s_dt[c][k];
        for (int k = 0; k < 3; ++k) s_drest[j][k] = drest[k];
    }
    __syncthreads();
    if (dcomps)
        for (int l = j; l < NB; l += 64) {
            float acc = 0.f;
            for (int k = 0; k < J; ++k)
                for (int c = 0; c < 3; ++c) acc = fmaf(s_drest[k][c], joint_dirs[(size_t)(3 * k + c) * NB + l], acc);
            if (EXT && dcomps_add) acc += dcomps_add[(size_t)b * NB + l];
            dcomps[(size_t)b * NB + l] = acc;
        }
}

// Backward of out[i] = a[i] X,  X = inverse(b[i % b_batch]):  da[i] = dout[i] X^T;  db[k] = -X^T (sum_{i % b_batch == k} a[i]^T dout[i]) X^T.
// One thread per b matrix; it walks its a's in ascending i (fixed order).  da / db may be NULL.
__global__ void __launch_bounds__(64) mat4_mul_inverse_backward_kernel(float* __restrict__ da, float* __restrict__ db,
                                                                      const float* __restrict__ dout, const float* __restrict__ a,
                                                                      const float* __restrict__ bm, int n, int b_batch)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= b_batch) return;
    float X[16], dX[16];
    inverse4(bm + (size_t)k * 16, X);
    for (int e = 0; e < 16; ++e) dX[e] = 0.f;
    for (int i = k; i < n; i += b_batch) {
        const float* g = dout + (size_t)i * 16;
        if (da)
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) {
                    float acc = 0.f;
                    for (int q = 0; q < 4; ++q) acc = fmaf(g[4 * r + q], X[4 * c + q], acc);
                    da[(size_t)i * 16 + 4 * r + c] = acc;
                }
        if (db) {
            const float* ai = a + (size_t)i * 16;
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) {
                    float acc = dX[4 * r + c];
                    for (int q = 0; q < 4; ++q) acc = fmaf(ai[4 * q + r], g[4 * q + c], acc);
                    dX[4 * r + c] = acc;
                }
        }
    }
    if (!db) return;
    float T[16];   // T = X^T dX
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            float acc = 0.f;
            for (int q = 0; q < 4; ++q) acc = fmaf(X[4 * q + r], dX[4 * q + c], acc);
            T[4 * r + c] = acc;
        }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            float acc = 0.f;
            for (int q = 0; q < 4; ++q) acc = fmaf(T[4 * r + q], X[4 * c + q], acc);
            db[(size_t)k * 16 + 4 * r + c] = -acc;
        }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Backward of the vertex path (ag_smplx_vertex_backward, ag_smplx_keypoints_backward, ag_smplx_shape_backward).  No float atomics:
// every sum has a fixed order, so two calls give the same bits.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kVbVerts = 64;        // vertices per workgroup of skin_backward_kernel = one slab of the joint sums
constexpr int kVbThreads = 768;     // >= 12 J + 3 for J = 55: one pass over the slab row
constexpr int kPdThreads = 1024;    // posedirs_t_kernel: one workgroup per basis row
constexpr int kSdCoords = 256;      // dirs_t_kernel: coordinates per workgroup = one slab of the component sums

// Key points -> vertices: dverts[b][idx[k][t]] += w[k][t] dkp[b][k].  Vertex ids repeat (landmark triangles share vertices, the vertex
// picks carry theirs three times), so the FIRST entry that names a vertex owns it: it adds its own and every later entry's term in
// ascending entry order and stores once.  dverts must hold zeros (or a gradient to add to) before the launch.  One workgroup per pose;
// the 3 K ids and weights sit in LDS for the scans.
__global__ void __launch_bounds__(256) smplx_keypoints_backward_kernel(float* __restrict__ dverts, const float* __restrict__ dkp,
                                                                      const int* __restrict__ idx, const float* __restrict__ w, int V, int K)
{
    extern __shared__ float smem[];
    const int n = 3 * K;
    int* s_idx = reinterpret_cast<int*>(smem);       // [3 K]
    float* s_w = smem + n;                            // [3 K]
    float* s_g = s_w + n;                             // [3 K]: dkp of this pose
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < n; e += 256) {
        s_idx[e] = idx[e];
        s_w[e] = w[e];
        s_g[e] = dkp[(size_t)b * n + e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const int v = s_idx[e];
        if (v < 0 || v >= V) continue;
        bool owner = true;
#pragma unroll 8
        for (int q = 0; q < e; ++q) owner = owner && s_idx[q] != v;
        if (!owner) continue;
        float* dst = dverts + ((size_t)b * V + v) * 3;
        float a0 = dst[0], a1 = dst[1], a2 = dst[2];
#pragma unroll 8
        for (int q = e; q < n; ++q)
            if (s_idx[q] == v) {
                const float wq = s_w[q];
                const float* gk = s_g + 3 * (q / 3);
                a0 = fmaf(wq, gk[0], a0);
                a1 = fmaf(wq, gk[1], a1);
                a2 = fmaf(wq, gk[2], a2);
            }
        dst[0] = a0; dst[1] = a1; dst[2] = a2;
    }
}

// Skinning backward for 64 vertices of one pose.  g = dL/dvertices.
//   dvp[v] = T_v[:3,:3]^T g[v],  T_v = sum_j W[v][j] A_skin[j]                                (lbs.py:241-246)
//   slab[wg][b][j][r][c] = sum_{v in the workgroup, ascending} W[v][j] g[v][r] [v_posed[v]; 1][c]     -> dL/dA_skin after the slab sum
//   slab[wg][b][12 J + r] = sum_v g[v][r]                                                             -> dL/dtransl
__global__ void __launch_bounds__(kVbThreads) smplx_skin_backward_kernel(float* __restrict__ dvp, float* __restrict__ slabs,
                                                                        const float* __restrict__ g, const float* __restrict__ v_posed,
                                                                        const float* __restrict__ A_skin,
                                                                        const float* __restrict__ lbs_weights, int V, int J)
{
    extern __shared__ float smem[];
    float* s_W = smem;                          // [kVbVerts][J]
    float* s_A = s_W + kVbVerts * J;            // [J][12]
    float* s_g = s_A + J * 12;                  // [kVbVerts][4]  (g, 0)
    float* s_x = s_g + kVbVerts * 4;            // [kVbVerts][4]  (v_posed, 1)
    const int tid = threadIdx.x, b = blockIdx.y;
    const int v0 = blockIdx.x * kVbVerts;
    const int nv = V - v0 < kVbVerts ? V - v0 : kVbVerts;
    const int width = 12 * J + 3;
    for (int i = tid; i < kVbVerts * J; i += kVbThreads) s_W[i] = i < nv * J ? lbs_weights[(size_t)v0 * J + i] : 0.f;
    for (int i = tid; i < J * 12; i += kVbThreads) s_A[i] = A_skin[(size_t)b * J * 12 + i];
    if (tid < 4 * kVbVerts) {
        const int lv = tid >> 2, c = tid & 3;
        const bool in = lv < nv && c < 3;
        const size_t at = ((size_t)b * V + v0 + lv) * 3 + c;
        s_g[tid] = in ? g[at] : 0.f;
        s_x[tid] = in ? v_posed[at] : (c == 3 && lv < nv ? 1.f : 0.f);
    }
    __syncthreads();
    if (tid < 3 * kVbVerts) {
        const int lv = tid / 3, c = tid % 3;
        if (lv < nv) {
            const float g0 = s_g[4 * lv], g1 = s_g[4 * lv + 1], g2 = s_g[4 * lv + 2];
            const float* wv = s_W + lv * J;
            float acc = 0.f;
            for (int j = 0; j < J; ++j) {
                const float* Aj = s_A + 12 * j + c;
                acc = fmaf(wv[j], fmaf(Aj[8], g2, fmaf(Aj[4], g1, Aj[0] * g0)), acc);
            }
            dvp[((size_t)b * V + v0 + lv) * 3 + c] = acc;
        }
    }
    float* slab = slabs + ((size_t)blockIdx.x * gridDim.y + b) * width;
    for (int e = tid; e < width; e += kVbThreads) {
        float acc = 0.f;
        if (e < 12 * J) {
            const int j = e / 12, r = (e % 12) >> 2, c = e & 3;
            for (int lv = 0; lv < kVbVerts; ++lv) acc = fmaf(s_W[lv * J + j] * s_g[4 * lv + r], s_x[4 * lv + c], acc);
        } else {
            const int r = e - 12 * J;
            for (int lv = 0; lv < kVbVerts; ++lv) acc += s_g[4 * lv + r];
        }
        slab[e] = acc;
    }
}

// Sum over slabs of one column i of slabs [n_slab][total], by a workgroup of 16 columns x 16 slab groups (tid = 16 q + column): group q
// adds slabs q, q + 16, q + 32, ... in ascending order, then the 16 groups are added in ascending q.  Returns the sum in the threads
// with q = 0 (tid < 16).  Every thread of the workgroup must call it.
__device__ __forceinline__ float slab_column_sum(const float* __restrict__ slabs, int n_slab, int total, int i, float* s_red)
{
    const int q = threadIdx.x >> 4;
    float acc = 0.f;
    if (i < total) {
#pragma unroll 4
        for (int sl = q; sl < n_slab; sl += 16) acc += slabs[(size_t)sl * total + i];
    }
    s_red[threadIdx.x] = acc;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x < 16)
        for (int k = 0; k < 16; ++k) r += s_red[16 * k + threadIdx.x];
    return r;
}

// The slab sums of the vertex backward in one launch.  Workgroups [0, n_skin_blocks): dL/dA_skin [B][J][12] and dL/dtransl [B][3] from
// the slabs [n_skin_slab][B][12 J + 3] of smplx_skin_backward_kernel; the rest: out [dirs_total] from the slabs
// [n_dirs_slab][dirs_total] of smplx_dirs_t_kernel.  Order: slab_column_sum.
__global__ void __launch_bounds__(256) smplx_slab_sums_kernel(float* __restrict__ dAs, float* __restrict__ dtr,
                                                             const float* __restrict__ skin_slabs, int n_skin_slab, int B, int J,
                                                             int n_skin_blocks, float* __restrict__ dcomps,
                                                             const float* __restrict__ dirs_slabs, int n_dirs_slab, int dirs_total)
{
    __shared__ float s_red[256];
    const int li = threadIdx.x & 15;
    if ((int)blockIdx.x < n_skin_blocks) {
        const int width = 12 * J + 3, total = B * width;
        const int i = blockIdx.x * 16 + li;
        const float r = slab_column_sum(skin_slabs, n_skin_slab, total, i, s_red);
        if (threadIdx.x < 16 && i < total) {
            const int b = i / width, e = i % width;
            if (e < 12 * J) dAs[(size_t)b * 12 * J + e] = r;
            else dtr[3 * b + (e - 12 * J)] = r;
        }
    } else {
        const int i = (blockIdx.x - n_skin_blocks) * 16 + li;
        const float r = slab_column_sum(dirs_slabs, n_dirs_slab, dirs_total, i, s_red);
        if (threadIdx.x < 16 && i < dirs_total) dcomps[i] = r;
    }
}

// The pose-corrective basis, transposed: dfeat[b][p] = sum_c posedirs[p][c] dvp[b][c].  One workgroup per row p (125.7 KB, contiguous),
// the row read ONCE for the NBATCH poses; dvp (126 KB per pose) comes from cache.  A thread walks c = tid, tid + 1024, ... in ascending
// order, eight loads in flight; then lanes by xor-shuffle (32, 16, ... 1), then the 16 waves in ascending order.
template <int NBATCH>
__global__ void __launch_bounds__(kPdThreads) smplx_posedirs_t_kernel(float* __restrict__ dfeat, const float* __restrict__ posedirs,
                                                                     const float* __restrict__ dvp, int n_coord, int P)
{
    __shared__ float s_part[NBATCH][kPdThreads / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const float* row = posedirs + (size_t)p * n_coord;
    float acc[NBATCH];
    for (int b = 0; b < NBATCH; ++b) acc[b] = 0.f;
    int c = tid;
    for (; c + 7 * kPdThreads < n_coord; c += 8 * kPdThreads) {
        float d[8];
        for (int u = 0; u < 8; ++u) d[u] = row[c + u * kPdThreads];
        for (int b = 0; b < NBATCH; ++b) {
            const float* x = dvp + (size_t)b * n_coord + c;
            for (int u = 0; u < 8; ++u) acc[b] = fmaf(d[u], x[u * kPdThreads], acc[b]);
        }
    }
#pragma unroll 4
    for (; c < n_coord; c += kPdThreads) {
        const float d = row[c];
        for (int b = 0; b < NBATCH; ++b) acc[b] = fmaf(d, dvp[(size_t)b * n_coord + c], acc[b]);
    }
    for (int b = 0; b < NBATCH; ++b) {
        const float a = wave_sum(acc[b]);
        if ((tid & 63) == 0) s_part[b][tid >> 6] = a;
    }
    __syncthreads();
    if (tid < NBATCH) {
        float a = 0.f;
        for (int wv = 0; wv < kPdThreads / 64; ++wv) a += s_part[tid][wv];
        dfeat[(size_t)tid * P + p] = a;
    }
}

// The shape basis, transposed, for 256 coordinates of one pose: slab[wg][b][k] = sum_{c in the workgroup} dirs[c][k] x[b][c]
// (lanes by xor-shuffle, then the four waves in ascending order).  x = dL/dv_posed or dL/dv_shaped.
__global__ void __launch_bounds__(kSdCoords) smplx_dirs_t_kernel(float* __restrict__ slabs, const float* __restrict__ dirs,
                                                                const float* __restrict__ x, int n_coord, int NB)
{
    extern __shared__ float s_sum[];            // [4][NB]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int c = blockIdx.x * kSdCoords + tid;
    const bool live = c < n_coord;
    const float xv = live ? x[(size_t)b * n_coord + c] : 0.f;
    const float* row = dirs + (size_t)(live ? c : 0) * NB;
    for (int k = 0; k < NB; ++k) {
        const float a = wave_sum(live ? row[k] * xv : 0.f);
        if ((tid & 63) == 0) s_sum[(tid >> 6) * NB + k] = a;
    }
    __syncthreads();
    float* slab = slabs + ((size_t)blockIdx.x * gridDim.y + b) * NB;
    for (int k = tid; k < NB; k += kSdCoords) slab[k] = (s_sum[k] + s_sum[NB + k]) + (s_sum[2 * NB + k] + s_sum[3 * NB + k]);
}

static bool model_ok(const AgSmplxModel* m)
{
    return m && m->V > 0 && m->J > 0 && m->J <= kMaxJoints && m->NB >= 0 && m->NB <= 4096 && m->v_template && m->posedirs &&
           m->J_regressor && m->parents && m->lbs_weights && (m->NB == 0 || m->shapedirs);
}

static bool folded_ok(const AgSmplxModel* m)
{
    return m->joint_template && (m->NB == 0 || m->joint_dirs);
}

// What the entry points of the forward and of its backward check first; `fn` names the caller in the message.  True: the call is over and
// *rc is its result (a refusal, or AG_OK for B = 0: nothing to do).
static bool call_is_over(const char* fn, const AgSmplxModel* m, int32_t B, bool folded, int* rc)
{
    *rc = AG_ERR_INVALID_ARGUMENT;
    if (!model_ok(m)) set_error("%s: bad model (need 0 < J <= 64, non-null arrays)", fn);
    else if (folded && !folded_ok(m)) set_error("%s: joint_template / joint_dirs missing -- run ag_smplx_prepare once per model", fn);
    else if (B < 0) set_error("%s: B < 0", fn);
    else { *rc = AG_OK; return B == 0; }
    return true;
}

// f(first pose, std::integral_constant<int, NBATCH>) for every run of up to four poses of B: the kernels that read a basis once for NBATCH poses
template <class F>
static void for_pose_runs(int B, F f)
{
    for (int b0 = 0; b0 < B; b0 += 4)
        switch (B - b0) {
            case 1: f(b0, std::integral_constant<int, 1>()); break;
            case 2: f(b0, std::integral_constant<int, 2>()); break;
            case 3: f(b0, std::integral_constant<int, 3>()); break;
            default: f(b0, std::integral_constant<int, 4>()); break;
        }
}

template <int NBATCH>
static void launch_skin(const AgSmplxModel* m, float* vertices, const float* feat, const float* v_shaped, const float* A,
                        const float* transl, float* v_posed, hipStream_t s)
{
    const int P = 9 * (m->J - 1);
    const size_t lds = sizeof(float) * ((size_t)NBATCH * P + (size_t)NBATCH * m->J * 12 + (size_t)kSkinSlices * NBATCH * kSkinCoords +
                                        (size_t)NBATCH * kSkinCoords);
    const int grid = (m->V + kSkinVerts - 1) / kSkinVerts;
    hipLaunchKernelGGL(smplx_skin_kernel<NBATCH>, dim3(grid), dim3(kSkinThreads), lds, s, vertices, m->posedirs, feat, v_shaped, A,
                       m->lbs_weights, transl, v_posed, m->V, m->J, P);
}

// ag_smplx_backward (EXT = false, the four handed-over gradients NULL) and ag_smplx_backward_full (EXT = true); `fn` names the caller in the
// messages.
template <bool EXT>
static int chain_backward_impl(const char* fn, const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose,
                               const float* dL_dA, const float* dL_djoints, const float* dL_dA_skin, const float* dL_dfeat,
                               const float* dL_dtransl_add, const float* dL_dshape_components_add, float* dL_dfull_pose, float* dL_dtransl,
                               float* dL_dshape_components, void* stream)
{
    int rc;
    if (call_is_over(fn, m, B, true, &rc)) return rc;
    if (!full_pose || !dL_dfull_pose || (m->NB > 0 && !shape_components)) { set_error("%s: null pointer", fn); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(smplx_chain_backward_kernel<EXT>, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), dL_dfull_pose, dL_dtransl,
                       m->NB > 0 ? dL_dshape_components : nullptr, dL_dA, dL_djoints, full_pose, shape_components, m->joint_template,
                       m->joint_dirs, m->parents, m->J, m->NB, dL_dA_skin, dL_dfeat, dL_dtransl_add,
                       m->NB > 0 ? dL_dshape_components_add : nullptr);
    return check_hip(hipGetLastError(), "smplx_chain_backward_kernel");
}

}  // namespace ag

using namespace ag;

extern "C" {

size_t ag_smplx_workspace_floats(const AgSmplxModel* m, int32_t B)
{
    if (!m || B <= 0) return 0;
    return (size_t)B * ((size_t)3 * m->V + (size_t)12 * m->J + (size_t)9 * (m->J - 1));
}

// ag_smplx_forward and ag_smplx_forward_keep: the same three launches; `saved` (NULL: nothing kept) receives v_posed from the skin
// kernel and takes the place of the workspace's A_skin block.
static int smplx_forward_impl(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* transl,
                              float* vertices, float* joints, float* A, float* workspace, size_t workspace_floats, float* saved, void* stream)
{
    int rc;
    if (call_is_over("smplx", m, B, true, &rc)) return rc;
    if (!full_pose || !vertices || !joints || !A || !workspace || (m->NB > 0 && !shape_components)) {
        set_error("smplx: null pointer");
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (workspace_floats < ag_smplx_workspace_floats(m, B)) { set_error("smplx: workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_coord = 3 * m->V, P = 9 * (m->J - 1);
    float* v_shaped = workspace;
    float* A_skin = saved ? saved + (size_t)B * n_coord : v_shaped + (size_t)B * n_coord;
    float* feat = v_shaped + (size_t)B * n_coord + (size_t)B * 12 * m->J;

    hipLaunchKernelGGL(smplx_shape_kernel, dim3((n_coord + 255) / 256, B), dim3(256), sizeof(float) * (m->NB > 0 ? m->NB : 1), s, v_shaped,
                       m->v_template, m->shapedirs, shape_components, n_coord, m->NB);
    hipLaunchKernelGGL(smplx_chain_kernel, dim3(B), dim3(64), 0, s, A, A_skin, joints, feat, full_pose, shape_components, m->joint_template,
                       m->joint_dirs, m->parents, transl, m->J, m->NB);
    for_pose_runs(B, [&](int b0, auto nb) {
        launch_skin<decltype(nb)::value>(m, vertices + (size_t)b0 * n_coord, feat + (size_t)b0 * P, v_shaped + (size_t)b0 * n_coord,
                                         A_skin + (size_t)b0 * m->J * 12, transl ? transl + (size_t)3 * b0 : nullptr,
                                         saved ? saved + (size_t)b0 * n_coord : nullptr, s);
    });
    return check_hip(hipGetLastError(), "ag_smplx_forward");
}

int ag_smplx_forward(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* transl,
                     float* vertices, float* joints, float* A, float* workspace, size_t workspace_floats, void* stream)
{
    return smplx_forward_impl(m, B, shape_components, full_pose, transl, vertices, joints, A, workspace, workspace_floats, nullptr, stream);
}

size_t ag_smplx_saved_floats(const AgSmplxModel* m, int32_t B)
{
    if (!m || B <= 0) return 0;
    return (size_t)B * ((size_t)3 * m->V + (size_t)12 * m->J);
}

int ag_smplx_forward_keep(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* transl,
                          float* vertices, float* joints, float* A, float* workspace, size_t workspace_floats, float* saved,
                          size_t saved_floats, void* stream)
{
    if (B > 0 && (!saved || !m || saved_floats < ag_smplx_saved_floats(m, B))) {
        set_error("smplx_forward_keep: `saved` missing or smaller than ag_smplx_saved_floats");
        return AG_ERR_INVALID_ARGUMENT;
    }
    return smplx_forward_impl(m, B, shape_components, full_pose, transl, vertices, joints, A, workspace, workspace_floats, saved, stream);
}

int ag_smplx_prepare(const AgSmplxModel* m, float* joint_template, float* joint_dirs, void* stream)
{
    if (!model_ok(m)) { set_error("smplx_prepare: bad model"); return AG_ERR_INVALID_ARGUMENT; }
    if (!joint_template || (m->NB > 0 && !joint_dirs)) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(smplx_joints_kernel, dim3(m->J, 1), dim3(256), 0, s, joint_template, m->J_regressor, m->v_template, m->V, 1, 1);
    if (m->NB > 0)
        hipLaunchKernelGGL(smplx_joints_kernel, dim3(m->J, m->NB), dim3(256), 0, s, joint_dirs, m->J_regressor, m->shapedirs, m->V, m->NB, m->NB);
    return check_hip(hipGetLastError(), "smplx_joints_kernel");
}

int ag_smplx_shape(const AgSmplxModel* m, int32_t B, const float* shape_components, float* v_shaped, void* stream)
{
    if (!model_ok(m) || B < 0) { set_error("smplx_shape: bad model or B < 0"); return AG_ERR_INVALID_ARGUMENT; }
    if (B == 0) return AG_OK;
    if (!v_shaped || (m->NB > 0 && !shape_components)) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    const int n_coord = 3 * m->V;
    hipLaunchKernelGGL(smplx_shape_kernel, dim3((n_coord + 255) / 256, B), dim3(256), sizeof(float) * (m->NB > 0 ? m->NB : 1),
                       reinterpret_cast<hipStream_t>(stream), v_shaped, m->v_template, m->shapedirs, shape_components, n_coord, m->NB);
    return check_hip(hipGetLastError(), "smplx_shape_kernel");
}

int ag_mat4_mul_inverse(float* out, const float* a, const float* b, int32_t n, int32_t b_batch, void* stream)
{
    if (n < 0 || b_batch <= 0) { set_error("mat4_mul_inverse: need n >= 0, b_batch >= 1"); return AG_ERR_INVALID_ARGUMENT; }
    if (n == 0) return AG_OK;
    if (!out || !a || !b) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(mat4_mul_inverse_kernel, dim3((n + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), out, a, b, n, b_batch);
    return check_hip(hipGetLastError(), "mat4_mul_inverse_kernel");
}

int ag_smplx_backward(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* dL_dA,
                      const float* dL_djoints, float* dL_dfull_pose, float* dL_dtransl, float* dL_dshape_components, void* stream)
{
    return chain_backward_impl<false>("smplx_backward", m, B, shape_components, full_pose, dL_dA, dL_djoints, nullptr, nullptr, nullptr, nullptr,
                                      dL_dfull_pose, dL_dtransl, dL_dshape_components, stream);
}

int ag_mat4_mul_inverse_backward(float* dL_da, float* dL_db, const float* dL_dout, const float* a, const float* b, int32_t n, int32_t b_batch,
                                 void* stream)
{
    if (n < 0 || b_batch <= 0 || (n > 0 && n % b_batch)) { set_error("mat4_mul_inverse_backward: need n >= 0, b_batch >= 1 dividing n"); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) return dL_db ? check_hip(hipMemsetAsync(dL_db, 0, (size_t)b_batch * 16 * sizeof(float), s), "memset") : AG_OK;
    if (!dL_dout || !b || (dL_db && !a)) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    if (!dL_da && !dL_db) return AG_OK;
    hipLaunchKernelGGL(mat4_mul_inverse_backward_kernel, dim3((b_batch + 63) / 64), dim3(64), 0, s, dL_da, dL_db, dL_dout, a, b, n, b_batch);
    return check_hip(hipGetLastError(), "mat4_mul_inverse_backward_kernel");
}

int ag_smplx_keypoints(float* out, const float* vertices, const int32_t* idx, const float* w, int32_t B, int32_t V, int32_t K, void* stream)
{
    if (B < 0 || K < 0 || V <= 0) { set_error("smplx_keypoints: bad sizes"); return AG_ERR_INVALID_ARGUMENT; }
    if (B == 0 || K == 0) return AG_OK;
    if (!out || !vertices || !idx || !w) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(smplx_keypoints_kernel, dim3((3 * K + 63) / 64, B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), out, vertices,
                       idx, w, V, K);
    return check_hip(hipGetLastError(), "smplx_keypoints_kernel");
}

int ag_smplx_keypoints_backward(float* dL_dvertices, const float* dL_dkeypoints, const int32_t* idx, const float* w, int32_t B, int32_t V,
                                int32_t K, void* stream)
{
    if (B < 0 || K < 0 || K > 1024 || V <= 0) { set_error("smplx_keypoints_backward: bad sizes (need K <= 1024)"); return AG_ERR_INVALID_ARGUMENT; }
    if (B == 0) return AG_OK;
    if (!dL_dvertices || (K > 0 && (!dL_dkeypoints || !idx || !w))) { set_error("null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = check_hip(hipMemsetAsync(dL_dvertices, 0, (size_t)B * V * 3 * sizeof(float), s), "smplx_keypoints_backward: memset");
    if (rc != AG_OK || K == 0) return rc;
    hipLaunchKernelGGL(smplx_keypoints_backward_kernel, dim3(B), dim3(256), sizeof(float) * 9 * K, s, dL_dvertices, dL_dkeypoints, idx, w, V, K);
    return check_hip(hipGetLastError(), "smplx_keypoints_backward_kernel");
}

static size_t vb_skin_slabs(const AgSmplxModel* m) { return (size_t)(m->V + kVbVerts - 1) / kVbVerts; }
static size_t vb_dirs_slabs(const AgSmplxModel* m) { return (size_t)(3 * m->V + kSdCoords - 1) / kSdCoords; }

size_t ag_smplx_vertex_backward_workspace_floats(const AgSmplxModel* m, int32_t B)
{
    if (!m || B <= 0 || m->V <= 0 || m->J <= 0 || m->NB < 0) return 0;
    // dL/dv_posed | skinning slabs | shape-basis slabs
    return (size_t)B * ((size_t)3 * m->V + vb_skin_slabs(m) * ((size_t)12 * m->J + 3) + vb_dirs_slabs(m) * (size_t)m->NB);
}

// slabs [n_slab][B][NB] of smplx_dirs_t_kernel over x [B][3 V]
static void launch_dirs_t(const AgSmplxModel* m, int32_t B, const float* x, float* slabs, hipStream_t s)
{
    hipLaunchKernelGGL(smplx_dirs_t_kernel, dim3((unsigned)vb_dirs_slabs(m), B), dim3(kSdCoords), sizeof(float) * 4 * m->NB, s, slabs, m->shapedirs,
                       x, 3 * m->V, m->NB);
}

int ag_smplx_vertex_backward(const AgSmplxModel* m, int32_t B, const float* saved, const float* dL_dvertices, float* dL_dA_skin,
                             float* dL_dfeat, float* dL_dtransl, float* dL_dshape_components, float* workspace, size_t workspace_floats,
                             void* stream)
{
    int rc;
    if (call_is_over("smplx_vertex_backward", m, B, false, &rc)) return rc;
    if (!saved || !dL_dvertices || !dL_dA_skin || !dL_dtransl || !workspace || (m->J > 1 && !dL_dfeat) || (m->NB > 0 && !dL_dshape_components)) {
        set_error("smplx_vertex_backward: null pointer");
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (workspace_floats < ag_smplx_vertex_backward_workspace_floats(m, B)) { set_error("smplx_vertex_backward: workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_coord = 3 * m->V, P = 9 * (m->J - 1), J = m->J;
    const int n_slab = (int)vb_skin_slabs(m), width = 12 * J + 3;
    const float* v_posed = saved;
    const float* A_skin = saved + (size_t)B * n_coord;
    float* dvp = workspace;
    float* skin_slabs = dvp + (size_t)B * n_coord;
    float* dirs_slabs = skin_slabs + (size_t)n_slab * B * width;

    const size_t lds = sizeof(float) * ((size_t)kVbVerts * J + (size_t)J * 12 + 8 * kVbVerts);
    hipLaunchKernelGGL(smplx_skin_backward_kernel, dim3(n_slab, B), dim3(kVbThreads), lds, s, dvp, skin_slabs, dL_dvertices, v_posed, A_skin,
                       m->lbs_weights, m->V, J);
    const int dirs_total = B * m->NB, n_skin_blocks = (B * width + 15) / 16;
    if (m->NB > 0) launch_dirs_t(m, B, dvp, dirs_slabs, s);
    hipLaunchKernelGGL(smplx_slab_sums_kernel, dim3(n_skin_blocks + (dirs_total + 15) / 16), dim3(256), 0, s, dL_dA_skin, dL_dtransl, skin_slabs,
                       n_slab, B, J, n_skin_blocks, dL_dshape_components, dirs_slabs, (int)vb_dirs_slabs(m), dirs_total);
    if (P > 0)
        for_pose_runs(B, [&](int b0, auto nb) {
            hipLaunchKernelGGL(smplx_posedirs_t_kernel<decltype(nb)::value>, dim3(P), dim3(kPdThreads), 0, s, dL_dfeat + (size_t)b0 * P, m->posedirs,
                               dvp + (size_t)b0 * n_coord, n_coord, P);
        });
    return check_hip(hipGetLastError(), "ag_smplx_vertex_backward");
}

size_t ag_smplx_shape_backward_workspace_floats(const AgSmplxModel* m, int32_t B)
{
    if (!m || B <= 0 || m->V <= 0 || m->NB < 0) return 0;
    return (size_t)B * vb_dirs_slabs(m) * (size_t)m->NB;
}

int ag_smplx_shape_backward(const AgSmplxModel* m, int32_t B, const float* dL_dv_shaped, float* dL_dshape_components, float* workspace,
                            size_t workspace_floats, void* stream)
{
    if (!model_ok(m) || B < 0) { set_error("smplx_shape_backward: bad model or B < 0"); return AG_ERR_INVALID_ARGUMENT; }
    if (B == 0 || m->NB == 0) return AG_OK;
    if (!dL_dv_shaped || !dL_dshape_components || !workspace) { set_error("smplx_shape_backward: null pointer"); return AG_ERR_INVALID_ARGUMENT; }
    if (workspace_floats < ag_smplx_shape_backward_workspace_floats(m, B)) { set_error("smplx_shape_backward: workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int dirs_total = B * m->NB;
    launch_dirs_t(m, B, dL_dv_shaped, workspace, s);
    hipLaunchKernelGGL(smplx_slab_sums_kernel, dim3((dirs_total + 15) / 16), dim3(256), 0, s, (float*)nullptr, (float*)nullptr, (const float*)nullptr,
                       0, B, m->J, 0, dL_dshape_components, workspace, (int)vb_dirs_slabs(m), dirs_total);
    return check_hip(hipGetLastError(), "ag_smplx_shape_backward");
}

int ag_smplx_backward_full(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* dL_dA,
                           const float* dL_djoints, const float* dL_dA_skin, const float* dL_dfeat, const float* dL_dtransl_add,
                           const float* dL_dshape_components_add, float* dL_dfull_pose, float* dL_dtransl, float* dL_dshape_components,
                           void* stream)
{
    return chain_backward_impl<true>("smplx_backward_full", m, B, shape_components, full_pose, dL_dA, dL_djoints, dL_dA_skin, dL_dfeat,
                                     dL_dtransl_add, dL_dshape_components_add, dL_dfull_pose, dL_dtransl, dL_dshape_components, stream);
}

}  // extern "C"
