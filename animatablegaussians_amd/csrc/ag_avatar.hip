// Per-Gaussian assembly (map gather + activations) and linear-blend skinning, forward and backward (gfx950).
//
// Replaces the torch-op chains of reference network/avatar.py:84-124 (see include/ag_avatar.h).  All four kernels are
// HBM-bound streaming kernels, one thread per Gaussian:
//   gather fwd : 14 strided-but-coalesced channel reads (consecutive Gaussians are consecutive map pixels) + 44 B of
//                canonical parameters in, 56 B out                                              ~160 B / Gaussian
//   gather bwd : the same reads + 56 B of upstream gradients, 14 scattered channel writes into pre-zeroed maps
//   lbs fwd/bwd: the [N, J] blend-weight rows (220 B / Gaussian at J = 55, the dominant stream) are staged through
//                wave-private LDS with fully coalesced loads and read back conflict-free (row stride J is odd);
//                the J joint matrices are wave-uniform and come in through scalar loads.
#include <atomic>
#include "ag_common.h"
#include "../../include/ag_avatar.h"

namespace ag {

// ------------------------------------------------------------------------------------------------------------------
// gather + activations
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t map_offset(int pix, int S, int C, int c)
{
    // canvas pixel (v, u) of the [S, 2S] front|back layout -> element of the NCHW [1, 2C, S, S] network output
    const int v = pix / (2 * S), u = pix - v * 2 * S;
    const int back = u >= S;
    return ((size_t)(back * C + c) * S + v) * S + (u - back * S);
}

// Each of the three parts (positions | opacity, scales, rotations | colours) is produced when its output pointer is set;
// a null MAP pointer stands for an all-zero network output (the activations of the canonical parameters alone:
// GaussianModel.get_opacity / get_scaling / get_rotation, gaussians/gaussian_model.py:115-147).  All wave-uniform.
__global__ void __launch_bounds__(256) gather_forward_kernel(AgGatherArgs a)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const int pix = a.pix[n];
    const size_t plane = (size_t)a.S * a.S;
    const size_t o3 = map_offset(pix, a.S, 3, 0), o8 = map_offset(pix, a.S, 8, 0);
    if (a.positions) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            a.positions[3 * n + c] = 0.05f * (a.position_map ? a.position_map[o3 + c * plane] : 0.f) + a.xyz[3 * n + c];
    }
    if (a.colors) {
#pragma unroll
        for (int c = 0; c < 3; c++) a.colors[3 * n + c] = a.color_map ? a.color_map[o3 + c * plane] : 0.f;
    }
    if (!a.opacity) return;
    float m[8];
#pragma unroll
    for (int c = 0; c < 8; c++) m[c] = a.other_map ? a.other_map[o8 + c * plane] : 0.f;
    const float o = m[0] + a.opacity_raw[n];
    a.opacity[n] = 1.0f / (1.0f + expf(-o));
#pragma unroll
    for (int c = 0; c < 3; c++) a.scales[3 * n + c] = expf(m[1 + c] + a.scaling_raw[3 * n + c]);
    float q[4], nn = 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        q[c] = m[4 + c] + a.rotation_raw[4 * n + c];
        nn += q[c] * q[c];
    }
    const float inv = 1.0f / fmaxf(sqrtf(nn), 1e-12f);   // F.normalize: x / max(||x||, eps)
#pragma unroll
    for (int c = 0; c < 4; c++) a.rotations[4 * n + c] = q[c] * inv;
}

// A null gradient-map pointer skips that part (its upstream-gradient slots are then not read).
__global__ void __launch_bounds__(256) gather_backward_kernel(AgGatherArgs a, float* __restrict__ g_pos_map,
                                                             float* __restrict__ g_other_map, float* __restrict__ g_col_map)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const int pix = a.pix[n];
    const size_t plane = (size_t)a.S * a.S;
    const size_t o3 = map_offset(pix, a.S, 3, 0), o8 = map_offset(pix, a.S, 8, 0);
    if (g_pos_map) {
#pragma unroll
        for (int c = 0; c < 3; c++) g_pos_map[o3 + c * plane] = 0.05f * a.positions[3 * n + c];
    }
    if (g_col_map) {
#pragma unroll
        for (int c = 0; c < 3; c++) g_col_map[o3 + c * plane] = a.colors[3 * n + c];
    }
    if (!g_other_map) return;
    // sigmoid'
    const float o = a.other_map[o8] + a.opacity_raw[n];
    const float sg = 1.0f / (1.0f + expf(-o));
    g_other_map[o8] = a.opacity[n] * sg * (1.0f - sg);
    // exp'
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float e = expf(a.other_map[o8 + (1 + c) * plane] + a.scaling_raw[3 * n + c]);
        g_other_map[o8 + (1 + c) * plane] = a.scales[3 * n + c] * e;
    }
    // normalize': y = x / max(|x|, eps); for |x| > eps: dx = (g - y (y.g)) / |x|, else dx = g / eps
    float q[4], nn = 0.f, g[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        q[c] = a.other_map[o8 + (4 + c) * plane] + a.rotation_raw[4 * n + c];
        nn += q[c] * q[c];
        g[c] = a.rotations[4 * n + c];
    }
    const float norm = sqrtf(nn);
    if (norm > 1e-12f) {
        const float inv = 1.0f / norm;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < 4; c++) dot += q[c] * inv * g[c];
#pragma unroll
        for (int c = 0; c < 4; c++) g_other_map[o8 + (4 + c) * plane] = (g[c] - q[c] * inv * dot) * inv;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) g_other_map[o8 + (4 + c) * plane] = g[c] * 1e12f;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// linear-blend skinning
// ------------------------------------------------------------------------------------------------------------------
constexpr int kMaxJ = 256;

// Blend the joint matrices of one Gaussian: M[3][4] = sum_j w_j A_j[:3, :4].  `row` points at this lane's weights in
// LDS; jnt is wave-uniform (scalar loads).
__device__ __forceinline__ void blend_matrix(const float* row, const float* __restrict__ jnt, int J, float (&M)[12])
{
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = 0.f;
    for (int j = 0; j < J; j++) {
        const float w = row[j];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] += w * jnt[16 * j + k];
    }
}

// The same blend from the sparse form of the weight rows: K (joint, weight) pairs per Gaussian in ascending joint order, padded
// with zero weights, stored [K][N] so that lanes read consecutive addresses.  Skipping the exact zeros of a row leaves every
// partial sum unchanged (x + 0 * a == x), so the result equals the dense loop's bit for bit (up to the sign of an exact zero).
__device__ __forceinline__ void blend_matrix_sparse(const uint8_t* __restrict__ idx, const float* __restrict__ wts, int K, int N, int n,
                                                    const float* __restrict__ jnt, float (&M)[12])
{
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = 0.f;
    for (int s = 0; s < K; s++) {
        const float w = wts[(size_t)s * N + n];
        const float* A = jnt + 16 * (int)idx[(size_t)s * N + n];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] += w * A[k];
    }
}

// Coalesced load of the 64 weight rows of this wave into its LDS slab (row stride J).
__device__ __forceinline__ void stage_rows(const float* __restrict__ lbs, int N, int J, int first, float* slab, int lane)
{
    const size_t base = (size_t)first * J;
    const int rows = min(64, N - first);
    const int total = rows * J;
    for (int i = lane; i < total; i += 64) slab[i] = lbs[base + i];
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void quat_to_mat(const float (&q)[4], float (&R)[9], float& two_s)
{
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    two_s = 2.0f / (r * r + i * i + j * j + k * k);
    R[0] = 1 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r);     R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);     R[4] = 1 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);     R[7] = two_s * (j * k + i * r);     R[8] = 1 - two_s * (i * i + j * j);
}

// The rotation head of one Gaussian, the part of the forward that the backward has to recompute bit for bit: R(q), m = M3 * R, then
// pytorch3d 0.7.4 matrix_to_quaternion up to its candidate row -- sqrt of the positive part, arg-max candidate, no sign fix.  The
// division by 2 max(qa[best], 0.1) is the caller's.  Everything lands in the caller's locals: returned as a struct, the dynamically
// indexed qa[best] puts the whole head into scratch ('Skinning kernels: what is stated once').
__device__ __forceinline__ void rotation_head(const float (&q)[4], const float (&M)[12], float (&R)[9], float& two_s, float (&m)[9],
                                              float (&x4)[4], float (&qa)[4], float (&cand)[4], int& best)
{
    quat_to_mat(q, R, two_s);
    // m = M3 * R = M[4x] R[z] + M[4x + 1] R[3 + z] + M[4x + 2] R[6 + z] with its fusing written out.  Left to -ffp-contract=fast, which of the
    // first two products stays a multiplication depends on how far the caller is optimised when this is inlined: lbs_backward_joints_kernel
    // used to get the other pairing in m[0], m[3], m[6] than the forward it recomputes.  This is the pairing lbs_forward_kernel always had.
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int z = 0; z < 3; z++) m[3 * x + z] = fmaf(M[4 * x + 2], R[6 + z], fmaf(M[4 * x], R[z], M[4 * x + 1] * R[3 + z]));
    x4[0] = 1.0f + m[0] + m[4] + m[8]; x4[1] = 1.0f + m[0] - m[4] - m[8]; x4[2] = 1.0f - m[0] + m[4] - m[8]; x4[3] = 1.0f - m[0] - m[4] + m[8];
#pragma unroll
    for (int c = 0; c < 4; c++) qa[c] = x4[c] > 0.f ? sqrtf(x4[c]) : 0.f;
    best = 0;
#pragma unroll
    for (int c = 1; c < 4; c++) if (qa[c] > qa[best]) best = c;
    if (best == 0)      { cand[0] = qa[0] * qa[0]; cand[1] = m[7] - m[5]; cand[2] = m[2] - m[6]; cand[3] = m[3] - m[1]; }
    else if (best == 1) { cand[0] = m[7] - m[5]; cand[1] = qa[1] * qa[1]; cand[2] = m[3] + m[1]; cand[3] = m[2] + m[6]; }
    else if (best == 2) { cand[0] = m[2] - m[6]; cand[1] = m[3] + m[1]; cand[2] = qa[2] * qa[2]; cand[3] = m[5] + m[7]; }
    else                { cand[0] = m[3] - m[1]; cand[1] = m[6] + m[2]; cand[2] = m[7] + m[5]; cand[3] = qa[3] * qa[3]; }
}

// What lbs_forward_kernel and lbs_backward_kernel start with: the wave's 64 weight rows staged in its LDS slab (dense) and the lane's
// Gaussian n with its blended matrix M.  False for a wave past N (before it stages anything) and for a lane past N (after its wave has
// staged): the kernel returns.
template <bool SPARSE>
__device__ __forceinline__ bool lbs_lane_matrix(const AgLbsArgs& a, int& n, float (&M)[12])
{
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = (blockIdx.x * 4 + wave) * 64;
    if (first >= a.N) return false;
    n = first + lane;
    if constexpr (SPARSE) {
        if (n >= a.N) return false;
        blend_matrix_sparse(a.sp_idx, a.sp_w, a.K, a.N, n, a.jnt_mats, M);
    } else {
        float* slab = lds + (size_t)wave * 64 * a.J;
        stage_rows(a.lbs, a.N, a.J, first, slab, lane);
        if (n >= a.N) return false;
        blend_matrix(slab + lane * a.J, a.jnt_mats, a.J, M);
    }
    return true;
}

template <bool SPARSE>
__global__ void __launch_bounds__(256) lbs_forward_kernel(AgLbsArgs a)
{
    int n;
    float M[12];
    if (!lbs_lane_matrix<SPARSE>(a, n, M)) return;
    const float px = a.positions[3 * n], py = a.positions[3 * n + 1], pz = a.positions[3 * n + 2];
    a.out_positions[3 * n + 0] = M[0] * px + M[1] * py + M[2] * pz + M[3];
    a.out_positions[3 * n + 1] = M[4] * px + M[5] * py + M[6] * pz + M[7];
    a.out_positions[3 * n + 2] = M[8] * px + M[9] * py + M[10] * pz + M[11];

    float q[4] = { a.rotations[4 * n], a.rotations[4 * n + 1], a.rotations[4 * n + 2], a.rotations[4 * n + 3] };
    float R[9], two_s, m[9], x4[4], qa[4], cand[4];
    int best;
    rotation_head(q, M, R, two_s, m, x4, qa, cand, best);
    const float den = 2.0f * fmaxf(qa[best], 0.1f);      // the 0.1 floor
#pragma unroll
    for (int c = 0; c < 4; c++) a.out_rotations[4 * n + c] = cand[c] / den;
}

// The backward of one Gaussian with its blended matrix M; a.out_positions / a.out_rotations hold the upstream gradients.  What it
// writes is fixed by the instantiation, so that dL/dq and dL/dA walk one text back from out = cand / den:
//   JOINTS = false  dL/dpositions and dL/drotations to g_positions / g_rotations (lbs_backward_kernel); GM is not touched
//   JOINTS = true   GM[12] = dL/dM (3x4), the per-Gaussian term of the joint-matrix gradient dL/dA_j = sum_n w_nj GM_n
//                   (lbs_backward_joints_kernel); the two pointers are not touched -- those gradients come from lbs_backward_kernel's
//                   own launch (ag_lbs_backward_joints), so that they are ag_lbs_backward's bits
template <bool JOINTS>
__device__ __forceinline__ void lbs_backward_gaussian(const AgLbsArgs& a, int n, const float (&M)[12], float* __restrict__ g_positions,
                                                      float* __restrict__ g_rotations, float (&GM)[12])
{
    const float gx = a.out_positions[3 * n], gy = a.out_positions[3 * n + 1], gz = a.out_positions[3 * n + 2];
    if constexpr (JOINTS) {
        // live p = M3 p + M[:, 3]  ->  dL/dM = g (x) [p, 1]
        const float p[3] = { a.positions[3 * n], a.positions[3 * n + 1], a.positions[3 * n + 2] };
        const float g[3] = { gx, gy, gz };
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) GM[4 * r + c] = g[r] * p[c];
            GM[4 * r + 3] = g[r];
        }
    } else {
        // positions: dL/dp = M3^T g
        g_positions[3 * n + 0] = M[0] * gx + M[4] * gy + M[8] * gz;
        g_positions[3 * n + 1] = M[1] * gx + M[5] * gy + M[9] * gz;
        g_positions[3 * n + 2] = M[2] * gx + M[6] * gy + M[10] * gz;
    }

    // rotations: recompute the forward, then walk the chain backwards
    float q[4] = { a.rotations[4 * n], a.rotations[4 * n + 1], a.rotations[4 * n + 2], a.rotations[4 * n + 3] };
    float R[9], two_s, m[9], x4[4], qa[4], cand[4];
    int best;
    rotation_head(q, M, R, two_s, m, x4, qa, cand, best);
    const float qsel = qa[best];
    const bool floored = !(qsel > 0.1f);
    const float den = 2.0f * (floored ? 0.1f : qsel);
    float go[4] = { a.out_rotations[4 * n], a.out_rotations[4 * n + 1], a.out_rotations[4 * n + 2], a.out_rotations[4 * n + 3] };
    // out = cand / den
    float gc[4], gden = 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++) { gc[c] = go[c] / den; gden -= go[c] * cand[c] / (den * den); }
    // den = 2 max(q_sel, 0.1): no gradient when the floor is active; the diagonal candidate is q_sel^2
    float gq_sel = floored ? 0.f : 2.0f * gden;
    gq_sel += 2.0f * qsel * gc[best];
    // q_sel = sqrt(max(0, x_sel)) (zero sub-gradient at x <= 0)
    const float gx_sel = (x4[best] > 0.f) ? gq_sel / (2.0f * qsel) : 0.f;
    float gm[9];
#pragma unroll
    for (int c = 0; c < 9; c++) gm[c] = 0.f;
    const float s0 = (best == 0 || best == 1) ? 1.f : -1.f;   // sign of m00 in x_best
    const float s1 = (best == 0 || best == 2) ? 1.f : -1.f;   // sign of m11
    const float s2 = (best == 0 || best == 3) ? 1.f : -1.f;   // sign of m22
    gm[0] += s0 * gx_sel; gm[4] += s1 * gx_sel; gm[8] += s2 * gx_sel;
    if (best == 0)      { gm[7] += gc[1]; gm[5] -= gc[1]; gm[2] += gc[2]; gm[6] -= gc[2]; gm[3] += gc[3]; gm[1] -= gc[3]; }
    else if (best == 1) { gm[7] += gc[0]; gm[5] -= gc[0]; gm[3] += gc[2]; gm[1] += gc[2]; gm[2] += gc[3]; gm[6] += gc[3]; }
    else if (best == 2) { gm[2] += gc[0]; gm[6] -= gc[0]; gm[3] += gc[1]; gm[1] += gc[1]; gm[5] += gc[3]; gm[7] += gc[3]; }
    else                { gm[3] += gc[0]; gm[1] -= gc[0]; gm[6] += gc[1]; gm[2] += gc[1]; gm[7] += gc[2]; gm[5] += gc[2]; }
    if constexpr (JOINTS) {
        // m = M3 R  ->  dL/dM3 = gm R^T
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) GM[4 * x + y] += gm[3 * x] * R[3 * y] + gm[3 * x + 1] * R[3 * y + 1] + gm[3 * x + 2] * R[3 * y + 2];
        return;
    }
    // m = M3 R  ->  dL/dR = M3^T gm
    float G[9];
#pragma unroll
    for (int y = 0; y < 3; y++)
#pragma unroll
        for (int z = 0; z < 3; z++) G[3 * y + z] = M[y] * gm[z] + M[4 + y] * gm[3 + z] + M[8 + y] * gm[6 + z];
    // R = I + two_s * U(q); dL/dq = two_s * dU^T G - two_s^2 q (U . G)
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float U[9] = { -(j * j + k * k), i * j - k * r, i * k + j * r,
                         i * j + k * r, -(i * i + k * k), j * k - i * r,
                         i * k - j * r, j * k + i * r, -(i * i + j * j) };
    float gs = 0.f;
#pragma unroll
    for (int c = 0; c < 9; c++) gs += G[c] * U[c];
    const float dr = -k * G[1] + j * G[2] + k * G[3] - i * G[5] - j * G[6] + i * G[7];
    const float di = j * G[1] + k * G[2] + j * G[3] - 2 * i * G[4] - r * G[5] + k * G[6] + r * G[7] - 2 * i * G[8];
    const float dj = -2 * j * G[0] + i * G[1] + r * G[2] + i * G[3] + k * G[5] - r * G[6] + k * G[7] - 2 * j * G[8];
    const float dk = -2 * k * G[0] - r * G[1] + i * G[2] + r * G[3] - 2 * k * G[4] + j * G[5] + i * G[6] + j * G[7];
    const float t2 = two_s * two_s * gs;
    g_rotations[4 * n + 0] = two_s * dr - t2 * r;
    g_rotations[4 * n + 1] = two_s * di - t2 * i;
    g_rotations[4 * n + 2] = two_s * dj - t2 * j;
    g_rotations[4 * n + 3] = two_s * dk - t2 * k;
}

template <bool SPARSE>
__global__ void __launch_bounds__(256) lbs_backward_kernel(AgLbsArgs a, float* __restrict__ g_positions,
                                                          float* __restrict__ g_rotations)
{
    int n;
    float M[12], no_gm[12];
    if (!lbs_lane_matrix<SPARSE>(a, n, M)) return;
    lbs_backward_gaussian<false>(a, n, M, g_positions, g_rotations, no_gm);
}

// Joint-matrix gradient, pass 1 (the blend and lbs_backward_gaussian<true>, plus the reduction of its workgroup; its own prologue, as its idle lanes stay to
// the reduction): every workgroup writes its
// slab [J][12] = sum over its 256 Gaussians of w_nj GM_n.  LDS: [4 waves][64][J] weight rows | [4][64][12] GM rows; the [J][12] partial of a wave goes over its
// own weight rows once every lane has read its columns (12 J <= 64 J floats), which is what lets J = 140 fit: (256 J + 3072) * 4 B = 155648 B of the 163840.
// The sparse form is expanded into the dense row layout (zeros, then its K weights), so both forms run the same summation over the same
// values in the same order: a skipped term is + 0 * GM, and the slabs are bit-identical.  Lane l of a wave sums columns l, l + 64, l + 128 over the 64 rows in
// order, into registers; the four wave partials are added in wave order.  No float atomics: the slabs are combined by lbs_joint_slab_reduce_kernel.
constexpr int kJointGradMaxJ = 140;                          // include/ag_avatar.h
constexpr int kJointCols = (kJointGradMaxJ + 63) / 64;       // columns of the weight rows per lane: the kernel covers J <= 64 * kJointCols and
                                                             // relies on ag_lbs_backward_joints refusing J > kJointGradMaxJ
static_assert(kJointGradMaxJ <= 64 * kJointCols && (256 * kJointGradMaxJ + 3072) * 4 <= 160 * 1024, "the joint-gradient pass at its largest J");
template <bool SPARSE>
__global__ void __launch_bounds__(256) lbs_backward_joints_kernel(AgLbsArgs a, float* __restrict__ slabs)
{
    extern __shared__ float lds[];
    const int J = a.J;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = (blockIdx.x * 4 + wave) * 64;
    const int rows = max(0, min(64, a.N - first));            // wave-uniform; 0 for the idle waves of the last workgroup
    float* tile = lds + (size_t)wave * 64 * J;
    float* gm_rows = lds + (size_t)4 * 64 * J + wave * 64 * 12;
    const int n = first + lane;
    float GM[12];
#pragma unroll
    for (int k = 0; k < 12; k++) GM[k] = 0.f;
    if (rows > 0) {
        float M[12];
        if constexpr (SPARSE) {
            for (int i = lane; i < rows * J; i += 64) tile[i] = 0.f;
            __builtin_amdgcn_wave_barrier();
            if (lane < rows) {
                for (int s = 0; s < a.K; s++) {
                    const int j = a.sp_idx[(size_t)s * a.N + n];
                    if (j < J) tile[lane * J + j] += a.sp_w[(size_t)s * a.N + n];
                }
                blend_matrix_sparse(a.sp_idx, a.sp_w, a.K, a.N, n, a.jnt_mats, M);
            }
            __builtin_amdgcn_wave_barrier();
        } else {
            stage_rows(a.lbs, a.N, J, first, tile, lane);
            if (lane < rows) blend_matrix(tile + lane * J, a.jnt_mats, J, M);
        }
        if (lane < rows) lbs_backward_gaussian<true>(a, n, M, nullptr, nullptr, GM);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) gm_rows[lane * 12 + k] = GM[k];
    __builtin_amdgcn_wave_barrier();
    float acc[kJointCols][12];
#pragma unroll
    for (int t = 0; t < kJointCols; t++) {
        const int j = lane + 64 * t;
#pragma unroll
        for (int k = 0; k < 12; k++) acc[t][k] = 0.f;
        if (j < J) {
            for (int r = 0; r < rows; r++) {
                const float w = tile[r * J + j];
                const float* g = gm_rows + r * 12;              // wave-uniform address: broadcast
#pragma unroll
                for (int k = 0; k < 12; k++) acc[t][k] = fmaf(w, g[k], acc[t][k]);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();                        // every lane of the wave has read its columns: the partial may overwrite the rows
    float* part = tile;                                     // [J][12]
#pragma unroll
    for (int t = 0; t < kJointCols; t++) {
        const int j = lane + 64 * t;
        if (j < J) {
#pragma unroll
            for (int k = 0; k < 12; k++) part[j * 12 + k] = acc[t][k];
        }
    }
    __syncthreads();
    const int JK = J * 12;
    const size_t wave_stride = (size_t)64 * J;              // between the partials of two waves
    float* out = slabs + (size_t)blockIdx.x * JK;
    for (int i = threadIdx.x; i < JK; i += 256) out[i] = ((lds[i] + lds[wave_stride + i]) + lds[2 * wave_stride + i]) + lds[3 * wave_stride + i];
}

// Joint-matrix gradient, pass 2: dL/dA [J][4][4] = the sum of the slabs, in a fixed order.  A workgroup owns 16 of the J * 12 outputs:
// thread (group g, output c) sums slabs g, g + 64, g + 128, ... in order, then a fixed tree over the 64 groups.  Row 3 of every
// matrix is written as 0 (the forward never reads it).
constexpr int kSlabOuts = 16, kSlabGroups = 64;
__global__ void __launch_bounds__(kSlabOuts * kSlabGroups) lbs_joint_slab_reduce_kernel(const float* __restrict__ slabs, int nslab, int J,
                                                                                        float* __restrict__ g_jnt)
{
    __shared__ float s_part[kSlabGroups][kSlabOuts + 1];
    const int c = threadIdx.x % kSlabOuts, g = threadIdx.x / kSlabOuts;
    const int JK = J * 12;
    const int o = blockIdx.x * kSlabOuts + c;
    float acc = 0.f;
    if (o < JK)
        for (int s = g; s < nslab; s += kSlabGroups) acc += slabs[(size_t)s * JK + o];
    s_part[g][c] = acc;
    __syncthreads();
    for (int h = kSlabGroups / 2; h > 0; h >>= 1) {
        if (g < h) s_part[g][c] += s_part[g + h][c];
        __syncthreads();
    }
    if (g == 0 && o < JK) g_jnt[(o / 12) * 16 + o % 12] = s_part[0][c];
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 4 * J; i += kSlabOuts * kSlabGroups) g_jnt[(i / 4) * 16 + 12 + i % 4] = 0.f;
}

}  // namespace ag

using namespace ag;

// Eval-time hand fusion (network/avatar.py:183-200): one thread per Gaussian, 11 attribute floats blended in place.
__global__ void __launch_bounds__(256) hand_fuse_kernel(AgHandFuseArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const float x = a.xyz[3 * i + 0], y = a.xyz[3 * i + 1];
    const float lmin = a.left_box[0], lmax = a.left_box[1], rmin = a.right_box[0], rmax = a.right_box[1];
    // utils/geo_util.py:104-114 with per_axis: 2 (v - 0.5 (max + min)) / (max - min), first coordinate
    const float nl = 2.0f * (x - 0.5f * (lmax + lmin)) / (lmax - lmin);
    const float nr = 2.0f * (x - 0.5f * (rmax + rmin)) / (rmax - rmin);
    float wl = 1.0f / (1.0f + __expf(-2.5f * (nl + 2.0f)));
    float wr = 1.0f / (1.0f + __expf(2.5f * (nr - 2.0f)));
    if (y < a.centre[1]) { wl = 0.f; wr = 0.f; }
    const float s = fmaxf(wl + wr, 1.0f);
    const float w = wl / s + wr / s;
    const float u = 1.0f - w;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.positions[3 * i + c] = w * a.hand_positions[3 * i + c] + u * a.positions[3 * i + c];
    a.opacity[i] = w * a.hand_opacity[i] + u * a.opacity[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.scales[3 * i + c] = w * a.hand_scales[3 * i + c] + u * a.scales[3 * i + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) a.rotations[4 * i + c] = w * a.hand_rotations[4 * i + c] + u * a.rotations[4 * i + c];
}

// One launch of a skinning kernel pair, a workgroup per 256 Gaussians: the sparse instantiation when a->K > 0, else the dense one, each with
// its bytes of dynamic LDS.  More than 48 KiB of it has to be asked for per kernel; a refusal is this call's error, not the launch's.
template <class Kernel, class... Rest>
static int launch_lbs_pair(const AgLbsArgs* a, Kernel sparse_kernel, Kernel dense_kernel, int sparse_lds, int dense_lds, const char* name,
                           hipStream_t s, Rest... rest)
{
    const Kernel kernel = a->K > 0 ? sparse_kernel : dense_kernel;
    const int lds = a->K > 0 ? sparse_lds : dense_lds;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) { set_error("%s (LDS size): %s", name, hipGetErrorString(e)); return AG_ERR_HIP; }
    }
    hipLaunchKernelGGL(kernel, dim3((a->N + 255) / 256), dim3(256), lds, s, *a, rest...);
    return check_hip(hipGetLastError(), name);
}

extern "C" {

int ag_hand_fuse(const AgHandFuseArgs* a, void* stream)
{
    if (!a || a->N < 0) { set_error("bad hand-fuse sizes"); return AG_ERR_INVALID_ARGUMENT; }
    if (a->N == 0) return AG_OK;
    if (!a->xyz || !a->left_box || !a->right_box || !a->centre || !a->hand_positions || !a->hand_opacity || !a->hand_scales ||
        !a->hand_rotations || !a->positions || !a->opacity || !a->scales || !a->rotations) {
        set_error("null pointer in AgHandFuseArgs");
        return AG_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(hand_fuse_kernel, dim3((a->N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a);
    return check_hip(hipGetLastError(), "hand_fuse_kernel");
}

static int check_gather_sizes(const AgGatherArgs* a)
{
    if (!a || a->N < 0 || a->S <= 0) { set_error("bad gather sizes"); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

static int check_gather(const AgGatherArgs* a)
{
    int rc = check_gather_sizes(a);
    if (rc || a->N == 0) return rc;
    const bool others_all = a->opacity && a->scales && a->rotations, others_none = !a->opacity && !a->scales && !a->rotations;
    if (!a->pix || (a->positions && !a->xyz) || !(others_all || others_none) ||
        (others_all && (!a->opacity_raw || !a->scaling_raw || !a->rotation_raw)) || (!a->positions && others_none && !a->colors)) {
        set_error("AgGatherArgs: pix, at least one output part, and the canonical parameters of every requested part are required");
        return AG_ERR_INVALID_ARGUMENT;
    }
    return AG_OK;
}

int ag_gather_activate_forward(const AgGatherArgs* a, void* stream)
{
    int rc = check_gather(a);
    if (rc || a->N == 0) return rc;
    hipLaunchKernelGGL(gather_forward_kernel, dim3((a->N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a);
    return check_hip(hipGetLastError(), "gather_forward_kernel");
}

int ag_gather_activate_backward(const AgGatherArgs* a, float* g_pos_map, float* g_other_map, float* g_col_map, void* stream)
{
    int rc = check_gather_sizes(a);
    if (rc) return rc;
    if (!g_pos_map && !g_other_map && !g_col_map) { set_error("no gradient map requested"); return AG_ERR_INVALID_ARGUMENT; }
    if (a->N > 0 && (!a->pix || (g_pos_map && !a->positions) || (g_col_map && !a->colors) ||
                     (g_other_map && (!a->other_map || !a->opacity_raw || !a->scaling_raw || !a->rotation_raw || !a->opacity ||
                                      !a->scales || !a->rotations)))) {
        set_error("AgGatherArgs: a requested gradient map needs its upstream gradients (and, for the other map, the forward inputs)");
        return AG_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t plane = (size_t)a->S * a->S * sizeof(float);
    if (g_pos_map && (rc = check_hip(hipMemsetAsync(g_pos_map, 0, 6 * plane, s), "memset"))) return rc;
    if (g_other_map && (rc = check_hip(hipMemsetAsync(g_other_map, 0, 16 * plane, s), "memset"))) return rc;
    if (g_col_map && (rc = check_hip(hipMemsetAsync(g_col_map, 0, 6 * plane, s), "memset"))) return rc;
    if (a->N == 0) return AG_OK;
    hipLaunchKernelGGL(gather_backward_kernel, dim3((a->N + 255) / 256), dim3(256), 0, s, *a, g_pos_map, g_other_map, g_col_map);
    return check_hip(hipGetLastError(), "gather_backward_kernel");
}

// The dense kernels stage the 4 x 64 weight rows of a workgroup in LDS: 4 * 64 * J floats, which has to fit the device's LDS per workgroup
// (163840 B on gfx950: J <= 160).  The sparse kernels use no LDS and take every J a uint8 index reaches.
static int lbs_dense_lds_bytes(int J) { return 4 * 64 * J * (int)sizeof(float); }

// LDS per workgroup of the current device (hipDeviceAttributeMaxSharedMemoryPerBlock), asked once per device.
static int device_lds_bytes(int* bytes)
{
    constexpr int kDevices = 64;
    static std::atomic<int> cached[kDevices];
    int dev = 0, rc;
    if ((rc = check_hip(hipGetDevice(&dev), "hipGetDevice"))) return rc;
    const bool slot = dev >= 0 && dev < kDevices;
    int v = slot ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (v <= 0) {
        if ((rc = check_hip(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev), "hipDeviceGetAttribute"))) return rc;
        if (slot) cached[dev].store(v, std::memory_order_relaxed);
    }
    *bytes = v;
    return AG_OK;
}

static int check_lbs(const AgLbsArgs* a)
{
    if (!a || a->N < 0 || a->J < 1) { set_error("bad lbs sizes (N >= 0, J >= 1)"); return AG_ERR_INVALID_ARGUMENT; }
    if (a->K <= 0) {            // dense: refuse here what the launch would refuse (also at N == 0: the contract does not depend on N)
        int lds_max = 0, rc;
        if ((rc = device_lds_bytes(&lds_max))) return rc;
        if (a->J > lds_max / lbs_dense_lds_bytes(1)) {
            set_error("dense lbs: J = %d stages %lld B of LDS per workgroup, the device has %d B (largest dense J = %d; the sparse form, K > 0, takes J <= %d)",
                      a->J, (long long)a->J * lbs_dense_lds_bytes(1), lds_max, lds_max / lbs_dense_lds_bytes(1), kMaxJ);
            return AG_ERR_INVALID_ARGUMENT;
        }
    }
    if (a->J > kMaxJ) { set_error("bad lbs sizes (sparse rows: 1 <= J <= %d)", kMaxJ); return AG_ERR_INVALID_ARGUMENT; }
    if (a->N == 0) return AG_OK;
    const bool sparse = a->K > 0;
    if ((sparse ? (!a->sp_idx || !a->sp_w || a->K > a->J) : !a->lbs) || !a->jnt_mats || !a->positions || !a->rotations || !a->out_positions ||
        !a->out_rotations) {
        set_error("null pointer in AgLbsArgs (dense: lbs; sparse, K > 0: sp_idx + sp_w, K <= J)");
        return AG_ERR_INVALID_ARGUMENT;
    }
    return AG_OK;
}

int ag_lbs_forward(const AgLbsArgs* a, void* stream)
{
    int rc = check_lbs(a);
    if (rc || a->N == 0) return rc;
    return launch_lbs_pair(a, lbs_forward_kernel<true>, lbs_forward_kernel<false>, 0, lbs_dense_lds_bytes(a->J), "lbs_forward_kernel",
                           reinterpret_cast<hipStream_t>(stream));
}

int ag_lbs_backward(const AgLbsArgs* a, float* g_positions, float* g_rotations, void* stream)
{
    int rc = check_lbs(a);
    if (rc || a->N == 0) return rc;
    if (!g_positions || !g_rotations) { set_error("null gradient output"); return AG_ERR_INVALID_ARGUMENT; }
    return launch_lbs_pair(a, lbs_backward_kernel<true>, lbs_backward_kernel<false>, 0, lbs_dense_lds_bytes(a->J), "lbs_backward_kernel",
                           reinterpret_cast<hipStream_t>(stream), g_positions, g_rotations);
}

size_t ag_lbs_backward_joints_workspace_bytes(int32_t N, int32_t J)
{
    if (N <= 0 || J <= 0) return 0;
    return (size_t)((N + 255) / 256) * (size_t)J * 12 * sizeof(float);
}

int ag_lbs_backward_joints(const AgLbsArgs* a, float* g_positions, float* g_rotations, float* g_jnt_mats, void* workspace,
                           size_t workspace_bytes, void* stream)
{
    int rc = check_lbs(a);
    if (rc) return rc;
    if (!g_jnt_mats) { set_error("null joint-matrix gradient output"); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->N == 0) return check_hip(hipMemsetAsync(g_jnt_mats, 0, (size_t)a->J * 16 * sizeof(float), s), "memset");
    if (!workspace || workspace_bytes < ag_lbs_backward_joints_workspace_bytes(a->N, a->J)) {
        set_error("lbs_backward_joints: workspace too small");
        return AG_ERR_SCRATCH_TOO_SMALL;
    }
    const int nslab = (a->N + 255) / 256;
    if (a->J > kJointGradMaxJ) { set_error("lbs_backward_joints: J = %d, the joint gradient takes J <= %d", a->J, kJointGradMaxJ); return AG_ERR_INVALID_ARGUMENT; }
    const int lds = (4 * 64 * a->J + 4 * 64 * 12) * (int)sizeof(float);         // <= 155648 B at J = 140
    float* slabs = static_cast<float*>(workspace);
    if (g_positions || g_rotations) {            // the position / rotation gradients: ag_lbs_backward's own launch, bit for bit
        if (!g_positions || !g_rotations) { set_error("lbs_backward_joints: dL_dpositions and dL_drotations are both set or both NULL"); return AG_ERR_INVALID_ARGUMENT; }
        if ((rc = ag_lbs_backward(a, g_positions, g_rotations, stream))) return rc;
    }
    if ((rc = launch_lbs_pair(a, lbs_backward_joints_kernel<true>, lbs_backward_joints_kernel<false>, lds, lds, "lbs_backward_joints_kernel", s, slabs)))
        return rc;
    hipLaunchKernelGGL(lbs_joint_slab_reduce_kernel, dim3((a->J * 12 + kSlabOuts - 1) / kSlabOuts), dim3(kSlabOuts * kSlabGroups), 0, s,
                       slabs, nslab, a->J, g_jnt_mats);
    return check_hip(hipGetLastError(), "lbs_joint_slab_reduce_kernel");
}

}  // extern "C"
