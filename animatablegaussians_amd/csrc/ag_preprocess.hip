// Forward per-Gaussian preprocess + per-tile instance counting (gfx950).
//
// Replaces preprocessCUDA<3> (reference cuda_rasterizer/forward.cu:155-256) and produces, instead of the
// reference's Gaussian-major `tiles_touched` prefix sum, per-TILE instance counts (one global atomic per
// (Gaussian, tile) instance).  The tile-major counts make the later binning a counting sort by tile, so no
// device-wide 64-bit radix sort is needed (see ag_binning.hip).
//
// THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off: the fp32 expression order below and in ag_gauss_geom.h is the contract that
// makes radii / tile rects / depth keys bit-identical to the CPU oracle (oracle/raster_oracle.c), which in turn
// restates the reference's expression order (GLM column-major mat3 products, left-to-right sums).
// HBM-bound streaming kernel: 44 B in, 48 B record + 24 B cov3D + 8 B out per Gaussian.
#include "ag_gauss_geom.h"
#include "ag_sh.h"

namespace ag {

__device__ __forceinline__ float ndc2pix(float v, int S)
{
    return (float)((((double)v + 1.0) * (double)S - 1.0) * 0.5);
}

struct PreParams {
    int P, W, H, gx, gy;
    float tan_fovx, tan_fovy;
    Focal focal;
    float scale_modifier;
    const float* __restrict__ means3D;
    const float* __restrict__ scales;
    const float* __restrict__ rotations;
    const float* __restrict__ opacities;
    const float* __restrict__ colors;       // precomputed colours, or NULL -> spherical harmonics below
    const float* __restrict__ shs;          // [P][sh_coeffs][3]
    const float* __restrict__ campos;
    uint8_t* __restrict__ clamped;          // [P][3], written on the SH path (the backward zeroes clamped channels' gradients)
    int sh_degree, sh_coeffs;
    const float* __restrict__ cov3D_precomp;
    const float* __restrict__ view;
    const float* __restrict__ proj;
    int* __restrict__ radii;
    GaussRec* __restrict__ rec;
    float* __restrict__ cov3Ds;
    uint32_t* __restrict__ tiles_touched;
    uint32_t* __restrict__ tile_count;
};

__global__ void __launch_bounds__(256) preprocess_kernel(PreParams p)
{
    // Workgroup-local tile histogram: the 256 Gaussians of a workgroup are neighbours on the canonical map, so
    // their tile rects fall into a small window of the tile grid.  Instances are counted with LDS atomics inside that
    // window and flushed with ONE global atomic per (workgroup, tile): ~20x fewer same-address global atomics than
    // one per instance (which serialise in L2 at ~5 M/s per address and cost 190 us at avatar scale).
    __shared__ int s_win[4];
    __shared__ uint32_t s_hist[kWinBins];
    // The 48-byte records and the 24-byte covariances leave through LDS: a thread's own record would be 12 + 6 dword stores at a
    // 48 / 24-byte lane stride (every store instruction touches 24 cache lines); staged, the workgroup writes its 12 + 6 KB as 16-byte
    // stores, lanes along addresses.  Round 2: 14.8 -> see DESIGN.md section 5.
    // (Round 5: the INPUT rows through LDS the same way -- 13 strided load instructions -> 4 contiguous ones + LDS reads, two more barriers --
    // measured 14.0 -> 15.3 us, profiles/r05b_ab_stage.txt: the loads are latency the 4 resident workgroups already overlap; not kept.)
    __shared__ __attribute__((aligned(16))) float s_rec[256 * 12];
    __shared__ __attribute__((aligned(16))) float s_cov[256 * 6];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) window_reset(s_win);
    __syncthreads();

    // wave-uniform camera: scalar loads
    float V[16], Pm[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { V[i] = p.view[i]; Pm[i] = p.proj[i]; }

    int my_radii = 0;
    bool cov_set = false, rec_set = false;
    uint32_t touched = 0;
    TileRect rect = { 0, 0, 0, 0 };
    const bool valid = idx < p.P;
    const int sidx = valid ? idx : 0;
    const float ox = p.means3D[3 * sidx + 0], oy = p.means3D[3 * sidx + 1], oz = p.means3D[3 * sidx + 2];

    // near-plane cull only (auxiliary.h:154)
    const float vz = view_depth(V, ox, oy, oz);
    if (valid && beyond_near_plane(vz)) {
        const float2 hp = homog_xy(Pm, ox, oy, oz);
        const float p_w = homog_inv_w(Pm, ox, oy, oz);
        const float projx = hp.x * p_w, projy = hp.y * p_w;

        float c3[6];
        if (p.cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) c3[k] = p.cov3D_precomp[6 * idx + k];
        } else {
            // computeCov3D, forward.cu:116-152 — quaternion used un-normalised
            const float3 s = modified_scale(p.scale_modifier, p.scales + 3 * idx);
            const float* q = p.rotations + 4 * idx;
            const M3 M = scaled_rotation(s, raw_quat_rotation(q[0], q[1], q[2], q[3]));
            const M3 Sigma = m3_mul(m3_t(M), M);
            c3[0] = Sigma.m[0][0]; c3[1] = Sigma.m[0][1]; c3[2] = Sigma.m[0][2];
            c3[3] = Sigma.m[1][1]; c3[4] = Sigma.m[1][2]; c3[5] = Sigma.m[2][2];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) s_cov[6 * threadIdx.x + k] = c3[k];
        cov_set = true;

        // computeCov2D, forward.cu:74-113
        // The clamp is frustum_clamp of ag_gauss_geom.h, written out: called from there, the negation of J's -(focal t) / tz^2 entries is
        // folded into the clamp instead of into tz and 98 of the unit's 1590 instructions are scheduled differently.
        // Keep the two equal.
        const float3 t = view_point(V, ox, oy, oz);
        float tx = t.x, ty = t.y;
        const float tz = t.z;
        const float limx = 1.3f * p.tan_fovx, limy = 1.3f * p.tan_fovy;
        const float txtz = tx / tz, tytz = ty / tz;
        tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
        ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
        const Cov2D cov = project_cov(V, p.focal, tx, ty, tz, c3);
        const float cxx = cov.xx, cxy = cov.xy, cyy = cov.yy;

        const float det = (cxx * cyy - cxy * cxy);
        if (det != 0.0f) {
            const float det_inv = 1.f / det;
            const float ca = cyy * det_inv, cb = -cxy * det_inv, cc = cxx * det_inv;
            const float mid = 0.5f * (cxx + cyy);
            const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
            const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
            const float px = ndc2pix(projx, p.W), py = ndc2pix(projy, p.H);
            const TileRect tr = tile_rect(px, py, (int)my_radius, p.gx, p.gy);
            const uint32_t n = (tr.x1 - tr.x0) * (tr.y1 - tr.y0);
            if (n != 0) {
                my_radii = (int)my_radius;
                touched = n;
                const float op = p.opacities[idx];
                GaussRec g;
                g.x = px; g.y = py; g.ca = ca; g.cb = cb; g.cc = cc; g.op = op;
                if (p.colors) {
                    g.r = p.colors[3 * idx + 0]; g.g = p.colors[3 * idx + 1]; g.b = p.colors[3 * idx + 2];
                } else {                                    // forward.cu:238-245: after the culls, only for Gaussians that are drawn
                    float rgb[3];
                    uint8_t cl[3];
                    sh_colour(p.sh_degree, sh_direction(ox, oy, oz, p.campos), p.shs + (size_t)idx * p.sh_coeffs * 3, rgb, cl);
                    g.r = rgb[0]; g.g = rgb[1]; g.b = rgb[2];
                    p.clamped[3 * idx + 0] = cl[0]; p.clamped[3 * idx + 1] = cl[1]; p.clamped[3 * idx + 2] = cl[2];
                }
                g.depth = vz;
                // Wave-level cull radius for the blend kernels.  power <= -0.5*d^2/lambda_max(cov2D) and
                // alpha = op*exp(power) < 1/255  <=>  power < -ln(255*op); lambda1 >= lambda_max (0.1 floor above).
                // 1 % + 0.01 slack in log space dwarfs every fp32 rounding of conic/power; huge or degenerate
                // splats are never culled.
                // qcut (round 5): the same threshold on the quadratic form itself, q = a dx^2 + 2 b dx dy + c dy^2 = -2 power: alpha < 1 / 255
                // wherever q > 2 ln(255 op).  The blend backward minimises q over its 4 x 4 pixels' rectangle exactly (ag_blend_backward.hip), which
                // needs a positive definite conic; any other conic is never culled by it.
                float r2 = 3.0e38f, qc = 3.0e38f;
                if (lambda1 < 1.0e4f && lambda1 > 0.f && op >= 0.f) {
                    // op < 1/255 needs no slack: alpha = op * exp(power <= 0) rounds to at most op, below the blend's threshold at every pixel
                    const float lg = (op < 1.0f / 255.0f) ? -1.0f : __logf(255.0f * op) + 0.01f;
                    r2 = (lg > 0.f) ? 2.0f * lambda1 * lg * 1.01f : -1.0f;
                    const bool pd = ca > 0.f && cc > 0.f && (ca * cc - cb * cb) > 0.f;
                    qc = (lg > 0.f) ? (pd ? 2.0f * lg * 1.01f : 3.0e38f) : -1.0f;
                }
                g.r2cut = r2;
                g.qcut = qc;
                *reinterpret_cast<GaussRec*>(s_rec + 12 * threadIdx.x) = g;
                rec_set = true;
                rect = tr;
            }
        }
    }
    if (valid) {
        p.radii[idx] = my_radii;
        p.tiles_touched[idx] = touched;
    }
    // culled Gaussians: their record / covariance is never read (no tile list names them); zeros keep the scratch deterministic
    if (!rec_set) {
#pragma unroll
        for (int k = 0; k < 12; k++) s_rec[12 * threadIdx.x + k] = 0.f;
    }
    if (!cov_set) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_cov[6 * threadIdx.x + k] = 0.f;
    }
    window_accumulate(s_win, touched != 0, rect);
    __syncthreads();
    {
        const int first = blockIdx.x * 256, nv = min(256, p.P - first);          // Gaussians of this workgroup
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4* drec = reinterpret_cast<f4*>(p.rec + first);                           // 48 B * 256 * blockIdx: 16-byte aligned
        const f4* srec = reinterpret_cast<const f4*>(s_rec);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int i = threadIdx.x + 256 * j;
            if (i < nv * 3) drec[i] = srec[i];
        }
        float* dcov = p.cov3Ds + (size_t)first * 6;                                // 24 B * 256 * blockIdx: 16-byte aligned
        const int nf = nv * 6, nf4 = nf >> 2;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int i = threadIdx.x + 256 * j;
            if (i < nf4) reinterpret_cast<f4*>(dcov)[i] = reinterpret_cast<const f4*>(s_cov)[i];
        }
        if ((int)threadIdx.x < (nf & 3)) dcov[4 * nf4 + threadIdx.x] = s_cov[4 * nf4 + threadIdx.x];
    }
    const int wx0 = s_win[0], wy0 = s_win[1];
    const int bw = s_win[2] - wx0, bh = s_win[3] - wy0;
    if (bw <= 0 || bh <= 0) return;                       // nothing visible in this workgroup (uniform)
    const int nb = bw * bh;
    if (nb <= kWinBins) {
        for (int i = threadIdx.x; i < nb; i += 256) s_hist[i] = 0u;
        __syncthreads();
        for (uint32_t y = rect.y0; y < rect.y1; y++)
            for (uint32_t x = rect.x0; x < rect.x1; x++) atomicAdd(&s_hist[window_bin(wx0, wy0, bw, x, y)], 1u);
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += 256) {
            const uint32_t c = s_hist[i];
            if (c) atomicAdd(&p.tile_count[window_tile(wx0, wy0, bw, p.gx, i)], c);
        }
    } else {
        // spatially incoherent input (e.g. randomly ordered Gaussians): plain per-instance atomics
        for (uint32_t y = rect.y0; y < rect.y1; y++)
            for (uint32_t x = rect.x0; x < rect.x1; x++) atomicAdd(&p.tile_count[y * (uint32_t)p.gx + x], 1u);
    }
}

int launch_preprocess(const AgRasterForwardArgs& a, hipStream_t s)
{
    PreParams p;
    p.P = a.P; p.W = a.W; p.H = a.H;
    const TileGrid tg = tile_grid(a.W, a.H);
    p.gx = tg.gx; p.gy = tg.gy;
    p.tan_fovx = a.tan_fovx; p.tan_fovy = a.tan_fovy;
    p.focal = focal_lengths(a.W, a.H, a.tan_fovx, a.tan_fovy);
    p.scale_modifier = a.scale_modifier;
    p.means3D = a.means3D; p.scales = a.scales; p.rotations = a.rotations; p.opacities = a.opacities;
    p.colors = a.colors_precomp; p.cov3D_precomp = a.cov3D_precomp;
    p.shs = a.shs; p.campos = a.campos; p.sh_degree = a.sh_degree; p.sh_coeffs = a.sh_coeffs;
    p.view = a.viewmatrix; p.proj = a.projmatrix;
    p.radii = a.radii;
    char* gb = aligned_base(a.geom_buffer);
    char* ib = aligned_base(a.image_buffer);
    GeomLayout gl((size_t)a.P);
    ImageLayout il((size_t)a.W, (size_t)a.H);
    p.rec = reinterpret_cast<GaussRec*>(gb + gl.rec);
    p.cov3Ds = reinterpret_cast<float*>(gb + gl.cov3d);
    p.tiles_touched = reinterpret_cast<uint32_t*>(gb + gl.tiles_touched);
    p.clamped = reinterpret_cast<uint8_t*>(gb + gl.clamped);
    p.tile_count = reinterpret_cast<uint32_t*>(ib + il.tile_count);
    if (check_hip(hipMemsetAsync(p.tile_count, 0, (size_t)tg.T() * sizeof(uint32_t), s), "memset tile_count")) return AG_ERR_HIP;
    { ProfScope ps(AG_K_PREPROCESS, s); hipLaunchKernelGGL(preprocess_kernel, dim3((a.P + 255) / 256), dim3(256), 0, s, p); }
    return check_hip(hipGetLastError(), "preprocess_kernel");
}

__global__ void __launch_bounds__(256) mark_visible_kernel(int P, const float* __restrict__ means3D,
                                                          const float* __restrict__ view, uint8_t* __restrict__ present)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const float ox = means3D[3 * idx + 0], oy = means3D[3 * idx + 1], oz = means3D[3 * idx + 2];
    const float vz = view_depth(view, ox, oy, oz);
    present[idx] = (vz <= kNearPlane) ? 0 : 1;      // auxiliary.h:154 as written: a NaN depth counts as present
}

int launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s)
{
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
    return check_hip(hipGetLastError(), "mark_visible_kernel");
}

}  // namespace ag
