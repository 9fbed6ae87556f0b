// Per-Gaussian geometry of the rasterizer, stated once for ag_preprocess.hip, ag_binning.hip and ag_preprocess_backward.hip (and the tile
// grid for the blend units' launchers).  READ THIS FIRST: the header sets no `fp contract` pragma, its functions take the contraction mode
// of the unit that includes them.  ag_preprocess.hip and ag_binning.hip are built with -ffp-contract=off: every expression below rounds op
// by op in the order written, and that order (GLM column-major mat3 products, left-to-right sums) and every constant are the bit-exact
// contract with oracle/raster_oracle.c -- reorder a sum, hoist a reciprocal or change a literal and radii, tile rects and depth keys change.
// ag_preprocess_backward.hip is built with contraction on: the same text, fused where the compiler chooses; its tests are tolerance tests.
// Two contracts hold because both sides call the same function:
//   count = scatter      tile_rect, window_bin and window_tile give preprocess_kernel's per-tile instance counts and scatter_kernel's key
//                        slots.  The scan sizes the tile segments from the first; a second rect that disagreed would store past them.
//   forward = backward   the backward differentiates the chain it recomputes: view point, J, W, T, Vrk, cov2D + dilation, raw-quaternion
//                        rotation and M = S R (the frustum clamp too, which the forward has to write out: see there).
// Not in ag_common.h because that one enters every unit of the library and the rule above concerns these.
#pragma once

#include "ag_common.h"

namespace ag {

// ---- 3x3 matrices -------------------------------------------------------------------------------------------------------------------------
struct M3 { float m[3][3]; };  // m[col][row], GLM convention

__device__ __forceinline__ M3 m3_cols(float a, float b, float c, float d, float e, float f, float g, float h, float i)
{
    M3 r;
    r.m[0][0] = a; r.m[0][1] = b; r.m[0][2] = c;
    r.m[1][0] = d; r.m[1][1] = e; r.m[1][2] = f;
    r.m[2][0] = g; r.m[2][1] = h; r.m[2][2] = i;
    return r;
}

__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b)
{
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int q = 0; q < 3; q++)
            r.m[c][q] = a.m[0][q] * b.m[c][0] + a.m[1][q] * b.m[c][1] + a.m[2][q] * b.m[c][2];
    return r;
}

__device__ __forceinline__ M3 m3_t(const M3& a)
{
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int q = 0; q < 3; q++) r.m[c][q] = a.m[q][c];
    return r;
}

// ---- tile grid and tile rect ----------------------------------------------------------------------------------------------------------------
struct TileGrid { int gx, gy; __host__ __device__ int T() const { return gx * gy; } };
inline __host__ __device__ TileGrid tile_grid(int W, int H) { return TileGrid{ (W + kTileX - 1) / kTileX, (H + kTileY - 1) / kTileY }; }

// tiles [x0, x1) x [y0, y1) a splat of `max_radius` pixels around (px, py) touches (auxiliary.h:46-56); only exact fp32 adds and a division by 16
struct TileRect { uint32_t x0, y0, x1, y1; };
__device__ __forceinline__ TileRect tile_rect(float px, float py, int max_radius, int gx, int gy)
{
    const float r = (float)max_radius;
    int x0 = (int)((px - r) / (float)kTileX);
    int y0 = (int)((py - r) / (float)kTileY);
    int x1 = (int)((px + r + (float)kTileX - 1.0f) / (float)kTileX);
    int y1 = (int)((py + r + (float)kTileY - 1.0f) / (float)kTileY);
    x0 = max(0, x0); y0 = max(0, y0); x1 = max(0, x1); y1 = max(0, y1);
    return TileRect{ (uint32_t)min(gx, x0), (uint32_t)min(gy, y0), (uint32_t)min(gx, x1), (uint32_t)min(gy, y1) };
}

// ---- workgroup tile window ------------------------------------------------------------------------------------------------------------------
// The 256 Gaussians of a workgroup are neighbours on the canonical map, so their tile rects fall into a small window of the tile grid.
// Both kernels histogram their instances over that window in LDS: s_win[4] = min x, min y, max x, max y (tile units, max exclusive).
constexpr int kWinBins = 2048;   // histogram bins per workgroup (8 KiB of LDS per array)

// one thread, before the barrier that precedes window_accumulate
__device__ __forceinline__ void window_reset(int* s_win) { s_win[0] = 0x7fffffff; s_win[1] = 0x7fffffff; s_win[2] = 0; s_win[3] = 0; }

// One LDS atomic per wave and bound after a wave reduction: 256 threads hammering the same four LDS words directly serialise lane
// by lane (1024 same-address atomics per workgroup).  Call from ALL lanes; lanes without a rect pass has = false.
__device__ __forceinline__ void window_accumulate(int* s_win, bool has, const TileRect& t)
{
    int a = has ? (int)t.x0 : 0x7fffffff, b = has ? (int)t.y0 : 0x7fffffff, c = has ? (int)t.x1 : 0, d = has ? (int)t.y1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a = min(a, __shfl_xor(a, o, 64));
        b = min(b, __shfl_xor(b, o, 64));
        c = max(c, __shfl_xor(c, o, 64));
        d = max(d, __shfl_xor(d, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && c > 0) {
        atomicMin(&s_win[0], a); atomicMin(&s_win[1], b);
        atomicMax(&s_win[2], c); atomicMax(&s_win[3], d);
    }
}

// The window as every thread reads it back after the barrier that follows window_accumulate (uniform over the workgroup): origin
// (wx0, wy0) = s_win[0], s_win[1], extent bw = s_win[2] - wx0, bh = s_win[3] - wy0.  bw <= 0 or bh <= 0: no Gaussian of the workgroup
// touches a tile.  bw * bh > kWinBins: spatially incoherent input, the caller falls back to one global atomic per instance.
// Those four values stay locals of each kernel: held in a struct they change the order in which scatter_kernel's rect is promoted to
// registers, and the unit no longer compiles to the code it had before this header.
// local bin of tile (x, y); global tile index of bin i
__device__ __forceinline__ int window_bin(int wx0, int wy0, int bw, uint32_t x, uint32_t y) { return ((int)y - wy0) * bw + ((int)x - wx0); }
__device__ __forceinline__ uint32_t window_tile(int wx0, int wy0, int bw, int gx, int i)
{
    return (uint32_t)(wy0 + i / bw) * (uint32_t)gx + (uint32_t)(wx0 + i % bw);
}

// ---- projection chain -----------------------------------------------------------------------------------------------------------------------
// V, Pm: the 16 floats of the view / full projection matrix, column-major (element [row r, column c] at 4 c + r).
constexpr float kNearPlane = 0.2f;   // auxiliary.h:154

__device__ __forceinline__ bool beyond_near_plane(float vz) { return vz > kNearPlane; }
__device__ __forceinline__ float view_depth(const float* V, float x, float y, float z) { return V[2] * x + V[6] * y + V[10] * z + V[14]; }
__device__ __forceinline__ float3 view_point(const float* V, float x, float y, float z)
{
    return make_float3(V[0] * x + V[4] * y + V[8] * z + V[12], V[1] * x + V[5] * y + V[9] * z + V[13], view_depth(V, x, y, z));
}

// homogeneous point (forward.cu:196-198, backward.cu:376): x, y before the division, and 1 / (w + 1e-7)
__device__ __forceinline__ float2 homog_xy(const float* Pm, float x, float y, float z)
{
    return make_float2(Pm[0] * x + Pm[4] * y + Pm[8] * z + Pm[12], Pm[1] * x + Pm[5] * y + Pm[9] * z + Pm[13]);
}

__device__ __forceinline__ float homog_inv_w(const float* Pm, float x, float y, float z)
{
    const float hw = Pm[3] * x + Pm[7] * y + Pm[11] * z + Pm[15];
    return 1.0f / (hw + 0.0000001f);
}

struct Focal { float x, y; };   // rasterizer_impl.cu:223-224 and :386-387
inline Focal focal_lengths(int W, int H, float tan_fovx, float tan_fovy) { return Focal{ W / (2.0f * tan_fovx), H / (2.0f * tan_fovy) }; }

// the 1.3 tan_fov guard on the view-space point (forward.cu:84-89, backward.cu:160-176): clamped tx, ty, the unclamped ratios and the limits
struct FrustumClamp { float tx, ty, txtz, tytz, limx, limy; };
__device__ __forceinline__ FrustumClamp frustum_clamp(float3 t, float tan_fovx, float tan_fovy)
{
    FrustumClamp f;
    f.limx = 1.3f * tan_fovx; f.limy = 1.3f * tan_fovy;
    f.txtz = t.x / t.z; f.tytz = t.y / t.z;
    f.tx = fminf(f.limx, fmaxf(-f.limx, f.txtz)) * t.z;
    f.ty = fminf(f.limy, fmaxf(-f.limy, f.tytz)) * t.z;
    return f;
}

// computeCov2D, forward.cu:74-113: T = W J, cov2D = T^T Vrk^T T with 0.3 added to the diagonal; c3 = the 6 floats of the 3D covariance
struct Cov2D { M3 Wm, T, Vrk; float xx, xy, yy; };
__device__ __forceinline__ Cov2D project_cov(const float* V, const Focal& focal, float tx, float ty, float tz, const float* c3)
{
    Cov2D o;
    const M3 J = m3_cols(
        focal.x / tz, 0.0f, -(focal.x * tx) / (tz * tz),
        0.0f, focal.y / tz, -(focal.y * ty) / (tz * tz),
        0.f, 0.f, 0.f);
    o.Wm = m3_cols(V[0], V[4], V[8], V[1], V[5], V[9], V[2], V[6], V[10]);
    o.T = m3_mul(o.Wm, J);
    o.Vrk = m3_cols(c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]);
    const M3 cov = m3_mul(m3_mul(m3_t(o.T), m3_t(o.Vrk)), o.T);
    o.xx = cov.m[0][0] + 0.3f; o.xy = cov.m[0][1]; o.yy = cov.m[1][1] + 0.3f;
    return o;
}

// ---- rotation and scale ---------------------------------------------------------------------------------------------------------------------
// computeCov3D, forward.cu:116-152: the quaternion (r, x, y, z) is used RAW, un-normalised (backward.cu:340 differentiates that);
// s = mod * scale, M = S R.  The forward's covariance is M^T M.
__device__ __forceinline__ M3 raw_quat_rotation(float r, float x, float y, float z)
{
    return m3_cols(
        1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
        2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
        2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y));
}

__device__ __forceinline__ float3 modified_scale(float mod, const float* s) { return make_float3(mod * s[0], mod * s[1], mod * s[2]); }

__device__ __forceinline__ M3 scaled_rotation(float3 s, const M3& R)
{
    M3 S = m3_cols(1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f);
    S.m[0][0] = s.x; S.m[1][1] = s.y; S.m[2][2] = s.z;
    return m3_mul(S, R);
}

}  // namespace ag
