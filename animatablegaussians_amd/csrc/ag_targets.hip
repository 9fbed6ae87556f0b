// Training targets from a decoded frame (include/ag_targets.h): float colour, subject mask, boundary band and the mask's row / column
// profiles, for all views in one launch.  Memory bound: 4 B in and 14 B out per pixel, most of it the 12 B of float colour.
//
// A workgroup of 256 threads does two independent things:
//   1. one 128 x 16 tile of mask and band.  The matte tile and its r-wide halo become one byte of class flags per pixel in LDS
//      (bit 0: class 1, bit 1: class 0, bit 2: class 128, bit 3: the soft band 5 < m < 250; 0 outside the image, so a clipped window
//      needs no special case).  "The window holds a 1 and a 0 and no 128" is an OR of three bits, which is separable: a row pass
//      over the flags (four pixels per thread as one dword, the 2 r + 1 shifted windows taken from five aligned dwords) and a column
//      pass over the row results.  Both results go back to LDS as one byte per pixel and leave from there.
//   2. its share of the colour conversion, which is a flat map over V H W 3 elements and knows nothing about tiles: groups of four
//      elements aligned to 16 B of the OUTPUT, one float4 store per thread and step.
// Every access to a byte plane is an aligned dword wherever all four bytes belong to the thread's run, whatever the plane's base
// address, W and H W are: a thread addresses by aligned ADDRESS and works out which pixels those are (the group then starts up to
// three pixels left of a multiple of four), and takes or shifts the bytes it needs out of aligned LDS / global dwords.  Groups that
// straddle the ends of a run fall back to byte accesses for the bytes that are theirs.  With the planes of a torch allocation and W
// a multiple of four every group is whole.
//
// The phases are host-callable functions of the thread index: a host program can walk them thread by thread over the same arrays
// (they touch nothing but their arguments), which is how the addressing was checked under a host AddressSanitizer
// (profiles/ub/targets_host_walk.hip).
#include "ag_common.h"
#include "../../include/ag_targets.h"

namespace ag {
namespace targets {

constexpr int kTW = 128, kTH = 16;           // output tile
constexpr int kThreads = 256;
constexpr int kMaxR = 7;
constexpr int kOrg = 8;                      // flag columns in front of the tile's first (>= kMaxR, a multiple of 4)
constexpr int kClsStride = 36;               // dwords per flag row: 8 + 128 + 8 bytes
constexpr int kHorStride = kTW / 4;          // dwords per row-pass row
constexpr int kResStride = 35;               // dwords per result row: one in front, 32, two behind (shifted reads)
constexpr int kLoadGroups = kClsStride + 1;  // aligned dwords that cover a flag row at any shift
constexpr int kStoreGroups = kTW / 4 + 1;    // aligned dwords that cover a result row at any shift
constexpr int kClsWords = (kTH + 2 * kMaxR) * kClsStride, kHorWords = (kTH + 2 * kMaxR) * kHorStride, kResWords = kTH * kResStride;
constexpr uint32_t kLow = 0x01010101u;

struct Args {
    const uint8_t* color;
    const uint8_t* matte;
    float* color_f;
    uint8_t* mask;
    uint8_t* boundary;
    uint8_t* row_any;       // both or neither
    uint8_t* col_any;
    int V, H, W;
    long long n_matte;      // V * H * W
    long long n_color;      // V * H * W * 3
    long long groups;       // 16-byte output groups of the colour map
    long long per_block;    // of which each workgroup takes this many
    int color_shift;        // elements in front of color_f[0] up to the 16-byte boundary below it (0 .. 3)
};

__host__ __device__ __forceinline__ uint32_t class_flags(uint32_t m)
{
    return (m > 128u ? 1u : m < 128u ? 2u : 4u) | ((m > 5u && m < 250u) ? 8u : 0u);
}

// bytes sh .. sh + 3 of the eight bytes lo, hi (sh = 0 .. 3)
__host__ __device__ __forceinline__ uint32_t shifted(uint32_t lo, uint32_t hi, int sh)
{
    return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
}

// Phase A: the flags of the tile's rows Y0 - R .. Y0 + kTH + R - 1, columns X0 - kOrg .. X0 + kTW + kOrg - 1.
template <int R>
__host__ __device__ __forceinline__ void load_flags(const Args& a, int tid, int v, int Y0, int X0, uint32_t* cls)
{
    uint8_t* cls8 = reinterpret_cast<uint8_t*>(cls);
    const int xs = X0 - kOrg;
    for (int i = tid; i < (kTH + 2 * R) * kLoadGroups; i += kThreads) {
        const int rr = i / kLoadGroups, j = i - rr * kLoadGroups;
        const int yy = Y0 - R + rr;
        uint32_t f[4] = {0u, 0u, 0u, 0u};
        int sh = 0;
        if (yy >= 0 && yy < a.H) {
            const long long row = ((long long)v * a.H + yy) * a.W;
            sh = (int)((reinterpret_cast<uintptr_t>(a.matte) + (uintptr_t)(row + xs)) & 3u);
            const int x0 = xs - sh + 4 * j;                      // image column of the aligned dword's first byte
            const bool wanted = x0 + 3 >= X0 - R && x0 < X0 + kTW + R && x0 + 3 >= 0 && x0 < a.W;
            if (wanted) {
                const long long d = row + x0;                    // its offset in the matte buffer
                uint32_t w = 0u;
                if (d >= 0 && d + 4 <= a.n_matte) {
                    w = *reinterpret_cast<const uint32_t*>(a.matte + d);
                } else {
                    for (int k = 0; k < 4; ++k)
                        if (x0 + k >= 0 && x0 + k < a.W) w |= (uint32_t)a.matte[d + k] << (8 * k);
                }
                for (int k = 0; k < 4; ++k)
                    if (x0 + k >= 0 && x0 + k < a.W) f[k] = class_flags((w >> (8 * k)) & 255u);
            }
        }
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * j - sh + k;
            if (q >= 0 && q < 4 * kClsStride) cls8[rr * 4 * kClsStride + q] = (uint8_t)f[k];
        }
    }
}

// Phase B: per flag row, the OR of the three class bits over columns x - R .. x + R, four columns per dword.
template <int R>
__host__ __device__ __forceinline__ void row_pass(int tid, const uint32_t* cls, uint32_t* hor)
{
    for (int i = tid; i < (kTH + 2 * R) * kHorStride; i += kThreads) {
        const int rr = i / kHorStride, t = i - rr * kHorStride;
        uint32_t D[5];
#pragma unroll
        for (int n = 0; n < 5; ++n) D[n] = cls[rr * kClsStride + t + n];      // flag columns 4 t .. 4 t + 19; the thread's own are 8 .. 11 of them
        uint32_t acc = 0u;
#pragma unroll
        for (int d = -R; d <= R; ++d) {
            const int s = kOrg + d;
            acc |= shifted(D[s >> 2], D[(s >> 2) + ((s & 3) ? 1 : 0)], s & 3);
        }
        hor[i] = acc & 0x07070707u;
    }
}

// Phase C: tile row oy, columns 4 t .. 4 t + 3 -> one result byte per pixel (bit 0: mask, bit 1: band); returns the mask bits.
template <int R>
__host__ __device__ __forceinline__ uint32_t column_pass(int oy, int t, const uint32_t* cls, const uint32_t* hor, uint32_t* res)
{
    uint32_t acc = 0u;
#pragma unroll
    for (int d = 0; d <= 2 * R; ++d) acc |= hor[(oy + d) * kHorStride + t];
    const uint32_t centre = cls[(oy + R) * kClsStride + kOrg / 4 + t];
    const uint32_t mask = centre & kLow;
    const uint32_t band = ((acc & (acc >> 1) & ~(acc >> 2)) | (centre >> 3)) & kLow;
    res[oy * kResStride + 1 + t] = mask | (band << 1);
    return mask;
}

// Phase D: bit `bit` of the tile's result bytes -> plane `out`, by aligned dwords of the plane.
__host__ __device__ __forceinline__ void store_plane(const Args& a, int tid, int v, int Y0, int X0, const uint32_t* res, uint8_t* out, int bit)
{
    const int X1 = min(a.W, X0 + kTW);
    for (int i = tid; i < kTH * kStoreGroups; i += kThreads) {
        const int oy = i / kStoreGroups, j = i - oy * kStoreGroups;
        const int y = Y0 + oy;
        if (y >= a.H) break;
        const long long o = ((long long)v * a.H + y) * a.W + X0;              // the tile row's first pixel
        const int sh = (int)((reinterpret_cast<uintptr_t>(out) + (uintptr_t)o) & 3u);
        const int x0 = X0 + 4 * j - sh;                                      // image column of the aligned dword's first byte
        if (x0 >= X1) continue;
        const int p = 4 + 4 * j - sh;                                        // the same as a byte index of the result row (1 .. 132)
        const uint32_t w = (shifted(res[oy * kResStride + (p >> 2)], res[oy * kResStride + (p >> 2) + 1], p & 3) >> bit) & kLow;
        uint8_t* dst = out + (o + (x0 - X0));
        if (x0 >= X0 && x0 + 4 <= X1) {
            *reinterpret_cast<uint32_t*>(dst) = w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (x0 + k >= X0 && x0 + k < X1) dst[k] = (uint8_t)((w >> (8 * k)) & 1u);
        }
    }
}

// The workgroup's share of color_f = float(color) / 255: group g holds elements 4 g - shift .. 4 g - shift + 3, 16-byte aligned in the output.
__host__ __device__ __forceinline__ void convert_colour(const Args& a, int tid, long long block)
{
    const long long g_end = min(a.groups, (block + 1) * a.per_block);
    for (long long g = block * a.per_block + tid; g < g_end; g += kThreads) {
        const long long e0 = 4 * g - a.color_shift;
        const uint8_t* src = a.color + e0;
        if (e0 >= 0 && e0 + 4 <= a.n_color) {
            const int sh = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
            uint32_t w;
            if (sh == 0) {
                w = *reinterpret_cast<const uint32_t*>(src);
            } else if (e0 - sh >= 0 && e0 - sh + 8 <= a.n_color) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(src - sh);
                w = shifted(p[0], p[1], sh);
            } else {
                w = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
            }
            float4 o;
            o.x = (float)(w & 255u) / 255.0f;
            o.y = (float)((w >> 8) & 255u) / 255.0f;
            o.z = (float)((w >> 16) & 255u) / 255.0f;
            o.w = (float)(w >> 24) / 255.0f;
            *reinterpret_cast<float4*>(a.color_f + e0) = o;
        } else {
            for (int k = 0; k < 4; ++k)
                if (e0 + k >= 0 && e0 + k < a.n_color) a.color_f[e0 + k] = (float)src[k] / 255.0f;
        }
    }
}

#ifndef AG_TARGETS_HOST_ONLY
template <int R>
__global__ void __launch_bounds__(kThreads) prepare_targets_kernel(Args a)
{
    __shared__ uint32_t cls[kClsWords];
    __shared__ uint32_t hor[kHorWords];
    __shared__ uint32_t res[kResWords];
    __shared__ uint32_t col[kTW / 4];
    const int tid = threadIdx.x;
    const int v = blockIdx.z, Y0 = blockIdx.y * kTH, X0 = blockIdx.x * kTW;
    const long long block = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;

    convert_colour(a, tid, block);

    if (tid < kTW / 4) col[tid] = 0u;
    load_flags<R>(a, tid, v, Y0, X0, cls);
    __syncthreads();
    row_pass<R>(tid, cls, hor);
    __syncthreads();
    const int t = tid & (kHorStride - 1), ty = tid / kHorStride;
    uint32_t in_column = 0u;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int oy = ty + half * (kThreads / kHorStride);
        const uint32_t m = column_pass<R>(oy, t, cls, hor, res);          // 0 outside the image, as its flags are
        in_column |= m;
        const unsigned long long rows = __ballot(m != 0u);                // a wave holds two tile rows: lanes 0-31 and lanes 32-63
        const int lane = tid & 63;
        if (a.row_any && (lane & 31) == 0 && ((rows >> lane) & 0xffffffffull)) a.row_any[(long long)v * a.H + Y0 + oy] = 1;
    }
    if (a.col_any && in_column) atomicOr(&col[t], in_column);
    __syncthreads();
    if (a.col_any && tid < kTW / 4) {
        const uint32_t w = col[tid];
        for (int k = 0; k < 4; ++k)
            if ((w >> (8 * k)) & 1u) a.col_any[(long long)v * a.W + X0 + 4 * tid + k] = 1;
    }
    store_plane(a, tid, v, Y0, X0, res, a.mask, 0);
    store_plane(a, tid, v, Y0, X0, res, a.boundary, 1);
}

template <int R>
static void launch(const Args& a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL(prepare_targets_kernel<R>, grid, dim3(kThreads), 0, s, a);
}
#endif

}  // namespace targets
}  // namespace ag

#ifndef AG_TARGETS_HOST_ONLY
using namespace ag;

extern "C" int ag_prepare_targets(const uint8_t* color_u8, const uint8_t* matte_u8, int32_t V, int32_t H, int32_t W, int32_t kernel_size,
                                  float* color_f32, uint8_t* mask_u8, uint8_t* boundary_u8, uint8_t* row_any_u8, uint8_t* col_any_u8, void* stream)
{
    using namespace ag::targets;
    if (!matte_u8 || !mask_u8 || !boundary_u8) { set_error("null pointer in ag_prepare_targets"); return AG_ERR_INVALID_ARGUMENT; }
    if ((color_u8 == nullptr) != (color_f32 == nullptr)) { set_error("prepare targets: color_u8 and color_f32 go together (both or neither)"); return AG_ERR_INVALID_ARGUMENT; }
    if (V <= 0 || H <= 0 || W <= 0) { set_error("prepare targets: bad sizes V = %d, H = %d, W = %d", V, H, W); return AG_ERR_INVALID_ARGUMENT; }
    if (kernel_size < 1 || kernel_size > 2 * kMaxR + 1 || kernel_size % 2 == 0) {
        set_error("prepare targets: kernel_size must be odd and in 1..%d, got %d", 2 * kMaxR + 1, kernel_size);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if ((row_any_u8 == nullptr) != (col_any_u8 == nullptr)) { set_error("prepare targets: row_any_u8 and col_any_u8 go together (both or neither)"); return AG_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<uintptr_t>(color_f32) & 3u) { set_error("prepare targets: color_f32 is not aligned to 4 bytes"); return AG_ERR_INVALID_ARGUMENT; }
    const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), (unsigned)V);
    if (grid.y > 65535u || grid.z > 65535u) { set_error("prepare targets: V = %d or H = %d exceeds one launch", V, H); return AG_ERR_INVALID_ARGUMENT; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Args a;
    a.color = color_u8; a.matte = matte_u8; a.color_f = color_f32; a.mask = mask_u8; a.boundary = boundary_u8;
    a.row_any = row_any_u8; a.col_any = col_any_u8;
    a.V = V; a.H = H; a.W = W;
    a.n_matte = (long long)V * H * W;
    a.n_color = color_u8 ? a.n_matte * 3 : 0;       // no colour: no groups, convert_colour does nothing
    a.color_shift = (int)((reinterpret_cast<uintptr_t>(color_f32) >> 2) & 3u);
    a.groups = (a.n_color + a.color_shift + 3) / 4;
    const long long blocks = (long long)grid.x * grid.y * grid.z;
    a.per_block = (a.groups + blocks - 1) / blocks;
    if (row_any_u8) {
        int rc = check_hip(hipMemsetAsync(row_any_u8, 0, (size_t)V * H, s), "clear row_any_u8");
        if (rc == AG_OK) rc = check_hip(hipMemsetAsync(col_any_u8, 0, (size_t)V * W, s), "clear col_any_u8");
        if (rc != AG_OK) return rc;
    }
    switch (kernel_size / 2) {
        case 0: launch<0>(a, grid, s); break;
        case 1: launch<1>(a, grid, s); break;
        case 2: launch<2>(a, grid, s); break;
        case 3: launch<3>(a, grid, s); break;
        case 4: launch<4>(a, grid, s); break;
        case 5: launch<5>(a, grid, s); break;
        case 6: launch<6>(a, grid, s); break;
        default: launch<7>(a, grid, s); break;
    }
    return check_hip(hipGetLastError(), "prepare_targets_kernel");
}
#endif
