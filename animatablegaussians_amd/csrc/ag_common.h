// Internal declarations shared by the HIP translation units of libag_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ag_raster.h"

namespace ag {

constexpr int kTileX = AG_TILE_X;
constexpr int kTileY = AG_TILE_Y;
constexpr int kWave = 64;  // CDNA4 wavefront

// Per-Gaussian record produced by the forward preprocess and consumed (gathered through the sorted tile lists) by
// the blend kernels: three 16-byte loads per instance instead of four separate gathers.
struct __attribute__((aligned(16))) GaussRec {
    float x, y;        // pixel-space mean (forward.cu:232 point_image)
    float ca, cb;      // conic a, b
    float cc, op;      // conic c, opacity
    float r, g;        // colour
    float b, depth;    // colour, view-space depth
    float r2cut;       // conservative squared pixel distance beyond which alpha < 1/255 (wave-level cull)
    float qcut;        // the same bound on q = a dx^2 + 2 b dx dy + c dy^2 = -2 power itself: 2 ln(255 op) with the same slack (exact cull of the blend backward)
};
static_assert(sizeof(GaussRec) == 48, "GaussRec must be 48 bytes");

// Per-Gaussian accumulator row of the blend backward: one 64-byte line.  With q = G * dL/dalpha of a (pixel, entry) pair and
// (dx, dy) = mean2D - pixel, the blend backward sums the six MOMENTS q, q dx, q dy, q dx^2, q dx dy, q dy^2 over the pixels; every
// geometric gradient of backward.cu:560-600 is a per-Gaussian linear map of those (opacity, conic and the viewport scale are constants
// of the Gaussian), applied once per Gaussian by the preprocess backward (accum_to_gradients) instead of once per (pixel, entry):
//   dL/dopacity = Q;  dL/dconic = -0.5 op (QXX, QXY, QYY);  dL/dmean2D = -0.5 op (W (ca QDX + cb QDY), H (cc QDY + cb QDX))
constexpr int kAccumFloats = 16;
enum AccumSlot { A_QDX = 0, A_QDY, A_QXX, A_QXY, A_QYY, A_Q, A_COLR, A_COLG, A_COLB, A_DEPTH };

// Blend kernels: a workgroup of 8 waves owns an 8x4 pixel region (8 regions per 16x16 tile); each wave blends
// 4 pixels (one per 16-lane DPP row) x 16 list entries per step.
constexpr int kRegW = 8, kRegH = 4, kRegionsPerTile = (kTileX / kRegW) * (kTileY / kRegH);
constexpr int kBlendThreads = 512;
constexpr int kChunk = 512;   // tile-list entries culled cooperatively per pass (one per thread)
constexpr int kQueues = 8;    // XCDs: the static work assignment keeps all regions of a tile on one of them

// Work distribution of the persistent blend kernels: STATIC.  (A global work queue was measured first: returning
// atomics on a few hot words sustain only ~5-10 pops/us on this part, 100+ us per frame for ~5000 items.)
// Tiles are ranked longest-list-first by tile_scan_kernel.  Workgroup b sits on XCD b % 8 (observed dispatcher
// placement, used for speed only) and is the (b / 8)-th workgroup of that XCD.  XCD x owns tile ranks x, x+8, x+16, ...
// and ALL regions of those tiles, so the workgroups that gather one tile's list share an L2; inside the XCD the
// (tile, region) items are dealt round-robin, which with the longest-first order is the usual LPT balance.
//
// Balance: the cost of an item depends on how many of the tile's entries survive the region's cull and on where its pixels
// saturate, which no length-based order predicts -- with exactly as many workgroups as resident slots (512 in the backward)
// their end times spread over 82-154 us of a 154-us kernel (busy fraction 0.63-0.76, profiles/bwd_wg_times.py).  A software
// queue costs more than it gains (32 counters, tickets drawn two items ahead: backward 166 -> 146 us but forward 67 -> 75 us
// and the whole step 10 % SLOWER: device-scope returning atomics take microseconds under the flush traffic).  The hardware
// dispatcher does it for free: with kBlendGrid = 2048 workgroups each takes 2-3 items by the same static rule and late
// workgroups start on whichever CU frees a slot first: forward 67 -> 59 us, backward 166 -> 152 us, step +14-20 %.
// (Rounds 1-2: 4096-8192 workgroups gave the same kernel times and two concurrent streams then starved each other.  Round 3, with the
// backward on 16384 single-wave workgroups and the leaner forward: 2048 / 4096 / 6144 / 8192 / 16384 workgroups = 50.2 / 47.1 / 46.1 /
// 46.3 / 48.4 us forward, 7423 / 7501 / 7534 / 7475 / 7375 views/s with three views in flight, 1793 -> 1844 views/s at 2048^2 --
// profiles/ab_kernels.sh.  One item per workgroup up to 768 active tiles.)
#ifndef AG_BLEND_GRID
#define AG_BLEND_GRID 6144
#endif
constexpr int kBlendGrid = AG_BLEND_GRID;

// ITEMS_PER_TILE: the forward's 8 regions (kRegionsPerTile), the backward's 16 single-wave blocks
template <int ITEMS_PER_TILE>
struct ItemIter {
    uint32_t i, stride, x, n_active;
    __device__ __forceinline__ ItemIter(uint32_t block, uint32_t grid, uint32_t n_active_)
        : i(block / kQueues), stride((grid + kQueues - 1 - (block % kQueues)) / kQueues), x(block % kQueues), n_active(n_active_) {}
    // next (tile rank, item of the tile) of this workgroup; false when exhausted
    __device__ __forceinline__ bool next(uint32_t& tile_rank, uint32_t& item)
    {
        tile_rank = (i / ITEMS_PER_TILE) * kQueues + x;      // all items of a tile on one XCD (they gather the same list)
        item = i % ITEMS_PER_TILE;
        i += stride;
        return tile_rank < n_active;
    }
};

// DPP row shifts of the blend kernels (a row = 16 lanes)
#define AG_DPP_ROW_SHR(n) (0x110 + (n))

template <int N>
__device__ __forceinline__ float row_shr(float v, float fill)
{
    // lane l of each 16-lane row receives lane l-N of the same row; the first N lanes receive `fill`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), AG_DPP_ROW_SHR(N), 0xf, 0xf, false));
}

__device__ __forceinline__ float row_read(float v, int lane, int k)   // value of lane k of this lane's 16-lane row
{
    return __shfl(v, (lane & 48) + k, 64);
}

// Sum over the 64 lanes of a wavefront by xor-shuffle (32, 16, .. 1); every lane ends with the result.  (The matching maximum stays
// written out where it is used, in ag_conv.hip and ag_styleunet_ops.hip: profiles/smplx_chain_ab.txt.)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope release fence, which on
// gfx950 makes every wave wait for the acknowledgement of its outstanding global stores/atomics (vmcnt(0)) -- and, because
// vmcnt retires in order, for any prefetch issued before them.  The blend kernels exchange data between waves through
// LDS only (global memory is written with fire-and-forget stores/atomics), so they use this instead.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

inline __host__ __device__ size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct GeomLayout {
    size_t rec, cov3d, tiles_touched, clamped, total;
    __host__ __device__ explicit GeomLayout(size_t P)
    {
        size_t o = 0;
        rec = o;            o = align_up(o + P * sizeof(GaussRec), 256);
        cov3d = o;          o = align_up(o + P * 6 * sizeof(float), 256);
        tiles_touched = o;  o = align_up(o + P * sizeof(uint32_t), 256);
        clamped = o;        o = align_up(o + P * 3, 256);
        total = o + 256;
    }
};

struct ImageLayout {
    size_t ranges, tile_count, cursor, n_contrib, num_rendered, tile_order, total;
    __host__ __device__ ImageLayout(size_t W, size_t H)
    {
        const size_t T = ((W + kTileX - 1) / kTileX) * ((H + kTileY - 1) / kTileY);
        size_t o = 0;
        ranges = o;        o = align_up(o + T * 2 * sizeof(uint32_t), 256);
        tile_count = o;    o = align_up(o + T * sizeof(uint32_t), 256);
        cursor = o;        o = align_up(o + T * sizeof(uint32_t), 256);
        n_contrib = o;     o = align_up(o + W * H * sizeof(uint32_t), 256);
        num_rendered = o;  o = align_up(o + 16, 256);
        tile_order = o;    o = align_up(o + T * 4 * sizeof(uint32_t), 256);   // uint4 {tile, begin, end, 0}, longest list first
        total = o + 256;
    }
};

struct BinLayout {
    size_t keys, point_list, total;
    __host__ __device__ explicit BinLayout(size_t R)
    {
        size_t o = 0;
        keys = o;        o = align_up(o + R * sizeof(uint64_t), 256);
        point_list = o;  o = align_up(o + R * sizeof(uint32_t), 256);
        total = o + 256;
    }
};

// Scratch base pointers may be arbitrarily aligned (torch uint8 tensors are 512-B aligned in practice, but the ABI
// does not require it): all sub-arrays are addressed from the base rounded up to 256 B.
inline __host__ __device__ char* aligned_base(const void* p)
{
    return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 255) & ~uintptr_t(255));
}

void set_error(const char* fmt, ...);

// Optional event bracketing of kernel launches (ag_prof_* in the ABI).  Usage: { ProfScope ps(AG_K_X, stream); launch; }
// `work` = what the launch computes in the kernel's roofline unit (FLOPs for the convolutions), summed by ag_prof_collect.
int prof_begin(int kernel_id, hipStream_t s, double work, const char* tag = nullptr);
void prof_end(int handle, hipStream_t s);
struct ProfScope {
    int handle; hipStream_t s;
    ProfScope(int id, hipStream_t s_, double work = 0.0, const char* tag = nullptr) : handle(prof_begin(id, s_, work, tag)), s(s_) {}
    ~ProfScope() { prof_end(handle, s); }
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};
int check_hip(hipError_t e, const char* what);

// launchers (one per translation unit)
int launch_preprocess(const AgRasterForwardArgs& a, hipStream_t s);
int launch_tile_scan(const AgRasterForwardArgs& a, hipStream_t s, uint32_t capacity = 0xffffffffu, bool skip_large = false);
int launch_bin_sort(const AgRasterForwardArgs& a, int R, hipStream_t s, bool skip_large = false);
int launch_blend_forward(const AgRasterForwardArgs& a, int R, hipStream_t s);
int launch_blend_backward(const AgRasterBackwardArgs& a, hipStream_t s);
int launch_preprocess_backward(const AgRasterBackwardArgs& a, hipStream_t s);
int launch_debug_atomic_rate(float* accum, int lines, int blocks, int iters, int comps, hipStream_t s);
int launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s);

}  // namespace ag
