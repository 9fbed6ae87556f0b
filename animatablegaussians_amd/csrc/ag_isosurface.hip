// Iso-surface extraction (include/ag_isosurface.h): marching cubes with a generated, face-consistent case table.
//
// Shape.  Two halves around the caller's one read of (V, F):
//   count:  classify_kernel   one thread per node as the low node of a cell: 8 corner loads (a wave covers a run of 64 nodes along k, so
//                             each of the eight loads is one 256-byte segment), the stored case byte and the cell's triangle count;
//           edge_kernel       one thread per node: its three grid edges carry a vertex iff they straddle and one of the (at most four)
//                             cells around them is active -- read from the case bytes, never recomputed;
//           exclusive scans   of the 3 N edge flags and the N triangle counts, in place: reduce blocks of kScanItems, scan the block
//                             sums (the same routine, recursively: three levels reach 2^30 items), add back.  Plain kernels in stream
//                             order; no workgroup waits on another.
//   emit:   vertex_kernel     one thread per node writes the vertices of its flagged edges at their scanned index;
//           face_kernel       one thread per cell writes its <= 5 triangles, looking vertex indices up in the scanned edge array.
// Integer sums only decide where things go, so the order of additions cannot change a bit of the result.
//
// The stored case byte of a cell is its case when the cell is processed and 0 otherwise; a cell is ACTIVE iff that byte is neither 0 nor
// 255, i.e. processed and crossed.  An edge that straddles has a processed cell around it iff it has an active one (a processed cell
// that contains a straddling edge is crossed), so one byte per cell serves both kernels.
//
// What one thread does is a host-callable function, so profiles/ub/isosurface_host_walk.hip runs every thread on the CPU under the host
// sanitizers.  Compiled WITHOUT fp contraction (build.sh EXACT): the header states rounded fp32 operations.
#include "ag_common.h"
#include "../../include/ag_isosurface.h"

#ifdef AG_ISOSURFACE_HOST_ONLY
#define AG_ISO_TABLE_QUALIFIER static const
#else
#define AG_ISO_TABLE_QUALIFIER __constant__ const
#endif
#include "ag_isosurface_table.h"

#define AG_ISO_FN __host__ __device__ __forceinline__

namespace ag {
namespace iso {

constexpr int kThreads = 256;
constexpr int kScanPerThread = 4;
constexpr int kScanItems = kThreads * kScanPerThread;       // items per scan block
constexpr int kMaxLevels = 4;                               // 1024^3 >= 2^30 items below the top block; 3 N + 1 <= 2^31

struct Grid {
    int X, Y, Z;
    long long N;            // nodes
    float iso;
    float spacing[3], origin[3];
};

// Workspace: every sub-array from the base rounded up to 256 bytes (ag_common.h aligned_base).
//   cases  [N] bytes; escan [3 N + 1] and tscan [N + 1] words (flags / counts, then their exclusive scans, the last word the total);
//   esums / tsums: the block sums of each scan level, level l + 1 holding one word per block of level l;
//   counts: V, F and the X, Y, Z they were counted for (what ag_isosurface_emit checks before it launches anything).
struct Layout {
    size_t cases, escan, tscan, esums[kMaxLevels], tsums[kMaxLevels], counts, total;
    long long elen[kMaxLevels + 1], tlen[kMaxLevels + 1];   // items per level; level 0 is the array itself
    int elevels, tlevels;                                   // levels that have more than one block
    __host__ explicit Layout(long long N)
    {
        size_t o = 0;
        cases = o;  o = align_up(o + (size_t)N, 256);
        escan = o;  o = align_up(o + (size_t)(3 * N + 1) * 4, 256);
        tscan = o;  o = align_up(o + (size_t)(N + 1) * 4, 256);
        elevels = levels(3 * N + 1, elen, esums, o);
        tlevels = levels(N + 1, tlen, tsums, o);
        counts = o; o = align_up(o + 5 * 4, 256);
        total = o + 256;
    }
    static int levels(long long items, long long* len, size_t* off, size_t& o)
    {
        int l = 0;
        len[0] = items;
        while (len[l] > kScanItems) {
            len[l + 1] = (len[l] + kScanItems - 1) / kScanItems;
            off[l] = o;
            o = align_up(o + (size_t)len[l + 1] * 4, 256);
            ++l;
        }
        return l;
    }
};

AG_ISO_FN bool finite_f(float v) { return fabsf(v) <= 3.4028234664e38f; }       // false for NaN and the infinities

// classify_kernel, thread n: the stored case byte of the cell whose low node is n (0: no such cell, or not processed) and its triangles
AG_ISO_FN void classify_node(const Grid& g, const float* __restrict__ vol, const uint8_t* __restrict__ mask, long long n, uint8_t* cases, uint32_t* tscan)
{
    const int k = (int)(n % g.Z);
    const long long ij = n / g.Z;
    const int j = (int)(ij % g.Y), i = (int)(ij / g.Y);
    unsigned c = 0;
    if (i + 1 < g.X && j + 1 < g.Y && k + 1 < g.Z) {
        bool ok = true;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const long long m = n + ((corner & 1) ? (long long)g.Y * g.Z : 0) + ((corner & 2) ? g.Z : 0) + ((corner & 4) ? 1 : 0);
            const float v = vol[m];
            ok = ok && finite_f(v) && (!mask || mask[m] != 0);
            c |= (v >= g.iso ? 1u : 0u) << corner;
        }
        if (!ok) c = 0;
    }
    cases[n] = (uint8_t)c;
    tscan[n] = kIsoTriCount[c];
}

AG_ISO_FN bool active_cell(const Grid& g, const uint8_t* __restrict__ cases, int i, int j, int k)
{
    if (i < 0 || j < 0 || k < 0 || i + 1 >= g.X || j + 1 >= g.Y || k + 1 >= g.Z) return false;
    const uint8_t c = cases[((long long)i * g.Y + j) * g.Z + k];
    return c != 0 && c != 255;
}

// edge_kernel, thread n: the flags of the three grid edges whose low node is n
AG_ISO_FN void flag_node(const Grid& g, const float* __restrict__ vol, const uint8_t* __restrict__ cases, long long n, uint32_t* escan)
{
    const int k = (int)(n % g.Z);
    const long long ij = n / g.Z;
    const int j = (int)(ij % g.Y), i = (int)(ij / g.Y);
    const bool a_in = vol[n] >= g.iso;
    const int idx[3] = {i, j, k}, ext[3] = {g.X, g.Y, g.Z};
    const long long step[3] = {(long long)g.Y * g.Z, g.Z, 1};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        uint32_t flag = 0;
        if (idx[axis] + 1 < ext[axis] && (vol[n + step[axis]] >= g.iso) != a_in) {
            const int p = axis == 0 ? 1 : 0, q = axis == 2 ? 1 : 2;     // the two other axes, ascending
            bool any = false;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                int c[3] = {i, j, k};
                c[p] -= s & 1;
                c[q] -= s >> 1;
                any = any || active_cell(g, cases, c[0], c[1], c[2]);
            }
            flag = any ? 1u : 0u;
        }
        escan[3 * n + axis] = flag;
    }
}

// vertex_kernel, thread n: the vertices of the flagged edges of node n (escan holds the exclusive scan: flagged iff the next entry is larger)
AG_ISO_FN void emit_node(const Grid& g, const float* __restrict__ vol, const uint32_t* __restrict__ escan, long long n, float* vertices)
{
    const uint32_t s0 = escan[3 * n], s1 = escan[3 * n + 1], s2 = escan[3 * n + 2], s3 = escan[3 * n + 3];
    if (s3 == s0) return;
    const int k = (int)(n % g.Z);
    const long long ij = n / g.Z;
    const int j = (int)(ij % g.Y), i = (int)(ij / g.Y);
    const float a = vol[n];
    const float base[3] = {g.origin[0] + (float)i * g.spacing[0], g.origin[1] + (float)j * g.spacing[1], g.origin[2] + (float)k * g.spacing[2]};
    const float fidx[3] = {(float)i, (float)j, (float)k};
    const uint32_t s[4] = {s0, s1, s2, s3};
    const long long step[3] = {(long long)g.Y * g.Z, g.Z, 1};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (s[axis + 1] == s[axis]) continue;
        const float b = vol[n + step[axis]];
        const float t = (g.iso - a) / (b - a);
        float* out = vertices + 3ll * s[axis];
#pragma unroll
        for (int d = 0; d < 3; ++d) out[d] = d == axis ? g.origin[d] + (fidx[d] + t) * g.spacing[d] : base[d];
    }
}

// face_kernel, thread n: the triangles of the cell whose low node is n
AG_ISO_FN void emit_cell(const Grid& g, const uint8_t* __restrict__ cases, const uint32_t* __restrict__ escan, const uint32_t* __restrict__ tscan, long long n,
                         int32_t* faces)
{
    const unsigned c = cases[n];
    const int nt = kIsoTriCount[c];
    if (nt == 0) return;
    int32_t* out = faces + 3ll * tscan[n];
    const long long step[3] = {(long long)g.Y * g.Z, g.Z, 1};
    for (int e = 0; e < 3 * nt; ++e) {
        const int edge = kIsoTriTable[c][e];
        const int axis = edge >> 2, u = edge & 1, v = (edge >> 1) & 1;
        const int p = axis == 0 ? 1 : 0, q = axis == 2 ? 1 : 2;
        const long long m = n + (u ? step[p] : 0) + (v ? step[q] : 0);
        out[e] = (int32_t)escan[3 * m + axis];
    }
}

#ifndef AG_ISOSURFACE_HOST_ONLY
__global__ void __launch_bounds__(kThreads) classify_kernel(Grid g, const float* __restrict__ vol, const uint8_t* __restrict__ mask, uint8_t* cases, uint32_t* tscan)
{
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) classify_node(g, vol, mask, n, cases, tscan);
    if (n == g.N) tscan[n] = 0;                                 // the scan's extra item: its result is the total
}

__global__ void __launch_bounds__(kThreads) edge_kernel(Grid g, const float* __restrict__ vol, const uint8_t* __restrict__ cases, uint32_t* escan)
{
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) flag_node(g, vol, cases, n, escan);
    if (n == g.N) escan[3 * n] = 0;
}

__global__ void __launch_bounds__(kThreads) vertex_kernel(Grid g, const float* __restrict__ vol, const uint32_t* __restrict__ escan, float* vertices)
{
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) emit_node(g, vol, escan, n, vertices);
}

__global__ void __launch_bounds__(kThreads) face_kernel(Grid g, const uint8_t* __restrict__ cases, const uint32_t* __restrict__ escan, const uint32_t* __restrict__ tscan,
                                                        int32_t* faces)
{
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) emit_cell(g, cases, escan, tscan, n, faces);
}

// the four items of a thread: items past `len` read as 0
__device__ __forceinline__ void load_items(const uint32_t* __restrict__ data, long long len, long long first, uint32_t v[kScanPerThread])
{
    if (first + kScanPerThread <= len) {
        const uint4 q = *reinterpret_cast<const uint4*>(data + first);         // first is a multiple of 4 and the array 256-byte aligned
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int r = 0; r < kScanPerThread; ++r) v[r] = first + r < len ? data[first + r] : 0u;
    }
}

// inclusive sum of `x` over the workgroup's threads in thread order; *total = the whole workgroup's sum.  Wave scan by shuffles, the four
// wave totals through LDS.
__device__ __forceinline__ uint32_t block_inclusive(uint32_t x, uint32_t* s_wave, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return x + before;
}

// sums[b] = the sum of block b's kScanItems items
__global__ void __launch_bounds__(kThreads) scan_reduce_kernel(const uint32_t* __restrict__ data, long long len, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t s_wave[kThreads / 64];
    uint32_t v[kScanPerThread], total;
    load_items(data, len, ((long long)blockIdx.x * kThreads + threadIdx.x) * kScanPerThread, v);
    block_inclusive((v[0] + v[1]) + (v[2] + v[3]), s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data <- its exclusive scan within each block, plus offsets[b] (the scanned block sums) when given
__global__ void __launch_bounds__(kThreads) scan_block_kernel(uint32_t* data, long long len, const uint32_t* __restrict__ offsets)
{
    __shared__ uint32_t s_wave[kThreads / 64];
    const long long first = ((long long)blockIdx.x * kThreads + threadIdx.x) * kScanPerThread;
    uint32_t v[kScanPerThread], total;
    load_items(data, len, first, v);
    const uint32_t mine = (v[0] + v[1]) + (v[2] + v[3]);
    uint32_t run = block_inclusive(mine, s_wave, &total) - mine + (offsets ? offsets[blockIdx.x] : 0u);
#pragma unroll
    for (int r = 0; r < kScanPerThread; ++r) {
        if (first + r < len) data[first + r] = run;
        run += v[r];
    }
}

__global__ void counts_kernel(Grid g, const uint32_t* __restrict__ escan_total, const uint32_t* __restrict__ tscan_total, int32_t* counts_ws, int32_t* counts)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int32_t V = (int32_t)*escan_total, F = (int32_t)*tscan_total;
        counts_ws[0] = V; counts_ws[1] = F; counts_ws[2] = g.X; counts_ws[3] = g.Y; counts_ws[4] = g.Z;
        counts[0] = V; counts[1] = F;
    }
}

// in-place exclusive scan of level 0 (len[0] items at `data`) through the block sums of the levels above it
static int scan_in_place(char* base, uint32_t* data, const long long* len, const size_t* sums, int levels, hipStream_t s)
{
    uint32_t* at[kMaxLevels + 1];
    at[0] = data;
    for (int l = 0; l < levels; ++l) {
        at[l + 1] = reinterpret_cast<uint32_t*>(base + sums[l]);
        hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)len[l + 1]), dim3(kThreads), 0, s, at[l], len[l], at[l + 1]);
    }
    hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(kThreads), 0, s, at[levels], len[levels], (const uint32_t*)nullptr);      // len <= kScanItems
    for (int l = levels - 1; l >= 0; --l)
        hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)len[l + 1]), dim3(kThreads), 0, s, at[l], len[l], at[l + 1]);
    return check_hip(hipGetLastError(), "isosurface scan");
}
#endif  // AG_ISOSURFACE_HOST_ONLY

// every refusal that depends on the sizes alone; fills g.X, g.Y, g.Z, g.N
inline int check_sizes(const char* what, int X, int Y, int Z, Grid& g)
{
    if (X < 2 || Y < 2 || Z < 2) { set_error("%s: every extent must be at least 2, got %d x %d x %d", what, X, Y, Z); return AG_ERR_INVALID_ARGUMENT; }
    const long long N = (long long)X * Y * Z;
    if (3 * N >= (1ll << 31)) { set_error("%s: 3 * %d * %d * %d = %lld vertex keys do not fit int32 (limit 2^31)", what, X, Y, Z, 3 * N); return AG_ERR_INVALID_ARGUMENT; }
    g.X = X; g.Y = Y; g.Z = Z; g.N = N;
    return AG_OK;
}

inline int check_iso(const char* what, float iso, Grid& g)
{
    if (!finite_f(iso)) { set_error("%s: iso = %g is not finite", what, (double)iso); return AG_ERR_INVALID_ARGUMENT; }
    g.iso = iso;
    return AG_OK;
}

inline int check_placement(const char* what, const float* spacing, const float* origin, Grid& g)
{
    if (!spacing || !origin) { set_error("%s: spacing or origin is NULL", what); return AG_ERR_INVALID_ARGUMENT; }
    for (int d = 0; d < 3; ++d) {
        if (!(spacing[d] > 0.f) || !finite_f(spacing[d])) { set_error("%s: spacing[%d] = %g is not finite and positive", what, d, (double)spacing[d]); return AG_ERR_INVALID_ARGUMENT; }
        if (!finite_f(origin[d])) { set_error("%s: origin[%d] = %g is not finite", what, d, (double)origin[d]); return AG_ERR_INVALID_ARGUMENT; }
        g.spacing[d] = spacing[d];
        g.origin[d] = origin[d];
    }
    return AG_OK;
}

}  // namespace iso
}  // namespace ag

#ifndef AG_ISOSURFACE_HOST_ONLY
using namespace ag;
using namespace ag::iso;

extern "C" size_t ag_isosurface_workspace_bytes(int32_t X, int32_t Y, int32_t Z)
{
    if (X < 2 || Y < 2 || Z < 2 || 3ll * X * Y * Z >= (1ll << 31)) return 0;
    return Layout((long long)X * Y * Z).total;
}

extern "C" int ag_isosurface_count(const float* volume, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, float iso, void* workspace,
                                   size_t workspace_bytes, int32_t* counts, void* stream)
{
    Grid g = {};
    if (int rc = check_sizes("isosurface count", X, Y, Z, g)) return rc;
    if (int rc = check_iso("isosurface count", iso, g)) return rc;
    if (!volume || !workspace || !counts) { set_error("null pointer in ag_isosurface_count"); return AG_ERR_INVALID_ARGUMENT; }
    const Layout L(g.N);
    if (workspace_bytes < L.total) { set_error("isosurface count: workspace of %zu bytes, %zu needed", workspace_bytes, L.total); return AG_ERR_SCRATCH_TOO_SMALL; }
    char* base = aligned_base(workspace);
    uint8_t* cases = reinterpret_cast<uint8_t*>(base + L.cases);
    uint32_t* escan = reinterpret_cast<uint32_t*>(base + L.escan);
    uint32_t* tscan = reinterpret_cast<uint32_t*>(base + L.tscan);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((g.N + 1 + kThreads - 1) / kThreads));          // one thread more than nodes: it clears the scans' extra item
    hipLaunchKernelGGL(classify_kernel, grid, dim3(kThreads), 0, s, g, volume, mask, cases, tscan);
    hipLaunchKernelGGL(edge_kernel, grid, dim3(kThreads), 0, s, g, volume, (const uint8_t*)cases, escan);
    if (int rc = check_hip(hipGetLastError(), "isosurface classify")) return rc;
    if (int rc = scan_in_place(base, escan, L.elen, L.esums, L.elevels, s)) return rc;
    if (int rc = scan_in_place(base, tscan, L.tlen, L.tsums, L.tlevels, s)) return rc;
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, s, g, (const uint32_t*)(escan + 3 * g.N), (const uint32_t*)(tscan + g.N),
                       reinterpret_cast<int32_t*>(base + L.counts), counts);
    return check_hip(hipGetLastError(), "isosurface counts_kernel");
}

extern "C" int ag_isosurface_emit(const float* volume, int32_t X, int32_t Y, int32_t Z, float iso, const float* spacing, const float* origin,
                                  const void* workspace, size_t workspace_bytes, float* vertices, int32_t V, int32_t* faces, int32_t F, void* stream)
{
    Grid g = {};
    if (int rc = check_sizes("isosurface emit", X, Y, Z, g)) return rc;
    if (int rc = check_iso("isosurface emit", iso, g)) return rc;
    if (int rc = check_placement("isosurface emit", spacing, origin, g)) return rc;
    if (V < 0 || F < 0) { set_error("isosurface emit: negative counts V = %d, F = %d", V, F); return AG_ERR_INVALID_ARGUMENT; }
    if (!volume || !workspace || (V > 0 && !vertices) || (F > 0 && !faces)) { set_error("null pointer in ag_isosurface_emit"); return AG_ERR_INVALID_ARGUMENT; }
    const Layout L(g.N);
    if (workspace_bytes < L.total) { set_error("isosurface emit: workspace of %zu bytes, %zu needed", workspace_bytes, L.total); return AG_ERR_SCRATCH_TOO_SMALL; }
    const char* base = aligned_base(workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int32_t have[5] = {-1, -1, -1, -1, -1};
    if (int rc = check_hip(hipMemcpyAsync(have, base + L.counts, sizeof(have), hipMemcpyDeviceToHost, s), "isosurface emit: reading the counts")) return rc;
    if (int rc = check_hip(hipStreamSynchronize(s), "isosurface emit: reading the counts")) return rc;
    if (have[2] != X || have[3] != Y || have[4] != Z) {
        set_error("isosurface emit: the workspace does not hold the counts of a %d x %d x %d volume (run ag_isosurface_count first)", X, Y, Z);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (have[0] != V || have[1] != F) {
        set_error("isosurface emit: V = %d, F = %d given, but ag_isosurface_count left V = %d, F = %d in this workspace", V, F, have[0], have[1]);
        return AG_ERR_INVALID_ARGUMENT;
    }
    const uint8_t* cases = reinterpret_cast<const uint8_t*>(base + L.cases);
    const uint32_t* escan = reinterpret_cast<const uint32_t*>(base + L.escan);
    const uint32_t* tscan = reinterpret_cast<const uint32_t*>(base + L.tscan);
    const dim3 grid((unsigned)((g.N + kThreads - 1) / kThreads));
    if (V > 0) hipLaunchKernelGGL(vertex_kernel, grid, dim3(kThreads), 0, s, g, volume, escan, vertices);
    if (F > 0) hipLaunchKernelGGL(face_kernel, grid, dim3(kThreads), 0, s, g, cases, escan, tscan, faces);
    return check_hip(hipGetLastError(), "isosurface emit");
}
#endif  // AG_ISOSURFACE_HOST_ONLY
