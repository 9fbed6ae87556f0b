// Per-subject assets from a triangle mesh (include/ag_subject_maps.h): orthographic vertex-attribute rasterizer, attribute resolve,
// exact grid k-NN.  Init-time kernels over <= 21 k faces, 2 M pixels and 268 k points: nothing here is MFMA work.
//
// Compiled WITHOUT fp contraction (build.sh EXACT).  The edge functions, the barycentrics, the depth and the squared distances are
// stated in the header as sequences of individually rounded fp32 operations; with contraction the compiler may fuse a product into
// the following sum at one call site and not at another, and then (a) the two faces sharing an edge no longer see opposite edge
// values at a pixel centre, (b) the second rasterizer pass no longer reproduces the first pass's depth, and (c) the test oracle's
// float32 restatement (numpy has no FMA) stops predicting the kernel's bits.  These kernels are latency / memory bound; the fused
// forms would buy nothing measurable.
//
// Determinism (requirement (a) of the rasterizer): a 64-bit atomic-min z-buffer rather than per-tile face lists.  The minimum of
// (depth bits << 32 | face) commutes, so the winner is independent of arrival order without any sort; the z-buffer costs 8 B per
// pixel (8 MB per 1024^2 view) and one pass over it, where tile binning would need a face-tile count, a scan, a keyed sort and a
// list walk for a mesh whose faces cover ~16 pixels each -- more launches and more code than the work they organise.
#include "ag_common.h"
#include "../../include/ag_subject_maps.h"

namespace ag {
namespace {

struct Edge {
    float ax, ay, dx, dy;   // canonical start point and direction (end - start), start <= end lexicographically in (x, y)
    float sgn;              // -1 when the face walks the edge from the canonical end to the canonical start
    int tl;                 // the edge owns samples that lie exactly on it (top-left rule, window space with y up, CCW faces)
};

__device__ __forceinline__ Edge make_edge(float x0, float y0, float x1, float y1)   // as the face walks it: (x0, y0) -> (x1, y1)
{
    Edge e;
    e.tl = (y1 < y0) || (y1 == y0 && x1 < x0);          // left edge: walked downwards; top edge: horizontal, walked towards -x
    const bool swap = (x1 < x0) || (x1 == x0 && y1 < y0);
    const float ax = swap ? x1 : x0, ay = swap ? y1 : y0, bx = swap ? x0 : x1, by = swap ? y0 : y1;
    e.ax = ax; e.ay = ay; e.dx = bx - ax; e.dy = by - ay; e.sgn = swap ? -1.f : 1.f;
    return e;
}

__device__ __forceinline__ float edge_value(const Edge& e, float px, float py)
{
    return e.sgn * (e.dx * (py - e.ay) - e.dy * (px - e.ax));
}

struct FaceSetup {
    Edge e12, e20, e01;
    float d0, d1, d2;
    float minx, maxx, miny, maxy;
    int swapped;            // corners 1 and 2 exchanged (clockwise face, culling off)
};

__device__ __forceinline__ void to_window(const AgMeshRasterArgs& a, int v, float& wx, float& wy, float& d)
{
    const float x = a.vertices[3 * v], y = a.vertices[3 * v + 1], z = a.vertices[3 * v + 2];
    const float* m = a.view;
    const float n0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float n1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    d = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    wx = (n0 + 1.f) * (0.5f * (float)a.W);
    wy = (n1 + 1.f) * (0.5f * (float)a.H);
}

__device__ __forceinline__ bool setup_face(const AgMeshRasterArgs& a, int f, FaceSetup& s)
{
    const int i0 = a.faces[3 * f], i1 = a.faces[3 * f + 1], i2 = a.faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) return false;
    float x0, y0, x1, y1, x2, y2, d1, d2;
    to_window(a, i0, x0, y0, s.d0);
    to_window(a, i1, x1, y1, d1);
    to_window(a, i2, x2, y2, d2);
    s.e01 = make_edge(x0, y0, x1, y1);
    const float area = edge_value(s.e01, x2, y2);
    if (!(area > 0.f || area < 0.f)) return false;     // degenerate (or NaN)
    s.swapped = 0;
    if (area < 0.f) {
        if (a.cull) return false;
        float t;
        t = x1; x1 = x2; x2 = t;
        t = y1; y1 = y2; y2 = t;
        t = d1; d1 = d2; d2 = t;
        s.swapped = 1;
        s.e01 = make_edge(x0, y0, x1, y1);
    }
    s.e12 = make_edge(x1, y1, x2, y2);
    s.e20 = make_edge(x2, y2, x0, y0);
    s.d1 = d1; s.d2 = d2;
    s.minx = fminf(x0, fminf(x1, x2)); s.maxx = fmaxf(x0, fmaxf(x1, x2));
    s.miny = fminf(y0, fminf(y1, y2)); s.maxy = fmaxf(y0, fmaxf(y1, y2));
    return true;
}

// coverage, barycentrics (in the walked corner order) and depth of the sample (px, py)
__device__ __forceinline__ bool sample_face(const FaceSetup& s, float px, float py, float& b0, float& b1, float& b2, float& depth)
{
    const float w0 = edge_value(s.e12, px, py), w1 = edge_value(s.e20, px, py), w2 = edge_value(s.e01, px, py);
    const bool in = (w0 > 0.f || (w0 == 0.f && s.e12.tl)) && (w1 > 0.f || (w1 == 0.f && s.e20.tl)) && (w2 > 0.f || (w2 == 0.f && s.e01.tl));
    if (!in) return false;
    const float A = (w0 + w1) + w2;
    if (!(A > 0.f)) return false;
    b0 = w0 / A;
    b1 = w1 / A;
    b2 = (1.f - b0) - b1;
    depth = ((b0 * s.d0 + b1 * s.d1) + b2 * s.d2) + 0.f;     // + 0: -0 and +0 are one depth
    return depth == depth;
}

__device__ __forceinline__ uint32_t depth_key(float d)         // unsigned order == float order
{
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One wavefront per face; its lanes stride over the pixel centres of the face's bounding box.
__global__ void __launch_bounds__(256) mesh_depth_kernel(AgMeshRasterArgs a, unsigned long long* zbuf)
{
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= a.F) return;
    FaceSetup s;
    if (!setup_face(a, f, s)) return;
    // centres gx + 0.5 inside [minx, maxx]; the float clamps come first so that the conversions are defined for any input
    const int gx0 = (int)ceilf(fminf(fmaxf(s.minx - 0.5f, 0.f), (float)a.W)), gx1 = (int)floorf(fminf(fmaxf(s.maxx - 0.5f, -1.f), (float)(a.W - 1)));
    const int gy0 = (int)ceilf(fminf(fmaxf(s.miny - 0.5f, 0.f), (float)a.H)), gy1 = (int)floorf(fminf(fmaxf(s.maxy - 0.5f, -1.f), (float)(a.H - 1)));
    if (gx1 < gx0 || gy1 < gy0) return;
    const int bw = gx1 - gx0 + 1, n = bw * (gy1 - gy0 + 1);          // <= W * H <= 2^28
    for (int i = lane; i < n; i += 64) {
        const int gy = gy0 + i / bw, gx = gx0 + i % bw;              // 0 <= gx < W, 0 <= gy < H by the clamps above
        float b0, b1, b2, d;
        if (!sample_face(s, (float)gx + 0.5f, (float)gy + 0.5f, b0, b1, b2, d)) continue;
        atomicMin(&zbuf[(size_t)gy * a.W + gx], ((unsigned long long)depth_key(d) << 32) | (uint32_t)f);
    }
}

__global__ void __launch_bounds__(256) mesh_resolve_ids_kernel(AgMeshRasterArgs a, const unsigned long long* zbuf)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.W * a.H) return;
    const int gy = p / a.W, gx = p % a.W;
    const int r = a.flip_rows ? a.H - 1 - gy : gy, c = a.mirror_cols ? a.W - 1 - gx : gx;
    const size_t o = (size_t)r * a.out_stride + a.out_col0 + c;
    const uint32_t f = (uint32_t)(zbuf[p] & 0xffffffffull);
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, d;
    int id = -1;
    FaceSetup s;
    if (f < (uint32_t)a.F && setup_face(a, (int)f, s) && sample_face(s, (float)gx + 0.5f, (float)gy + 0.5f, b0, b1, b2, d)) {
        id = (int)f;
        if (s.swapped) { const float t = b1; b1 = b2; b2 = t; }
    } else {
        b0 = b1 = b2 = 0.f;
    }
    a.face_id[o] = id;
    a.bary[3 * o] = b0; a.bary[3 * o + 1] = b1; a.bary[3 * o + 2] = b2;
}

__global__ void __launch_bounds__(256) resolve_attribute_kernel(const int32_t* __restrict__ face_id, const float* __restrict__ bary,
                                                                const int32_t* __restrict__ faces, const float* __restrict__ attr, int V, int F,
                                                                int C, int n_pixels, const int32_t* __restrict__ pix, long long total,
                                                                float* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int row = (int)(t / C), c = (int)(t % C);
    const int p = pix ? pix[row] : row;
    float v = 0.f;
    if ((unsigned)p < (unsigned)n_pixels) {
        const int f = face_id[p];
        if ((unsigned)f < (unsigned)F) {
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
                const float b0 = bary[3 * (size_t)p], b1 = bary[3 * (size_t)p + 1], b2 = bary[3 * (size_t)p + 2];
                v = (b0 * attr[(size_t)i0 * C + c] + b1 * attr[(size_t)i1 * C + c]) + b2 * attr[(size_t)i2 * C + c];
            }
        }
    }
    out[t] = v;
}

// ---------------------------------------------------------------- k-NN ----------------------------------------------------------------
struct KnnGrid {
    float ox, oy, oz, cell, inv_cell;
    float slack;            // length by which the closing distance is shortened: covers the rounding of the cell assignment and of the cell planes
    int nx, ny, nz;
};

__device__ __forceinline__ int cell_coord(float p, float o, float inv, int n)
{
    const float t = fminf(fmaxf((p - o) * inv, 0.f), (float)(n - 1));     // NaN -> 0
    return (int)t;
}

__global__ void __launch_bounds__(256) knn_count_kernel(const float* __restrict__ pts, int N, KnnGrid g, int* __restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int cx = cell_coord(pts[3 * i], g.ox, g.inv_cell, g.nx), cy = cell_coord(pts[3 * i + 1], g.oy, g.inv_cell, g.ny),
              cz = cell_coord(pts[3 * i + 2], g.oz, g.inv_cell, g.nz);
    atomicAdd(&count[(cz * g.ny + cy) * g.nx + cx], 1);
}

// Offsets pass: exclusive prefix sum of count[0, n_pad) in place (n_pad a multiple of 4096 that exceeds n_cells, so start[n_cells] = N),
// with a copy in `cursor` for the scatter.  Three launches over tiles of 4096 cells (int4 per thread): tile sums, one workgroup that
// scans the <= 4097 tile sums, then every tile scans itself on top of its offset.  Integer sums: the result is the same in any order.
constexpr int kScanThreads = 1024, kScanTile = 4 * kScanThreads;

// exclusive scan of one tile across the workgroup; returns this thread's offset inside the tile, `total` = the tile's sum
__device__ __forceinline__ int tile_exclusive(int mine, int* s_wave, int* s_total, int& total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) { const int t = s_wave[w]; s_wave[w] = acc; acc += t; }
        *s_total = acc;
    }
    __syncthreads();
    const int excl = s_wave[wave] + incl - mine;
    total = *s_total;
    __syncthreads();                                     // s_wave / s_total may be rewritten by the caller's next tile
    return excl;
}

__global__ void __launch_bounds__(kScanThreads) knn_tile_sums_kernel(const int* __restrict__ count, int* __restrict__ sums)
{
    __shared__ int s_wave[kScanThreads / 64];
    __shared__ int s_total;
    const int4 v = *reinterpret_cast<const int4*>(count + (size_t)blockIdx.x * kScanTile + 4 * threadIdx.x);
    int total;
    tile_exclusive(v.x + v.y + v.z + v.w, s_wave, &s_total, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0, n_pad) -> exclusive, in place
__global__ void __launch_bounds__(kScanThreads) knn_scan_sums_kernel(int* __restrict__ sums, int n_pad)
{
    __shared__ int s_wave[kScanThreads / 64];
    __shared__ int s_total;
    int running = 0;
    for (int base = 0; base < n_pad; base += kScanTile) {
        int4 v = *reinterpret_cast<const int4*>(sums + base + 4 * threadIdx.x);
        int total;
        const int excl = running + tile_exclusive(v.x + v.y + v.z + v.w, s_wave, &s_total, total);
        int4 o4;
        o4.x = excl; o4.y = excl + v.x; o4.z = o4.y + v.y; o4.w = o4.z + v.z;
        *reinterpret_cast<int4*>(sums + base + 4 * threadIdx.x) = o4;
        running += total;
    }
}

__global__ void __launch_bounds__(kScanThreads) knn_tile_scan_kernel(int* __restrict__ count, int* __restrict__ cursor, const int* __restrict__ sums)
{
    __shared__ int s_wave[kScanThreads / 64];
    __shared__ int s_total;
    const size_t at = (size_t)blockIdx.x * kScanTile + 4 * threadIdx.x;
    const int4 v = *reinterpret_cast<const int4*>(count + at);
    int total;
    const int excl = sums[blockIdx.x] + tile_exclusive(v.x + v.y + v.z + v.w, s_wave, &s_total, total);
    int4 o4;
    o4.x = excl; o4.y = excl + v.x; o4.z = o4.y + v.y; o4.w = o4.z + v.z;
    *reinterpret_cast<int4*>(count + at) = o4;
    *reinterpret_cast<int4*>(cursor + at) = o4;
}

__global__ void __launch_bounds__(256) knn_scatter_kernel(const float* __restrict__ pts, int N, KnnGrid g, int* __restrict__ cursor,
                                                          float4* __restrict__ sorted)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    const int cx = cell_coord(x, g.ox, g.inv_cell, g.nx), cy = cell_coord(y, g.oy, g.inv_cell, g.ny), cz = cell_coord(z, g.oz, g.inv_cell, g.nz);
    const int pos = atomicAdd(&cursor[(cz * g.ny + cy) * g.nx + cx], 1);
    if ((unsigned)pos < (unsigned)N) sorted[pos] = make_float4(x, y, z, __int_as_float(i));   // (pos < N always: the counts sum to N)
}

// One thread per point, in cell order (neighbouring threads walk the same cells).  The order of the points inside a cell depends on
// the scatter's arrival order; the four kept VALUES do not.
__global__ void __launch_bounds__(256) knn_search_kernel(const float4* __restrict__ sorted, int N, KnnGrid g, const int* __restrict__ start,
                                                         float* __restrict__ mean_dist2, float* __restrict__ dist2)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const float4 q = sorted[t];
    const int cx = cell_coord(q.x, g.ox, g.inv_cell, g.nx), cy = cell_coord(q.y, g.oy, g.inv_cell, g.ny), cz = cell_coord(q.z, g.oz, g.inv_cell, g.nz);
    const float inf = __builtin_inff();
    float d0 = inf, d1 = inf, d2 = inf, d3 = inf;
    const int rmax = max(g.nx, max(g.ny, g.nz));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const bool face = (z == cz - r) || (z == cz + r) || (y == cy - r) || (y == cy + r);   // whole x-row lies on the shell
                const int row = (z * g.ny + y) * g.nx;
                for (int part = 0; part < 2; ++part) {
                    int xa, xb;
                    if (face) { if (part) break; xa = x0; xb = x1; }
                    else { xa = xb = part ? cx + r : cx - r; if (xa < 0 || xa >= g.nx || (part && r == 0)) continue; }
                    const int e = start[row + xb + 1];
                    for (int j = start[row + xa]; j < e; ++j) {
                        const float4 p = sorted[j];
                        const float ux = p.x - q.x, uy = p.y - q.y, uz = p.z - q.z;
                        float d = (ux * ux + uy * uy) + uz * uz;
                        if (d < d3) {                                    // insert into the ascending four
                            d3 = d;
                            if (d3 < d2) { const float s = d2; d2 = d3; d3 = s; }
                            if (d2 < d1) { const float s = d1; d1 = d2; d2 = s; }
                            if (d1 < d0) { const float s = d0; d0 = d1; d1 = s; }
                        }
                    }
                }
            }
        // closed?  every unseen point lies beyond a face of the searched block that the grid continues behind
        float dmin = inf;
        if (cx - r > 0) dmin = fminf(dmin, q.x - (g.ox + (float)(cx - r) * g.cell));
        if (cy - r > 0) dmin = fminf(dmin, q.y - (g.oy + (float)(cy - r) * g.cell));
        if (cz - r > 0) dmin = fminf(dmin, q.z - (g.oz + (float)(cz - r) * g.cell));
        if (cx + r < g.nx - 1) dmin = fminf(dmin, (g.ox + (float)(cx + r + 1) * g.cell) - q.x);
        if (cy + r < g.ny - 1) dmin = fminf(dmin, (g.oy + (float)(cy + r + 1) * g.cell) - q.y);
        if (cz + r < g.nz - 1) dmin = fminf(dmin, (g.oz + (float)(cz + r + 1) * g.cell) - q.z);
        if (dmin == inf) break;                                          // the block covers the grid: everything was seen
        dmin -= g.slack;
        if (dmin > 0.f && d3 <= dmin * dmin) break;
    }
    const int i = __float_as_int(q.w);
    if ((unsigned)i >= (unsigned)N) return;
    mean_dist2[i] = ((d1 + d2) + d3) / 3.f;
    if (dist2) { dist2[3 * i] = d1; dist2[3 * i + 1] = d2; dist2[3 * i + 2] = d3; }
}

struct KnnLayout {
    size_t start, cursor, sums, sorted, total;
    int n_pad, n_tiles, sums_pad;
    KnnLayout(size_t N, size_t n_cells)
    {
        n_pad = (int)((n_cells + 1 + kScanTile - 1) / kScanTile * kScanTile);
        size_t o = 0;
        start = o;   o = align_up(o + (size_t)n_pad * sizeof(int), 256);
        cursor = o;  o = align_up(o + (size_t)n_pad * sizeof(int), 256);
        n_tiles = n_pad / kScanTile;
        sums_pad = (n_tiles + kScanTile - 1) / kScanTile * kScanTile;
        sums = o;    o = align_up(o + (size_t)sums_pad * sizeof(int), 256);
        sorted = o;  o = align_up(o + N * sizeof(float4), 256);
        total = o + 256;
    }
};

}  // namespace
}  // namespace ag

using namespace ag;

extern "C" {

size_t ag_mesh_rasterize_ortho_workspace_bytes(int32_t W, int32_t H)
{
    if (W < 1 || H < 1) return 0;
    return (size_t)W * (size_t)H * sizeof(unsigned long long) + 256;
}

int ag_mesh_rasterize_ortho(const AgMeshRasterArgs* a, void* stream)
{
    if (!a || a->V < 0 || a->F < 0 || a->W < 1 || a->H < 1 || a->W > 16384 || a->H > 16384) { set_error("bad mesh-raster sizes"); return AG_ERR_INVALID_ARGUMENT; }
    if (a->out_col0 < 0 || (long long)a->out_col0 + a->W > (long long)a->out_stride) { set_error("mesh raster: out_col0 + W exceeds out_stride"); return AG_ERR_INVALID_ARGUMENT; }
    if (!a->face_id || !a->bary || !a->workspace || (a->F > 0 && (!a->vertices || !a->faces))) { set_error("null pointer in AgMeshRasterArgs"); return AG_ERR_INVALID_ARGUMENT; }
    if (a->workspace_bytes < ag_mesh_rasterize_ortho_workspace_bytes(a->W, a->H)) { set_error("mesh raster workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(aligned_base(a->workspace));
    const size_t npix = (size_t)a->W * a->H;
    int rc;
    if ((rc = check_hip(hipMemsetAsync(zbuf, 0xff, npix * sizeof(unsigned long long), s), "memset"))) return rc;
    if (a->F > 0) {
        hipLaunchKernelGGL(mesh_depth_kernel, dim3((a->F + 3) / 4), dim3(256), 0, s, *a, zbuf);
        if ((rc = check_hip(hipGetLastError(), "mesh_depth_kernel"))) return rc;
    }
    hipLaunchKernelGGL(mesh_resolve_ids_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, *a, zbuf);
    return check_hip(hipGetLastError(), "mesh_resolve_ids_kernel");
}

size_t ag_mesh_resolve_attribute_workspace_bytes(int32_t, int32_t, int32_t) { return 0; }

int ag_mesh_resolve_attribute(const int32_t* face_id, const float* bary, const int32_t* faces, const float* attribute, int32_t V, int32_t F,
                              int32_t C, int32_t n_pixels, const int32_t* pix, int32_t N, float* out, void* stream)
{
    if (V < 0 || F < 0 || C < 1 || n_pixels < 0 || N < 0) { set_error("bad resolve sizes"); return AG_ERR_INVALID_ARGUMENT; }
    const long long rows = pix ? N : n_pixels;
    if (rows == 0) return AG_OK;
    if (!face_id || !bary || !faces || !attribute || !out) { set_error("null pointer in ag_mesh_resolve_attribute"); return AG_ERR_INVALID_ARGUMENT; }
    const long long total = rows * C;
    if ((total + 255) / 256 > 0x7fffffffll) { set_error("resolve: too many outputs"); return AG_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(resolve_attribute_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       face_id, bary, faces, attribute, V, F, C, n_pixels, pix, total, out);
    return check_hip(hipGetLastError(), "resolve_attribute_kernel");
}

size_t ag_knn_mean_dist2_workspace_bytes(int32_t N, int32_t n_cells)
{
    if (N < 0 || n_cells < 1) return 0;
    return KnnLayout((size_t)N, (size_t)n_cells).total;
}

int ag_knn_mean_dist2(const float* points, int32_t N, const float* origin, float cell, const int32_t* dims, float* mean_dist2, float* dist2,
                      void* workspace, size_t workspace_bytes, void* stream)
{
    if (N < 4) { set_error("k-NN (K = 4 including the point itself) needs at least 4 points"); return AG_ERR_INVALID_ARGUMENT; }
    if (!points || !origin || !dims || !mean_dist2 || !workspace) { set_error("null pointer in ag_knn_mean_dist2"); return AG_ERR_INVALID_ARGUMENT; }
    if (!(cell > 0.f) || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) { set_error("k-NN: bad grid"); return AG_ERR_INVALID_ARGUMENT; }
    const long long n_cells = (long long)dims[0] * dims[1] * dims[2];
    if (dims[0] > (1 << 24) || dims[1] > (1 << 24) || dims[2] > (1 << 24) || n_cells > (1ll << 24)) { set_error("k-NN: more than 2^24 cells"); return AG_ERR_INVALID_ARGUMENT; }
    const KnnLayout L((size_t)N, (size_t)n_cells);
    if (workspace_bytes < L.total) { set_error("k-NN workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* base = aligned_base(workspace);
    int* start = reinterpret_cast<int*>(base + L.start);
    int* cursor = reinterpret_cast<int*>(base + L.cursor);
    int* sums = reinterpret_cast<int*>(base + L.sums);
    float4* sorted = reinterpret_cast<float4*>(base + L.sorted);
    KnnGrid g;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2]; g.cell = cell; g.inv_cell = 1.f / cell;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    // A point at cell coordinate t = (p - o) / cell is assigned with (p - o) * inv_cell: three roundings, 3 u t <= 3 u max(dims) cells; the
    // plane o + k cell of the closing test is itself rounded by <= 2 u (|o| + dims cell).  Doubled, plus 1e-3 cell.
    // For a grid far from the origin with small cells (|o| / cell > 2^22) the second term alone exceeds a cell: the search then always
    // walks one ring more than geometry needs.  That costs time only; the result stays exact.
    {
        const double u = 5.9604644775390625e-08;
        double md = 1.0, ext = 0.0;
        for (int k = 0; k < 3; ++k) {
            md = dims[k] > md ? dims[k] : md;
            const double e = fabs((double)origin[k]) + (double)dims[k] * cell;
            ext = e > ext ? e : ext;
        }
        g.slack = (float)(cell * (1e-3 + 6.0 * u * md) + 4.0 * u * ext);
    }
    int rc;
    if ((rc = check_hip(hipMemsetAsync(start, 0, (size_t)L.n_pad * sizeof(int), s), "memset"))) return rc;
    if ((rc = check_hip(hipMemsetAsync(sums, 0, (size_t)L.sums_pad * sizeof(int), s), "memset"))) return rc;
    const dim3 grid((N + 255) / 256), block(256);
    hipLaunchKernelGGL(knn_count_kernel, grid, block, 0, s, points, N, g, start);
    if ((rc = check_hip(hipGetLastError(), "knn_count_kernel"))) return rc;
    hipLaunchKernelGGL(knn_tile_sums_kernel, dim3(L.n_tiles), dim3(kScanThreads), 0, s, start, sums);
    if ((rc = check_hip(hipGetLastError(), "knn_tile_sums_kernel"))) return rc;
    hipLaunchKernelGGL(knn_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, s, sums, L.sums_pad);
    if ((rc = check_hip(hipGetLastError(), "knn_scan_sums_kernel"))) return rc;
    hipLaunchKernelGGL(knn_tile_scan_kernel, dim3(L.n_tiles), dim3(kScanThreads), 0, s, start, cursor, sums);
    if ((rc = check_hip(hipGetLastError(), "knn_tile_scan_kernel"))) return rc;
    hipLaunchKernelGGL(knn_scatter_kernel, grid, block, 0, s, points, N, g, cursor, sorted);
    if ((rc = check_hip(hipGetLastError(), "knn_scatter_kernel"))) return rc;
    hipLaunchKernelGGL(knn_search_kernel, grid, block, 0, s, sorted, N, g, start, mean_dist2, dist2);
    return check_hip(hipGetLastError(), "knn_search_kernel");
}

}  // extern "C"
