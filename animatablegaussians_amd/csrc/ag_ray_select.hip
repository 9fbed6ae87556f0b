// Ray selection of the template stage (include/ag_ray_select.h): the box's image-space mask and the candidate classes, the ordered
// compaction of a class / flag array into ascending index lists, and the ray, box near / far and targets of a list of pixels.
//
// classify: one thread per pixel, six quads of four int64 edge functions each on corners that arrive by value.  1 B (+ 1 B) in, 1 B out.
// compact:  a wave owns a run of kRun = 512 consecutive flags (8 steps of 64 lanes, one byte per lane and step).  Launch 1 counts the
//           two classes of every run (popcount of a ballot), launch 2 scans the run counts in one workgroup, launch 3 walks the runs
//           again and stores index i at run offset + number of set lower lanes (mbcnt of the ballot).  No LDS outside the scan, no
//           atomics: the lists are ascending by construction.
// build:    one thread per list entry; the float32 operations are those of the header, one statement each, compiled without contraction.
#include "ag_common.h"
#include "../../include/ag_ray_select.h"

namespace ag {
namespace ray_select {

constexpr int kThreads = 256;
constexpr int kRun = 512;                    // flags per wave
constexpr int kRunsPerBlock = kThreads / kWave;
constexpr int kScanThreads = 256;
constexpr long long kMaxCount = 2147483647ll;
constexpr int kMaxCorner = 1 << 29;

struct Corners { int32_t xy[16]; };

__device__ __forceinline__ bool in_quad(const Corners& c, int i0, int i1, int i2, int i3, long long x, long long y)
{
    const int idx[5] = {i0, i1, i2, i3, i0};
    bool all_ge = true, all_le = true;
    long long xmin = c.xy[2 * i0], xmax = xmin, ymin = c.xy[2 * i0 + 1], ymax = ymin;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long ax = c.xy[2 * idx[i]], ay = c.xy[2 * idx[i] + 1], bx = c.xy[2 * idx[i + 1]], by = c.xy[2 * idx[i + 1] + 1];
        const long long e = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
        all_ge = all_ge && e >= 0;
        all_le = all_le && e <= 0;
        xmin = min(xmin, ax); xmax = max(xmax, ax); ymin = min(ymin, ay); ymax = max(ymax, ay);
    }
    return (all_ge || all_le) && x >= xmin && x <= xmax && y >= ymin && y <= ymax;
}

__global__ void __launch_bounds__(kThreads) classify_kernel(Corners c, int W, long long n, const uint8_t* __restrict__ mask,
                                                            const uint8_t* __restrict__ unsample, uint8_t* __restrict__ cls)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long y = i / W, x = i - y * W;
    const bool bound = in_quad(c, 0, 1, 3, 2, x, y) || in_quad(c, 4, 5, 7, 6, x, y) || in_quad(c, 0, 1, 5, 4, x, y) ||
                       in_quad(c, 2, 3, 7, 6, x, y) || in_quad(c, 0, 2, 6, 4, x, y) || in_quad(c, 1, 3, 7, 5, x, y);
    uint8_t out = 0;
    if (bound && !(unsample && unsample[i] != 0)) out = (!mask || mask[i] != 0) ? 1 : 2;
    cls[i] = out;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lower_lanes(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// counts[2 r], counts[2 r + 1] = number of flags 1 / 2 in run r.  Every lane of a wave takes every step (the ballots need them all).
__global__ void __launch_bounds__(kThreads) count_runs_kernel(const uint8_t* __restrict__ flags, long long n, long long runs, int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)blockIdx.x * kRunsPerBlock + (threadIdx.x / kWave);
    if (r >= runs) return;                                  // wave-uniform
    int c1 = 0, c2 = 0;
#pragma unroll
    for (int s = 0; s < kRun / kWave; ++s) {
        const long long i = r * kRun + s * kWave + lane;
        const uint8_t f = i < n ? flags[i] : (uint8_t)0;
        c1 += __popcll(__ballot(f == 1));
        c2 += __popcll(__ballot(f == 2));
    }
    if (lane == 0) { counts[2 * r] = c1; counts[2 * r + 1] = c2; }
}

// One workgroup: counts -> exclusive offsets, in place; totals -> totals_out[0 .. 1] (the second is 0 when class 2 has no list).  Thread t
// owns `per` consecutive runs.
__global__ void __launch_bounds__(kScanThreads) scan_runs_kernel(int32_t* __restrict__ counts, long long runs, long long per, int32_t* __restrict__ totals_out,
                                                                 int two_lists)
{
    __shared__ int32_t part[2][2][kScanThreads];            // [buffer][class][thread]
    const int t = threadIdx.x;
    const long long r0 = min(runs, t * per), r1 = min(runs, r0 + per);
    int32_t s1 = 0, s2 = 0;
    for (long long r = r0; r < r1; ++r) { s1 += counts[2 * r]; s2 += counts[2 * r + 1]; }
    part[0][0][t] = s1; part[0][1][t] = s2;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < kScanThreads; o <<= 1) {            // inclusive scan over the threads' sums
        const int32_t a1 = part[cur][0][t] + (t >= o ? part[cur][0][t - o] : 0);
        const int32_t a2 = part[cur][1][t] + (t >= o ? part[cur][1][t - o] : 0);
        part[cur ^ 1][0][t] = a1; part[cur ^ 1][1][t] = a2;
        cur ^= 1;
        __syncthreads();
    }
    int32_t b1 = part[cur][0][t] - s1, b2 = part[cur][1][t] - s2;
    for (long long r = r0; r < r1; ++r) {
        const int32_t c1 = counts[2 * r], c2 = counts[2 * r + 1];
        counts[2 * r] = b1; counts[2 * r + 1] = b2;
        b1 += c1; b2 += c2;
    }
    if (t == kScanThreads - 1) { totals_out[0] = part[cur][0][t]; totals_out[1] = two_lists ? part[cur][1][t] : 0; }
}

__global__ void __launch_bounds__(kThreads) scatter_runs_kernel(const uint8_t* __restrict__ flags, long long n, long long runs,
                                                                const int32_t* __restrict__ offsets, int32_t* __restrict__ list1, int32_t* __restrict__ list2)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)blockIdx.x * kRunsPerBlock + (threadIdx.x / kWave);
    if (r >= runs) return;                                  // wave-uniform
    long long o1 = offsets[2 * r], o2 = offsets[2 * r + 1]; // <= the number of flags in front of the run: inside the lists
#pragma unroll
    for (int s = 0; s < kRun / kWave; ++s) {
        const long long i = r * kRun + s * kWave + lane;
        const uint8_t f = i < n ? flags[i] : (uint8_t)0;
        const unsigned long long m1 = __ballot(f == 1), m2 = __ballot(f == 2);
        if (f == 1) list1[o1 + lower_lanes(m1)] = (int32_t)i;
        if (f == 2 && list2) list2[o2 + lower_lanes(m2)] = (int32_t)i;
        o1 += __popcll(m1); o2 += __popcll(m2);
    }
}

// ---- build --------------------------------------------------------------------------------------------------------------------------
struct Box { float lo[3], hi[3]; };

__device__ __forceinline__ Box padded(const float* bounds)
{
    Box b;
#pragma unroll
    for (int a = 0; a < 3; ++a) { b.lo[a] = bounds[a] - 0.01f; b.hi[a] = bounds[3 + a] + 0.01f; }
    return b;
}

// get_rays of the pixel (x, y) -> d
__device__ __forceinline__ void pixel_ray(const AgRayCamera& c, int x, int y, float d[3])
{
    const float X = (float)x, Y = (float)y;
    float p[3], g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = (c.inv_intr[3 * i] * X + c.inv_intr[3 * i + 1] * Y) + c.inv_intr[3 * i + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float w = ((c.inv_rot[3 * i] * p[0] + c.inv_rot[3 * i + 1] * p[1]) + c.inv_rot[3 * i + 2] * p[2]) + c.cam[i];
        g[i] = w - c.cam[i];
    }
    const float l = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const float den = l + 1e-8f;
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = g[i] / den;
}

// get_near_far of one ray -> hit; near / far are 0 without one
__device__ __forceinline__ bool box_near_far(const Box& b, const float o[3], const float d[3], float& near, float& far)
{
    int passed = 0;
    float s[2] = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int a = j % 3;
        const float plane = j < 3 ? b.lo[a] : b.hi[a];
        const float t = (plane - o[a]) / (d[a] + 1e-9f);
        float q[3];
        bool in = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            q[i] = t * d[i] + o[i];
            in = in && q[i] >= b.lo[i] - 1e-6f && q[i] <= b.hi[i] + 1e-6f;
        }
        if (in) {
            if (passed < 2) {
                const float e0 = q[0] - o[0], e1 = q[1] - o[1], e2 = q[2] - o[2];
                s[passed] = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
            }
            ++passed;
        }
    }
    const bool hit = passed == 2;
    near = far = 0.0f;
    if (hit) {
        const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const float s0 = s[0] / n, s1 = s[1] / n;
        near = fminf(s0, s1);
        far = fmaxf(s0, s1);
    }
    return hit;
}

struct BuildArgs {
    AgRayCamera cam;
    const int32_t* pix;
    const int32_t* uv_in;
    long long n;
    const float* color;
    const uint8_t* mask;
    const float* depth;
    int32_t* uv;
    float *ray_o, *ray_d, *near, *far;
    uint8_t* hit;
    float *color_gt, *mask_gt, *depth_gt, *dist;
};

__global__ void __launch_bounds__(kThreads) build_kernel(BuildArgs a)
{
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= a.n) return;
    const AgRayCamera& c = a.cam;
    int x, y;
    long long p = -1;                       // the pixel's flat index where there is a frame
    bool valid = true;
    if (a.uv_in) {
        x = a.uv_in[2 * k]; y = a.uv_in[2 * k + 1];
    } else {
        p = a.pix ? (long long)a.pix[k] : k;
        valid = p >= 0 && p < (long long)c.W * c.H;
        if (!valid) p = 0;
        y = (int)(p / c.W); x = (int)(p - (long long)y * c.W);
    }
    float d[3] = {0.0f, 0.0f, 0.0f}, o[3] = {0.0f, 0.0f, 0.0f};
    float near = 0.0f, far = 0.0f;
    bool hit = false;
    if (valid) {
        pixel_ray(c, x, y, d);
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = c.cam[i];
        if (a.hit) hit = box_near_far(padded(c.bounds), o, d, near, far);
    } else {
        x = y = 0;
    }
    if (a.uv) { a.uv[2 * k] = x; a.uv[2 * k + 1] = y; }
    if (a.ray_o) { a.ray_o[3 * k] = o[0]; a.ray_o[3 * k + 1] = o[1]; a.ray_o[3 * k + 2] = o[2]; }
    if (a.ray_d) { a.ray_d[3 * k] = d[0]; a.ray_d[3 * k + 1] = d[1]; a.ray_d[3 * k + 2] = d[2]; }
    if (a.hit) { a.near[k] = near; a.far[k] = far; a.hit[k] = hit ? 1 : 0; }
    if (a.color) {
        float col[3] = {0.0f, 0.0f, 0.0f}, m = 0.0f, depth = 0.0f, dist = 0.0f;
        if (valid) {
            const bool on = a.mask[p] != 0;
            m = on ? 1.0f : 0.0f;
            if (on) { col[0] = a.color[3 * p]; col[1] = a.color[3 * p + 1]; col[2] = a.color[3 * p + 2]; }
            depth = a.depth ? a.depth[p] : 0.0f;
            const float ex = (((float)x + 0.5f) - c.cx) * depth / c.fx;
            const float ey = (((float)y + 0.5f) - c.cy) * depth / c.fy;
            dist = sqrtf((ex * ex + ey * ey) + depth * depth);
        }
        a.color_gt[3 * k] = col[0]; a.color_gt[3 * k + 1] = col[1]; a.color_gt[3 * k + 2] = col[2];
        a.mask_gt[k] = m; a.depth_gt[k] = depth; a.dist[k] = dist;
    }
}

struct Bounds { float v[6]; };

__global__ void __launch_bounds__(kThreads) box_near_far_kernel(Bounds bounds, const float* __restrict__ ray_o, const float* __restrict__ ray_d, long long n,
                                                                float* __restrict__ near, float* __restrict__ far, uint8_t* __restrict__ hit)
{
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const float o[3] = {ray_o[3 * k], ray_o[3 * k + 1], ray_o[3 * k + 2]}, d[3] = {ray_d[3 * k], ray_d[3 * k + 1], ray_d[3 * k + 2]};
    float nr, fr;
    const bool h = box_near_far(padded(bounds.v), o, d, nr, fr);
    near[k] = nr; far[k] = fr; hit[k] = h ? 1 : 0;
}

static unsigned blocks_of(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace ray_select
}  // namespace ag

using namespace ag;
using namespace ag::ray_select;

extern "C" int ag_ray_classify(const int32_t* corners_xy, int32_t H, int32_t W, const uint8_t* mask_u8, const uint8_t* unsample_u8, uint8_t* cls_u8,
                               void* stream)
{
    if (!corners_xy || !cls_u8) { set_error("null pointer in ag_ray_classify"); return AG_ERR_INVALID_ARGUMENT; }
    if (H <= 0 || W <= 0 || (long long)H * W > kMaxCount) { set_error("ray classify: bad frame H = %d, W = %d", H, W); return AG_ERR_INVALID_ARGUMENT; }
    Corners c;
    for (int i = 0; i < 16; ++i) {
        if (corners_xy[i] > kMaxCorner || corners_xy[i] < -kMaxCorner) {
            set_error("ray classify: corner coordinate %d is beyond 2^29", corners_xy[i]);
            return AG_ERR_INVALID_ARGUMENT;
        }
        c.xy[i] = corners_xy[i];
    }
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(classify_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), c, W, n, mask_u8,
                       unsample_u8, cls_u8);
    return check_hip(hipGetLastError(), "classify_kernel");
}

extern "C" size_t ag_ray_compact_workspace_bytes(int64_t n)
{
    if (n < 0 || n > kMaxCount) return 0;
    const size_t runs = (size_t)((n + kRun - 1) / kRun);
    return align_up(runs * 2 * sizeof(int32_t), 256) + 256;
}

extern "C" int ag_ray_compact(const uint8_t* flags_u8, int64_t n, int32_t* list1, int32_t* list2, int32_t* counts_i32, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    if (n < 0 || n > kMaxCount) { set_error("ray compact: n = %lld is outside 0 .. 2^31 - 1", (long long)n); return AG_ERR_INVALID_ARGUMENT; }
    if (!counts_i32 || !workspace || (n > 0 && (!flags_u8 || !list1))) { set_error("null pointer in ag_ray_compact"); return AG_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < ag_ray_compact_workspace_bytes(n)) {
        set_error("ray compact: workspace of %zu bytes, %zu needed", workspace_bytes, ag_ray_compact_workspace_bytes(n));
        return AG_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) return check_hip(hipMemsetAsync(counts_i32, 0, 2 * sizeof(int32_t), s), "clear counts_i32");
    int32_t* counts = reinterpret_cast<int32_t*>(aligned_base(workspace));
    const long long runs = (n + kRun - 1) / kRun;
    const unsigned grid = blocks_of(runs, kRunsPerBlock);
    hipLaunchKernelGGL(count_runs_kernel, dim3(grid), dim3(kThreads), 0, s, flags_u8, (long long)n, runs, counts);
    int rc = check_hip(hipGetLastError(), "count_runs_kernel");
    if (rc != AG_OK) return rc;
    hipLaunchKernelGGL(scan_runs_kernel, dim3(1), dim3(kScanThreads), 0, s, counts, runs, (runs + kScanThreads - 1) / kScanThreads, counts_i32,
                       list2 ? 1 : 0);
    rc = check_hip(hipGetLastError(), "scan_runs_kernel");
    if (rc != AG_OK) return rc;
    hipLaunchKernelGGL(scatter_runs_kernel, dim3(grid), dim3(kThreads), 0, s, flags_u8, (long long)n, runs, counts, list1, list2);
    return check_hip(hipGetLastError(), "scatter_runs_kernel");
}

extern "C" size_t ag_ray_camera_bytes(void) { return sizeof(AgRayCamera); }

extern "C" int ag_ray_build(const AgRayCamera* camera, const int32_t* pix_i32, const int32_t* uv_in_i32, int64_t n, const float* color_img,
                            const uint8_t* mask_u8, const float* depth_img, int32_t* uv_i32, float* ray_o, float* ray_d, float* near, float* far,
                            uint8_t* hit_u8, float* color_gt, float* mask_gt, float* depth_gt, float* dist, void* stream)
{
    if (!camera) { set_error("null camera in ag_ray_build"); return AG_ERR_INVALID_ARGUMENT; }
    if (n < 0 || n > kMaxCount) { set_error("ray build: n = %lld is outside 0 .. 2^31 - 1", (long long)n); return AG_ERR_INVALID_ARGUMENT; }
    if (pix_i32 && uv_in_i32) { set_error("ray build: pix_i32 and uv_in_i32 are alternatives"); return AG_ERR_INVALID_ARGUMENT; }
    const bool images = color_img || mask_u8;
    if ((color_img == nullptr) != (mask_u8 == nullptr) || (depth_img && !images)) {
        set_error("ray build: color_img and mask_u8 go together, depth_img only with them");
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (uv_in_i32 && images) { set_error("ray build: explicit coordinates (uv_in_i32) take no images"); return AG_ERR_INVALID_ARGUMENT; }
    if (!uv_in_i32) {
        if (camera->W <= 0 || camera->H <= 0 || (long long)camera->W * camera->H > kMaxCount) {
            set_error("ray build: bad frame H = %d, W = %d", camera->H, camera->W);
            return AG_ERR_INVALID_ARGUMENT;
        }
        if (!pix_i32 && n != (long long)camera->W * camera->H) {
            set_error("ray build: without a pixel list n must be W H = %lld, got %lld", (long long)camera->W * camera->H, (long long)n);
            return AG_ERR_INVALID_ARGUMENT;
        }
    }
    const int targets = (color_gt != nullptr) + (mask_gt != nullptr) + (depth_gt != nullptr) + (dist != nullptr);
    if (targets != (images ? 4 : 0)) { set_error("ray build: color_gt, mask_gt, depth_gt and dist are all given with images and none without"); return AG_ERR_INVALID_ARGUMENT; }
    const int box = (near != nullptr) + (far != nullptr) + (hit_u8 != nullptr);
    if (box != 0 && box != 3) { set_error("ray build: near, far and hit_u8 go together (all or none)"); return AG_ERR_INVALID_ARGUMENT; }
    if (n == 0) return AG_OK;
    BuildArgs a;
    a.cam = *camera; a.pix = pix_i32; a.uv_in = uv_in_i32; a.n = n; a.color = color_img; a.mask = mask_u8; a.depth = depth_img;
    a.uv = uv_i32; a.ray_o = ray_o; a.ray_d = ray_d; a.near = near; a.far = far; a.hit = hit_u8;
    a.color_gt = color_gt; a.mask_gt = mask_gt; a.depth_gt = depth_gt; a.dist = dist;
    hipLaunchKernelGGL(build_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return check_hip(hipGetLastError(), "build_kernel");
}

extern "C" int ag_ray_box_near_far(const float* bounds, const float* ray_o, const float* ray_d, int64_t n, float* near, float* far, uint8_t* hit_u8,
                                   void* stream)
{
    if (n < 0 || n > kMaxCount) { set_error("ray box near far: n = %lld is outside 0 .. 2^31 - 1", (long long)n); return AG_ERR_INVALID_ARGUMENT; }
    if (!bounds || (n > 0 && (!ray_o || !ray_d || !near || !far || !hit_u8))) { set_error("null pointer in ag_ray_box_near_far"); return AG_ERR_INVALID_ARGUMENT; }
    if (n == 0) return AG_OK;
    Bounds c;
    for (int i = 0; i < 6; ++i) c.v[i] = bounds[i];
    hipLaunchKernelGGL(box_near_far_kernel, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), c, ray_o, ray_d,
                       (long long)n, near, far, hit_u8);
    return check_hip(hipGetLastError(), "box_near_far_kernel");
}
