// Closest point on a triangle mesh, brute force over all faces (include/ag_mesh_query.h): the nearest-face search behind
// interpolate_lbs / nearest_face_pytorch3d and the unsigned half of igl.signed_distance over the grid of a blend-weight volume, and the
// pseudonormal sign that makes it signed.  Init-time; 128^3 grid nodes x 21 k faces = 4.4e10 pair tests: VALU bound.
//
// Mapping: one lane per query, all lanes of a wave on the same face.  A face is a 64-byte record (corner, two edge vectors, their dot
// products and four reciprocals) made once per call by face_record_kernel, so a pair test divides nothing and gathers nothing; the
// record is wave-uniform and arrives either through the scalar cache (the loop index is uniform: walk 1) or from an LDS tile as four
// broadcast 16-byte reads (walk 2).  The pair test is straight-line code: the in-plane projection and the three clamped edge points
// are all evaluated and the smallest squared distance kept (selects, no region branches: a divergent region branch would cost every
// lane every arm anyway).  The walk carries (best d2, best face) only; the winner's barycentrics and feature code are evaluated once
// more after the walk by the same device function, so the hot loop keeps no per-candidate state.  The one branch in the loop is the
// update of the best pair, taken O(log F) times per lane.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states the pair test as individually rounded fp32 operations, which is
// what the float32 run of tests/mesh_query_oracle.py (numpy has no FMA) evaluates and profiles/ub/mesh_query_host_walk.hip walks on
// the host.  No atomics; the tie rule (lower face index on equal d2) makes the result independent of the visiting order.
#include "ag_common.h"
#include "../../include/ag_mesh_query.h"

#include <math.h>

#define AG_MQ_FN __host__ __device__ inline

namespace ag {
namespace meshq {

constexpr int kThreads = 256;
constexpr int kTile = AG_MESH_QUERY_FACE_TILE;

struct __attribute__((aligned(16))) FaceRec {
    float v0x, v0y, v0z, a;
    float e0x, e0y, e0z, b;
    float e1x, e1y, e1z, c;
    float ia, ic, ih, idet;
};
static_assert(sizeof(FaceRec) == 64, "FaceRec must be 64 bytes");

AG_MQ_FN float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
AG_MQ_FN float recip_or_zero(float x) { return x > 0.f ? 1.f / x : 0.f; }
AG_MQ_FN float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// the record of face f; a face with an index outside [0, V) gets NaNs: every comparison with its distances is false
AG_MQ_FN FaceRec face_record(const float* vertices, const int32_t* faces, int V, int f)
{
    FaceRec r;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
        const float q = NAN;
        r.v0x = r.v0y = r.v0z = r.a = r.e0x = r.e0y = r.e0z = r.b = r.e1x = r.e1y = r.e1z = r.c = q;
        r.ia = r.ic = r.ih = r.idet = 0.f;
        return r;
    }
    const float* p0 = vertices + 3 * (size_t)i0;
    const float* p1 = vertices + 3 * (size_t)i1;
    const float* p2 = vertices + 3 * (size_t)i2;
    r.v0x = p0[0]; r.v0y = p0[1]; r.v0z = p0[2];
    r.e0x = p1[0] - p0[0]; r.e0y = p1[1] - p0[1]; r.e0z = p1[2] - p0[2];
    r.e1x = p2[0] - p0[0]; r.e1y = p2[1] - p0[1]; r.e1z = p2[2] - p0[2];
    const float e2x = r.e1x - r.e0x, e2y = r.e1y - r.e0y, e2z = r.e1z - r.e0z;
    r.a = dot3(r.e0x, r.e0y, r.e0z, r.e0x, r.e0y, r.e0z);
    r.b = dot3(r.e0x, r.e0y, r.e0z, r.e1x, r.e1y, r.e1z);
    r.c = dot3(r.e1x, r.e1y, r.e1z, r.e1x, r.e1y, r.e1z);
    const float h = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
    r.ia = recip_or_zero(r.a);
    r.ic = recip_or_zero(r.c);
    r.ih = recip_or_zero(h);
    r.idet = recip_or_zero(r.a * r.c - r.b * r.b);
    return r;
}

// the four candidates of one (query, face) pair: their squared distances (candidate 0: +inf unless `inside`) and parameters
struct Candidates {
    float d2[4];
    float s0, t0, s1, u2, t3;
};

AG_MQ_FN float dist2_at(const FaceRec& r, float Dx, float Dy, float Dz, float s, float t)
{
    const float rx = (Dx + s * r.e0x) + t * r.e1x, ry = (Dy + s * r.e0y) + t * r.e1y, rz = (Dz + s * r.e0z) + t * r.e1z;
    return dot3(rx, ry, rz, rx, ry, rz);
}

// t = 0 (edge v0v1) and s = 0 (edge v2v0): the zero term of r(s, t) adds nothing (x + 0 * y = x for finite y), so it is left out
AG_MQ_FN float dist2_along(float Dx, float Dy, float Dz, float p, float ex, float ey, float ez)
{
    const float rx = Dx + p * ex, ry = Dy + p * ey, rz = Dz + p * ez;
    return dot3(rx, ry, rz, rx, ry, rz);
}

AG_MQ_FN Candidates candidates(const FaceRec& r, float qx, float qy, float qz)
{
    Candidates k;
    const float Dx = r.v0x - qx, Dy = r.v0y - qy, Dz = r.v0z - qz;
    const float d = dot3(r.e0x, r.e0y, r.e0z, Dx, Dy, Dz);
    const float e = dot3(r.e1x, r.e1y, r.e1z, Dx, Dy, Dz);
    const float det = r.a * r.c - r.b * r.b;
    const float sn = r.b * e - r.c * d, tn = r.b * d - r.a * e;
    const bool inside = (sn >= 0.f) & (tn >= 0.f) & (sn + tn <= det) & (det > 0.f);
    k.s0 = sn * r.idet;
    k.t0 = tn * r.idet;
    k.s1 = clamp01(0.f - d * r.ia);
    k.u2 = clamp01(((r.a - r.b) + (d - e)) * r.ih);
    k.t3 = clamp01(0.f - e * r.ic);
    const float di = dist2_at(r, Dx, Dy, Dz, k.s0, k.t0);
    k.d2[0] = inside ? di : INFINITY;
    k.d2[1] = dist2_along(Dx, Dy, Dz, k.s1, r.e0x, r.e0y, r.e0z);
    k.d2[2] = dist2_at(r, Dx, Dy, Dz, 1.f - k.u2, k.u2);
    k.d2[3] = dist2_along(Dx, Dy, Dz, k.t3, r.e1x, r.e1y, r.e1z);
    return k;
}

// the face's squared distance alone: what the walk needs.  `x < y ? x : y` keeps the FIRST on equality, as the detail pass does;
// a NaN (a skipped face) never replaces anything and candidate 0 of such a face is +inf.
AG_MQ_FN float pair_dist2(const FaceRec& r, float qx, float qy, float qz)
{
    const Candidates k = candidates(r, qx, qy, qz);
    float m = k.d2[0];
    m = k.d2[1] < m ? k.d2[1] : m;
    m = k.d2[2] < m ? k.d2[2] : m;
    m = k.d2[3] < m ? k.d2[3] : m;
    return m;
}

AG_MQ_FN bool wins(float d2, int f, float best, int best_f) { return d2 < best || (d2 == best && f < best_f); }

AG_MQ_FN int edge_feature(float p, int edge, int at0, int at1) { return p <= 0.f ? at0 : (p >= 1.f ? at1 : edge); }

// the winner once more, with its barycentrics and feature code
AG_MQ_FN void pair_detail(const FaceRec& r, float qx, float qy, float qz, float& d2, float& b0, float& b1, float& b2, int& feature)
{
    const Candidates k = candidates(r, qx, qy, qz);
    d2 = k.d2[0]; b0 = fmaxf((1.f - k.s0) - k.t0, 0.f); b1 = k.s0; b2 = k.t0; feature = 0;
    if (k.d2[1] < d2) { d2 = k.d2[1]; b0 = 1.f - k.s1; b1 = k.s1; b2 = 0.f; feature = edge_feature(k.s1, 1, 4, 5); }
    if (k.d2[2] < d2) { d2 = k.d2[2]; b0 = 0.f; b1 = 1.f - k.u2; b2 = k.u2; feature = edge_feature(k.u2, 2, 5, 6); }
    if (k.d2[3] < d2) { d2 = k.d2[3]; b0 = 1.f - k.t3; b1 = 0.f; b2 = k.t3; feature = edge_feature(k.t3, 3, 4, 6); }
}

struct Query {
    int N, V, F, gx, gy, gz;
    const float* points;
    const float* axis_x;
    const float* axis_y;
    const float* axis_z;
};

AG_MQ_FN void load_query(const Query& a, int n, float& qx, float& qy, float& qz)
{
    if (a.points) {
        qx = a.points[3 * (size_t)n]; qy = a.points[3 * (size_t)n + 1]; qz = a.points[3 * (size_t)n + 2];
    } else {                                                                   // n < N = gx * gy * gz: every index is inside its axis
        const int k = n % a.gz, ij = n / a.gz;
        qx = a.axis_x[ij / a.gy]; qy = a.axis_y[ij % a.gy]; qz = a.axis_z[k];
    }
}

AG_MQ_FN void store_result(const FaceRec* recs, int n, float qx, float qy, float qz, int best_f, float* dist2, int32_t* face_id, float* bary,
                           int32_t* feature)
{
    float d2 = INFINITY, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    int feat = 0;
    if (best_f >= 0) pair_detail(recs[best_f], qx, qy, qz, d2, b0, b1, b2, feat);
    dist2[n] = d2;
    face_id[n] = best_f;
    bary[3 * (size_t)n] = b0; bary[3 * (size_t)n + 1] = b1; bary[3 * (size_t)n + 2] = b2;
    if (feature) feature[n] = feat;
}

// sign of one query (header: ag_mesh_pseudonormal_sign)
AG_MQ_FN float pseudonormal_sign(const Query& a, int n, const float* vertices, const int32_t* faces, const int32_t* face_id, const float* bary,
                                 const int32_t* feature, const float* face_normals, const float* edge_normals, const float* vertex_normals)
{
    const int f = face_id[n];
    if ((unsigned)f >= (unsigned)a.F) return 0.f;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) return 0.f;
    float qx, qy, qz;
    load_query(a, n, qx, qy, qz);
    const float b0 = bary[3 * (size_t)n], b1 = bary[3 * (size_t)n + 1], b2 = bary[3 * (size_t)n + 2];
    const float* p0 = vertices + 3 * (size_t)i0;
    const float* p1 = vertices + 3 * (size_t)i1;
    const float* p2 = vertices + 3 * (size_t)i2;
    const float wx = qx - ((b0 * p0[0] + b1 * p1[0]) + b2 * p2[0]);
    const float wy = qy - ((b0 * p0[1] + b1 * p1[1]) + b2 * p2[1]);
    const float wz = qz - ((b0 * p0[2] + b1 * p1[2]) + b2 * p2[2]);
    const int feat = feature[n];
    const float* nrm = face_normals + 3 * (size_t)f;
    if (feat >= 1 && feat <= 3) nrm = edge_normals + 9 * (size_t)f + 3 * (feat - 1);
    else if (feat >= 4 && feat <= 6) nrm = vertex_normals + 3 * (size_t)(feat == 4 ? i0 : (feat == 5 ? i1 : i2));
    const float s = dot3(wx, wy, wz, nrm[0], nrm[1], nrm[2]);
    return s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
}

#ifndef AG_MESH_QUERY_HOST_ONLY
__global__ void __launch_bounds__(kThreads) face_record_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V, int F,
                                                               FaceRec* __restrict__ recs)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f < F) recs[f] = face_record(vertices, faces, V, f);
}

// walk 1: the loop index is wave-uniform and `recs` is read-only for the kernel, so each record is one scalar 64-byte load
__global__ void __launch_bounds__(kThreads) closest_point_uniform_kernel(Query a, const FaceRec* __restrict__ recs, float* __restrict__ dist2,
                                                                         int32_t* __restrict__ face_id, float* __restrict__ bary,
                                                                         int32_t* __restrict__ feature)
{
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= a.N) return;
    float qx, qy, qz;
    load_query(a, n, qx, qy, qz);
    float best = INFINITY;
    int best_f = -1;
#pragma unroll 2
    for (int f = 0; f < a.F; ++f) {
        const float d2 = pair_dist2(recs[f], qx, qy, qz);
        if (wins(d2, f, best, best_f)) { best = d2; best_f = f; }
    }
    store_result(recs, n, qx, qy, qz, best_f, dist2, face_id, bary, feature);
}

// walk 2: kTile records per step through LDS; every lane reads the same record (a broadcast, no bank conflict)
__global__ void __launch_bounds__(kThreads) closest_point_tiled_kernel(Query a, const FaceRec* __restrict__ recs, float* __restrict__ dist2,
                                                                       int32_t* __restrict__ face_id, float* __restrict__ bary,
                                                                       int32_t* __restrict__ feature)
{
    __shared__ FaceRec tile[kTile];
    static_assert(kTile == kThreads, "one record per thread and step");
    const int n = blockIdx.x * kThreads + threadIdx.x;
    const bool live = n < a.N;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) load_query(a, n, qx, qy, qz);
    float best = INFINITY;
    int best_f = -1;
    for (int base = 0; base < a.F; base += kTile) {
        const int count = min(kTile, a.F - base);
        if ((int)threadIdx.x < count) tile[threadIdx.x] = recs[base + threadIdx.x];
        __syncthreads();
        for (int j = 0; j < count; ++j) {
            const float d2 = pair_dist2(tile[j], qx, qy, qz);
            if (wins(d2, base + j, best, best_f)) { best = d2; best_f = base + j; }
        }
        __syncthreads();
    }
    if (live) store_result(recs, n, qx, qy, qz, best_f, dist2, face_id, bary, feature);
}

__global__ void __launch_bounds__(kThreads) pseudonormal_sign_kernel(Query a, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                     const int32_t* __restrict__ face_id, const float* __restrict__ bary,
                                                                     const int32_t* __restrict__ feature, const float* __restrict__ face_normals,
                                                                     const float* __restrict__ edge_normals, const float* __restrict__ vertex_normals,
                                                                     float* __restrict__ sign)
{
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n < a.N) sign[n] = pseudonormal_sign(a, n, vertices, faces, face_id, bary, feature, face_normals, edge_normals, vertex_normals);
}
#endif  // AG_MESH_QUERY_HOST_ONLY

}  // namespace meshq
}  // namespace ag

#ifndef AG_MESH_QUERY_HOST_ONLY
using namespace ag;
using namespace ag::meshq;

// the default walk ("Closest point on a mesh")
static constexpr int kDefaultWalk = 1;

static int check_query(const AgMeshQueryArgs* q, const char* what, Query& a)
{
    if (!q) { set_error("%s: null argument struct", what); return AG_ERR_INVALID_ARGUMENT; }
    if (q->N < 0 || q->V < 0 || q->F < 0) { set_error("%s: bad sizes N = %d, V = %d, F = %d", what, q->N, q->V, q->F); return AG_ERR_INVALID_ARGUMENT; }
    a.N = q->N; a.V = q->V; a.F = q->F; a.gx = q->gx; a.gy = q->gy; a.gz = q->gz;
    a.points = q->points; a.axis_x = q->axis_x; a.axis_y = q->axis_y; a.axis_z = q->axis_z;
    if (q->N == 0) return AG_OK;
    if (!q->points) {
        if (!q->axis_x || !q->axis_y || !q->axis_z) { set_error("%s: neither points nor three grid axes", what); return AG_ERR_INVALID_ARGUMENT; }
        if (q->gx < 1 || q->gy < 1 || q->gz < 1 || (long long)q->gx * q->gy * q->gz != (long long)q->N) {
            set_error("%s: grid %d x %d x %d does not have N = %d nodes", what, q->gx, q->gy, q->gz, q->N);
            return AG_ERR_INVALID_ARGUMENT;
        }
    }
    if (q->F > 0 && (!q->vertices || !q->faces)) { set_error("%s: null mesh", what); return AG_ERR_INVALID_ARGUMENT; }
    if (!q->face_id || !q->bary) { set_error("%s: null face_id or bary", what); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

extern "C" size_t ag_mesh_closest_point_workspace_bytes(int32_t F)
{
    if (F < 0) return 0;
    return align_up((size_t)F * sizeof(FaceRec), 256) + 256;
}

extern "C" int ag_mesh_closest_point(const AgMeshQueryArgs* q, void* stream)
{
    Query a;
    if (int rc = check_query(q, "ag_mesh_closest_point", a)) return rc;
    if (q->N == 0) return AG_OK;
    if (!q->dist2) { set_error("ag_mesh_closest_point: null dist2"); return AG_ERR_INVALID_ARGUMENT; }
    if (q->walk < 0 || q->walk > 2) { set_error("ag_mesh_closest_point: walk must be 0, 1 or 2, got %d", q->walk); return AG_ERR_INVALID_ARGUMENT; }
    if (q->F > 0 && (!q->workspace || q->workspace_bytes < ag_mesh_closest_point_workspace_bytes(q->F))) {
        set_error("ag_mesh_closest_point: workspace too small");
        return AG_ERR_SCRATCH_TOO_SMALL;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FaceRec* recs = q->F > 0 ? reinterpret_cast<FaceRec*>(aligned_base(q->workspace)) : nullptr;
    if (q->F > 0) {
        hipLaunchKernelGGL(face_record_kernel, dim3((unsigned)((q->F + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, q->vertices, q->faces, q->V,
                           q->F, recs);
        if (int rc = check_hip(hipGetLastError(), "face_record_kernel")) return rc;
    }
    const dim3 grid((unsigned)(((long long)q->N + kThreads - 1) / kThreads));
    if ((q->walk ? q->walk : kDefaultWalk) == 1) {
        hipLaunchKernelGGL(closest_point_uniform_kernel, grid, dim3(kThreads), 0, s, a, recs, q->dist2, q->face_id, q->bary, q->feature);
        return check_hip(hipGetLastError(), "closest_point_uniform_kernel");
    }
    hipLaunchKernelGGL(closest_point_tiled_kernel, grid, dim3(kThreads), 0, s, a, recs, q->dist2, q->face_id, q->bary, q->feature);
    return check_hip(hipGetLastError(), "closest_point_tiled_kernel");
}

extern "C" int ag_mesh_pseudonormal_sign(const AgMeshQueryArgs* q, const float* face_normals, const float* edge_normals,
                                         const float* vertex_normals, float* sign, void* stream)
{
    Query a;
    if (int rc = check_query(q, "ag_mesh_pseudonormal_sign", a)) return rc;
    if (q->N == 0) return AG_OK;
    if (!q->feature || !sign || (q->F > 0 && (!face_normals || !edge_normals)) || (q->V > 0 && !vertex_normals)) {
        set_error("null pointer in ag_mesh_pseudonormal_sign");
        return AG_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(pseudonormal_sign_kernel, dim3((unsigned)(((long long)q->N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a, q->vertices, q->faces, q->face_id, q->bary, q->feature, face_normals, edge_normals,
                       vertex_normals, sign);
    return check_hip(hipGetLastError(), "pseudonormal_sign_kernel");
}
#endif  // AG_MESH_QUERY_HOST_ONLY
