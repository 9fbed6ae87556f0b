/*
 * ag_mesh_query.h — C ABI of the closest-point-on-a-mesh query (libag_hip.so): for every query point the exact closest point of a
 * triangle mesh (squared distance, face, barycentrics, the feature it lies on) and the pseudonormal sign of the query.
 *
 * They replace what the reference computes with pytorch3d's point-to-face distance and libigl's signed distance:
 *   nearest_face_pytorch3d                                   utils/posevocab_custom_ops/nearest_face.py:30-61
 *   interpolate_lbs                                          gen_data/gen_pos_maps.py:24-39
 *   calc_blending_weight(method = 'barycentric')             utils/smpl_util.py:46-53
 *   igl.signed_distance over the grid of the weight volume   gen_data/gen_weight_volume.py:152-162
 * Same conventions as ag_subject_maps.h: device pointers, fp32 / int32, contiguous, 0 on success, ag_last_error() on failure.
 * No atomics of any kind and no reduction across threads: every result is a pure function of its inputs, two calls agree bit for bit.
 * The interpolated attributes  sum_k b_k attr[faces[f][k]]  are ag_mesh_resolve_attribute (ag_subject_maps.h) in dense mode on
 * (face_id, bary); this header adds no second copy of it.
 */
#ifndef AG_MESH_QUERY_H
#define AG_MESH_QUERY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_MESH_QUERY_FACE_TILE 256     /* faces staged in LDS per step of the tiled walk */

/*
 * Closest point.  Every operation below is one individually rounded fp32 operation in the written operand order (the file is compiled
 * without contraction); (x . y) stands for (x_0 * y_0 + x_1 * y_1) + x_2 * y_2.
 *
 * Face record, once per face f with corners (v0, v1, v2) = vertices[faces[f]]:
 *     e0 = v1 - v0,  e1 = v2 - v0,  e2 = e1 - e0
 *     a = (e0 . e0),  b = (e0 . e1),  c = (e1 . e1),  h = (e2 . e2)
 *     ia = a > 0 ? 1 / a : 0,   ic = c > 0 ? 1 / c : 0,   ih = h > 0 ? 1 / h : 0          (correctly rounded divisions)
 *     det = a * c - b * b,      idet = det > 0 ? 1 / det : 0
 * A face with an index outside [0, V) has no record and never wins.
 *
 * Pair (query q, face f):
 *     D = v0 - q,   d = (e0 . D),   e = (e1 . D),   det = a * c - b * b
 *     sn = b * e - c * d,   tn = b * d - a * e,   inside = sn >= 0 && tn >= 0 && sn + tn <= det && det > 0
 *     r(s, t)  = (D + s * e0) + t * e1      per component: the vector from q to the point v0 + s e0 + t e1 of the face's plane
 *     d2(s, t) = (r . r)
 *     clamp(x) = min(max(x, 0), 1)
 *   four candidates, each a point OF the closed triangle, as (b0, b1, b2; s, t):
 *     0  interior   s = sn * idet, t = tn * idet                    (max((1 - s) - t, 0), s, t)          only when `inside`
 *     1  edge v0v1  s = clamp(0 - d * ia), t = 0                    (1 - s, s, 0)
 *     2  edge v1v2  u = clamp(((a - b) + (d - e)) * ih), s = 1 - u, t = u      (0, 1 - u, u)
 *     3  edge v2v0  s = 0, t = clamp(0 - e * ic)                    (1 - t, 0, t)
 *   The face's answer is the candidate of smallest d2, the FIRST of them in the order 0, 1, 2, 3 on equality.  Either the projection
 *   of q lies in the triangle and is the closest point, or the closest point lies on an edge: the minimum over the four is the exact
 *   closest point of the closed triangle, and no rounding of `inside` can return a point off the triangle.
 *   feature: 0 for candidate 0; for an edge candidate with parameter p (s, u, t): the edge's code 1 / 2 / 3 when 0 < p < 1, the
 *   code of the vertex it was clamped to otherwise (4 = v0, 5 = v1, 6 = v2: edge 1 -> 4 | 5, edge 2 -> 5 | 6, edge 3 -> 4 | 6).
 *   A zero-area face: det <= 0 or idet = 0 makes candidate 0 at best the corner v0, a zero-length edge has parameter 0; nothing
 *   divides by zero, the barycentrics are >= 0 and sum to 1 (within 2^-23), the answer is the closest point of the face's edges.
 *
 * Over the faces: a face wins if  d2 < best || (d2 == best && f < best_f): the result does not depend on the order in which faces
 * are visited.  The walk keeps only (best d2, best f); the winner's candidate is evaluated once more, by the same operations, to
 * write bary and feature.  F == 0 or no face with a record: face_id = -1, dist2 = +inf, bary = 0, feature = 0.
 *
 * Queries: `points` [N, 3], or -- `points` NULL -- the nodes of a grid given by three axes: N = gx * gy * gz and query
 * n = (i * gy + j) * gz + k is (axis_x[i], axis_y[j], axis_z[k]): the caller states the coordinates, the kernel derives none.
 *
 * walk: 0 = the default below; 1 = every lane walks the record array with a wave-uniform index (records reach the wave through the
 * scalar cache); 2 = workgroups stage AG_MESH_QUERY_FACE_TILE records at a time in LDS and read them back as broadcast 16-byte
 * reads.  Same operations per pair, bit-identical results; the default is the faster one ("Closest point on a mesh").
 */
typedef struct AgMeshQueryArgs {
    int32_t N;                  /* queries */
    int32_t V;                  /* vertices */
    int32_t F;                  /* faces */
    int32_t gx, gy, gz;         /* grid mode only */
    int32_t walk;
    int32_t reserved;
    const float* points;        /* [N,3], or NULL for grid mode */
    const float* axis_x;        /* [gx] */
    const float* axis_y;        /* [gy] */
    const float* axis_z;        /* [gz] */
    const float* vertices;      /* [V,3] */
    const int32_t* faces;       /* [F,3]; a face with an index outside [0, V) is skipped */
    float* dist2;               /* [N] */
    int32_t* face_id;           /* [N] */
    float* bary;                /* [N,3], in the face's own corner order: closest point = b0 v0 + b1 v1 + b2 v2 */
    int32_t* feature;           /* [N] or NULL */
    void* workspace;            /* >= ag_mesh_closest_point_workspace_bytes(F): the face records */
    size_t workspace_bytes;
} AgMeshQueryArgs;

size_t ag_mesh_closest_point_workspace_bytes(int32_t F);
int ag_mesh_closest_point(const AgMeshQueryArgs* args, void* stream);

/*
 * Pseudonormal sign of each query with respect to its closest point (Baerentzen & Aanaes 2005):
 *     c = (b0 * v0 + b1 * v1) + b2 * v2   per component (the resolve's order),   w = q - c
 *     n = face_normals[f]                          feature 0
 *         edge_normals[f][feature - 1]             feature 1..3  (edges v0v1, v1v2, v2v0)
 *         vertex_normals[faces[f][feature - 4]]    feature 4..6
 *     sign = 1 if (w . n) > 0, -1 if (w . n) < 0, else 0;   0 where face_id < 0
 * The three tables are inputs, built once per mesh by the caller (mesh_query.pseudonormals): unit face normals, per edge the sum
 * of the unit normals of the faces that share it (a border edge: its own face's), angle-weighted vertex normals.  Positive =
 * outside for a closed mesh wound counter-clockwise seen from outside.  Exact for closed, consistently wound manifold meshes; with
 * several intersecting components it is the sign with respect to the closest face's component.  Parity with libigl's
 * signed_distance is not claimed (libigl is not available to this package).  Queries as in AgMeshQueryArgs (points or axes).
 */
int ag_mesh_pseudonormal_sign(const AgMeshQueryArgs* query /* N, V, F, points | axes, vertices, faces, face_id, bary, feature read */,
                              const float* face_normals /*[F,3]*/, const float* edge_normals /*[F,3,3]*/,
                              const float* vertex_normals /*[V,3]*/, float* sign /*[N]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_MESH_QUERY_H */
