/*
 * ag_subject_maps.h — C ABI of the per-subject asset kernels (libag_hip.so): from a triangle mesh to the canonical front|back
 * position / normal maps, the per-point skinning weights and the k-NN scale initialiser.
 *
 * They replace, for the SMPL-X-as-template branch, what the reference computes with an OpenGL context, pytorch3d and OpenCV:
 *   Renderer.render() with the `vertex_attribute` shader, orthographic     utils/renderer/renderer_gl.py:363-375,465-475,525-549
 *   the two canonical views and their row / column flips                   gen_data/gen_pos_maps.py:93-124
 *   interpolate_lbs                                                        gen_data/gen_pos_maps.py:24-39,126-134
 *   knn_points(K = 4)[..., 1:].mean(-1)                                    gaussians/gaussian_model.py:170-171
 * Same conventions as ag_raster.h: device pointers, fp32 / int32, contiguous, 0 on success, ag_last_error() on failure.
 * Every result is a pure function of its inputs (bit-identical between runs): no float atomic is used anywhere, and the integer
 * atomics that are used (a 64-bit minimum, counters) commute.
 */
#ifndef AG_SUBJECT_MAPS_H
#define AG_SUBJECT_MAPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Orthographic rasterizer: per pixel the winning face and its barycentric coordinates.
 *
 * Vertex stage (fp32, in this operand order, no contraction):
 *     n_k = ((view[4k] * x + view[4k+1] * y) + view[4k+2] * z) + view[4k+3]        k = 0, 1, 2      (world -> NDC)
 *     wx = (n_0 + 1) * (0.5 W),  wy = (n_1 + 1) * (0.5 H),  depth = n_2                               (window space, y UP)
 * These fp32 window coordinates ARE the vertices that get rasterized (the "snapping" step of a hardware rasterizer); everything
 * below is a function of them.  No clipping against the depth range: `view` maps the mesh where the caller wants it.
 *
 * Coverage: sample points are the pixel centres (gx + 0.5, gy + 0.5).  A face whose window-space signed area is 0 is dropped; a
 * clockwise one is dropped when `cull` is set and otherwise rasterized with its second and third corner exchanged.  Each edge
 * function is evaluated from the edge's end points in a canonical order (lexicographic in (wx, wy)) and negated when the face
 * walks the edge the other way, so the two faces that share an edge see exactly opposite values; a centre with edge value 0 belongs
 * to the face for which the edge is a left edge (walked downwards) or a top edge (horizontal, walked towards -x): the top-left rule.
 * Barycentrics: b0 = E_12 / A, b1 = E_20 / A with A = (E_12 + E_20) + E_01, b2 = (1 - b0) - b1, in the face's own corner order.
 * Depth = (b0 * d0 + b1 * d1) + b2 * d2.
 *
 * Tie rules: depth test "less"; equal depth keeps the LOWER face index (draw order).  Implemented as one 64-bit atomic minimum
 * per covered sample on (order-preserving bits of depth << 32 | face index): a minimum commutes, so the winner does not depend on
 * the order in which faces arrive.  A second pass recomputes the winner's barycentrics with the same device function.
 *
 * Output addressing: window pixel (gx, gy) is written to row r = flip_rows ? H-1-gy : gy (the reference's data[::-1]) and column
 * c = mirror_cols ? W-1-gx : gx (cv.flip(., 1)) of a target whose rows are `out_stride` pixels long, at column `out_col0 + c`:
 * the front and the back view land in the two halves of one [S, 2S] canvas.  Empty pixels: face_id -1, bary 0.
 */
typedef struct AgMeshRasterArgs {
    int32_t V;                  /* vertices */
    int32_t F;                  /* faces */
    int32_t W;                  /* target of this view, 1 <= W, H <= 16384 */
    int32_t H;
    int32_t cull;               /* 1: drop faces that are clockwise in window space (y up) */
    int32_t flip_rows;
    int32_t mirror_cols;
    int32_t out_col0;           /* first canvas column of this view */
    int32_t out_stride;         /* canvas row length in pixels, >= out_col0 + W */
    int32_t reserved;
    float view[12];             /* row-major 3 x 4, world -> NDC */
    const float* vertices;      /* [V,3] */
    const int32_t* faces;       /* [F,3]; a face with an index outside [0, V) is dropped */
    int32_t* face_id;           /* [H, out_stride] */
    float* bary;                /* [H, out_stride, 3] */
    void* workspace;            /* >= ag_mesh_rasterize_ortho_workspace_bytes(W, H) */
    size_t workspace_bytes;
} AgMeshRasterArgs;

size_t ag_mesh_rasterize_ortho_workspace_bytes(int32_t W, int32_t H);
int ag_mesh_rasterize_ortho(const AgMeshRasterArgs* args, void* stream);

/*
 * Attribute resolve: out[row, c] = (b0 * a[f0, c] + b1 * a[f1, c]) + b2 * a[f2, c]   (this order, no contraction), with
 * (f0, f1, f2) = faces[face_id[p]], (b0, b1, b2) = bary[p].
 *   dense      (pix == NULL): rows = n_pixels, p = row          -> out [n_pixels, C]; pixels with face_id < 0 are exactly 0
 *   compacted  (pix != NULL): rows = N,        p = pix[row]     -> out [N, C]; a row whose pixel is empty or out of range is 0
 * No reduction across threads; needs no workspace (the query returns 0 and exists for symmetry with the other entry points).
 */
size_t ag_mesh_resolve_attribute_workspace_bytes(int32_t n_pixels, int32_t N, int32_t C);
int ag_mesh_resolve_attribute(const int32_t* face_id /*[n_pixels]*/, const float* bary /*[n_pixels,3]*/, const int32_t* faces /*[F,3]*/,
                              const float* attribute /*[V,C]*/, int32_t V, int32_t F, int32_t C, int32_t n_pixels,
                              const int32_t* pix /*[N] or NULL*/, int32_t N, float* out, void* stream);

/*
 * Exact k-nearest-neighbour distances of a point set to itself (K = 4 including the point itself, as knn_points(K = 4)):
 *     d(i, j) = ((xi - xj)^2 + (yi - yj)^2) + (zi - zj)^2          (fp32, this order, no contraction)
 * For each point the 4 smallest d over ALL j (j = i included, value 0) are kept in ascending order; the smallest is dropped --
 * with exact duplicates that drops ONE zero, as the reference's [..., 1:] does -- and
 *     mean_dist2[i] = ((d1 + d2) + d3) / 3,        dist2[i] = (d1, d2, d3)   (optional)
 * Ties: only distance VALUES are kept, so which of two equidistant neighbours is "the" neighbour never matters.
 * Search: uniform grid of `cell`-sized cells over the bounding box [origin, origin + dims * cell): a counting pass (integer
 * atomics), an offsets pass, a scatter, then per point rings of cells of growing Chebyshev radius until the 4th distance is not
 * larger than the squared distance from the point to the boundary of the searched block or the block covers the grid.  That distance
 * is first shortened by cell * (1e-3 + 6 u max(dims)) + 4 u max_k(|origin_k| + dims_k * cell), u = 2^-24: twice the rounding of the cell
 * assignment (p - o) * (1 / cell) and of the block's planes o + k * cell, so "exact" holds for every admitted grid.  The result does not depend on `cell`, only the time does.
 * N >= 4; dims[k] >= 1; dims[0] * dims[1] * dims[2] <= 2^24.  Points outside the box are assigned to the nearest border cell
 * (still exact: the closing distance is computed from the point's own position).
 */
size_t ag_knn_mean_dist2_workspace_bytes(int32_t N, int32_t n_cells);
int ag_knn_mean_dist2(const float* points /*[N,3]*/, int32_t N, const float* origin /*host [3]*/, float cell, const int32_t* dims /*host [3]*/,
                      float* mean_dist2 /*[N]*/, float* dist2 /*[N,3] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_SUBJECT_MAPS_H */
