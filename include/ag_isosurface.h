/*
 * ag_isosurface.h — C ABI of iso-surface extraction (libag_hip.so): a scalar volume on a regular grid -> triangle mesh (marching cubes).
 *
 * It replaces what the reference's utils/recon_util.recon_mesh (recon_util.py:51-75) asks of skimage.measure.marching_cubes on the
 * host.  The result is DEFINED here, not by skimage: the case table is generated (csrc/gen_isosurface_table.py ->
 * csrc/ag_isosurface_table.h) from a rule that reads each cube face on its own, so the mesh is watertight; no comparison with skimage
 * was possible (it is not installed anywhere this project is built).
 *
 * Same conventions as ag_raster.h: device pointers unless marked HOST, fp32, contiguous, 0 on success, ag_last_error() on failure.
 * Every position is stated as fp32 operations, each rounded on its own, in the order written (no contraction; the file is compiled
 * with -ffp-contract=off).  No atomics and no order decided by timing: every output is a pure function of the inputs and bit-identical
 * between calls.  No workgroup waits on another (the scans are multi-kernel: block sums, scan of the sums, add back).
 *
 * Definition.  `volume` is [X, Y, Z] float32, row-major: node (i, j, k) has linear index n = (i * Y + j) * Z + k.
 *   Inside.     A node is inside iff value >= iso (the reference's SDFs and occupancies are larger inside).
 *   Cells.      The cell with low node (i, j, k), i < X - 1, j < Y - 1, k < Z - 1, has corners c = dx + 2 dy + 4 dz at nodes
 *               (i + dx, j + dy, k + dz); bit c of its case is set iff that corner is inside.  A cell is PROCESSED iff all eight
 *               corner values are finite and, when `mask` ([X, Y, Z] bytes) is given, all eight mask bytes are non-zero.  The mask
 *               rule is this project's: the reference never passes a mask in its template stage, and skimage's rule for partially
 *               masked cubes could not be checked.
 *   Vertices.   One per grid edge (n, axis) -- from node n to its upper neighbour along `axis`, which must be in the grid -- whose end
 *               values a (at n) and b straddle, (a >= iso) != (b >= iso), and which touches at least one processed cell.  Order:
 *               ascending key 3 * n + axis.  Position, with (idx_0, idx_1, idx_2) = (i, j, k) of n:
 *                   t = (iso - a) / (b - a)
 *                   coordinate d == axis:  origin_d + ((float)idx_d + t) * spacing_d
 *                   the other two:         origin_d + (float)idx_d * spacing_d
 *   Faces.      int32 vertex indices, three per triangle: processed cells in ascending low-node index n, and within a cell the
 *               triangles of its case in the order of csrc/ag_isosurface_table.h (loops in ascending order of their lowest edge id).
 *               Cube edge e = 4 axis + (u + 2 v) of a cell is the grid edge along `axis` whose low node has the two other
 *               coordinates raised by (u, v), in ascending axis order.  Triangles are wound counter-clockwise seen from OUTSIDE
 *               (the side of lower values), the convention of synth._lattice_surface and mesh_query.signed_distance.
 *   Degenerate  A node whose value equals iso is inside and gives t = 0 on its edges towards outside nodes: their vertices coincide
 *   triangles.  and triangles of zero area appear.  They are KEPT: the surface stays a manifold in its connectivity.
 *
 * Limits: X, Y, Z >= 2; 3 * X * Y * Z < 2^31 (vertex keys and indices are int32; (256, 256, 128) is 2.5e7); spacing finite and
 * positive, origin and iso finite.  Anything else returns AG_ERR_INVALID_ARGUMENT with a message before any launch.
 */
#ifndef AG_ISOSURFACE_H
#define AG_ISOSURFACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a volume of X x Y x Z nodes (about 17 bytes per node); 0 if the sizes are outside the limits. */
size_t ag_isosurface_workspace_bytes(int32_t X, int32_t Y, int32_t Z);

/*
 * First half: classifies the cells, flags the grid edges that carry a vertex, and scans both (edge flags -> vertex index of every
 * edge, triangles per cell -> first face of every cell) in `workspace`.  Leaves counts[0] = V (vertices) and counts[1] = F (faces) in
 * two device words; the caller reads them (its one synchronisation), allocates, and calls ag_isosurface_emit with the same volume,
 * mask, sizes, iso and workspace.  `mask`: [X, Y, Z] bytes or NULL.  Only enqueues work on `stream`.
 * AG_ERR_SCRATCH_TOO_SMALL if workspace_bytes < ag_isosurface_workspace_bytes(X, Y, Z).
 */
int ag_isosurface_count(const float* volume /*[X,Y,Z]*/, const uint8_t* mask /*[X,Y,Z] or NULL*/, int32_t X, int32_t Y, int32_t Z, float iso,
                        void* workspace, size_t workspace_bytes, int32_t* counts /*[2]: V, F*/, void* stream);

/*
 * Second half: writes the V vertices and F faces defined above.  `workspace` must hold what ag_isosurface_count left for the same
 * volume, mask, sizes and iso.  V and F must be the counts it produced: this call reads them and the sizes back from the workspace (one
 * 20-byte copy, which waits for `stream`) and returns AG_ERR_INVALID_ARGUMENT before any launch when they differ, so a buffer allocated for
 * other counts is never written.  `vertices` may be NULL when V = 0 and `faces` when F = 0.  `spacing`, `origin`: HOST [3].
 */
int ag_isosurface_emit(const float* volume /*[X,Y,Z]*/, int32_t X, int32_t Y, int32_t Z, float iso, const float* spacing /*host [3]*/,
                       const float* origin /*host [3]*/, const void* workspace, size_t workspace_bytes, float* vertices /*[V,3]*/, int32_t V,
                       int32_t* faces /*[F,3]*/, int32_t F, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_ISOSURFACE_H */
