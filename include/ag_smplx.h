/*
 * ag_smplx.h — C ABI of the SMPL-X body-model forward (libag_hip.so), fp32, B poses of one subject per call.
 *
 * the producer of `cano2live_jnt_mats` (what AvatarNet.transform_cano2live skins the Gaussians with)
 * is the dataset-side SMPL-X forward -- three `smpl_model.forward` calls per item (live, canonical, live without root:
 * dataset/dataset_mv_rgb.py:118-143) followed by `live.A @ inv(cano.A)` (:170-171).  The reference runs it on the CPU in
 * the data loader (smplx/body_models.py:1114-1290 -> smplx/lbs.py:152-246); here the B poses go through three launches
 * that read the 61-MB pose-corrective basis ONCE for all of them.
 *
 * Replaces, stage by stage (smplx/lbs.py):
 *   :208  v_shaped = v_template + blend_shapes(betas ++ expression, shapedirs ++ expr_dirs)      (ag_smplx_forward, kernel 1)
 *   :212  J = vertices2joints(J_regressor, v_shaped)           (kernel 2, through the per-model fold of ag_smplx_prepare)
 *   :218  rot_mats = batch_rodrigues(pose)  (:299-330, incl. its `+ 1e-8` inside the norm)        (kernel 2)
 *   :221  pose_feature = (rot_mats[1:] - I).view(-1)                                              (kernel 2)
 *   :235  J_transformed, A = batch_rigid_transform(rot_mats, J, parents)  (:347-405)              (kernel 2)
 *   :223  pose_offsets = pose_feature @ posedirs;  :233 v_posed = pose_offsets + v_shaped         (kernel 3)
 *   :239-248  T = W @ A;  verts = (T @ [v_posed, 1])[:3]                                          (kernel 3)
 *   body_models.py:1272-1275  `+ transl` on vertices, joints and A[:, :3, 3] AFTER the skinning   (kernels 2, 3)
 * Device pointers, contiguous row-major; 0 on success (codes in ag_raster.h).
 */
#ifndef AG_SMPLX_H
#define AG_SMPLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The constant arrays of one body model, as smplx/body_models.py:237-260,1049-1073 registers them. */
typedef struct AgSmplxModel {
    int32_t V;                 /* vertices (10475 for SMPL-X) */
    int32_t J;                 /* joints of the kinematic tree (55), J <= 64 */
    int32_t NB;                /* shape + expression coefficients in use (10 + 10) */
    int32_t reserved;
    const float* v_template;   /* [V][3] */
    const float* shapedirs;    /* [V][3][NB]  = cat(shapedirs[..., :num_betas], expr_dirs) (body_models.py:1233) */
    const float* posedirs;     /* [9 (J-1)][3 V]  (body_models.py:248-252: reshape(-1, P).T) */
    const float* J_regressor;  /* [J][V] dense */
    const int32_t* parents;    /* [J], parents[0] = -1, parents[j] < j */
    const float* lbs_weights;  /* [V][J] */
    const float* joint_template; /* [J][3]      = J_regressor . v_template   } written once per model by ag_smplx_prepare */
    const float* joint_dirs;     /* [J][3][NB]  = J_regressor . shapedirs    } (device memory owned by the caller)        */
} AgSmplxModel;

/* Folds the joint regressor through the (linear) shape model: lbs.py:208-212 computes J_regressor . (v_template + shapedirs . c)
 * per call, a 10475-long reduction per joint; J_regressor . v_template + (J_regressor . shapedirs) . c is the same sum
 * re-associated (difference ~1e-7 of the joint positions).  joint_template [J][3], joint_dirs [J][3][NB]: device outputs;
 * the model's own joint_template / joint_dirs fields are not read by this call. */
int ag_smplx_prepare(const AgSmplxModel* m, float* joint_template, float* joint_dirs, void* stream);

/* Floats of workspace ag_smplx_forward needs for B poses (v_shaped, un-translated joint matrices, pose features). */
size_t ag_smplx_workspace_floats(const AgSmplxModel* m, int32_t B);

/*
 * B poses of one subject.  shape_components [B][NB]; full_pose [B][J][3] axis-angle (pose mean already added,
 * body_models.py:1203-1213); transl [B][3] or NULL.
 * Outputs: vertices [B][V][3]; joints [B][J][3] (posed joint locations, the first J rows of the reference's `joints`);
 * A [B][J][4][4] (the reference's `A`, relative to the rest pose, translation included).  workspace: device floats.
 */
int ag_smplx_forward(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* transl,
                     float* vertices, float* joints, float* A, float* workspace, size_t workspace_floats, void* stream);

/*
 * Backward of ag_smplx_forward for its outputs A and joints (the kinematic chain; the vertices and the vertex key points have no
 * backward here).  dL_dA [B][J][4][4] (as returned, transl included; row 3 is not read) and dL_djoints [B][J][3]: either may be NULL
 * (no gradient).  Writes dL_dfull_pose [B][J][3] (Rodrigues with the reference's `+ 1e-8` inside the norm, so the zero pose has its
 * finite gradient), dL_dtransl [B][3] when not NULL (the gradient is the same whether or not the forward had a transl), and
 * dL_dshape_components [B][NB] when NB > 0, through the folded joint_dirs of ag_smplx_prepare.  One wave per pose; deterministic.
 */
int ag_smplx_backward(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* dL_dA,
                      const float* dL_djoints, float* dL_dfull_pose, float* dL_dtransl, float* dL_dshape_components, void* stream);

/* v_shaped [B][V][3] = v_template + shapedirs . shape_components alone (body_models.py:1277-1279 `return_shaped`, where the
 * reference passes the betas without the expression: the caller zeroes those components). */
int ag_smplx_shape(const AgSmplxModel* m, int32_t B, const float* shape_components, float* v_shaped, void* stream);

/* out[i] = a[i] @ inverse(b[i % b_batch]) for n row-major 4x4 matrices (dataset_mv_rgb.py:170-171: cano2live_jnt_mats =
 * live.A @ inv(cano.A), and the same canonical matrices again for the pose without root: n = 2 J, b_batch = J). */
int ag_mat4_mul_inverse(float* out, const float* a, const float* b, int32_t n, int32_t b_batch, void* stream);
/* Its backward: dL_da[i] = dL_dout[i] inverse(b)^T;  dL_db[k] = -inverse(b_k)^T (sum over i % b_batch == k of a[i]^T dL_dout[i]) inverse(b_k)^T,
 * summed in ascending i.  Either output may be NULL (not computed); n must be a multiple of b_batch. */
int ag_mat4_mul_inverse_backward(float* dL_da, float* dL_db, const float* dL_dout, const float* a, const float* b, int32_t n, int32_t b_batch,
                                 void* stream);

/* Barycentric key points (vertex picks and face landmarks: vertex_joint_selector.py:72-76, lbs.py:108-149):
 * out[b][k] = sum_t w[k][t] * vertices[b][idx[k][t]], t < 3.  idx [K][3] int32, w [K][3]. */
int ag_smplx_keypoints(float* out, const float* vertices, const int32_t* idx, const float* w, int32_t B, int32_t V, int32_t K, void* stream);

/*
 * The backward of the vertex path: `vertices`, the vertex key points and `v_shaped`.  Notation of lbs.py:223-246:
 *   v_posed = v_shaped + pose_feature . posedirs;  T_v = sum_j W[v][j] A_skin[j]  (A_skin: A before `transl` is added);
 *   vertices = T_v[:3,:3] v_posed + T_v[:3,3] (+ transl).
 * Five additive entry points; ag_smplx_forward and ag_smplx_backward keep their signatures and their bits.  No float atomics anywhere:
 * every sum below has a fixed order, two calls give the same bits.
 */

/* Floats of `saved` that ag_smplx_forward_keep fills for B poses: v_posed [B][V][3] | A_skin [B][J][12] (rows 0-2 of the 4x4). */
size_t ag_smplx_saved_floats(const AgSmplxModel* m, int32_t B);

/* ag_smplx_forward (same arguments, same three launches, same output bits) that also keeps what ag_smplx_vertex_backward reads, so that
 * the 61-MB basis is not streamed a second time to rebuild v_posed.  saved: device floats, at least ag_smplx_saved_floats(m, B). */
int ag_smplx_forward_keep(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* transl,
                          float* vertices, float* joints, float* A, float* workspace, size_t workspace_floats, float* saved,
                          size_t saved_floats, void* stream);

/* Backward of ag_smplx_keypoints (vertex_joint_selector.py:72-76, lbs.py:108-149) with respect to the vertices:
 * dL_dvertices [B][V][3] is ZEROED by the call, then dL_dvertices[b][idx[k][t]] += w[k][t] dL_dkeypoints[b][k].  Vertex ids may repeat
 * (landmark triangles share vertices): the first entry (k, t) that names a vertex gathers every entry with the same id in ascending
 * 3 k + t and stores once.  Ids outside [0, V) are skipped.  K <= 1024.  No pointer may be NULL unless K = 0. */
int ag_smplx_keypoints_backward(float* dL_dvertices, const float* dL_dkeypoints, const int32_t* idx, const float* w, int32_t B, int32_t V,
                                int32_t K, void* stream);

/* Floats of workspace ag_smplx_vertex_backward needs (dL/dv_posed, one slab per 64 vertices, one slab per 256 coordinates). */
size_t ag_smplx_vertex_backward_workspace_floats(const AgSmplxModel* m, int32_t B);

/*
 * Backward of lbs.py:223-246 (+ body_models.py:1274) for g = dL_dvertices [B][V][3], from `saved` of ag_smplx_forward_keep:
 *   dL/dv_posed[v] = T_v[:3,:3]^T g[v]                                                       (kept in the workspace)
 *   dL_dA_skin [B][J][12]   = sum_v W[v][j] g[v] (x) [v_posed[v]; 1]      hand to ag_smplx_backward_full
 *   dL_dtransl [B][3]       = sum_v g[v]                                   (the same whether or not the forward had a transl)
 *   dL_dfeat [B][9 (J-1)]   = posedirs . dL/dv_posed                       (lbs.py:223 transposed; may be NULL only when J = 1)
 *   dL_dshape_components [B][NB] = shapedirs^T . dL/dv_posed               (lbs.py:208 transposed, the DIRECT term: v_shaped enters v_posed;
 *                                                                           the path through the rest joints is ag_smplx_backward_full's)
 * All outputs are overwritten.  Order of the sums: over vertices, 64 consecutive vertices in ascending order per slab, then the slabs
 * in 16 running sums (slab index mod 16, each ascending) added in ascending order of the remainder; over the 3 V coordinates of a
 * posedirs row (read once for up to four poses), 1024 running sums (coordinate mod 1024, ascending), then lanes by xor-shuffle 32, 16,
 * .. 1, then the 16 waves in ascending order; over the coordinates for the shape basis, 256 per slab (lanes by xor-shuffle, four waves
 * as (w0 + w1) + (w2 + w3)), then the slabs as above.
 */
int ag_smplx_vertex_backward(const AgSmplxModel* m, int32_t B, const float* saved, const float* dL_dvertices, float* dL_dA_skin,
                             float* dL_dfeat, float* dL_dtransl, float* dL_dshape_components, float* workspace, size_t workspace_floats,
                             void* stream);

/* Backward of ag_smplx_shape: dL_dshape_components [B][NB] = shapedirs^T . dL_dv_shaped [B][V][3] (the shape-basis kernel and sum order
 * of ag_smplx_vertex_backward).  workspace: at least ag_smplx_shape_backward_workspace_floats(m, B) device floats. */
size_t ag_smplx_shape_backward_workspace_floats(const AgSmplxModel* m, int32_t B);
int ag_smplx_shape_backward(const AgSmplxModel* m, int32_t B, const float* dL_dv_shaped, float* dL_dshape_components, float* workspace,
                            size_t workspace_floats, void* stream);

/*
 * ag_smplx_backward extended by what the vertex path hands over; each of the four may be NULL (absent):
 *   dL_dA_skin [B][J][12]: added to dL_dA's rows 0-2 everywhere except in dL_dtransl (the skinning read the matrices before transl);
 *   dL_dfeat [B][J-1][9]: a gradient on the local rotations R[1:] (lbs.py:221 pose_feature = R[1:] - I), added ahead of the Rodrigues
 *   backward; dL_dtransl_add [B][3] and dL_dshape_components_add [B][NB]: added last to the two outputs of the same name.
 * Outputs and everything else as ag_smplx_backward.  One wave per pose; deterministic.
 */
int ag_smplx_backward_full(const AgSmplxModel* m, int32_t B, const float* shape_components, const float* full_pose, const float* dL_dA,
                           const float* dL_djoints, const float* dL_dA_skin, const float* dL_dfeat, const float* dL_dtransl_add,
                           const float* dL_dshape_components_add, float* dL_dfull_pose, float* dL_dtransl, float* dL_dshape_components,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_SMPLX_H */
