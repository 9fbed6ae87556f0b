#!/bin/bash
# Builds libag_hip.so for gfx950 (cross-compiles without a GPU).  Output: animatablegaussians_amd/lib/libag_hip.so
set -eo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
OBJ="$HERE/../lib/obj"
mkdir -p "$OUT" "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
# No packed fp32 VALU (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in any kernel.  Measured on MI355X (profiles/r02_packed_fp32_hazard.md):
# while a wave of the split-bf16 convolution kernel is resident on the same SIMD, the LOW half of packed-fp32 results of another wave
# comes out wrong in lanes 48-63 now and then (the 3 -> C pointwise convolution under the three concurrent StyleUNets); the scalar
# forms are bit-identical in value and the guides list the packed forms as a loss beside MFMAs anyway.  The feature switch is a device
# target feature; the host pass of the same command does not know it and says so (that one line is filtered below).
NOPK="-Xclang -target-feature -Xclang -packed-fp32-ops"
# fp32 op order is a parity contract in the preprocess kernels: no FMA contraction there.
EXACT="-ffp-contract=off"
FAST="-ffp-contract=fast"
compile() { # src flags
  local src="$1"; shift
  local obj="$OBJ/$(basename "${src%.hip}").o"
  if [ ! -f "$obj" ] || [ "$src" -nt "$obj" ] || [ -n "$(find "$HERE" "$HERE/../../include" -maxdepth 1 -name '*.h' -newer "$obj" -print -quit)" ]; then
    echo "hipcc $(basename "$src") $*"
    rm -f "$obj"
    local log; log="$(mktemp)"
    if ! "$HIPCC" $COMMON $NOPK "$@" -c "$src" -o "$obj" 2> "$log"; then grep -v "packed-fp32-ops' is not a recognized feature" "$log" >&2; rm -f "$log"; return 1; fi
    grep -v "packed-fp32-ops' is not a recognized feature" "$log" >&2 || true
    rm -f "$log"
  fi
}
compile "$HERE/ag_abi.hip" $FAST &
compile "$HERE/ag_preprocess.hip" $EXACT &
compile "$HERE/ag_binning.hip" $EXACT &
compile "$HERE/ag_blend_forward.hip" $FAST &
compile "$HERE/ag_blend_backward.hip" $FAST &
compile "$HERE/ag_preprocess_backward.hip" $FAST &
compile "$HERE/ag_avatar.hip" $FAST &
compile "$HERE/ag_styleunet_ops.hip" $FAST &
compile "$HERE/ag_conv.hip" $FAST &
compile "$HERE/ag_conv_pointwise.hip" $FAST &
compile "$HERE/ag_lpips.hip" $FAST &
compile "$HERE/ag_smplx.hip" $FAST &
compile "$HERE/ag_layers.hip" $FAST &
compile "$HERE/ag_optim.hip" $FAST &
compile "$HERE/ag_linear.hip" $FAST &
# edge functions, depth and squared distances are stated op by op in include/ag_subject_maps.h (shared edges see opposite values)
compile "$HERE/ag_subject_maps.hip" $EXACT &
# fp64 window sums (include/ag_metrics.h): contraction changes nothing the contract states
compile "$HERE/ag_metrics.hip" $FAST &
# the trilinear weights and the eight-corner sum are stated op by op in include/ag_weight_volume.h
compile "$HERE/ag_weight_volume.hip" $EXACT &
# integer flag logic and one fp32 division per colour element (include/ag_targets.h).  EXACT because the contract is bit-exact, but the
# flag set does not matter here: contraction fuses a multiply with an add and the file has neither, and hipcc rounds an fp32 `/`
# correctly under both sets (-fhip-fp32-correctly-rounded-divide-sqrt is its default; neither set passes -ffast-math)
compile "$HERE/ag_targets.hip" $EXACT &
# the face record and the four candidates of a (query, face) pair are stated op by op in include/ag_mesh_query.h
compile "$HERE/ag_mesh_query.hip" $EXACT &
# the stencil and the CG updates are stated as rounded fp32 operations in include/ag_weight_diffuse.h
compile "$HERE/ag_weight_diffuse.hip" $EXACT &
# the Sobel gradient, the lane sums, their fold and the Newton step are stated op by op in include/ag_inverse_skinning.h
compile "$HERE/ag_inverse_skinning.hip" $EXACT &
# the vertex position is stated op by op in include/ag_isosurface.h; everything else there is integer work
compile "$HERE/ag_isosurface.hip" $EXACT &
# the embedding, the activations and the density are stated op by op in include/ag_template_field.h; the product sums are MFMA chains,
# which contraction cannot touch
compile "$HERE/ag_template_field.hip" $EXACT &
# the training path repeats that embedding and those activations bit for bit (include/ag_template_field_train.h)
compile "$HERE/ag_template_field_train.hip" $EXACT &
# near / far, the sample positions and the compositing sums are stated op by op in include/ag_ray_march.h
compile "$HERE/ag_ray_march.hip" $EXACT &
# the reverse recurrence of the compositing and the density's derivatives are stated op by op in include/ag_ray_march_grad.h
compile "$HERE/ag_ray_march_grad.hip" $EXACT &
# the gates, the interpolation, the hand's signed distance, the blend and the density are stated op by op in include/ag_hand_fusion.h
compile "$HERE/ag_hand_fusion.hip" $EXACT &
# the ray, the six plane steps, near / far and dist are stated op by op in include/ag_ray_select.h and matched bit for bit by a numpy
# float32 restatement: a fused multiply-add in `t * d + o` or in the sums of squares would round once where numpy rounds twice
compile "$HERE/ag_ray_select.hip" $EXACT &
fail=0
for job in $(jobs -p); do wait "$job" || fail=1; done
if [ "$fail" -ne 0 ]; then echo "build.sh: compilation failed" >&2; exit 1; fi
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/libag_hip.so" "$OBJ"/*.o
echo "built $OUT/libag_hip.so"
