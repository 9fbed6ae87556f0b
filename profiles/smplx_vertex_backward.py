#!/usr/bin/env python
"""Workload for the kernel trace of the SMPL-X vertex backward: forward + backward of a loss on the vertices, all 127 joints and A on a
``vertex_grad`` model, B poses per call, then the chain alone, then the dataset path (`data_item`).  Run it under the profiler, one run per batch size:
`rocprofv3 --kernel-trace --stats -f csv -d OUT -- python profiles/smplx_vertex_backward.py B`; the yardstick for the new backward
kernels is `smplx_skin_kernel<B>` (the forward's pass over the same 61-MB basis) in the same trace."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import synth  # noqa: E402
from animatablegaussians_amd.smplx import SMPLX  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
dev = torch.device("cuda", 0)
model = SMPLX(synth.smplx_model_arrays(), use_pca=False, flat_hand_mean=True, device=dev, vertex_grad=True)
g = torch.Generator().manual_seed(B)
sizes = {"betas": 10, "expression": 10, "global_orient": 3, "body_pose": 63, "jaw_pose": 3, "left_hand_pose": 45, "right_hand_pose": 45, "transl": 3}
x = {k: (torch.randn(B, n, generator=g) * 0.3).to(dev).requires_grad_(True) for k, n in sizes.items()}
wV, wJ = torch.randn(B, 10475, 3, generator=g).to(dev), torch.randn(B, 127, 3, generator=g).to(dev)
wA = torch.randn(B, 55, 4, 4, generator=g).to(dev)
for i in range(5 + 50):          # 5 warm-up iterations, then 50; the trace's min / avg columns tell them apart
    out = model(**x)
    ((out.vertices * wV).sum() + (out.joints * wJ).sum() + (out.A * wA).sum()).backward()
    for v in x.values():
        v.grad = None
for i in range(5 + 50):          # the chain alone (a loss on A): smplx_chain_backward_kernel<false>, for comparison with <true>
    out = model(**x)
    (out.A * wA).sum().backward()
    for v in x.values():
        v.grad = None
params = synth.smplx_pose_params(n=1)     # the dataset path (no autograd): smplx_skin_kernel<3> and mat4_mul_inverse_kernel
cano = torch.zeros(75)
with torch.no_grad():
    for i in range(5 + 50):
        model.data_item(params, 0, cano[3:6], cano[:3], cano[6:69])
torch.cuda.synchronize()
print(f"B={B}: 2 x 55 forward + backward iterations and 55 data items done")
