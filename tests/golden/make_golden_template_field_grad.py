"""Writes ``template_field_grad_ref.npz``: the reference's own ``Embedder`` / ``SdfMLP`` modules run on the host in float32 and float64 on
the weights of ``tests/template_field_oracle.make_net(REFERENCE, 11)`` with ``xyz.requires_grad_()`` and the ``torch.autograd.grad`` call of
``TemplateNet.forward_cano_body_nerf`` under ``compute_grad`` (``network/template.py:106-112, 129-136``): the raw SDF and ``'normal'``.

Generation time only: it needs a checkout of the reference (first argument, or ``AG_REFERENCE_DIR``).  The fixture holds the points and the
outputs; the weights are NOT stored, they come from the recipe.

    python tests/golden/make_golden_template_field_grad.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import template_field_oracle as tfo  # noqa: E402

SEED, N_POINTS = 11, 257


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    import config
    config.device = torch.device("cpu")
    from network.mlp import SdfMLP
    from utils.embedder import get_embedder

    arch = tfo.REFERENCE
    xyz = tfo.box_points(N_POINTS, 5)
    out = {"xyz": xyz, "seed": np.int64(SEED)}
    sd = tfo.state_dict(tfo.make_net(arch, SEED))
    pos_embedder, pos_dim = get_embedder(arch["multires"], 3)
    geo = SdfMLP(in_channels=pos_dim, out_channels=arch["out"], inter_channels=list(arch["widths"]), nlactv=nn.Softplus(beta=100),
                 res_layers=list(arch["skip"]), geometric_init=True, bias=0.7, weight_norm=True)
    geo.load_state_dict({k[len("geo_mlp."):]: v for k, v in sd.items() if k.startswith("geo_mlp.")}, strict=True)
    geo.eval()
    for dtype, name in ((torch.float32, "32"), (torch.float64, "64")):
        geo.to(dtype)
        x = torch.from_numpy(xyz).to(dtype)
        x.requires_grad_()
        feat = geo(pos_embedder(x))
        sdf, feat = torch.split(feat, [1, feat.shape[-1] - 1], -1)
        d_output = torch.ones_like(sdf, requires_grad=False, device=sdf.device)
        normal = torch.autograd.grad(outputs=sdf, inputs=x, grad_outputs=d_output, create_graph=False, retain_graph=False, only_inputs=True)[0]
        out[f"sdf{name}"], out[f"normal{name}"] = (-sdf).detach().numpy(), normal.detach().numpy()
    path = os.path.join(HERE, "template_field_grad_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["AG_REFERENCE_DIR"])
