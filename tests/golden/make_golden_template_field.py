"""Writes ``template_field_ref.npz``: the reference's own ``SdfMLP`` / ``MLPLinear`` / ``Embedder`` / ``LaplaceDensity`` modules, run on the
host in float32 and float64 on the weights of ``tests/template_field_oracle.make_net`` (reference architecture, trained-like, with and
without ``use_viewdir``), chained as ``TemplateNet.forward_cano_body_nerf`` chains them (``network/template.py:110-127``).

Generation time only: it needs a checkout of the reference (first argument, or ``AG_REFERENCE_DIR``).  The fixture holds the points, the view
directions and the outputs; the weights are NOT stored, they come from the recipe.

    python tests/golden/make_golden_template_field.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import template_field_oracle as tfo  # noqa: E402

SEED, N_POINTS = 11, 300


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    import config
    config.device = torch.device("cpu")                       # LaplaceDensity moves its beta_min there
    from network.density import LaplaceDensity
    from network.mlp import MLPLinear, SdfMLP
    from utils.embedder import get_embedder

    arch = tfo.REFERENCE
    xyz, dirs = tfo.box_points(N_POINTS, 5), tfo.unit_dirs(N_POINTS, 6)
    out = {"xyz": xyz, "viewdirs": dirs, "seed": np.int64(SEED)}
    for use_viewdir in (False, True):
        net = tfo.make_net(arch, SEED, use_viewdir=use_viewdir)
        sd = tfo.state_dict(net)
        pos_embedder, pos_dim = get_embedder(arch["multires"], 3)
        view_embedder, view_dim = get_embedder(arch["multires_viewdir"], 3) if use_viewdir else (None, 0)
        geo = SdfMLP(in_channels=pos_dim, out_channels=arch["out"], inter_channels=list(arch["widths"]), nlactv=nn.Softplus(beta=100),
                     res_layers=list(arch["skip"]), geometric_init=True, bias=0.7, weight_norm=True)
        tex = MLPLinear(in_channels=arch["out"] - 1 + view_dim, out_channels=3, inter_channels=list(arch["color"]), nlactv=nn.ReLU(), last_op=nn.Sigmoid())
        density = LaplaceDensity(params_init={"beta": 0.01})
        geo.load_state_dict({k[len("geo_mlp."):]: v for k, v in sd.items() if k.startswith("geo_mlp.")}, strict=True)
        tex.load_state_dict({k[len("tex_mlp."):]: v for k, v in sd.items() if k.startswith("tex_mlp.")}, strict=True)
        density.load_state_dict({"beta": sd["density_func.beta"]}, strict=True)
        tag = "view" if use_viewdir else "plain"
        for dtype, name in ((torch.float32, "32"), (torch.float64, "64")):
            geo.to(dtype), tex.to(dtype), density.to(dtype)
            with torch.no_grad():
                x = torch.from_numpy(xyz).to(dtype)
                feat = geo(pos_embedder(x))
                sdf, feat = torch.split(feat, [1, feat.shape[-1] - 1], -1)
                if view_embedder is not None:
                    feat = torch.cat([feat, view_embedder(torch.from_numpy(dirs).to(dtype))], -1)
                color = tex(feat)
                dens = density(sdf)
            out[f"{tag}_sdf{name}"], out[f"{tag}_density{name}"], out[f"{tag}_color{name}"] = (-sdf).numpy(), dens.numpy(), color.numpy()
    path = os.path.join(HERE, "template_field_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["AG_REFERENCE_DIR"])
