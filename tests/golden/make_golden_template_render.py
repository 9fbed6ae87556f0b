"""Writes ``template_render_ref.npz``: the reference's own ``nerf_util.sample_pts_on_rays`` and ``nerf_util.raw2outputs`` (with the alpha of
``network/template.py:345-346, 372``), run on the host in float32 and float64 on the scenes of ``tests/template_render_oracle.py``.

Generation time only: it needs a checkout of the reference (first argument, or ``AG_REFERENCE_DIR``).  ``utils/nerf_util.py`` imports
``cv2`` for its dataset-side functions; none of the two functions used here touches it, so an empty stand-in module is registered under
that name before the import.  The fixture holds inputs and outputs only:

* sampling, S in ``SAMPLES``, ``N_RAYS`` rays of ``ray_scene``: ``z_vals`` / ``pts`` in float32, unperturbed and perturbed; the first
  ``N_RAYS64`` rays also in float64.  For the perturbed run torch is seeded, the reference called (``perturb = True``), then torch is
  seeded again and the same ``torch.rand`` drawn: that ``u`` is stored.
* compositing, S in ``COMPOSITE_SAMPLES``, ``N_COMPOSITE`` rays of ``composite_case``: the inputs and the five outputs in float32 and
  float64, ``white_bkgd`` off and on (only ``rgb_map`` differs).

The reference's near / far kernel is CUDA and cannot be run on the host: near / far has no fixture and is pinned to the formulas of
``include/ag_ray_march.h``.

    python tests/golden/make_golden_template_render.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import template_render_oracle as tro  # noqa: E402

SAMPLES, N_RAYS, N_RAYS64, SEED = (2, 63, 64, 65), 19, 5, 7
COMPOSITE_SAMPLES, N_COMPOSITE = (2, 63, 64, 65, 130), 9


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from utils import nerf_util

    o, d, near, far = tro.ray_scene(N_RAYS, SEED)
    out = {"ray_o": o, "ray_d": d, "near": near, "far": far, "seed": np.int64(SEED)}
    for S in SAMPLES:
        for dtype, name, n in ((torch.float32, "32", N_RAYS), (torch.float64, "64", N_RAYS64)):
            args = [torch.from_numpy(a[:n])[None].to(dtype) for a in (o, d, near, far)]
            pts, z = nerf_util.sample_pts_on_rays(*args, N_samples=S, perturb=False)
            out[f"s{S}_z{name}"], out[f"s{S}_pts{name}"] = z[0].numpy(), pts[0].numpy()
            torch.manual_seed(SEED + S)
            pts, z = nerf_util.sample_pts_on_rays(*args, N_samples=S, perturb=True)
            torch.manual_seed(SEED + S)
            u = torch.rand((n, S))
            out[f"s{S}_zp{name}"], out[f"s{S}_ptsp{name}"] = z[0].numpy(), pts[0].numpy()
            if name == "32":
                out[f"s{S}_u"] = u.numpy()
            else:                                   # the float64 run draws the first rows of a smaller tensor: its own u
                out[f"s{S}_u64"] = u.numpy()
    for S in COMPOSITE_SAMPLES:
        density, color, z = tro.composite_case(N_COMPOSITE, S, SEED + S)
        out[f"c{S}_density"], out[f"c{S}_color"], out[f"c{S}_z"] = density, color, z
        for dtype, name in ((torch.float32, "32"), (torch.float64, "64")):
            dn, rgb, zz = (torch.from_numpy(a)[None].to(dtype) for a in (density[..., None], color, z))
            dists = zz[..., 1:] - zz[..., :-1]
            dists = torch.cat([dists, dists[..., -1:]], -1)
            alpha = 1. - torch.exp(-dn * dists[..., None])
            raw = torch.cat([rgb, alpha], dim=-1)
            for white, tag in ((False, ""), (True, "_white")):
                rgb_map, disp_map, acc_map, weights, depth_map = nerf_util.raw2outputs(raw, zz, white_bkgd=white)
                out[f"c{S}_rgb{tag}{name}"] = rgb_map[0].numpy()
            out[f"c{S}_disp{name}"], out[f"c{S}_acc{name}"] = disp_map[0].numpy(), acc_map[0].numpy()
            out[f"c{S}_weights{name}"], out[f"c{S}_depth{name}"] = weights[0].numpy(), depth_map[0].numpy()
    path = os.path.join(HERE, "template_render_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["AG_REFERENCE_DIR"])
