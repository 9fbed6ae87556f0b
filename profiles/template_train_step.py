"""Forward + backward of the template field's training path (``template_train.TemplateFieldModule``) against a plain torch module of
the same layers (fp32 ``F.linear``: rocBLAS), the path ``render_train`` had before.  The reference's architecture with view directions at
N = 65 536 points (1024 rays x 64 samples), random upstream gradients for ``sdf`` and ``color``.

    timeout 600 python profiles/template_train_step.py [--points 65536] [--iters 20] [--warmup 3] [--only device|torch]

Device time by events around each window, the two paths alternating; one JSON line.  For the kernels' shares run it under
``rocprofv3 --kernel-trace --stats -- python profiles/template_train_step.py --only device --iters 5`` in a run of its own.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from animatablegaussians_amd.template_train import TemplateFieldModule  # noqa: E402


def embed(x, L):
    cols = [x]
    for k in range(L):
        cols += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(cols, -1)


def torch_field(m, xyz, dirs, skip=(4,)):
    """The same field on the module's own parameters in plain torch ops: what a torch-module ``field_fn`` computes."""
    layers = m.folded_weights()
    n_geo = len(m.geo_mlp.linears())
    e = embed(xyz, m._arch["multires"])
    h = e
    for l, (w, b) in enumerate(layers[:n_geo]):
        if l in skip:
            h = torch.cat([h, e], -1)
        z = F.linear(h, w, b)
        h = z if l == n_geo - 1 else F.softplus(z, beta=m._arch["softplus_beta"], threshold=20)
    sdf, c = -h[:, :1], torch.cat([h[:, 1:], embed(dirs, m._arch["multires_viewdir"])], -1)
    for l, (w, b) in enumerate(layers[n_geo:]):
        z = F.linear(c, w, b)
        c = torch.sigmoid(z) if l == len(layers) - n_geo - 1 else torch.relu(z)
    return sdf, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("device", "torch"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this measures device time and has no host path")
    g = torch.Generator().manual_seed(0)
    m = TemplateFieldModule.geometric_init(use_viewdir=True, generator=g).cuda()
    N = a.points
    xyz = (torch.rand((N, 3), generator=g) * 2.4 - 1.2).cuda()
    dirs = F.normalize(torch.randn((N, 3), generator=g), dim=-1).cuda()
    g_sdf, g_color = torch.randn((N, 1), generator=g).cuda(), torch.randn((N, 3), generator=g).cuda()

    def step(fn):
        m.zero_grad(set_to_none=True)
        sdf, color = fn(xyz, dirs)
        torch.autograd.backward([sdf, color], [g_sdf, g_color])

    paths = {"device": lambda: step(m), "torch": lambda: step(lambda p, v: torch_field(m, p, v))}
    if a.only:
        paths = {a.only: paths[a.only]}
    for fn in paths.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, fn in paths.items():                     # alternating
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    from animatablegaussians_amd import _lib
    import ctypes
    d = m.plan.desc()
    out = {"points": N, "iters": a.iters,
           "stash_MB": _lib.lib().ag_template_field_train_stash_floats(ctypes.byref(d), N) * 4 / 1e6,
           "workspace_MB": _lib.lib().ag_template_field_train_workspace_floats(ctypes.byref(d), N) * 4 / 1e6}
    for k, v in ms.items():
        out[k + "_ms_median"], out[k + "_ms_min"], out[k + "_ms_max"] = float(np.median(v)), float(np.min(v)), float(np.max(v))
    if len(ms) == 2:
        grads = {}
        for k, fn in paths.items():
            fn()
            grads[k] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        out["max_rel_grad_difference"] = max(float((grads["device"][n] - grads["torch"][n]).abs().max() / grads["torch"][n].abs().max().clamp_min(1e-30))
                                             for n in grads["torch"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
