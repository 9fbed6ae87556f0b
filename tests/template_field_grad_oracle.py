"""Plain-torch restatement of the template field's gradient (``include/ag_template_field_grad.h``, ``TemplateField.sdf_normal``): the
gradient of the RAW SDF with respect to the query points, the reference's ``'normal'`` (``network/template.py:129-139``), derived twice
on the host in float32 and float64:

(a) ``autograd``: ``torch.autograd.grad`` through the chain of ``template_field_oracle`` with the very call of ``template.py:130-136``;
(b) ``tangents``: the forward-mode tangents of the header's definition, written out -- three tangent rows per point pushed through the
    embedding, every linear map (without the bias) and every activation's derivative beside the value row.

Both return ``raw`` [N, 1], ``sdf`` = -raw, ``normal`` [N, 3] and ``pre_geo``, the pre-activation of every geometry layer.
"""
import numpy as np
import torch
import torch.nn.functional as F

import template_field_oracle as tfo


def _activation(net):
    return (lambda t: F.softplus(t, beta=tfo.SOFTPLUS_BETA, threshold=20)) if net["geo_activation"] == "softplus" else torch.relu


def autograd(net, xyz, dtype=torch.float64):
    """(a).  ``xyz`` [N, 3] numpy float32 -> dict of numpy arrays in ``dtype``."""
    arch = net["arch"]
    x = torch.from_numpy(np.asarray(xyz, np.float32)).to(dtype).requires_grad_()
    e = tfo.embed(x, arch["multires"])
    act = _activation(net)
    h, pre = e, []
    for l, (v, g, b) in enumerate(net["geo"]):
        if l in arch["skip"]:
            h = torch.cat([h, e], -1)
        z = F.linear(h, tfo.fold(v, g, dtype), torch.from_numpy(b).to(dtype))
        pre.append(z.detach().numpy())
        h = z if l == len(net["geo"]) - 1 else act(z)
    sdf = h[:, :1]
    d_output = torch.ones_like(sdf, requires_grad=False, device=sdf.device)
    normal = torch.autograd.grad(outputs=sdf, inputs=x, grad_outputs=d_output, create_graph=False, retain_graph=False, only_inputs=True)[0]   # eval mode
    raw = sdf.detach().numpy()
    return dict(raw=raw, sdf=-raw, normal=normal.detach().numpy(), pre_geo=pre)


def embed_tangents(x, multires):
    """[N, 3 (axis b), 3 + 6 L]: the tangent of ``tfo.embed(x, L)`` along each axis, column by column as the header states it."""
    eye = torch.eye(3, dtype=x.dtype)
    cols = [eye.expand(x.shape[0], 3, 3)]
    for k in range(multires):
        f = float(2 ** k)
        s, c = torch.sin(x * f), torch.cos(x * f)
        cols += [eye * (f * c)[:, None, :], eye * (-(f * s))[:, None, :]]
    return torch.cat(cols, -1)


def slope(z, net):
    if net["geo_activation"] == "softplus":
        bz = tfo.SOFTPLUS_BETA * z
        return torch.where(bz > 20, torch.ones_like(z), 1 / (1 + torch.exp(-bz)))
    return (z > 0).to(z.dtype)


def tangents(net, xyz, dtype=torch.float64):
    """(b).  No autograd anywhere."""
    arch = net["arch"]
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(xyz, np.float32)).to(dtype)
        e, te = tfo.embed(x, arch["multires"]), embed_tangents(x, arch["multires"])
        act = _activation(net)
        h, th, pre = e, te, []
        for l, (v, g, b) in enumerate(net["geo"]):
            if l in arch["skip"]:
                h, th = torch.cat([h, e], -1), torch.cat([th, te], -1)
            w = tfo.fold(v, g, dtype)
            z, tz = F.linear(h, w, torch.from_numpy(b).to(dtype)), F.linear(th, w)
            pre.append(z.numpy())
            if l == len(net["geo"]) - 1:
                h, th = z, tz
            else:
                h, th = act(z), tz * slope(z, net)[:, None, :]
        raw = h[:, :1].numpy()
    return dict(raw=raw, sdf=-raw, normal=th[:, :, 0].numpy(), pre_geo=pre)


def unit(n):
    """``n / max(||n||, 1e-12)`` along the last axis, numpy."""
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)


def eikonal(n):
    return float(((np.linalg.norm(np.asarray(n, np.float64), axis=-1) - 1.0) ** 2).mean())
