"""Host oracle of the template field's training path (``include/ag_template_field_train.h``, ``template_train.TemplateFieldModule``): the
field of ``template_field_oracle.forward`` restated on torch TENSORS, so that autograd applies, in float64 and float32 on the CPU.
Nothing here touches a GPU.

* ``leaves`` turns a ``make_net`` recipe into leaf tensors under the reference's state-dict names; ``field`` evaluates them (weight norm
  folded as torch's ``weight_norm`` does, ``v * (g / ||v||_row)``, in the run's dtype) and keeps every folded weight and every hidden
  pre-activation;
* ``gradients`` is autograd of ``sum(g_sdf * sdf) + sum(g_color * color)``: per layer ``dW`` (the folded weight's), ``db``, and the
  ``weight_g`` / ``weight_v`` gradients behind the fold;
* ``train_chain`` is ``render_train`` + ``training_loss`` on the host: field -> ``laplace_torch`` -> ``composite_torch`` -> the L1 terms
  (the chain of ``template_render_grad_oracle.train_chain`` with this field in place of its small one).
"""
import numpy as np
import torch
import torch.nn.functional as F

from template_field_oracle import NARROW, REFERENCE, SOFTPLUS_BETA, box_points, embed, make_net, state_dict, unit_dirs  # noqa: F401
from template_render_grad_oracle import composite_torch, laplace_b, laplace_torch

F32 = np.float32


def leaves(net, dtype):
    """{state-dict name: leaf tensor of ``dtype`` that requires grad} of every MLP parameter of ``net`` (``density_func.beta`` left out)."""
    return {k: v.to(dtype).requires_grad_(True) for k, v in state_dict(net).items() if k != "density_func.beta"}


def names(net):
    """Per layer in plan order the parameter names: ``(weight_g, weight_v, bias)`` for geometry, ``(None, weight, bias)`` for colour."""
    out = []
    for i in range(len(net["geo"])):
        p = f"geo_mlp.fc_list.{i}." + ("" if i == len(net["geo"]) - 1 else "0.")
        out.append((p + "weight_g", p + "weight_v", p + "bias"))
    for i in range(len(net["color"])):
        p = f"tex_mlp.fc_list.{i}." + ("" if i == len(net["color"]) - 1 else "0.")
        out.append((None, p + "weight", p + "bias"))
    return out


def field(P, net, x, d):
    """``P``: tensors by state-dict name; ``x`` [N, 3], ``d`` [N, 3] or None, tensors of the same dtype -> ``(sdf [N, 1], color [N, 3],
    folded: the weight [out, in] of every layer as used (graph kept), pre: the hidden geometry layers' pre-activations)``."""
    arch, n_geo = net["arch"], len(net["geo"])
    act = (lambda t: F.softplus(t, beta=SOFTPLUS_BETA, threshold=20)) if net["geo_activation"] == "softplus" else torch.relu
    e = embed(x, arch["multires"])
    h, folded, pre = e, [], []
    for l, (gk, vk, bk) in enumerate(names(net)[:n_geo]):
        if l in arch["skip"]:
            h = torch.cat([h, e], -1)
        w = P[vk] * (P[gk] / P[vk].norm(dim=1, keepdim=True))
        folded.append(w)
        z = F.linear(h, w, P[bk])
        if l < n_geo - 1:
            pre.append(z)
        h = z if l == n_geo - 1 else act(z)
    raw, c = h[:, :1], h[:, 1:]
    if net["use_viewdir"]:
        c = torch.cat([c, embed(torch.zeros_like(x) if d is None else d, arch["multires_viewdir"])], -1)
    n_col = len(net["color"])
    for l, (_, wk, bk) in enumerate(names(net)[n_geo:]):
        folded.append(P[wk])
        z = F.linear(c, P[wk], P[bk])
        c = torch.sigmoid(z) if l == n_col - 1 else torch.relu(z)
    return -raw, c, folded, pre


def softplus_shares(pre):
    """Shares of the hidden softplus pre-activations ``z`` on the linear branch (``beta z > 20``), in the curved part (``|beta z| < 5``) and
    below -20, over every hidden geometry layer."""
    bz = SOFTPLUS_BETA * np.concatenate([np.asarray(z.detach().numpy(), np.float64).reshape(-1) for z in pre])
    return float((bz > 20).mean()), float((np.abs(bz) < 5).mean()), float((bz < -20).mean())


def gradients(net, xyz, viewdirs, g_sdf, g_color, dtype):
    """-> ``(sdf, color, grads, shares)``: numpy outputs, ``grads`` = {"dW.{l}" / "db.{l}" per layer in plan order, and every
    ``weight_g`` / ``weight_v`` / ``weight`` / ``bias`` by state-dict name}, ``shares`` = ``softplus_shares``.  A None upstream is zeros."""
    P = leaves(net, dtype)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, F32)).to(dtype)  # noqa: E731
    sdf, color, folded, pre = field(P, net, t(xyz), t(viewdirs))
    for w in folded:
        w.retain_grad()
    loss = sdf.sum() * 0
    if g_sdf is not None:
        loss = loss + (sdf * t(g_sdf).reshape(sdf.shape)).sum()
    if g_color is not None:
        loss = loss + (color * t(g_color)).sum()
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad  # noqa: E731
    grads = {k: zero(p).numpy() for k, p in P.items()}
    for l, ((_, _, bk), w) in enumerate(zip(names(net), folded)):
        grads[f"dW.{l}"] = zero(w).numpy()
        grads[f"db.{l}"] = grads[bk]
    return sdf.detach().numpy(), color.detach().numpy(), grads, softplus_shares(pre)


def train_chain(net, beta, pts, z, ray_d, dir_noise, color_gt, mask_gt, weights, dtype):
    """``render_train`` + ``training_loss`` (no ``mask_within_patch``, black background) on the host in ``dtype`` from the float32 samples
    ``pts`` [R * S, 3] / ``z`` [R, S]: -> ``(loss, {state-dict name or "density_func.beta": gradient array})``."""
    R, S = z.shape
    P = leaves(net, dtype)
    b, sign = laplace_b(beta, dtype)
    d = torch.from_numpy(np.asarray(ray_d, F32)).to(dtype)
    dirs = (d / torch.norm(d, dim=-1, keepdim=True))[:, None, :].expand(-1, S, -1).reshape(-1, 3)
    dirs = dirs + torch.from_numpy(np.asarray(dir_noise, F32)).to(dtype)
    dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
    sdf, color, _, _ = field(P, net, torch.from_numpy(np.asarray(pts, F32)).to(dtype).reshape(-1, 3), dirs)
    out = composite_torch(laplace_torch(sdf, b).view(R, S), color.view(R, S, 3), torch.from_numpy(np.asarray(z, F32)).to(dtype))
    cgt, mgt = torch.from_numpy(np.asarray(color_gt, F32)).to(dtype), torch.from_numpy(np.asarray(mask_gt, F32)).to(dtype)
    loss = weights["color"] * (out["rgb_map"] - cgt).abs().mean() + weights["mask"] * (out["acc_map"] - mgt).abs().mean()
    keys = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in keys] + [b])
    by_name = {k: g.numpy() for k, g in zip(keys, grads[:-1])}
    by_name["density_func.beta"] = np.asarray(sign * grads[-1].numpy())
    return float(loss.detach()), by_name


def net_of_state_dict(sd, like):
    """A ``make_net``-shaped recipe holding the parameters of ``sd`` (a module's ``state_dict()``), the rest taken from ``like``."""
    a = lambda k: sd[k].detach().cpu().numpy().astype(F32)  # noqa: E731
    n_geo = len(like["geo"])
    geo = [(a(vk), a(gk), a(bk)) for gk, vk, bk in names(like)[:n_geo]]
    color = [(a(wk), a(bk)) for _, wk, bk in names(like)[n_geo:]]
    return dict(like, geo=geo, color=color, beta=F32(a("density_func.beta")))
