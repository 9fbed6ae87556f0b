"""Host oracles of the template renderer's reverse pass (``include/ag_ray_march_grad.h``, ``template_render.composite_backward`` /
``laplace_density`` / ``render_train``).  Nothing here touches a GPU.

* float64 oracle: torch autograd of the reference's text -- the chain of ``template_render_oracle.composite`` (``template.py:345-346,
  372-374`` + ``nerf_util.raw2outputs``: ``torch.cumprod``, ``torch.sum``) and the ``LaplaceDensity`` expression (``density.py:22-36``).
* float32 oracle: the header's division-free recurrence, sample by sample in float32 (numpy has no FMA: every operation is one
  rounded float32 operation), and the density's closed-form derivatives element by element.
* ``b = |beta| + 1e-4`` is a float32 sum in every precision (the kernel and the reference both form it in float32).
* the small torch field and the training chain of ``render_train``'s end-to-end test, in any dtype.
"""
import numpy as np
import torch

from template_field_oracle import BETA_MIN

F32 = np.float32
GRADS = ("rgb_map", "acc_map", "depth_map", "weights")


# ---- compositing ------------------------------------------------------------------------------------------------------------------------
def composite_torch(dn, rgb, z, white_bkgd=False):
    """``template_render_oracle.composite``'s chain on torch tensors ``dn`` [R, S], ``rgb`` [R, S, 3], ``z`` [R, S], keeping the graph."""
    dn = dn[..., None]
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, dists[..., -1:]], -1)
    alpha = (1. - torch.exp(-dn * dists[..., None]))[..., 0]
    weights = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1. - alpha + 1e-10], -1), -1)[..., :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z, -1)
    acc_map = torch.sum(weights, -1)
    if white_bkgd:
        rgb_map = rgb_map + (1. - acc_map[..., None])
    return dict(rgb_map=rgb_map, acc_map=acc_map, depth_map=depth_map, weights=weights, alpha=alpha)


def upstream(R, S, seed=0):
    """Random upstream gradients of the four differentiable maps, float32."""
    rs = np.random.RandomState(seed)
    return dict(rgb_map=rs.normal(size=(R, 3)).astype(F32), acc_map=rs.normal(size=R).astype(F32), depth_map=rs.normal(size=R).astype(F32),
                weights=rs.normal(size=(R, S)).astype(F32))


def composite_autograd(density, color, z_vals, grads, white_bkgd=False, dtype=torch.float64):
    """``(grad_density [R, S], grad_color [R, S, 3])`` by torch autograd of the reference's text in ``dtype``; ``grads``: name -> array."""
    R, S = np.shape(z_vals)
    dn = torch.tensor(np.asarray(density).reshape(R, S), dtype=dtype, requires_grad=True)       # copies: the inputs may be read-only
    rgb = torch.tensor(np.asarray(color).reshape(R, S, 3), dtype=dtype, requires_grad=True)
    z = torch.tensor(np.asarray(z_vals), dtype=dtype)
    out = composite_torch(dn, rgb, z, white_bkgd)
    loss = sum((out[k] * torch.tensor(np.asarray(g), dtype=dtype)).sum() for k, g in grads.items())
    gd, gc = torch.autograd.grad(loss, (dn, rgb), allow_unused=True)
    gc = torch.zeros_like(rgb) if gc is None else gc
    return gd.numpy(), gc.numpy()


def composite_recurrence(density, color, z_vals, grads, white_bkgd=False, dtype=np.float64):
    """The header's recurrence, one sample after the other in ``dtype`` (vectorised over the rays only): ``(grad_density, grad_color,
    weights, alpha)``.  ``np.float32``: every operation is one rounded float32 operation, in the header's order."""
    R, S = np.shape(z_vals)
    dn = np.ascontiguousarray(density).reshape(R, S).astype(dtype)
    col = np.ascontiguousarray(color).reshape(R, S, 3).astype(dtype)
    z = np.ascontiguousarray(z_vals).astype(dtype)
    one, tiny = dtype(1), dtype(1e-10)             # the reference's literal: 1e-10f in float32, 1e-10 in float64
    G = {k: (np.asarray(grads[k]).astype(dtype) if k in grads else None) for k in GRADS}
    zero = np.zeros(R, dtype)
    G_rgb = G["rgb_map"] if G["rgb_map"] is not None else np.zeros((R, 3), dtype)
    G_acc = G["acc_map"] if G["acc_map"] is not None else zero
    G_dep = G["depth_map"] if G["depth_map"] is not None else zero
    G_w = G["weights"] if G["weights"] is not None else np.zeros((R, S), dtype)
    if white_bkgd:
        G_acc = G_acc - ((G_rgb[:, 0] + G_rgb[:, 1]) + G_rgb[:, 2])
    dist = np.concatenate([z[:, 1:] - z[:, :-1], z[:, -1:] - z[:, -2:-1]], 1)
    e = np.exp(-dn * dist)
    alpha = one - e
    f = (one - alpha) + tiny
    T = np.empty((R, S), dtype)
    t = np.ones(R, dtype)
    for s in range(S):
        T[:, s] = t
        t = t * f[:, s]
    w = alpha * T
    g = G_rgb[:, None, 0] * col[..., 0] + G_rgb[:, None, 1] * col[..., 1] + G_rgb[:, None, 2] * col[..., 2] + G_acc[:, None] + G_dep[:, None] * z + G_w
    gd = np.empty((R, S), dtype)
    B = np.zeros(R, dtype)
    for s in range(S - 1, -1, -1):
        gd[:, s] = T[:, s] * (g[:, s] - B) * dist[:, s] * e[:, s]
        B = alpha[:, s] * g[:, s] + f[:, s] * B
    gc = w[..., None] * G_rgb[:, None, :]
    assert gd.dtype == dtype and gc.dtype == dtype and w.dtype == dtype
    return gd, gc, w, alpha


# ---- LaplaceDensity ---------------------------------------------------------------------------------------------------------------------
def laplace_b(beta, dtype):
    """``b = |beta| + 1e-4`` summed in float32, as a leaf tensor of ``dtype`` that requires grad, and ``sign(beta)``:
    ``d/d beta = sign(beta) * d/d b`` (the float32 sum is what the reference and the kernel form; its derivative is exact)."""
    beta = F32(beta)
    return torch.tensor(float(np.abs(beta) + BETA_MIN), dtype=dtype, requires_grad=True), float(np.sign(beta))


def laplace_torch(sdf, b):
    """The reference's expression of the raw column ``-sdf`` with ``b`` given: same shape as ``sdf``."""
    raw = -sdf
    return (1 / b) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / b))


def laplace_autograd(sdf, beta, g_density, dtype=torch.float64):
    """``(density, grad_sdf, grad_beta)`` numpy, by autograd of the reference's expression in ``dtype`` (``b`` a float32 sum)."""
    s = torch.from_numpy(np.asarray(sdf, F32)).to(dtype).requires_grad_(True)
    b, sign = laplace_b(beta, dtype)
    d = laplace_torch(s, b)
    gs, gb = torch.autograd.grad((d * torch.from_numpy(np.asarray(g_density, F32)).to(dtype)).sum(), (s, b))
    return d.detach().numpy(), gs.numpy(), sign * float(gb)


def laplace_closed(sdf, beta, g_density, dtype=np.float64):
    """The header's closed forms element by element in ``dtype``: ``(density, grad_sdf, terms)`` with ``grad_beta = sign(beta) *
    sum(terms)``; the sum is left to the caller (its order is the kernel's business)."""
    s, g = np.asarray(sdf, F32).astype(dtype), np.asarray(g_density, F32).astype(dtype)
    b = dtype(np.abs(F32(beta)) + BETA_MIN)
    v = -s
    sgn, av = np.sign(v), np.abs(v)
    inv = dtype(1) / b
    dens = inv * (dtype(0.5) + (dtype(0.5) * sgn) * np.expm1(-av / b))
    ex = np.exp(-av / b)
    gs = g * ((sgn * sgn * ex) / ((dtype(2) * b) * b))
    terms = g * (-dens / b + (((inv * dtype(0.5)) * sgn) * ex) * av / (b * b))
    assert gs.dtype == dtype and terms.dtype == dtype
    return dens, gs, terms


def sdf_case(N, seed=0):
    """``sdf`` [N] and ``g_density`` [N] float32: signed distances within a few ``b`` of the surface and far from it, both signs, and
    exact zeros (every 7th element; element 0)."""
    rs = np.random.RandomState(seed)
    s = (rs.normal(size=N) * np.where(rs.uniform(size=N) < 0.5, 0.01, 0.3)).astype(F32)
    s[::7] = 0.0
    return s, rs.normal(size=N).astype(F32)


# ---- the small field and the training chain -------------------------------------------------------------------------------------------
def tiny_net(seed=0):
    """A 3 -> 16 -> 4 field: softplus hidden layer, column 0 the signed distance (about ``0.5 - |p|`` plus a learned part), columns 1-3
    through a sigmoid the colour.  Float32 numpy parameters."""
    rs = np.random.RandomState(seed)
    return dict(w1=rs.normal(0, 1.0, (16, 3)).astype(F32), b1=rs.normal(0, 0.5, 16).astype(F32),
                w2=rs.normal(0, 0.15, (4, 16)).astype(F32), b2=np.array([0.0, 0.1, -0.2, 0.3], F32))


def tiny_field(params, pts, dirs):
    """``(sdf [N, 1], color [N, 3])`` of torch parameters ``params`` (any dtype / device) at ``pts`` seen from ``dirs``: the three inputs
    are ``pts + 0.05 * dirs``, so the view directions (and their noise) reach both outputs."""
    x = pts + 0.05 * dirs
    h = torch.nn.functional.softplus(torch.nn.functional.linear(x, params["w1"], params["b1"]))
    out = torch.nn.functional.linear(h, params["w2"], params["b2"])
    sdf = 0.5 - torch.sqrt((x * x).sum(-1, keepdim=True)) + 0.1 * out[:, :1]
    return sdf, torch.sigmoid(out[:, 1:])


def train_chain(net, beta, pts, z, ray_d, dir_noise, mask, color_gt, mask_gt, weights, white_bkgd, dtype):
    """``render_train`` + ``training_loss`` on the host in ``dtype`` from the float32 samples ``pts`` [R, S, 3] / ``z`` [R, S]: ->
    ``(loss, {parameter name or "beta": gradient array}, {"rgb_map": [P, 3], "acc_map": [P]})``."""
    R, S = z.shape
    params = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in net.items()}
    b, sign = laplace_b(beta, dtype)
    d = torch.from_numpy(np.asarray(ray_d, F32)).to(dtype)
    dirs = (d / torch.norm(d, dim=-1, keepdim=True))[:, None, :].expand(-1, S, -1).reshape(-1, 3)
    dirs = dirs + torch.from_numpy(np.asarray(dir_noise, F32)).to(dtype)
    dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
    sdf, color = tiny_field(params, torch.from_numpy(np.asarray(pts, F32)).to(dtype).reshape(-1, 3), dirs)
    density = laplace_torch(sdf, b)
    out = composite_torch(density.view(R, S), color.view(R, S, 3), torch.from_numpy(np.asarray(z, F32)).to(dtype), white_bkgd)
    m = torch.from_numpy(np.asarray(mask, bool))
    rgb = torch.zeros((len(m), 3), dtype=dtype).index_put((m,), out["rgb_map"])
    acc = torch.zeros(len(m), dtype=dtype).index_put((m,), out["acc_map"])
    cgt = torch.from_numpy(np.asarray(color_gt, F32)).to(dtype) * m[:, None]
    mgt = torch.from_numpy(np.asarray(mask_gt, F32)).to(dtype) * m
    loss = weights["color"] * (rgb - cgt).abs().mean() + weights["mask"] * (acc - mgt).abs().mean()
    names = list(params)
    grads = torch.autograd.grad(loss, [params[k] for k in names] + [b])
    by_name = {k: g.numpy() for k, g in zip(names, grads[:-1])}
    by_name["beta"] = np.asarray(sign * grads[-1].numpy())
    return float(loss.detach()), by_name, dict(rgb_map=rgb.detach().numpy(), acc_map=acc.detach().numpy())
