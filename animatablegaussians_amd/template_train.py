"""Training the template stage's field on the GPU (``include/ag_template_field_train.h``): the body field of the reference's ``TemplateNet``
as a ``torch.nn.Module`` whose forward and reverse pass are this project's HIP kernels.

``TemplateFieldModule`` holds the reference's parameters under the reference's names (``geo_mlp.fc_list.{i}.0.weight_g`` / ``weight_v`` /
``bias``, ``tex_mlp.fc_list.*.weight`` / ``bias``, ``density_func.beta``), so its ``state_dict()`` is a reference ``net.pt['network']`` for the
body field and ``TemplateField.from_state_dict`` reads it.  ``module(xyz, viewdirs) -> (sdf, color)`` is the callable
``template_render.render_train`` takes, and ``module.beta`` what it takes as ``beta``:

    out = render_train(module, module.beta, ray_o, ray_d, near, far, ...)
    loss, _ = training_loss(out, color_gt, mask_gt, weights); loss.backward(); optimizer.step()

The forward runs the field LAYER BY LAYER and keeps every layer's activations (the stash, 11.8 KB per point for the reference's
networks); it equals the fused inference kernel (``TemplateField``) on the same folded weights bit for bit.  The reverse pass yields
the gradient of every weight and bias without atomics: two backward calls agree bit for bit.

NOT here: any gradient with respect to the points or the view directions (the eikonal term's second-order pass), the hand fusion's
backward, gradients to ``z_vals``.  Every tensor must be on the GPU; there is no host path and no PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib
from .mlp_blob import _order, ptr, stream
from .template_field import TemplateField, _array, _mlp, embed_dim

SLAB = 1024                         # AG_FIELD_TRAIN_SLAB of include/ag_template_field_train.h: points per slab of the weight gradient


class _Linear(nn.Module):
    """The parameters of one linear: ``weight_g`` [out, 1] / ``weight_v`` [out, in] (``nn.utils.weight_norm``) or ``weight``, and ``bias``."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor, g: Optional[torch.Tensor] = None):
        super().__init__()
        if g is None:
            self.weight = nn.Parameter(w.detach().clone().to(torch.float32))
        else:
            self.weight_g = nn.Parameter(g.detach().clone().to(torch.float32).reshape(-1, 1))
            self.weight_v = nn.Parameter(w.detach().clone().to(torch.float32))
        self.bias = nn.Parameter(b.detach().clone().to(torch.float32))

    def folded(self) -> torch.Tensor:
        """torch's weight-norm forward in fp32: ``v * (g / ||v||_row)``; autograd carries ``dW`` on to ``g`` and ``v``."""
        if hasattr(self, "weight"):
            return self.weight
        return self.weight_v * (self.weight_g / self.weight_v.norm(dim=1, keepdim=True))


class _Mlp(nn.Module):
    """``fc_list`` as the reference's ``MLPLinear``: ``nn.Sequential(linear)`` for the hidden layers (the activation has no parameters), the
    bare linear last: the keys are ``fc_list.{i}.0.*`` and ``fc_list.{n}.*``."""

    def __init__(self, linears: Sequence[_Linear]):
        super().__init__()
        self.fc_list = nn.ModuleList([nn.Sequential(lin) for lin in linears[:-1]] + list(linears[-1:]))

    def linears(self):
        return [m[0] if isinstance(m, nn.Sequential) else m for m in self.fc_list]


class _Density(nn.Module):
    def __init__(self, beta: float):
        super().__init__()
        self.beta = nn.Parameter(torch.tensor(float(beta), dtype=torch.float32))


class _FieldTrain(torch.autograd.Function):
    """``flat`` (every folded weight in plan order, then every bias) -> ``(sdf [N, 1], color [N, 3] or None)`` through
    ``ag_template_field_train_forward``; the backward is ``ag_template_field_train_backward``.  ``xyz`` and ``viewdirs`` get None."""

    @staticmethod
    def forward(ctx, flat, xyz, viewdirs, mod):
        L, dev, N = _lib.lib(), xyz.device, xyz.shape[0]
        flat_z = torch.cat([flat.detach(), flat.new_zeros(1)])          # the padding's zero behind the parameters
        idx_fwd, idx_t = mod._maps_on(dev)
        blob, blob_t = flat_z[idx_fwd], flat_z[idx_t]                    # ONE gather each
        d = mod.plan.desc()
        want_color = bool(mod.plan.color)
        stash = torch.empty(int(L.ag_template_field_train_stash_floats(ctypes.byref(d), N)), dtype=torch.float32, device=dev)
        sdf = torch.empty((N, 1), dtype=torch.float32, device=dev)
        color = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_color else None
        with _lib.on_device(dev):
            _lib.check(L.ag_template_field_train_forward(ctypes.byref(d), ptr(blob), blob.numel(), ptr(xyz), ptr(viewdirs), N, ptr(stash), stash.numel(),
                                                         ptr(sdf), ptr(color), stream(dev)), "ag_template_field_train_forward")
        ctx.mod, ctx.N, ctx.n_flat = mod, N, flat.numel()
        ctx.save_for_backward(blob_t, stash)
        ctx.set_materialize_grads(False)
        if color is None:
            return sdf, None
        return sdf, color

    @staticmethod
    def backward(ctx, g_sdf, g_color):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        blob_t, stash = ctx.saved_tensors
        L, dev, N, mod = _lib.lib(), stash.device if stash.numel() else blob_t.device, ctx.N, ctx.mod
        d = mod.plan.desc()
        g_sdf = None if g_sdf is None else g_sdf.contiguous().to(torch.float32)
        g_color = None if g_color is None else g_color.contiguous().to(torch.float32)
        ws = torch.empty(int(L.ag_template_field_train_workspace_floats(ctypes.byref(d), N)), dtype=torch.float32, device=dev)
        g_flat = torch.empty(ctx.n_flat, dtype=torch.float32, device=dev)
        g_bias = g_flat[mod._n_weights:]
        with _lib.on_device(dev):
            _lib.check(L.ag_template_field_train_backward(ctypes.byref(d), ptr(blob_t), blob_t.numel(), ptr(stash), stash.numel(),
                                                          ptr(g_sdf), ptr(g_color), N, ptr(ws), ws.numel(),
                                                          ctypes.c_void_p(g_flat.data_ptr()), ctypes.c_void_p(g_bias.data_ptr()), stream(dev)),
                       "ag_template_field_train_backward")
        return g_flat, None, None, None


class TemplateFieldModule(nn.Module):
    """The body field of the reference's ``TemplateNet`` for training.  ``geo``: ``[(weight_v [out, in], weight_g [out, 1], bias [out])]``,
    ``color``: ``[(weight [out, in], bias [out])]``, arrays or tensors; the architecture's limits are ``TemplateField``'s."""

    def __init__(self, geo: Sequence, color: Sequence, multires: int = 6, use_viewdir: bool = False, multires_viewdir: int = 3,
                 density_beta: float = 0.01, softplus_beta: float = 100.0, geo_activation: str = "softplus"):
        super().__init__()
        t = lambda a: a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, np.float32))  # noqa: E731
        self.geo_mlp = _Mlp([_Linear(t(v), t(b), t(g)) for v, g, b in geo])
        self.tex_mlp = _Mlp([_Linear(t(w), t(b)) for w, b in color]) if len(color) else None
        self.density_func = _Density(density_beta)
        self._arch = dict(multires=int(multires), use_viewdir=bool(use_viewdir), multires_viewdir=int(multires_viewdir),
                          softplus_beta=float(softplus_beta), geo_activation=geo_activation)
        # the plan: a TemplateField of zeros with these shapes -- its checks, its layer table, its desc and its blob layout
        zeros = lambda lins: [(np.zeros(tuple(l.folded().shape), np.float32), np.zeros(tuple(l.bias.shape), np.float32)) for l in lins]  # noqa: E731
        self.plan = TemplateField(zeros(self.geo_mlp.linears()), zeros(self._color_linears()), density_beta=0.01, **self._arch)
        self._idx_fwd, self._idx_t, self._n_weights, self._n_biases = self._index_maps()
        self._device_maps = {}

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, multires: int = 6, use_viewdir: bool = False, multires_viewdir: int = 3, *, softplus_beta: float = 100.0,
                        geo_activation: str = "softplus") -> "TemplateFieldModule":
        """``sd``: the reference's ``TemplateNet.state_dict()`` (``weight_g`` / ``weight_v`` or ``parametrizations.weight.original0`` /
        ``original1``), as ``TemplateField.from_state_dict`` reads it; the parameters are kept UNFOLDED under the first spelling."""
        geo = []
        for i in range(len(_mlp(sd, "geo_mlp", must_be_normalised=True))):          # the same refusals
            hidden, last = f"geo_mlp.fc_list.{i}.0.", f"geo_mlp.fc_list.{i}."
            p = hidden if any(k.startswith(hidden) for k in sd) else last
            gk, vk = (p + "weight_g", p + "weight_v") if p + "weight_v" in sd else (p + "parametrizations.weight.original0", p + "parametrizations.weight.original1")
            geo.append((_array(sd, vk).astype(np.float32), _array(sd, gk).astype(np.float32), _array(sd, p + "bias").astype(np.float32)))
        color = _mlp(sd, "tex_mlp", must_be_normalised=False)
        beta = _array(sd, "density_func.beta")
        if beta.size != 1:
            raise ValueError(f"density_func.beta: expected a scalar, got {beta.shape}")
        return cls(geo, color, multires, use_viewdir, multires_viewdir, density_beta=float(beta.reshape(())), softplus_beta=softplus_beta,
                   geo_activation=geo_activation)

    @classmethod
    def from_checkpoint(cls, path, **kwargs) -> "TemplateFieldModule":
        """The ``'network'`` entry of the reference's ``net.pt``."""
        ckpt = torch.load(path, map_location="cpu")
        if not isinstance(ckpt, dict) or "network" not in ckpt:
            raise KeyError(f"{path}: no 'network' entry")
        return cls.from_state_dict(ckpt["network"], **kwargs)

    @classmethod
    def geometric_init(cls, multires: int = 6, widths: Sequence[int] = (512, 256, 256, 256, 256, 256), out: int = 257, skip: Sequence[int] = (4,),
                       color: Sequence[int] = (256, 256, 256), use_viewdir: bool = False, multires_viewdir: int = 3, bias: float = 0.7,
                       generator: Optional[torch.Generator] = None, density_beta: float = 0.01, softplus_beta: float = 100.0,
                       geo_activation: str = "softplus") -> "TemplateFieldModule":
        """A field to start a training from: ``SdfMLP``'s geometric initialisation (``network/mlp.py:213-241`` with ``bias = 0.7``,
        ``network/template.py:36-60``) -- about a sphere of radius ``bias`` -- with ``weight_g = ||weight_v||_row`` as ``weight_norm`` sets
        it, and ``nn.Linear``'s default initialisation for the colour MLP.  Every random number comes from ``generator`` (host)."""
        e_pos = embed_dim(multires)
        chans = [e_pos] + [int(w) for w in widths] + [int(out)]
        normal = lambda shape, mean, std: torch.empty(shape, dtype=torch.float32).normal_(mean, std, generator=generator)  # noqa: E731
        geo = []
        for l in range(len(chans) - 1):
            out_dim, in_dim = chans[l + 1], chans[l] + (e_pos if l in skip else 0)
            if l == len(chans) - 2:
                v, b = normal((out_dim, in_dim), float(np.sqrt(np.pi) / np.sqrt(in_dim)), 0.0001), torch.full((out_dim,), -float(bias))
            else:
                v, b = normal((out_dim, in_dim), 0.0, float(np.sqrt(2) / np.sqrt(out_dim))), torch.zeros(out_dim)
                if l == 0:
                    v[:, 3:] = 0.0
                elif l in skip and e_pos > 3:
                    v[:, -(e_pos - 3):] = 0.0
            geo.append((v, v.norm(dim=1, keepdim=True), b))
        cch = [int(out) - 1 + (embed_dim(multires_viewdir) if use_viewdir else 0)] + [int(c) for c in color] + [3]
        col = []
        for l in range(len(cch) - 1):
            bound = 1.0 / float(np.sqrt(cch[l]))                          # kaiming_uniform_(a = sqrt 5) and the bias: both U(-1 / sqrt in, 1 / sqrt in)
            col.append((torch.empty((cch[l + 1], cch[l])).uniform_(-bound, bound, generator=generator),
                        torch.empty(cch[l + 1]).uniform_(-bound, bound, generator=generator)))
        return cls(geo, col, multires, use_viewdir, multires_viewdir, density_beta=density_beta, softplus_beta=softplus_beta, geo_activation=geo_activation)

    # ---- the two blobs as gathers ---------------------------------------------------------------------------------------------------
    def _color_linears(self):
        return self.tex_mlp.linears() if self.tex_mlp is not None else []

    def _index_maps(self):
        """``(idx_fwd, idx_t, weights, biases)``: with ``flat`` = every folded weight [out, in] row-major in plan order, then every bias,
        then ONE zero, ``flat[idx_fwd]`` is the blob of ``include/ag_template_field.h`` and ``flat[idx_t]`` the transposed blob of
        ``include/ag_template_field_train.h``.  Built once on the host from ``TemplateField._layout`` / ``_columns`` and ``mlp_blob._order``."""
        f = self.plan
        layout, total = f._layout()
        n_w = sum(width * K for _, K, width, *_ in f.layers)
        n_b = sum(width for _, K, width, *_ in f.layers)
        zero = n_w + n_b
        idx_fwd, idx_t = np.full(total, zero, np.int64), []
        w_at, b_at = 0, n_w
        for i, ((net, K, width, *_), (Ka, e_cols, Ke, Np, w_off, b_off)) in enumerate(zip(f.layers, layout)):
            wi = w_at + np.arange(width * K, dtype=np.int64).reshape(width, K)
            bi = b_at + np.arange(width, dtype=np.int64)
            cols = f._columns(i)
            rows = np.full((Ka + Ke, Np), zero, np.int64)                  # [packed k][packed n]
            rows[:Ka + e_cols, cols] = wi.T
            idx_fwd[w_off:b_off] = rows.reshape(-1)[_order(Ka + Ke, Np)]
            idx_fwd[b_off + cols] = bi
            if Ka:
                wp = np.full((Np, Ka), zero, np.int64)                     # [packed n][k]: the block is [n / 4][k][4]
                wp[cols] = wi[:, :Ka]
                idx_t.append(wp.reshape(-1)[_order(Np, Ka)])
            w_at += width * K
            b_at += width
        return idx_fwd, np.concatenate(idx_t) if idx_t else np.zeros(0, np.int64), n_w, n_b

    def _maps_on(self, dev):
        key = (dev.type, dev.index)
        if key not in self._device_maps:
            self._device_maps[key] = (torch.from_numpy(self._idx_fwd).to(dev), torch.from_numpy(self._idx_t).to(dev))
        return self._device_maps[key]

    def folded_weights(self):
        """``[(W [out, in], bias)]`` of every layer in plan order as fp32 tensors on the parameters' device, the weight norm folded in torch."""
        return [(lin.folded(), lin.bias) for lin in self.geo_mlp.linears() + self._color_linears()]

    def flat_parameters(self) -> torch.Tensor:
        """Every folded weight in plan order, then every bias: the vector the kernels' gradient is taken with respect to."""
        layers = self.folded_weights()
        return torch.cat([w.reshape(-1) for w, _ in layers] + [b for _, b in layers])

    def pack(self, flat: Optional[torch.Tensor] = None):
        """``(blob, transposed blob)`` of ``flat`` (default: ``flat_parameters()``) by the two gathers of the forward, on ``flat``'s
        device (a host tensor works: the maps need no GPU)."""
        flat = self.flat_parameters().detach() if flat is None else flat
        flat_z = torch.cat([flat, flat.new_zeros(1)])
        return flat_z[torch.from_numpy(self._idx_fwd).to(flat.device)], flat_z[torch.from_numpy(self._idx_t).to(flat.device)]

    def unpack_transposed(self, blob_t) -> list:
        """Per layer the ``[Ka, out]`` array ``W[:, :Ka].T`` read back from a transposed blob (None for layer 0, which has none)."""
        blob_t = np.asarray(blob_t, np.float32)
        layout, _ = self.plan._layout()
        out, off = [], 0
        for i, ((net, K, width, *_), (Ka, e_cols, Ke, Np, _, _)) in enumerate(zip(self.plan.layers, layout)):
            if not Ka:
                out.append(None)
                continue
            wp = np.empty(Np * Ka, np.float32)
            wp[_order(Np, Ka)] = blob_t[off:off + Np * Ka]
            out.append(np.ascontiguousarray(wp.reshape(Np, Ka)[self.plan._columns(i)].T))
            off += Np * Ka
        return out

    # ---- evaluation -----------------------------------------------------------------------------------------------------------------
    @property
    def beta(self) -> torch.Tensor:
        """``density_func.beta``: what ``render_train`` / ``laplace_density`` take as ``beta``."""
        return self.density_func.beta

    def forward(self, xyz: torch.Tensor, viewdirs: Optional[torch.Tensor] = None):
        """``xyz`` [N, 3], ``viewdirs`` [N, 3] or None (zeros; ignored without ``use_viewdir``), float32 on the GPU -> ``(sdf [N, 1], color
        [N, 3])`` (``color`` None for a field without a colour MLP), differentiable with respect to every parameter of the two MLPs.

        The weight norm is folded in torch on the device in fp32, the two blobs are one gather each from the flat parameter vector, and
        the rest is ``ag_template_field_train_forward`` / ``_backward``.  The gradient with respect to ``xyz`` and ``viewdirs`` is None: the
        eikonal term's second-order pass is not built."""
        if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be a float32 [N, 3] tensor on the GPU (there is no host path)")
        if self.beta.device != xyz.device:
            raise ValueError(f"the module's parameters are on {self.beta.device}, xyz on {xyz.device}")
        xyz = xyz.detach().contiguous()
        if viewdirs is not None:
            if not isinstance(viewdirs, torch.Tensor) or viewdirs.device != xyz.device or viewdirs.dtype != torch.float32 or tuple(viewdirs.shape) != tuple(xyz.shape):
                raise ValueError(f"viewdirs must be float32 {tuple(xyz.shape)} on the device of xyz")
            viewdirs = viewdirs.detach().contiguous() if self._arch["use_viewdir"] else None
        return _FieldTrain.apply(self.flat_parameters(), xyz, viewdirs, self)

    def to_field(self) -> TemplateField:
        """A ``TemplateField`` of the current parameters for inference, mesh extraction and ``render``, through ``state_dict()`` and
        ``TemplateField.from_state_dict``: the weight norm folded ONCE in float64 there, in fp32 here, so the two forwards differ by
        the fold's rounding only."""
        a = self._arch
        return TemplateField.from_state_dict(self.state_dict(), a["multires"], a["use_viewdir"], a["multires_viewdir"], softplus_beta=a["softplus_beta"],
                                             geo_activation=a["geo_activation"])
