"""The template stage's SDF and colour field on the GPU (``include/ag_template_field.h``): points -> sdf, density, colour.

Re-host of the reference's ``TemplateNet.forward_cano_body_nerf`` (``network/template.py:98-140``) without ``compute_grad``: the
positional embedding (``utils/embedder.py``), the weight-normalised ``SdfMLP`` and the colour ``MLPLinear`` (``network/mlp.py``) and
``LaplaceDensity`` (``network/density.py:22-36``), evaluated by ONE fused HIP kernel that keeps a tile of points in LDS from the embedding to
the outputs.  ``sdf_grid`` / ``extract_mesh`` are ``TemplateTrainer.test_geometry`` in canonical space (``main_template.py:103-133``): a
reference template checkpoint becomes the mesh that ``obj_io.save_mesh_ply`` writes as ``template.ply``.

``sdf_normal`` is the same function with ``compute_grad`` (``template.py:129-139``): the gradient of the raw SDF with respect to the points,
the reference's ``'normal'``, by a second fused kernel that pushes three tangents through the geometry MLP beside the value
(``include/ag_template_field_grad.h``); ``eikonal_loss`` is ``main_template.py:53-58`` on it.

NOT here: the gradient with respect to the weights, which is ``template_train.TemplateFieldModule`` (a layer-wise path beside this fused
kernel; ``module.to_field()`` comes back here); the eikonal term's second-order pass is not built.  Ray sampling and compositing, the other half
of ``TemplateNet.render``, are ``template_render.py``; the hand fusion (``fuse_hands``, a checkpoint's ``left_hand.*`` / ``right_hand.*``) is
``hand_fusion.py``.  Every tensor must be on the GPU; there is no host path
and no PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import isosurface
from .mlp_blob import pack_rows, pad, ptr, stream, unpack_rows

ACT_NONE, ACT_SOFTPLUS, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3          # include/ag_template_field.h
CONCAT_NONE, CONCAT_POSITION, CONCAT_VIEW = 0, 1, 2
MAX_LAYERS, MAX_WIDTH, MAX_MULTIRES, MAX_MULTIRES_VIEW = 8, 512, 10, 4
GRID_CHUNK = 256 * 256 * 4          # points per launch of sdf_grid, the chunk of the reference's test_geometry


def embed_dim(multires: int) -> int:
    return 3 + 6 * int(multires)


def fold_weight_norm(g, v) -> np.ndarray:
    """``W = g * v / ||v||_row`` (``torch.nn.utils.weight_norm``, dim 0) in float64, rounded ONCE to float32."""
    v64 = np.asarray(v, np.float64)
    g64 = np.asarray(g, np.float64).reshape(-1, 1)
    return (g64 * v64 / np.sqrt((v64 * v64).sum(axis=1, keepdims=True))).astype(np.float32)


def _array(sd, key):
    if key not in sd:
        raise KeyError(f"state dict has no {key!r}")
    t = sd[key]
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _linear(sd, prefix):
    """(W [out, in] float32, bias [out] float32) of the linear at ``prefix``: weight-normalised in either spelling, or plain."""
    if prefix + "weight_v" in sd or prefix + "weight_g" in sd:
        gk, vk = prefix + "weight_g", prefix + "weight_v"
    elif prefix + "parametrizations.weight.original1" in sd or prefix + "parametrizations.weight.original0" in sd:
        gk, vk = prefix + "parametrizations.weight.original0", prefix + "parametrizations.weight.original1"
    else:
        gk, vk = None, prefix + "weight"
    v = _array(sd, vk)
    if v.ndim != 2:
        raise ValueError(f"{vk}: expected [out, in], got {v.shape}")
    if gk is None:
        w = v.astype(np.float32)
    else:
        g = _array(sd, gk)
        if g.size != v.shape[0] or g.shape not in ((v.shape[0], 1), (v.shape[0],)):
            raise ValueError(f"{gk}: expected [{v.shape[0]}, 1], got {g.shape}")
        w = fold_weight_norm(g, v)
    b = _array(sd, prefix + "bias")
    if b.shape != (v.shape[0],):
        raise ValueError(f"{prefix}bias: expected [{v.shape[0]}], got {b.shape}")
    return w, b.astype(np.float32)


def _mlp(sd, root, must_be_normalised):
    """The linears of ``root.fc_list``: ``{i}.0.*`` for the hidden ones (``nn.Sequential(linear, activation)``), ``{i}.*`` for the last."""
    out = []
    for i in range(MAX_LAYERS + 1):
        hidden, last = f"{root}.fc_list.{i}.0.", f"{root}.fc_list.{i}."
        is_hidden = any(k.startswith(hidden) for k in sd)
        if not is_hidden and not any(k.startswith(last) for k in sd):
            raise KeyError(f"state dict has no {hidden}weight* and no {last}weight*: {root} has no last layer")
        prefix = hidden if is_hidden else last
        if must_be_normalised and prefix + "weight" in sd:
            raise KeyError(f"state dict has no {prefix}weight_g: every linear of {root} is weight-normalised")
        out.append(_linear(sd, prefix))
        if not is_hidden:
            return out
    raise ValueError(f"{root} has more than {MAX_LAYERS} linears")


def volume_axes(bounds, res):
    """The three coordinate vectors of ``net_util.generate_volume_points`` (``utils/net_util.py:48-62``): ``torch.linspace(0, 1, n)`` in
    float32, ``* (b1 - b0) + b0``, each operation rounded on its own.  Host tensors: ``3 * n`` values decide every point of the grid."""
    b = bounds.detach().cpu() if isinstance(bounds, torch.Tensor) else torch.from_numpy(np.asarray(bounds))
    b = b.to(torch.float32)
    if tuple(b.shape) != (2, 3):
        raise ValueError(f"bounds must be [2, 3], got {tuple(b.shape)}")
    res = tuple(int(r) for r in res)
    if len(res) != 3 or min(res) < 1:
        raise ValueError(f"res must be three positive sizes, got {res}")
    return [torch.linspace(0, 1, steps=res[d], dtype=torch.float32) * (b[1, d] - b[0, d]) + b[0, d] for d in range(3)]


def volume_points(axes, x0: int, x1: int) -> torch.Tensor:
    """Rows ``x0 * Y * Z .. x1 * Y * Z`` of ``generate_volume_points``' [X * Y * Z, 3] (row-major, Z fastest), on the axes' device."""
    ax, ay, az = axes
    nx, ny, nz = x1 - x0, ay.shape[0], az.shape[0]
    pts = torch.empty((nx, ny, nz, 3), dtype=torch.float32, device=ax.device)
    pts[..., 0] = ax[x0:x1].view(nx, 1, 1)
    pts[..., 1] = ay.view(1, ny, 1)
    pts[..., 2] = az.view(1, 1, nz)
    return pts.view(-1, 3)


def _points(xyz) -> torch.Tensor:
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise ValueError("xyz must be a tensor on the GPU (there is no host path)")
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be float32 [N, 3], got {xyz.dtype} {tuple(xyz.shape)}")
    return xyz.detach().contiguous()


def eikonal_loss(normal: torch.Tensor) -> torch.Tensor:
    """``((||normal||_2 - 1)^2).mean()`` over the last axis (``main_template.py:55``), in torch ops on the tensor's device."""
    return ((torch.linalg.norm(normal, ord=2, dim=-1) - 1.0) ** 2).mean()


class TemplateField:
    """``geo`` / ``color``: lists of ``(W [out, in], bias [out])`` float32 arrays, already folded.  Layer 0 of ``geo`` takes the positional
    embedding; a later geometry layer whose input is ``previous width + embedding`` wide is a skip layer (the embedding AFTER the
    activations, ``mlp.py:116-119``).  The last geometry layer is ``1 + features`` wide; the first colour layer takes the features,
    followed by the view embedding when ``use_viewdir``."""

    def __init__(self, geo: Sequence, color: Sequence, multires: int = 6, use_viewdir: bool = False, multires_viewdir: int = 3,
                 density_beta: float = 0.01, softplus_beta: float = 100.0, geo_activation: str = "softplus"):
        if geo_activation not in ("softplus", "relu"):
            raise ValueError(f"geo_activation must be 'softplus' or 'relu', got {geo_activation!r}")
        self.multires, self.use_viewdir = int(multires), bool(use_viewdir)
        self.multires_viewdir = int(multires_viewdir) if self.use_viewdir else 0
        if not 0 <= self.multires <= MAX_MULTIRES or not 0 <= self.multires_viewdir <= MAX_MULTIRES_VIEW:
            raise ValueError(f"multires must be 0 .. {MAX_MULTIRES} and multires_viewdir 0 .. {MAX_MULTIRES_VIEW}, got {multires}, {multires_viewdir}")
        self.softplus_beta = float(softplus_beta)
        self.density_beta = float(density_beta)
        # LaplaceDensity.get_beta in fp32: |beta| + beta_min
        self.density_b = float(np.abs(np.float32(density_beta)) + np.float32(1e-4))
        if not (np.isfinite(self.softplus_beta) and self.softplus_beta > 0 and np.isfinite(self.density_b)):
            raise ValueError(f"softplus_beta must be finite and positive and density_beta finite, got {softplus_beta}, {density_beta}")
        self.geo = [(np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)) for w, b in geo]
        self.color = [(np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)) for w, b in color]
        self.layers = self._table(ACT_SOFTPLUS if geo_activation == "softplus" else ACT_RELU)
        self.blob = self.pack()
        self._device_blobs = {}

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, multires: int = 6, use_viewdir: bool = False, multires_viewdir: int = 3, *, softplus_beta: float = 100.0,
                        geo_activation: str = "softplus") -> "TemplateField":
        """``sd``: the reference's ``TemplateNet.state_dict()``.  ``geo_mlp.fc_list.{0..n-1}.0.*`` and ``geo_mlp.fc_list.{n}.*`` carry
        ``weight_g`` / ``weight_v`` (or ``parametrizations.weight.original0`` / ``original1``) and ``bias``; ``tex_mlp.fc_list.*`` plain
        ``weight`` / ``bias``; ``density_func.beta`` a scalar.  Everything else in ``sd`` is ignored: the volumes, and the two hands' networks, which
        ``hand_fusion.HandField.from_state_dict`` reads."""
        geo = _mlp(sd, "geo_mlp", must_be_normalised=True)
        color = _mlp(sd, "tex_mlp", must_be_normalised=False)
        beta = _array(sd, "density_func.beta")
        if beta.size != 1:
            raise ValueError(f"density_func.beta: expected a scalar, got {beta.shape}")
        return cls(geo, color, multires, use_viewdir, multires_viewdir, density_beta=float(beta.reshape(())), softplus_beta=softplus_beta,
                   geo_activation=geo_activation)

    @classmethod
    def from_checkpoint(cls, path, **kwargs) -> "TemplateField":
        """The ``'network'`` entry of the reference's ``net.pt`` (``base_trainer.py:59-66``)."""
        ckpt = torch.load(path, map_location="cpu")
        if not isinstance(ckpt, dict) or "network" not in ckpt:
            raise KeyError(f"{path}: no 'network' entry")
        return cls.from_state_dict(ckpt["network"], **kwargs)

    def _table(self, geo_act):
        """[(net, K, width, act, concat, prev)] per layer, checked against the limits of the header (the key-free restatement of
        ``make_plan`` in ``csrc/ag_template_field.hip``)."""
        e_pos, e_view = embed_dim(self.multires), embed_dim(self.multires_viewdir)
        if not 1 <= len(self.geo) <= MAX_LAYERS or len(self.color) > MAX_LAYERS:
            raise ValueError(f"1 .. {MAX_LAYERS} geometry and 0 .. {MAX_LAYERS} colour layers, got {len(self.geo)} and {len(self.color)}")
        rows, prev = [], 0
        for net, layers in (("geo", self.geo), ("color", self.color)):
            for li, (w, b) in enumerate(layers):
                name = f"{'geo_mlp' if net == 'geo' else 'tex_mlp'}.fc_list.{li}"
                if w.ndim != 2 or b.shape != (w.shape[0],):
                    raise ValueError(f"{name}: weight {w.shape} and bias {b.shape} do not fit")
                width, K = int(w.shape[0]), int(w.shape[1])
                last = li == len(layers) - 1
                if net == "geo":
                    if li == 0:
                        concat, want = CONCAT_POSITION, [e_pos]
                    else:
                        concat, want = (CONCAT_POSITION, [prev, prev + e_pos]) if K == prev + e_pos else (CONCAT_NONE, [prev, prev + e_pos])
                else:
                    concat = CONCAT_VIEW if (li == 0 and self.use_viewdir) else CONCAT_NONE
                    want = [prev + e_view] if concat == CONCAT_VIEW else [prev]
                if K not in want:
                    raise ValueError(f"{name}: weight is {w.shape}, its input has {' or '.join(str(k) for k in want)} columns")
                if not last:
                    ok = width % 32 == 0 and 32 <= width <= MAX_WIDTH
                elif net == "geo":
                    ok = (width - 1) % 32 == 0 and width - 1 <= MAX_WIDTH and (not self.color or width > 1)
                else:
                    ok = width == 3
                if not ok:
                    raise ValueError(f"{name}: width {width} (hidden layers: multiples of 32 up to {MAX_WIDTH}; last geometry layer 1 + 32 m; last colour layer 3)")
                act = (geo_act if net == "geo" else ACT_RELU) if not last else (ACT_NONE if net == "geo" else ACT_SIGMOID)
                rows.append((net, K, width, act, concat, prev))
                prev = width - 1 if (last and net == "geo") else width
        return rows

    def desc(self) -> "_lib.AgTemplateFieldDesc":
        d = _lib.AgTemplateFieldDesc()
        d.multires, d.multires_view = self.multires, self.multires_viewdir
        d.n_geo, d.n_color = len(self.geo), len(self.color)
        d.softplus_beta, d.density_b = self.softplus_beta, self.density_b
        for i, (net, K, width, act, concat, _) in enumerate(self.layers):
            row = d.geo[i] if net == "geo" else d.color[i - len(self.geo)]
            row.K, row.width, row.act, row.concat = K, width, act, concat
        return d

    # ---- the packed blob (include/ag_template_field.h "Packed weights") ----------------------------------------------------------------
    def _layout(self):
        """Per layer (Ka, e_cols, Ke, Np, w_off, b_off) and the total floats."""
        out, off = [], 0
        for net, K, width, act, concat, prev in self.layers:
            e_cols = K - prev
            Ke, Np = pad(e_cols, 8), pad(width, 32)
            out.append((prev, e_cols, Ke, Np, off, off + (prev + Ke) * Np))
            off += (prev + Ke) * Np + Np
        return out, off

    def _columns(self, i):
        """Packed column of every output column of layer ``i`` (the last geometry layer: features first, the SDF column last)."""
        net, K, width, *_ = self.layers[i]
        if net == "geo" and i == len(self.geo) - 1:
            return np.concatenate([[pad(width, 32) - 32], np.arange(width - 1)]).astype(np.int64)
        return np.arange(width, dtype=np.int64)

    def pack(self) -> np.ndarray:
        layout, total = self._layout()
        blob = np.zeros(total, np.float32)
        for i, ((w, b), (Ka, e_cols, Ke, Np, w_off, b_off)) in enumerate(zip(self.geo + self.color, layout)):
            rows = np.zeros((Ka + Ke, Np), np.float32)                      # [packed k][packed n]
            cols = self._columns(i)
            rows[:Ka + e_cols, cols] = w.T
            blob[w_off:b_off] = pack_rows(rows, Ka + Ke, Np)
            blob[b_off + cols] = b
        return blob

    def unpack(self, blob: Optional[np.ndarray] = None):
        """The inverse of ``pack``: ``([(W, bias)] of every layer, every padding element of the blob)``."""
        blob = self.blob if blob is None else np.asarray(blob, np.float32)
        layout, total = self._layout()
        if blob.shape != (total,):
            raise ValueError(f"blob of {blob.shape}, expected ({total},)")
        layers, padding = [], []
        for i, (Ka, e_cols, Ke, Np, w_off, b_off) in enumerate(layout):
            rows = unpack_rows(blob[w_off:b_off], Ka + Ke, Np)
            bias = blob[b_off:b_off + Np]
            cols = self._columns(i)
            layers.append((np.ascontiguousarray(rows[:Ka + e_cols, cols].T), bias[cols].copy()))
            used = np.zeros((Ka + Ke, Np), bool)
            used[:Ka + e_cols, cols] = True
            padding += [rows[~used], np.delete(bias, cols)]
        return layers, np.concatenate(padding)

    def _blob_on(self, dev) -> torch.Tensor:
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in self._device_blobs:
            self._device_blobs[key] = torch.from_numpy(self.blob).to(dev)
        return self._device_blobs[key]

    # ---- evaluation -----------------------------------------------------------------------------------------------------------------
    def _forward(self, xyz, viewdirs, sdf, density, color):
        L = _lib.lib()
        dev = xyz.device
        blob = self._blob_on(dev)
        d = self.desc()
        with _lib.on_device(dev):
            _lib.check(L.ag_template_field_forward(ctypes.byref(d), ptr(blob), blob.numel(), ptr(xyz), ptr(viewdirs), xyz.shape[0], ptr(sdf), ptr(density),
                                                   ptr(color), stream(dev)), "ag_template_field_forward")

    def __call__(self, xyz: torch.Tensor, viewdirs: Optional[torch.Tensor] = None, want=("sdf",)):
        """``xyz`` [N, 3] float32 on the GPU -> dict of device tensors: ``sdf`` [N, 1] (always; positive inside, ``template.py:123``),
        ``density`` [N, 1] and ``color`` [N, 3] when named in ``want``, and ``cano_xyz`` (the points, as the reference's dict).
        ``viewdirs`` [N, 3] or None (zeros, ``template.py:115-116``); ignored by a field built without ``use_viewdir``, as in the
        reference.  Without ``"color"`` the feature columns of the last geometry layer and the colour MLP are not computed."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= {"sdf", "density", "color"}:
            raise ValueError(f"want names 'sdf', 'density', 'color', got {want}")
        if "color" in want and not self.color:
            raise ValueError("this field has no colour MLP")
        xyz = _points(xyz)
        if viewdirs is not None:
            if not isinstance(viewdirs, torch.Tensor) or viewdirs.device != xyz.device:
                raise ValueError("viewdirs must be a tensor on the device of xyz")
            if viewdirs.dtype != torch.float32 or tuple(viewdirs.shape) != tuple(xyz.shape):
                raise ValueError(f"viewdirs must be float32 {tuple(xyz.shape)}, got {viewdirs.dtype} {tuple(viewdirs.shape)}")
            viewdirs = viewdirs.detach().contiguous() if self.use_viewdir else None
        n = xyz.shape[0]
        out = {"sdf": torch.empty((n, 1), dtype=torch.float32, device=xyz.device)}
        if "density" in want:
            out["density"] = torch.empty((n, 1), dtype=torch.float32, device=xyz.device)
        if "color" in want:
            out["color"] = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
        if n:
            self._forward(xyz, viewdirs, out["sdf"], out.get("density"), out.get("color"))
        out["cano_xyz"] = xyz
        return out

    def sdf_normal(self, xyz: torch.Tensor, want=("sdf", "normal")):
        """``forward_cano_body_nerf`` with ``compute_grad``: ``xyz`` [N, 3] float32 on the GPU -> dict of device tensors: ``sdf`` [N, 1],
        ``normal`` [N, 3] (both always), ``density`` [N, 1] when named in ``want``, and ``cano_xyz``.  ``normal`` is the reference's: the
        gradient of the RAW SDF (minus the gradient of ``sdf``) with respect to the points, NOT normalised; it points out of the body.
        ``sdf`` and ``density`` are ``__call__``'s bit for bit.  The colour MLP does not run and view directions play no part."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= {"sdf", "normal", "density"}:
            raise ValueError(f"want names 'sdf', 'normal', 'density', got {want}")
        xyz = _points(xyz)
        n, dev = xyz.shape[0], xyz.device
        out = {"sdf": torch.empty((n, 1), dtype=torch.float32, device=dev), "normal": torch.empty((n, 3), dtype=torch.float32, device=dev)}
        if "density" in want:
            out["density"] = torch.empty((n, 1), dtype=torch.float32, device=dev)
        if n:
            blob = self._blob_on(dev)
            d = self.desc()
            with _lib.on_device(dev):
                _lib.check(_lib.lib().ag_template_field_sdf_grad(ctypes.byref(d), ptr(blob), blob.numel(), ptr(xyz), n, ptr(out["sdf"]), ptr(out["normal"]),
                                                                 ptr(out.get("density")), stream(dev)), "ag_template_field_sdf_grad")
        out["cano_xyz"] = xyz
        return out

    def surface_normals(self, points: torch.Tensor) -> torch.Tensor:
        """Unit normals [N, 3] of the level set through each of ``points``: ``normal / max(||normal||, 1e-12)``.  They point outward, the
        orientation of the normals ``extract_mesh`` returns."""
        n = self.sdf_normal(points)["normal"]
        return n / torch.linalg.norm(n, dim=-1, keepdim=True).clamp_min(1e-12)

    def sdf_grid(self, bounds, res, device=None) -> torch.Tensor:
        """The SDF at the nodes of ``net_util.generate_volume_points(bounds, res)`` as ``[X, Y, Z]`` float32 on ``device`` (default: the
        current GPU).  The points are assembled on the device slab by slab along X (about ``GRID_CHUNK`` points each) from the three host
        coordinate vectors of ``volume_axes``, so no [X * Y * Z, 3] buffer exists; every slab's SDF is written in place."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("sdf_grid runs on the GPU (there is no host path)")
        axes = [a.to(dev) for a in volume_axes(bounds, res)]
        X, Y, Z = (int(a.shape[0]) for a in axes)
        vol = torch.empty((X, Y, Z), dtype=torch.float32, device=dev)
        flat = vol.view(-1)
        step = max(1, GRID_CHUNK // (Y * Z))
        for x0 in range(0, X, step):
            x1 = min(X, x0 + step)
            self._forward(volume_points(axes, x0, x1), None, flat[x0 * Y * Z:x1 * Y * Z], None, None)
        return vol

    def extract_mesh(self, bounds, res=(256, 256, 128), device=None):
        """``template.ply``'s mesh: ``(vertices [V, 3], faces [F, 3] int32, normals [V, 3])`` of the zero level set, as
        ``test_geometry`` + ``recon_mesh`` (``main_template.py:103-133``) with ``iso_value = 0``."""
        return isosurface.recon_mesh(self.sdf_grid(bounds, res, device), res, bounds, iso_value=0.0)
