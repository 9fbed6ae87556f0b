"""Fuse the hand fields into the template field on the GPU (``include/ag_hand_fusion.h``): near the hands ``sdf``, ``density`` and ``color``
of the body field become a blend with a signed distance to the MANO mesh and a small per-hand colour MLP.

Re-host of the reference's ``TemplateNet.fuse_hands`` (``network/template.py:146-202``) for one batch element with the two ``HandAvatar``
colour networks (``network/hand_avatar.py``): what a template checkpoint trained with ``with_hand: true`` needs to be rendered.

    gate (cano_xyz, the two canonical boxes)  ->  active points  ->  mesh_query.closest_point on each hand  ->  ONE fused kernel:
    interpolate, signed distance, embedding, six-layer MLP per hand, blend, density  ->  scatter into copies of the body's values

The gate is a kernel of its own in the same file as the fused kernel and shares its device function, so both take the same decision
bit for bit; picking the active points, gathering them and scattering the results back are torch ops (``nonzero``, indexing,
``index_copy_``): exact copies, nothing to restate.  ``compact=False`` runs every point through the closest-point queries and the fused
kernel; the results are bit-identical, because a point's outputs depend on nothing but its own inputs.

``hand_pose``: the reference's only call site passes zeros (``template.py:178``).  Its 60 quaternion columns are constant over the points
and are folded into the first layer's bias on the host (``HandField.folded_bias``); a caller's pose goes through the same fold.

NOT here: any backward (template training).  The vertex normals of ``hand_meshes`` are ``subject_maps.vertex_normals``; parity with
trimesh's ``vertex_normals`` (``dataset/commons.py:22-31``) is not claimed, trimesh is not available to this package.  Every tensor must be on
the GPU; there is no host path and no PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .mlp_blob import pack_rows, pad, ptr as _p, stream as _stream, unpack_rows
from .template_field import _array, embed_dim

MAX_LAYERS, MAX_MULTIRES = 8, 10             # include/ag_hand_fusion.h
# How the closest-point kernel reads the face records (mesh_query.WALKS; time only, the results are bit-identical).  A hand has about
# 1500 faces and a chunk tens of thousands of active points: measured at 9 229 / 65 536 / 262 144 points x 1536 faces, 'tiled' takes
# 0.46 / 0.48 / 0.79 ms per query where the default takes 0.76 / 0.75 / 0.95 ms (profiles/hand_fusion.txt).
QUERY_WALK = "tiled"
WIDTHS = (32, 64)
SIDES = ("left", "right")


def axis_angle_to_quaternion(axis_angle) -> np.ndarray:
    """[..., 3] -> [..., 4] (w, x, y, z) in float64: ``pytorch3d.transforms.axis_angle_to_quaternion``'s formula, its small-angle series
    (``0.5 - angle^2 / 48`` below 1e-6) included."""
    aa = np.asarray(axis_angle, np.float64)
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    small = np.abs(angle) < 1e-6
    k = np.where(small, 0.5 - angle * angle / 48.0, np.sin(0.5 * angle) / np.where(small, 1.0, angle))
    return np.concatenate([np.cos(0.5 * angle), aa * k], -1)


def _linears(sd, root):
    """[(W, bias)] of ``root.fc_list``: ``{i}.0.*`` for the hidden linears, ``{i}.*`` for the last; every error names its key."""
    out = []
    for i in range(MAX_LAYERS + 1):
        hidden, last = f"{root}.fc_list.{i}.0.", f"{root}.fc_list.{i}."
        is_hidden = hidden + "weight" in sd or hidden + "bias" in sd
        prefix = hidden if is_hidden else last
        w, b = _array(sd, prefix + "weight"), _array(sd, prefix + "bias")          # KeyError names the key
        if w.ndim != 2:
            raise ValueError(f"{prefix}weight: expected [out, in], got {w.shape}")
        if b.shape != (w.shape[0],):
            raise ValueError(f"{prefix}bias: expected [{w.shape[0]}], got {b.shape}")
        out.append((prefix, w.astype(np.float32), b.astype(np.float32)))
        if not is_hidden:
            return out
    raise ValueError(f"{root} has more than {MAX_LAYERS} linears")


class HandField:
    """One hand's colour MLP.  ``layers``: ``[(W [out, in], bias [out])]`` float32; layer 0 takes ``[emb(x, multires), sdf_h, quat]``
    (``4 + 6 multires + 4 joints`` columns), the hidden layers are 32 or 64 wide with ReLU, the last is 3 wide with a sigmoid."""

    def __init__(self, layers: Sequence, multires: int = 4, names: Optional[Sequence[str]] = None):
        self.multires = int(multires)
        if not 0 <= self.multires <= MAX_MULTIRES:
            raise ValueError(f"multires must be 0 .. {MAX_MULTIRES}, got {multires}")
        self.layers = [(np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)) for w, b in layers]
        names = list(names) if names is not None else [f"layer {i} " for i in range(len(self.layers))]
        if not 2 <= len(self.layers) <= MAX_LAYERS:
            raise ValueError(f"2 .. {MAX_LAYERS} linears, got {len(self.layers)}")
        self.k_point = embed_dim(self.multires) + 1                     # columns of layer 0 that vary with the point
        prev = None
        for i, ((w, b), name) in enumerate(zip(self.layers, names)):
            last = i == len(self.layers) - 1
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"{name}weight: {w.shape} and bias {b.shape} do not fit")
            if i == 0:
                pose = w.shape[1] - self.k_point
                if pose < 0 or pose % 4:
                    raise ValueError(f"{name}weight: {w.shape[1]} input columns, expected {self.k_point} + 4 per joint (88 for the reference's hand)")
            elif w.shape[1] != prev:
                raise ValueError(f"{name}weight: {w.shape[1]} input columns, the previous layer has {prev} outputs")
            if (w.shape[0] != 3) if last else (w.shape[0] not in WIDTHS):
                raise ValueError(f"{name}weight: {w.shape[0]} outputs (hidden layers {WIDTHS[0]} or {WIDTHS[1]}, the last layer 3)")
            prev = w.shape[0]
        self.n_joints = (self.layers[0][0].shape[1] - self.k_point) // 4
        self._device_blobs = {}

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, side: str, multires: int = 4) -> "HandField":
        """``sd``: the reference's ``TemplateNet.state_dict()``; ``side``: ``'left'`` or ``'right'``.  Reads
        ``{side}_hand.tex_mlp.fc_list.{0..n-1}.0.{weight,bias}`` and ``fc_list.{n}.{weight,bias}``."""
        if side not in SIDES:
            raise ValueError(f"side must be 'left' or 'right', got {side!r}")
        rows = _linears(sd, f"{side}_hand.tex_mlp")
        return cls([(w, b) for _, w, b in rows], multires, names=[p for p, _, _ in rows])

    # ---- the packed blob (include/ag_hand_fusion.h "Packed weights") ---------------------------------------------------------------------
    def folded_bias(self, hand_pose=None) -> np.ndarray:
        """``bias0' = bias0 + W0[:, 4 + 6 L:] . quat(hand_pose)`` in float64, rounded once; ``hand_pose`` [3 joints] axis-angle or None
        (zeros: every quaternion is (1, 0, 0, 0))."""
        w0, b0 = self.layers[0]
        pose = np.zeros(3 * self.n_joints) if hand_pose is None else host_pose(hand_pose)
        if pose.shape != (3 * self.n_joints,):
            raise ValueError(f"hand_pose must hold {3 * self.n_joints} values, got {pose.shape}")
        quat = axis_angle_to_quaternion(pose.reshape(-1, 3)).reshape(-1)
        return (b0.astype(np.float64) + w0[:, self.k_point:].astype(np.float64) @ quat).astype(np.float32)

    def desc(self) -> "_lib.AgHandFusionDesc":
        d = _lib.AgHandFusionDesc()
        d.multires, d.n_layers = self.multires, len(self.layers)
        for i, (w, _) in enumerate(self.layers):
            d.width[i] = w.shape[0]
        return d

    def _layout(self):
        """Per layer (K, Kp, Np, w_off, b_off) and the total floats."""
        out, off = [], 0
        for i, (w, _) in enumerate(self.layers):
            K = self.k_point if i == 0 else w.shape[1]
            Kp, Np = pad(K, 8), pad(w.shape[0], 32)
            out.append((K, Kp, Np, off, off + Kp * Np))
            off += Kp * Np + Np
        return out, off

    def pack(self, hand_pose=None) -> np.ndarray:
        layout, total = self._layout()
        blob = np.zeros(total, np.float32)
        for i, ((w, b), (K, Kp, Np, w_off, b_off)) in enumerate(zip(self.layers, layout)):
            blob[w_off:b_off] = pack_rows(w[:, :K].T, Kp, Np)
            blob[b_off:b_off + w.shape[0]] = self.folded_bias(hand_pose) if i == 0 else b
        return blob

    def unpack(self, blob: np.ndarray):
        """The inverse of ``pack``: ``([(W[:, :K], bias)] of every layer (layer 0: the point columns and the folded bias), every padding
        element of the blob)``."""
        blob = np.asarray(blob, np.float32)
        layout, total = self._layout()
        if blob.shape != (total,):
            raise ValueError(f"blob of {blob.shape}, expected ({total},)")
        layers, padding = [], []
        for (w, _), (K, Kp, Np, w_off, b_off) in zip(self.layers, layout):
            rows = unpack_rows(blob[w_off:b_off], Kp, Np)
            bias = blob[b_off:b_off + Np]
            layers.append((np.ascontiguousarray(rows[:K, :w.shape[0]].T), bias[:w.shape[0]].copy()))
            padding += [rows[K:].reshape(-1), rows[:K, w.shape[0]:].reshape(-1), bias[w.shape[0]:]]
        return layers, np.concatenate(padding)

    def same_shape(self, other: "HandField") -> bool:
        return self.multires == other.multires and [w.shape[0] for w, _ in self.layers] == [w.shape[0] for w, _ in other.layers]

    def _blob_on(self, dev, hand_pose=None) -> torch.Tensor:
        """The packed blob on ``dev``.  Per device one blob for the zero pose, kept, and one for the LAST other pose, replaced when the pose
        changes: a caller with a new pose every frame holds two blobs, not one per frame.  A hit folds nothing."""
        pose = host_pose(hand_pose)
        index = torch.cuda.current_device() if dev.type == "cuda" and dev.index is None else dev.index
        slot = self._device_blobs.setdefault((dev.type, index), {})
        if pose is None or not pose.any():
            if "zero" not in slot:
                slot["zero"] = torch.from_numpy(self.pack(None)).to(dev)
            return slot["zero"]
        key = pose.tobytes()
        if slot.get("posed", (None, None))[0] != key:
            slot["posed"] = (key, torch.from_numpy(self.pack(pose)).to(dev))
        return slot["posed"][1]


def host_pose(hand_pose) -> Optional[np.ndarray]:
    """``hand_pose`` as a flat float64 array on the host (None stays None).  A device tensor costs one copy and sync: ``render`` does it
    once, before its chunk loop."""
    if hand_pose is None or (isinstance(hand_pose, np.ndarray) and hand_pose.dtype == np.float64 and hand_pose.ndim == 1):
        return hand_pose
    return np.asarray(hand_pose.detach().cpu().numpy() if isinstance(hand_pose, torch.Tensor) else hand_pose, np.float64).reshape(-1)


def hand_fields_from_checkpoint(path, multires: int = 4):
    """``(left, right)`` ``HandField`` of the ``'network'`` entry of the reference's ``net.pt``, beside ``TemplateField.from_checkpoint``."""
    ckpt = torch.load(path, map_location="cpu")
    if not isinstance(ckpt, dict) or "network" not in ckpt:
        raise KeyError(f"{path}: no 'network' entry")
    return tuple(HandField.from_state_dict(ckpt["network"], side, multires) for side in SIDES)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def hand_topology(left_ids, right_ids, faces_closed):
    """Host part of ``hand_meshes``: ``(left_ids [Vh] int64, right_ids [Vh] int64, left_faces [Fh, 3] int32, right_faces [Fh, 3] int32)``
    as numpy arrays.  The ids pick the hands' vertices out of the SMPL-X vertices (``smpl_vert_id_to_mano``); ``faces_closed`` is the
    closed MANO topology of a RIGHT hand, so the left hand, its mirror image, takes every face reversed: ``faces[:, [2, 1, 0]]``
    (``dataset/commons.py:22-31``, ``template.py:96``)."""
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    li, ri = to_np(left_ids).astype(np.int64).reshape(-1), to_np(right_ids).astype(np.int64).reshape(-1)
    f = to_np(faces_closed).astype(np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces_closed must be [F, 3], got {f.shape}")
    if li.shape != ri.shape:
        raise ValueError(f"left_ids {li.shape} and right_ids {ri.shape} must have one length")
    if f.size and (f.min() < 0 or f.max() >= len(li)):
        raise ValueError(f"faces_closed indexes vertices {f.min()} .. {f.max()}, the hands have {len(li)}")
    if min(li.min(initial=0), ri.min(initial=0)) < 0:
        raise ValueError("left_ids / right_ids must not be negative")
    return li, ri, np.ascontiguousarray(f[:, [2, 1, 0]].astype(np.int32)), np.ascontiguousarray(f.astype(np.int32))


def hand_meshes(smplx_vertices: torch.Tensor, left_ids, right_ids, faces_closed) -> dict:
    """``smplx_vertices`` [V, 3] on the GPU (posed or canonical) -> ``{'left': {'v', 'n', 'f'}, 'right': {'v', 'n', 'f'}}``: the two hands'
    vertices [Vh, 3], angle-weighted unit vertex normals [Vh, 3] (``subject_maps.vertex_normals``, outward for both hands) and faces
    [Fh, 3] int32; the reference's ``generate_two_manos`` (``dataset/commons.py:22-31``) with this package's normals."""
    from .subject_maps import _dev, vertex_normals
    v = _dev(smplx_vertices, "smplx_vertices", torch.float32, 3)
    li, ri, lf, rf = hand_topology(left_ids, right_ids, faces_closed)
    if max(li.max(initial=-1), ri.max(initial=-1)) >= v.shape[0]:
        raise ValueError(f"left_ids / right_ids index vertex {max(li.max(), ri.max())}, smplx_vertices has {v.shape[0]}")
    out = {}
    for side, ids, f in (("left", li, lf), ("right", ri, rf)):
        hv = v[torch.from_numpy(ids).to(v.device)].contiguous()
        ft = torch.from_numpy(f).to(v.device)
        out[side] = {"v": hv, "n": vertex_normals(hv, ft), "f": ft}
    return out


# ---- the fusion -----------------------------------------------------------------------------------------------------------------------
class _Hand:
    """One hand's device tensors as the kernel reads them, and its canonical box on the host."""

    def __init__(self, side, mesh, dev):
        from .subject_maps import _dev
        if not isinstance(mesh, dict) or not {"v", "n", "f", "cano_v"} <= set(mesh):
            raise ValueError(f"hands[{side!r}] must be dict(v=, n=, f=, cano_v=): vertices and normals in the render's space, faces, canonical vertices")
        self.v = _dev(mesh["v"], f"{side} v", torch.float32, 3)
        self.n = _dev(mesh["n"], f"{side} n", torch.float32, 3)
        self.cano_v = _dev(mesh["cano_v"], f"{side} cano_v", torch.float32, 3)
        self.f = _dev(mesh["f"], f"{side} f", torch.int32, 3)
        for name, t in (("v", self.v), ("n", self.n), ("cano_v", self.cano_v), ("f", self.f)):
            if t.device != dev:
                raise ValueError(f"{side} {name} is on {t.device}, expected {dev}")
        V = self.v.shape[0]
        if V < 1 or self.n.shape[0] != V or self.cano_v.shape[0] != V:
            raise ValueError(f"{side} hand: v {tuple(self.v.shape)}, n {tuple(self.n.shape)} and cano_v {tuple(self.cano_v.shape)} must be one [V, 3], V >= 1")
        box = torch.stack([self.cano_v.min(0).values, self.cano_v.max(0).values]).cpu().numpy()       # exact; one host sync per prepare
        if not np.isfinite(box).all() or not (box[1] > box[0]).all():
            raise ValueError(f"{side} hand: the box of cano_v, {box.tolist()}, is empty or not finite")
        self.box = box.astype(np.float32)


class PreparedHands:
    """``hands`` checked, made contiguous and with the two canonical boxes reduced: built once per ``render`` (or per ``fuse_hands``)."""

    def __init__(self, hands, dev):
        if not isinstance(hands, dict) or not set(SIDES) <= set(hands):
            raise ValueError("hands must be dict(left=dict(v=, n=, f=, cano_v=), right=dict(...))")
        self.left, self.right = _Hand("left", hands["left"], dev), _Hand("right", hands["right"], dev)


def active_mask(cano_xyz: torch.Tensor, left_box, right_box, centre_y: float) -> torch.Tensor:
    """bool [N]: the points with a non-zero gate (``ag_hand_field_gate``); ``left_box`` / ``right_box``: (min_x, max_x) of the canonical hands."""
    n, dev = cano_xyz.shape[0], cano_xyz.device
    active = torch.empty(n, dtype=torch.uint8, device=dev)
    lb, rb = (ctypes.c_float * 2)(*[float(x) for x in left_box]), (ctypes.c_float * 2)(*[float(x) for x in right_box])
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ag_hand_field_gate(_p(cano_xyz), n, lb, rb, float(centre_y), _p(active), _stream(dev)), "ag_hand_field_gate")
    return active.to(torch.bool)


def _side_args(side: "_lib.AgHandSide", hand: _Hand, query, blob):
    dist2, face_id, bary = query
    side.dist2, side.face_id, side.bary = _p(dist2), _p(face_id), _p(bary)
    side.vertices, side.normals, side.cano_vertices, side.faces = _p(hand.v), _p(hand.n), _p(hand.cano_v), _p(hand.f)
    side.blob = _p(blob)
    side.V, side.F = hand.v.shape[0], hand.f.shape[0]
    for c in range(3):
        side.bbox_min[c], side.bbox_max[c] = float(hand.box[0, c]), float(hand.box[1, c])


def fuse_kernel(points, cano_xyz, sdf, density, color, prepared: PreparedHands, queries, left: HandField, right: HandField, centre_y: float,
                density_b: float, hand_pose=None):
    """The fused kernel alone, IN PLACE on ``sdf`` [N], ``density`` [N] and ``color`` [N, 3] (or None): ``queries`` =
    ``((dist2, face_id, bary) of the left hand, (..) of the right hand)`` as ``mesh_query.closest_point`` returns them for ``points``."""
    if not left.same_shape(right):
        raise ValueError("the two HandFields must have one multires and one list of widths")
    dev, n = points.device, points.shape[0]

    def fits(t, name, dtype, shape):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor {shape} on {dev}")
    fits(points, "points", torch.float32, (n, 3))
    fits(cano_xyz, "cano_xyz", torch.float32, (n, 3))
    fits(sdf, "sdf", torch.float32, (n,))
    fits(density, "density", torch.float32, (n,))
    if color is not None:
        fits(color, "color", torch.float32, (n, 3))
    for side, (dist2, face_id, bary) in zip(SIDES, queries):
        fits(dist2, f"{side} dist2", torch.float32, (n,))
        fits(face_id, f"{side} face_id", torch.int32, (n,))
        fits(bary, f"{side} bary", torch.float32, (n, 3))
    a = _lib.AgHandFieldFuseArgs()
    a.N, a.desc = points.shape[0], left.desc()
    a.centre_y, a.density_b = float(centre_y), float(density_b)
    a.points, a.cano_xyz = _p(points), _p(cano_xyz)
    a.sdf_in = a.sdf = _p(sdf)
    a.density_in = a.density = _p(density)
    a.color_in = a.color = _p(color)
    lb, rb = left._blob_on(dev, hand_pose), right._blob_on(dev, hand_pose)
    a.blob_floats = lb.numel()
    _side_args(a.left, prepared.left, queries[0], lb)
    _side_args(a.right, prepared.right, queries[1], rb)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ag_hand_field_fuse(ctypes.byref(a), _stream(dev)), "ag_hand_field_fuse")


def check_fields(left, right, hand_pose):
    """The checks of the two nets and the pose that need no device: -> ``hand_pose`` on the host (``host_pose``)."""
    if not isinstance(left, HandField) or not isinstance(right, HandField):
        raise ValueError("left and right must be HandFields")
    if not left.same_shape(right):
        raise ValueError("the two HandFields must have one multires and one list of widths")
    pose = host_pose(hand_pose)
    for side, f in zip(SIDES, (left, right)):
        if pose is not None and pose.shape != (3 * f.n_joints,):
            raise ValueError(f"hand_pose must hold {3 * f.n_joints} values for the {side} hand, got {pose.shape}")
    return pose


def _flat(t, name, cols, n, dev):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
        raise ValueError(f"{name} must be a tensor on {dev} (there is no host path)")
    if t.dtype != torch.float32 or t.numel() != n * cols:
        raise ValueError(f"{name} must hold {n} x {cols} float32 values, got {t.dtype} {tuple(t.shape)}")
    return t.detach().reshape(n, cols).contiguous()


def fuse_hands(body_ret: dict, posed_xyz: torch.Tensor, hands, left: HandField, right: HandField, *, cano_smpl_center, density_b: float,
               hand_pose=None, compact: bool = True) -> dict:
    """``TemplateNet.fuse_hands`` for one batch element.  ``body_ret``: the field's dict (``sdf`` [N, 1], ``density`` [N, 1], ``cano_xyz``
    [N, 3] and optionally ``color`` [N, 3]); ``posed_xyz`` [N, 3]: the same samples in the space they are rendered in (``cano_xyz`` itself
    for ``space='cano'``); ``hands``: ``dict(left=dict(v=, n=, f=, cano_v=), right=...)`` with ``v`` / ``n`` in the space of ``posed_xyz``
    (``hand_meshes`` + the canonical vertices) or a ``PreparedHands``; ``left`` / ``right``: the two ``HandField``; ``cano_smpl_center``
    [3] (its y is used); ``density_b``: the field's (``TemplateField.density_b``); ``hand_pose`` [45] or None (zeros).

    Returns a NEW dict: fused ``sdf``, ``density``, ``color`` (when ``body_ret`` has one) and ``cano_xyz`` passed through; ``body_ret`` is
    not modified.  A point whose two gates are 0 keeps the body's values bit for bit.  ``compact=False`` runs every point through the
    queries and the kernel instead of the active ones only: same bits, more time."""
    hand_pose = check_fields(left, right, hand_pose)
    if not isinstance(body_ret, dict) or not {"sdf", "density", "cano_xyz"} <= set(body_ret):
        raise ValueError("body_ret must hold sdf, density and cano_xyz (evaluate the field with want=('sdf', 'density', ..))")
    from .template_field import _points
    cano = _points(body_ret["cano_xyz"])
    n, dev = cano.shape[0], cano.device
    pts = _flat(posed_xyz, "posed_xyz", 3, n, dev)
    sdf = _flat(body_ret["sdf"], "body_ret['sdf']", 1, n, dev)
    density = _flat(body_ret["density"], "body_ret['density']", 1, n, dev)
    color = _flat(body_ret["color"], "body_ret['color']", 3, n, dev) if body_ret.get("color") is not None else None
    centre = cano_smpl_center.detach().cpu().numpy() if isinstance(cano_smpl_center, torch.Tensor) else np.asarray(cano_smpl_center)
    centre_y = float(np.float32(centre.reshape(-1)[1]))
    density_b = float(density_b)
    if not (np.isfinite(centre_y) and np.isfinite(density_b) and density_b > 0):
        raise ValueError(f"cano_smpl_center's y must be finite and density_b finite and positive, got {centre_y}, {density_b}")
    prepared = hands if isinstance(hands, PreparedHands) else PreparedHands(hands, dev)
    if prepared.left.v.device != dev:
        raise ValueError(f"the hands are on {prepared.left.v.device}, the points on {dev}")
    from .mesh_query import closest_point
    out_sdf, out_density = sdf.clone(), density.clone()
    out_color = color.clone() if color is not None else None
    if n:
        if compact:
            idx = torch.nonzero(active_mask(cano, prepared.left.box[:, 0], prepared.right.box[:, 0], centre_y)).reshape(-1)
            m = int(idx.numel())
            if m:
                sub_p, sub_c = pts[idx], cano[idx]
                sub = [out_sdf[idx], out_density[idx], out_color[idx] if out_color is not None else None]
                queries = tuple(closest_point(sub_p, h.v, h.f, walk=QUERY_WALK) for h in (prepared.left, prepared.right))
                fuse_kernel(sub_p, sub_c, sub[0].view(-1), sub[1].view(-1), sub[2], prepared, queries, left, right, centre_y, density_b, hand_pose)
                out_sdf.index_copy_(0, idx, sub[0])
                out_density.index_copy_(0, idx, sub[1])
                if out_color is not None:
                    out_color.index_copy_(0, idx, sub[2])
        else:
            queries = tuple(closest_point(pts, h.v, h.f, walk=QUERY_WALK) for h in (prepared.left, prepared.right))
            fuse_kernel(pts, cano, out_sdf.view(-1), out_density.view(-1), out_color, prepared, queries, left, right, centre_y, density_b, hand_pose)
    out = {"sdf": out_sdf, "density": out_density, "cano_xyz": cano}
    if out_color is not None:
        out["color"] = out_color
    return out
