"""Posed-Gaussian PLY export / import -- SURVEY.md §8(f)-4; mirrors ``gaussians/obj_io.py:9-100`` (called per test frame at
``main_avatar.py:768``) without the ``plyfile`` package: the standard 3DGS vertex layout, binary little-endian, 62 floats per
Gaussian -- ``x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3`` -- with the reference's conventions: colours are
swapped to R, G, B and stored as the degree-0 SH coefficient ``(c - 0.5) / C0``, opacity as its logit, scales as logarithms, normals
and higher SH bands zero.  ``plyfile`` is not in this image: byte-level parity with its writer is unpinned (the header below is
what ``PlyData([PlyElement.describe(float32 structured array, 'vertex')]).write`` emits); values round-trip (tests/test_formats_cpu.py)."""
from __future__ import annotations

import os

import numpy as np
import torch

C0 = 0.28209479177387814                     # utils/sh_utils.py:26
_NAMES = (['x', 'y', 'z', 'nx', 'ny', 'nz'] + [f'f_dc_{i}' for i in range(3)] + [f'f_rest_{i}' for i in range(45)] + ['opacity']
          + [f'scale_{i}' for i in range(3)] + [f'rot_{i}' for i in range(4)])


def save_gaussians_as_ply(path: str, gaussian_vals: dict) -> None:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    f32 = lambda t: t.detach().to('cpu', torch.float32).numpy()  # noqa: E731
    xyz = f32(gaussian_vals['positions'])
    n = xyz.shape[0]
    out = np.zeros((n, len(_NAMES)), '<f4')
    out[:, 0:3] = xyz
    out[:, 6:9] = (f32(gaussian_vals['colors'])[:, [2, 1, 0]] - 0.5) / C0                       # RGB2SH of the swapped colours
    op = f32(gaussian_vals['opacity']).reshape(n, 1)
    out[:, 54:55] = np.log(op / (1 - op))                                                          # inverse_sigmoid
    out[:, 55:58] = np.log(f32(gaussian_vals['scales']))
    out[:, 58:62] = f32(gaussian_vals['rotations'])
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join(f"property float {k}\n" for k in _NAMES) + "end_header\n"
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(out.tobytes())


def load_gaussians_from_ply(path: str, device="cuda") -> dict:
    with open(path, 'rb') as f:
        buf = f.read()
    end = buf.index(b'end_header\n') + len(b'end_header\n')
    lines = buf[:end].decode('ascii').split('\n')
    if lines[0] != 'ply' or not lines[1].startswith('format binary_little_endian'):
        raise ValueError(f"{path}: only binary little-endian PLY files are read")
    n, props, in_vertex = 0, [], False
    for ln in lines[2:]:
        tok = ln.split()
        if tok[:1] == ['element']:
            in_vertex = tok[1] == 'vertex'
            if in_vertex:
                n = int(tok[2])
        elif tok[:1] == ['property'] and in_vertex:
            if tok[1] not in ('float', 'float32'):
                raise ValueError(f"{path}: property {tok[2]} is {tok[1]}, expected float")
            props.append(tok[2])
    a = np.frombuffer(buf, '<f4', n * len(props), end).reshape(n, len(props))
    col = lambda k: a[:, props.index(k)]  # noqa: E731
    by_idx = lambda pre: sorted((p for p in props if p.startswith(pre)), key=lambda s: int(s.split('_')[-1]))  # noqa: E731
    xyz = np.stack([col('x'), col('y'), col('z')], 1)
    dc = np.stack([col('f_dc_0'), col('f_dc_1'), col('f_dc_2')], 1)
    extra = np.stack([col(k) for k in by_idx('f_rest_')], 1).reshape(n, 3, 15)
    scales = np.stack([col(k) for k in by_idx('scale_')], 1)
    rots = np.stack([col(k) for k in by_idx('rot')], 1)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float, device=device)  # noqa: E731
    return {
        'positions': t(xyz),
        'colors': t((dc * C0 + 0.5)[:, [2, 1, 0]]),
        'opacity': torch.sigmoid(t(col('opacity')[:, None])),
        'scales': torch.exp(t(scales)),
        'rotations': torch.nn.functional.normalize(t(rots)),
        'features_extr': t(extra),
    }


# ---- triangle-mesh PLY (a subject's template.ply) -------------------------------------------------------------------------------
# gen_pos_maps.py:81 reads the template with trimesh.load(process=False); trimesh is not in this image, so its reader is unpinned.
# What follows is the format's own definition (Turk, "The PLY Polygon File Format"): a header of element / property lines, then the
# elements in header order, ascii or binary in either byte order.
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_header(buf: bytes, path: str):
    if buf[:3] != b'ply':
        raise ValueError(f"{path}: not a PLY file")
    end = buf.find(b'end_header')
    nl = buf.find(b'\n', end)
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: truncated PLY header")
    fmt, elements = None, []                                   # elements: [name, count, [(property name, type) | (name, count type, item type)]]
    for ln in buf[:end].decode('ascii', 'replace').splitlines()[1:]:
        tok = ln.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == 'property' and elements:
            types = tok[2:4] if tok[1] == 'list' else tok[1:2]
            if any(t not in _PLY_TYPES for t in types):
                raise ValueError(f"{path}: unknown property type in '{ln}'")
            elements[-1][2].append((tok[4], tok[2], tok[3]) if tok[1] == 'list' else (tok[2], tok[1]))
    if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
        raise ValueError(f"{path}: unknown PLY format {fmt}")
    return fmt, elements, nl + 1


def load_mesh_ply(path: str):
    """-> (vertices float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3] or None) of a triangle-mesh PLY: ``ascii``,
    ``binary_little_endian`` or ``binary_big_endian``; vertex properties of any scalar type in any order (``x y z``, optional
    ``nx ny nz``; others are skipped); faces in a list property ``vertex_indices`` or ``vertex_index`` with any integer count and
    index types.  A face that is not a triangle and a file shorter than its header promises raise ``ValueError``.  Host numpy only."""
    with open(path, 'rb') as f:
        buf = f.read()
    fmt, elements, pos = _ply_header(buf, path)
    order = {'binary_little_endian': '<', 'binary_big_endian': '>'}.get(fmt)
    tokens = buf[pos:].split() if fmt == 'ascii' else None
    tpos = 0
    vertex = faces = None
    for name, count, props in elements:
        scalar = all(len(p) == 2 for p in props)
        is_faces = name == 'face'
        if scalar:
            if order is None:
                if tpos + count * len(props) > len(tokens):
                    raise ValueError(f"{path}: truncated PLY body (element {name})")
                try:
                    table = np.array(tokens[tpos:tpos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                except ValueError as e:
                    raise ValueError(f"{path}: malformed ascii PLY body (element {name})") from e
                tpos += count * len(props)
                cols = {p[0]: table[:, i] for i, p in enumerate(props)}
            else:
                dt = np.dtype([(p[0], order + _PLY_TYPES[p[1]]) for p in props])
                if pos + count * dt.itemsize > len(buf):
                    raise ValueError(f"{path}: truncated PLY body (element {name})")
                table = np.frombuffer(buf, dt, count, pos)
                pos += count * dt.itemsize
                cols = {p[0]: table[p[0]] for p in props}
            if name == 'vertex':
                vertex = cols
            continue
        # an element with list properties: rows of varying length, walked one by one (faces of a 21 k-face template: milliseconds)
        rows = []
        for _ in range(count):
            for p in props:
                if len(p) == 2:
                    if order is None:
                        if tpos + 1 > len(tokens):
                            raise ValueError(f"{path}: truncated PLY body (element {name})")
                        tpos += 1
                    else:
                        pos += np.dtype(_PLY_TYPES[p[1]]).itemsize
                    continue
                if order is None:
                    if tpos + 1 > len(tokens):
                        raise ValueError(f"{path}: truncated PLY body (element {name})")
                    k = int(tokens[tpos])
                    if tpos + 1 + k > len(tokens):
                        raise ValueError(f"{path}: truncated PLY body (element {name})")
                    items = [int(t) for t in tokens[tpos + 1:tpos + 1 + k]]
                    tpos += 1 + k
                else:
                    ct, it = np.dtype(order + _PLY_TYPES[p[1]]), np.dtype(order + _PLY_TYPES[p[2]])
                    if pos + ct.itemsize > len(buf):
                        raise ValueError(f"{path}: truncated PLY body (element {name})")
                    k = int(np.frombuffer(buf, ct, 1, pos)[0])
                    pos += ct.itemsize
                    if k < 0 or pos + k * it.itemsize > len(buf):
                        raise ValueError(f"{path}: truncated PLY body (element {name})")
                    items = np.frombuffer(buf, it, k, pos)
                    pos += k * it.itemsize
                if is_faces and p[0] in ('vertex_indices', 'vertex_index'):
                    if k != 3:
                        raise ValueError(f"{path}: face {len(rows)} has {k} vertices; only triangle meshes are read")
                    rows.append(items)
            if order is not None and pos > len(buf):
                raise ValueError(f"{path}: truncated PLY body (element {name})")
        if is_faces:
            faces = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if vertex is None or not all(k in vertex for k in 'xyz'):
        raise ValueError(f"{path}: no vertex element with x, y, z")
    v = np.stack([vertex[k] for k in 'xyz'], 1).astype(np.float32)
    n = np.stack([vertex[k] for k in ('nx', 'ny', 'nz')], 1).astype(np.float32) if all(k in vertex for k in ('nx', 'ny', 'nz')) else None
    if faces is None:
        faces = np.zeros((0, 3), np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(v)):
        raise ValueError(f"{path}: a face index lies outside [0, {len(v)})")
    return v, faces.astype(np.int32), n


def save_mesh_ply(path: str, vertices, faces, normals=None) -> None:
    """Write a triangle mesh as binary little-endian PLY: ``float x y z`` (+ ``nx ny nz``), ``list uchar int vertex_indices``."""
    v = np.asarray(vertices, dtype='<f4').reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    names = ['x', 'y', 'z']
    if normals is not None:
        nm = np.asarray(normals, dtype='<f4').reshape(-1, 3)
        if nm.shape != v.shape:
            raise ValueError("normals must have one row per vertex")
        v = np.concatenate([v, nm], 1)
        names += ['nx', 'ny', 'nz']
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + "".join(f"property float {k}\n" for k in names)
              + "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f))
    rec = np.zeros(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(np.ascontiguousarray(v).tobytes())
        fh.write(rec.tobytes())
