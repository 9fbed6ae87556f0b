"""numpy oracle of iso-surface extraction (``include/ag_isosurface.h``): the case table built by its OWN restatement of the rule (it does
not import ``csrc/gen_isosurface_table.py``), ``extract`` in float32 (the header's operations in the header's order) and float64, a
torch-CPU restatement of the reference's normals (``recon_util.py:9-48``) and mesh helpers (directed-edge census, Euler characteristic per
connected component, signed volume).

Run as a program it writes the case file of ``profiles/ub/isosurface_host_walk.hip``:  python tests/isosurface_oracle.py cases.bin
"""
import itertools
import struct
import sys

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- the table
# Worked in coordinates: a corner is (x, y, z) in {0, 1}^3 with id x + 2 y + 4 z; a cube edge is the pair of its end corners with
# id 4 axis + (u + 2 v), (u, v) the low corner's two other coordinates in ascending axis order.


def _cid(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def _edge_id(p, q):
    axis = [d for d in range(3) if p[d] != q[d]]
    assert len(axis) == 1
    axis = axis[0]
    lo = min(p, q)
    u, v = [lo[d] for d in range(3) if d != axis]
    return 4 * axis + u + 2 * v


def _edge_corners(e):
    axis, uv = e // 4, e % 4
    lo = [0, 0, 0]
    rest = [d for d in range(3) if d != axis]
    lo[rest[0]], lo[rest[1]] = uv % 2, uv // 2
    hi = list(lo)
    hi[axis] = 1
    return tuple(lo), tuple(hi)


def _face_walks():
    """The four corners of each of the six faces, counter-clockwise seen from outside: the walk (0,0) (1,0) (1,1) (0,1) in tangents
    (s, t) whose cross product is the outward normal."""
    unit = np.eye(3, dtype=int)
    walks = []
    for axis, side in itertools.product(range(3), (0, 1)):
        normal = unit[axis] * (1 if side else -1)
        others = [d for d in range(3) if d != axis]
        s, t = unit[others[0]], unit[others[1]]
        if np.dot(np.cross(s, t), normal) < 0:
            s, t = t, s
        base = unit[axis] * side
        walks.append([tuple(int(c) for c in base + a * s + b * t) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))])
    return walks


FACE_WALKS = _face_walks()


def face_segments(walk, case):
    """The rule for one face: directed segments (exit edge id, entry edge id) from its four corner bits alone."""
    bits = [(case >> _cid(p)) & 1 for p in walk]
    segs = []
    for i in range(4):
        if bits[i] and not bits[(i + 1) % 4]:                       # an exit: walk on to the next entry
            j = i
            while not (not bits[j % 4] and bits[(j + 1) % 4]):
                j += 1
            segs.append((_edge_id(walk[i], walk[(i + 1) % 4]), _edge_id(walk[j % 4], walk[(j + 1) % 4])))
    return segs


def _share_face(e0, e1):
    c = _edge_corners(e0) + _edge_corners(e1)
    return any(len({p[d] for p in c}) == 1 for d in range(3))


def case_triangles(case):
    follow = {}
    for walk in FACE_WALKS:
        for a, b in face_segments(walk, case):
            assert a not in follow
            follow[a] = b
    left = sorted(follow)
    tris = []
    while left:
        loop = [left[0]]                                                # loops by ascending lowest edge id, starting there
        while follow[loop[-1]] != loop[0]:
            loop.append(follow[loop[-1]])
        left = [e for e in left if e not in loop]
        n = len(loop)
        for apex in range(n):
            ring = [loop[(apex + i) % n] for i in range(n)]
            if not any(_share_face(ring[0], ring[i]) for i in range(2, n - 1)):
                break
        else:
            raise AssertionError(f"case {case}: no fan without a diagonal in a face plane for {loop}")
        tris += [(ring[0], ring[i + 1], ring[i]) for i in range(1, n - 1)]         # reversed: counter-clockwise seen from outside
    return tris


def build_table():
    """[256, 16] int8 (edge ids, three per triangle, -1 padded) and [256] triangle counts."""
    table = -np.ones((256, 16), np.int8)
    count = np.zeros(256, np.int64)
    for case in range(256):
        tris = case_triangles(case)
        count[case] = len(tris)
        table[case, :3 * len(tris)] = np.asarray(tris, np.int8).reshape(-1)
    return table, count


TRI_TABLE, TRI_COUNT = build_table()

# ---------------------------------------------------------------------------------------------------------------- extraction


def extract(volume, iso=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), mask=None, dtype=np.float32):
    """(vertices [V, 3] dtype, faces [F, 3] int32) in the contract's order.  The classification always compares the float32 values with
    the float32 ``iso`` (the same in both precisions); positions are computed in ``dtype`` from the float32 inputs, each operation
    rounded on its own in the header's order."""
    vol32 = np.ascontiguousarray(volume, np.float32)
    X, Y, Z = vol32.shape
    N = X * Y * Z
    iso32 = np.float32(iso)
    inside = vol32 >= iso32
    ok = np.isfinite(vol32)
    if mask is not None:
        ok &= np.asarray(mask).reshape(X, Y, Z) != 0
    cut = lambda a, dx, dy, dz: a[(slice(0, X - 1) if not dx else slice(1, X)), (slice(0, Y - 1) if not dy else slice(1, Y)),   # noqa: E731
                                  (slice(0, Z - 1) if not dz else slice(1, Z))]
    processed = np.ones((X - 1, Y - 1, Z - 1), bool)
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        processed &= cut(ok, dx, dy, dz)
        case |= cut(inside, dx, dy, dz).astype(np.int64) << c
    # P[i + 1, j + 1, k + 1] = cell (i, j, k) is processed; zero around, so a cell outside the grid reads as not processed
    P = np.zeros((X + 1, Y + 1, Z + 1), bool)
    P[1:X, 1:Y, 1:Z] = processed
    flag = np.zeros((X, Y, Z, 3), bool)
    ext = (X, Y, Z)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, ext[axis] - 1), slice(1, ext[axis])
        straddle = inside[tuple(lo)] != inside[tuple(hi)]
        p, q = [d for d in range(3) if d != axis]
        near = np.zeros_like(straddle)
        for s, t in itertools.product((0, 1), (0, 1)):
            idx = [None] * 3
            idx[axis] = slice(1, ext[axis])                          # cell index = node index along the edge's axis
            idx[p] = slice(1 - s, 1 - s + ext[p])
            idx[q] = slice(1 - t, 1 - t + ext[q])
            near |= P[tuple(idx)]
        flag[tuple(lo) + (axis,)] = straddle & near
    keys = np.flatnonzero(flag.reshape(-1))
    vindex = np.cumsum(flag.reshape(-1)) - 1
    n, axis = keys // 3, keys % 3
    step = np.array([Y * Z, Z, 1], np.int64)
    flat = vol32.reshape(-1).astype(dtype)
    a, b = flat[n], flat[n + step[axis]]
    with np.errstate(all="ignore"):
        t = (dtype(iso32) - a) / (b - a)
        sp = np.asarray(spacing, np.float32).astype(dtype)
        org = np.asarray(origin, np.float32).astype(dtype)
        index = np.stack([n // (Y * Z), (n // Z) % Y, n % Z], 1).astype(dtype)
        vertices = org[None] + index * sp[None]
        on_axis = org[axis] + (index[np.arange(len(n)), axis] + t) * sp[axis]
    vertices[np.arange(len(n)), axis] = on_axis
    vertices = vertices.astype(dtype)
    # faces: processed cells in ascending low-node index, table order within the cell
    count = np.where(processed, TRI_COUNT[case], 0)
    ci, cj, ck = np.nonzero(count)
    cells = (ci * Y + cj) * Z + ck                                   # ascending: np.nonzero is row-major
    rows = TRI_TABLE[case[ci, cj, ck]].astype(np.int64)[:, :15]       # [cells, 15]
    valid = rows >= 0
    e = np.where(valid, rows, 0)
    e_axis, e_u, e_v = e // 4, e % 2, (e // 2) % 2
    p_step = np.where(e_axis == 0, step[1], step[0])
    q_step = np.where(e_axis == 2, step[1], step[2])
    m = cells[:, None] + e_u * p_step + e_v * q_step
    vid = vindex[3 * m + e_axis]
    assert flag.reshape(-1)[(3 * m + e_axis)[valid]].all(), "a triangle uses an edge that carries no vertex"
    faces = vid[valid].reshape(-1, 3).astype(np.int32)
    assert 3 * N < 2 ** 31
    return vertices, faces


# ---------------------------------------------------------------------------------------------------------------- normals


def reference_normals(volume, voxel_size, grid_pts, dtype=None):
    """torch-CPU restatement of ``extract_normal_from_volume`` (``recon_util.py:9-48``): Sobel ``F.conv3d`` with padding 1, then
    ``F.grid_sample(..., padding_mode='border', align_corners=True)`` at ``2 * grid_pts - 1``, divided by the norm.  NOT negated."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    vol = torch.as_tensor(np.asarray(volume, np.float32)).to(dtype)
    vs = [float(np.float32(v)) for v in voxel_size]
    sobel_x = torch.zeros((3, 3, 3), dtype=dtype)
    sobel_x[0] = torch.tensor([[-1, -2, -1], [-2, -4, -2], [-1, -2, -1]], dtype=dtype)
    sobel_x[2] = -sobel_x[0]
    sobel_z = sobel_x.permute((1, 2, 0))
    sobel_y = sobel_x.permute((2, 0, 1))
    filt = torch.stack([sobel_x / (16 * 2 * vs[0]), sobel_y / (16 * 2 * vs[1]), sobel_z / (16 * 2 * vs[2])], 0).unsqueeze(1)
    nv = F.conv3d(vol.view(1, 1, *vol.shape), filt, padding=1)        # [1, 3, X, Y, Z]
    pts = torch.as_tensor(np.asarray(grid_pts)).to(dtype) * 2 - 1
    pts = pts[:, [2, 1, 0]].unsqueeze(0).unsqueeze(2).unsqueeze(3)
    nrm = F.grid_sample(nv, pts, padding_mode="border", align_corners=True).reshape(3, -1).permute(1, 0)
    return (nrm / torch.norm(nrm, dim=1, keepdim=True)).numpy()


# ---------------------------------------------------------------------------------------------------------------- mesh helpers


def directed_edge_census(faces):
    """(keys, counts) of the directed edges (a -> b as a * big + b) of the faces, and whether the mesh is closed and oriented: every
    directed edge occurs once and its reverse once."""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    big = int(f.max()) + 1 if f.size else 1
    keys, counts = np.unique(a * big + b, return_counts=True)
    rev = np.unique(b * big + a)
    closed = bool((counts == 1).all() and len(rev) == len(keys) and np.array_equal(rev, keys))
    return keys, counts, closed


def components(faces, n_vertices):
    """Label of the connected component of every vertex (min-label propagation over the faces' edges; -1 for unused vertices)."""
    f = np.asarray(faces, np.int64)
    label = np.arange(n_vertices)
    while True:
        low = label[f].min(1)
        new = label.copy()
        for c in range(3):
            np.minimum.at(new, f[:, c], low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    used = np.zeros(n_vertices, bool)
    used[f.reshape(-1)] = True
    return np.where(used, label, -1)


def euler_characteristics(faces, n_vertices):
    """Sorted list of V - E + F of every connected component."""
    f = np.asarray(faces, np.int64)
    label = components(f, n_vertices)
    out = []
    for lab in np.unique(label[label >= 0]):
        sub = f[label[f[:, 0]] == lab]
        e = np.sort(np.concatenate([sub[:, [0, 1]], sub[:, [1, 2]], sub[:, [2, 0]]]), 1)
        out.append(int(len(np.unique(sub)) - len(np.unique(e, axis=0)) + len(sub)))
    return sorted(out)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- fields


def noise_field(shape, seed, closed=False):
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal(shape).astype(np.float32)
    if closed:                                                       # a negative outer layer: the surface does not reach the border
        vol[0], vol[-1], vol[:, 0], vol[:, -1], vol[:, :, 0], vol[:, :, -1] = (-1.0,) * 6
    return vol


def sphere_field(shape, centre, radius):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1)
    return (radius - np.linalg.norm(g - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_field(shape, centre, major, minor):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1) - np.asarray(centre, np.float64)
    ring = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - major
    return (minor - np.sqrt(ring ** 2 + g[..., 2] ** 2)).astype(np.float32)


def every_case_volume(seed=0):
    """[2, 2, 768] float32 and its mask: cell 3 c carries case c (values +-(0.25 .. 1), sign by bit); the mask is false on every third
    slice k = 3 c + 2, so the cells between the carriers are skipped."""
    rng = np.random.default_rng(seed)
    vol = -(0.25 + 0.75 * rng.random((2, 2, 768))).astype(np.float32)
    mag = (0.25 + 0.75 * rng.random((256, 8))).astype(np.float32)
    for c in range(256):
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
            vol[dx, dy, 3 * c + dz] = mag[c, corner] * (1 if (c >> corner) & 1 else -1)
    mask = np.ones((2, 2, 768), bool)
    mask[:, :, 2::3] = False
    return vol, mask


def walk_cases():
    """The small shapes of the host walk: (volume, mask or None, iso, spacing, origin)."""
    sp, org = (0.03, 0.02, 0.01), (-0.4, 1.1, 0.05)
    cases = []
    vol, mask = every_case_volume()
    cases.append((vol, mask, 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    for shape in ((2, 2, 2), (2, 7, 2), (5, 4, 3), (17, 9, 33)):
        for iso in (0.0, 0.137):
            cases.append((noise_field(shape, 11), None, iso, sp, org))
    rng = np.random.default_rng(5)
    cases.append((rng.integers(-1, 2, (9, 8, 7)).astype(np.float32), None, 0.0, sp, org))
    vol = noise_field((12, 11, 10), 6)
    mask = rng.random(vol.shape) >= 0.1
    vol.reshape(-1)[[17, 400, 901]] = np.nan
    vol.reshape(-1)[555] = np.inf
    cases.append((vol, mask, 0.0, sp, org))
    cases.append((np.full((3, 4, 5), -1.0, np.float32), None, 0.0, sp, org))
    return cases


def main(path):
    cases = walk_cases()
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for vol, mask, iso, sp, org in cases:
            v, f = extract(vol, iso, sp, org, mask, np.float32)
            X, Y, Z = vol.shape
            fh.write(struct.pack("<6i", X, Y, Z, 0 if mask is None else 1, len(v), len(f)))
            fh.write(struct.pack("<7f", iso, *sp, *org))
            fh.write(vol.astype("<f4").tobytes())
            if mask is not None:
                fh.write(mask.astype(np.uint8).tobytes())
            fh.write(v.astype("<f4").tobytes())
            fh.write(f.astype("<i4").tobytes())
    print(f"{path}: {len(cases)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
