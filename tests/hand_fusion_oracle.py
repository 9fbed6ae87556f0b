"""Plain-torch restatement of the template stage's hand fusion (``include/ag_hand_fusion.h``, ``hand_fusion.fuse_hands``): the reference's
``TemplateNet.fuse_hands`` (``network/template.py:146-202``) with ``HandAvatar.forward`` (``network/hand_avatar.py:28-36``) for one batch
element, line by line, in float32 and float64 on the host.  The closest point of every sample on a hand comes from
``tests/mesh_query_oracle.closest_point`` in the same precision, or is given (what the kernel-alone tests feed to both).

The oracle follows the reference's arithmetic (``wl * left + wr * right + (1 - w) * body`` at every point); the header's two rules that
the reference does not have are applied on top: a hand without a closest face has weight 0 and contributes 0, and a point with both
weights 0 returns the body's values themselves.  Both change a result only in the sign of a zero.

``make_hand_net`` is a deterministic numpy recipe (seeded; no torch RNG, no stored weights): ``nn.Linear``'s uniform
initialisation, with the ``sdf_h`` column of layer 0 scaled up (the hand's signed distance is centimetres where the embedding is of
order 1) so that this column, like the 60 pose columns, moves the colour visibly: a wrong fold or a dropped column shows.

The shared scenes (``scene``) are two closed "hands" -- ellipsoids from a subdivided icosahedron, the left one with every face reversed
in the recipe and reversed again by the mirror, so both are wound counter-clockwise seen from outside -- at the ends of a box of body
points, one rigid motion away from their canonical copies.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import mesh_query_oracle as mqo

BETA_MIN = np.float32(1e-4)          # LaplaceDensity's beta_min: an fp32 constant in every precision
CENTRE = np.float32([0.0, 0.1, 0.0])
DENSITY_BETA = 0.01
SIDES = ("left", "right")
SIZES = (1, 31, 32, 33, 257, 1031)
EXCLUSION_CAP = 0.01


# ------------------------------------------------------------------ networks ------------------------------------------------------------------
def make_hand_net(seed, multires=4, widths=(64, 64, 64, 64, 64), n_joints=15, sdf_gain=30.0):
    """[(W [out, in], bias [out])] float32 of one hand's ``tex_mlp``: in = 3 + 6 multires + 1 + 4 n_joints (88), then ``widths``, then 3."""
    rs = np.random.RandomState(seed)
    e = 3 + 6 * multires
    chans = [e + 1 + 4 * n_joints] + list(widths) + [3]
    layers = []
    for l in range(len(chans) - 1):
        bound = 1.0 / np.sqrt(chans[l])
        gain = 1.0 if l == 0 else (6.0 if l == len(chans) - 2 else 2.0)         # keeps the signal alive through 5 ReLUs and spreads the colours
        w = rs.uniform(-bound, bound, (chans[l + 1], chans[l])) * gain
        b = rs.uniform(-bound, bound, chans[l + 1])
        if l == 0:
            w[:, e] *= sdf_gain
        layers.append((w.astype(np.float32), b.astype(np.float32)))
    return layers


def state_dict(left, right):
    """The reference's ``TemplateNet.state_dict()`` keys of the two hands."""
    sd = {}
    for side, layers in (("left", left), ("right", right)):
        for i, (w, b) in enumerate(layers):
            p = f"{side}_hand.tex_mlp.fc_list.{i}." + ("" if i == len(layers) - 1 else "0.")
            sd[p + "weight"], sd[p + "bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    return sd


def axis_angle_to_quaternion(axis_angle):
    """pytorch3d's ``axis_angle_to_quaternion`` restated (pytorch3d is not available): (w, x, y, z), the small-angle series below 1e-6."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    small = angles.abs() < 1e-6
    k = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / torch.where(small, torch.ones_like(angles), angles))
    return torch.cat([torch.cos(half), axis_angle * k], dim=-1)


def embed(x, multires):
    cols = [x]
    for k in range(multires):
        f = float(2 ** k)
        cols += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(cols, -1)


def box_normalise(hand, x=None):
    """The header's per-axis box normalisation: ``(2 (x - (mx + mn) / 2)) / (mx - mn)`` with ``mn`` / ``mx`` the per-axis extremes of the
    vertices ``hand`` [V, 3], applied to ``x`` [N, 3] or, without ``x``, to the vertices themselves (what the reference takes from
    ``geo_util.normalize_vert_bbox(..., per_axis=True)``)."""
    mn, mx = hand.amin(0, keepdim=True), hand.amax(0, keepdim=True)
    return (2 * ((hand if x is None else x) - 0.5 * (mx + mn))) / (mx - mn)


def hand_color(layers, x, sdf, hand_pose, multires, dtype):
    """``HandAvatar.forward``: sigmoid(MLP([emb(x), sdf, quat(hand_pose) repeated]))."""
    quat = axis_angle_to_quaternion(hand_pose.reshape(-1, 3)).reshape(1, -1)
    h = torch.cat([embed(x, multires), sdf, quat.expand(x.shape[0], -1)], -1)
    for l, (w, b) in enumerate(layers):
        h = F.linear(h, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype))
        if l < len(layers) - 1:
            h = torch.relu(h)
    return torch.sigmoid(h)


# ------------------------------------------------------------------ the chain ------------------------------------------------------------------
def closest(sc, dtype=torch.float64):
    """{side: dict(dist2, face, bary)} of the scene's points on its two hands, in ``dtype``'s precision."""
    nd = np.float64 if dtype == torch.float64 else np.float32
    return {s: mqo.closest_point(sc["p"], sc["hands"][s]["v"], sc["hands"][s]["f"], nd) for s in SIDES}


def fuse(sc, dtype=torch.float64, closest_points=None):
    """The scene ``sc`` -> dict of numpy arrays in ``dtype``: ``sdf`` [N, 1], ``density`` [N, 1], ``color`` [N, 3] (None without a body
    colour), the weights ``wl`` / ``wr`` [N, 1] after normalisation, and the discrete decisions: ``sign_left`` / ``sign_right`` [N]
    (of ``n . (p - q)``), ``face_left`` / ``face_right`` [N], ``below`` [N] (the centre-y test)."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)  # noqa: E731
    cp = closest_points if closest_points is not None else closest(sc, dtype)
    p, cano = t(sc["p"]), t(sc["cano_xyz"])
    n_pts = p.shape[0]
    pose = t(np.zeros(45, np.float32) if sc.get("hand_pose") is None else sc["hand_pose"])
    out, hand_sdf, hand_col, missing = {}, {}, {}, {}
    for side in SIDES:
        h = sc["hands"][side]
        hand_v, hand_n, cano_v = t(h["v"]), t(h["n"]), t(h["cano_v"])
        f = torch.from_numpy(np.asarray(h["f"], np.int64))
        face = torch.from_numpy(np.asarray(cp[side]["face"], np.int64))
        missing[side] = face < 0
        d2 = torch.from_numpy(np.where(np.isfinite(cp[side]["dist2"]), cp[side]["dist2"], 0)).to(dtype)
        dists = torch.sqrt(d2)
        bc = torch.from_numpy(np.asarray(cp[side]["bary"])).to(dtype)
        ids = f[face.clamp_min(0)].clamp(0, hand_v.shape[0] - 1)                          # [N, 3]; a missing hand's rows are discarded below
        cano_hand_v = box_normalise(cano_v)
        pts_cano = (bc[..., None] * cano_hand_v[ids]).sum(1)
        pts_v = (bc[..., None] * hand_v[ids]).sum(1)
        pts_n = (bc[..., None] * hand_n[ids]).sum(1)
        dot = torch.einsum("ni,ni->n", pts_n, p - pts_v)
        sdf_h = (-torch.sign(dot) * dists).unsqueeze(-1)
        hand_sdf[side] = torch.where(missing[side][:, None], torch.zeros_like(sdf_h), sdf_h)
        col = hand_color(sc["nets"][side], pts_cano, sdf_h, pose, sc["multires"], dtype)
        hand_col[side] = torch.where(missing[side][:, None], torch.zeros_like(col), col)
        out["sign_" + side], out["face_" + side] = torch.sign(dot).numpy(), face.numpy()
    wl = torch.sigmoid(25 * (box_normalise(t(sc["hands"]["left"]["cano_v"]), cano)[..., 0:1] + 0.8))
    wr = torch.sigmoid(-25 * (box_normalise(t(sc["hands"]["right"]["cano_v"]), cano)[..., 0:1] - 0.8))
    below = cano[..., 1] < t(sc["centre"])[1]
    wl[below] = 0.
    wr[below] = 0.
    wl[missing["left"]] = 0.
    wr[missing["right"]] = 0.
    s = torch.maximum(wl + wr, torch.ones_like(wl))
    wl, wr = wl / s, wr / s
    w = wl + wr
    body_sdf = t(sc["sdf_b"]).reshape(-1, 1)
    sdf = wl * hand_sdf["left"] + wr * hand_sdf["right"] + (1.0 - w) * body_sdf
    beta = torch.tensor(float(sc["density_beta"]), dtype=torch.float32).to(dtype).abs() + torch.tensor(BETA_MIN).to(dtype)
    raw = -sdf
    density = (1 / beta) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / beta))
    inactive = ((wl == 0) & (wr == 0))
    sdf = torch.where(inactive, body_sdf, sdf)
    if sc.get("density_b_in") is not None:
        density = torch.where(inactive, t(sc["density_b_in"]).reshape(-1, 1), density)
    color = None
    if sc.get("color_b") is not None:
        body_col = t(sc["color_b"])
        color = wl * hand_col["left"] + wr * hand_col["right"] + (1.0 - w) * body_col
        color = torch.where(inactive, body_col, color).numpy()
    out.update(sdf=sdf.numpy(), density=density.numpy(), color=color, wl=wl.numpy(), wr=wr.numpy(), below=below.numpy(),
               inactive=inactive.reshape(-1).numpy())
    return out


def body_density(sdf_b, density_beta=DENSITY_BETA):
    """float32 LaplaceDensity of the body's sdf (what the field hands to the fusion beside it): [N, 1] float32."""
    raw = -torch.from_numpy(np.asarray(sdf_b, np.float32)).reshape(-1, 1)
    beta = torch.tensor(float(density_beta), dtype=torch.float32).abs() + torch.tensor(BETA_MIN)
    return ((1 / beta) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / beta))).numpy()


def density_b(density_beta=DENSITY_BETA):
    return float(np.abs(np.float32(density_beta)) + BETA_MIN)


def disagree(o32, o64, end_to_end):
    """bool [N]: the points where the two oracles take different discrete decisions: the sign of ``n . (p - q)`` of a hand that has weight,
    the centre-y test and, when each oracle searched its own closest point, the closest face."""
    bad = o32["below"] != o64["below"]
    for side, w in (("left", "wl"), ("right", "wr")):
        has = np.maximum(o64[w].reshape(-1), o32[w].reshape(-1)) >= 2.0 ** -149       # below fp32's smallest number the hand's term is nothing
        bad |= has & (o32["sign_" + side] != o64["sign_" + side])
        if end_to_end:
            bad |= has & (o32["face_" + side] != o64["face_" + side])
    return bad


def bars(o32, o64, keep):
    """The project's bar per output over the kept points: ``4 max|o32 - o64| + 2^-22 max|o64|``."""
    out = {}
    for k in ("sdf", "density", "color"):
        if o64.get(k) is None or not keep.any():
            continue
        a, b = o64[k][keep].astype(np.float64), o32[k][keep].astype(np.float64)
        out[k] = 4.0 * float(np.abs(a - b).max()) + 2.0 ** -22 * float(np.abs(a).max())
    return out


# ------------------------------------------------------------------ shared scenes ------------------------------------------------------------------
def icosphere(subdiv):
    """Unit sphere from an icosahedron: (v [V, 3] float64, f [F, 3] int64), 20 * 4^subdiv faces, counter-clockwise seen from outside."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int64)


RADII = np.array([0.09, 0.03, 0.05])
ROT = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.96, -0.28], [0.0, 0.28, 0.96]])
SHIFT = np.array([0.05, -0.1, 0.3])


def to_live(x):
    """The scene's rigid motion canonical -> live, float64 in, float32 out."""
    return (np.asarray(x, np.float64) @ ROT.T + SHIFT).astype(np.float32)


def synthetic_hands(subdiv=1, x_left=0.75, mano_faces=None, live=True):
    """{side: dict(v, n, f, cano_v)}: ellipsoids of ``RADII`` at (+-x_left, 0.3, 0) in canonical space, the left one at +x (a body in
    T-pose facing +z).  The right hand is the recipe's mesh; the left hand is its MIRROR IMAGE with every face reversed, the way the
    reference builds the left MANO hand from the right hand's topology.  ``mano_faces`` [1552, 3] replaces the icosphere by 778 seeded
    vertices on the ellipsoid under that topology: a triangle soup with the real vertex and face counts, not a hand.  ``live=False``:
    ``v`` / ``n`` are the canonical ones (``space='cano'``).  Normals: ``mesh_query_oracle.pseudonormals`` in float64, rounded once."""
    hands = {}
    for side in SIDES:
        if mano_faces is None:
            u, f = icosphere(subdiv)
        else:
            f = np.asarray(mano_faces, np.int64)
            d = np.random.RandomState(778).normal(size=(int(f.max()) + 1, 3))
            u = d / np.linalg.norm(d, axis=1, keepdims=True)
        cano = u * RADII + np.array([-x_left, 0.3, 0.0])
        if side == "left":
            cano = cano * np.array([-1.0, 1.0, 1.0])
            f = f[:, [2, 1, 0]]
        cano_v = cano.astype(np.float32)
        v = to_live(cano_v) if live else cano_v
        n = mqo.pseudonormals(v, f)[2].astype(np.float32)
        hands[side] = dict(v=v, n=n, f=np.ascontiguousarray(f.astype(np.int32)), cano_v=cano_v)
    return hands


def _near_hand(rs, hand, n, spread):
    """Canonical points about a hand: surface samples pushed along a random direction by N(0, spread)."""
    s = mqo.surface_samples(hand["cano_v"], hand["f"], rs, n)
    return s + rs.normal(0.0, spread, (n, 3))


def _over_faces(rs, hand, n, reach=0.01):
    """Canonical points whose closest point lies well inside a face: barycentrics of at least 0.15 each, pushed along the FACE normal by
    up to ``reach`` either way (the hands are convex, so the foot of the perpendicular is the closest point)."""
    v, f = hand["cano_v"].astype(np.float64), hand["f"].astype(np.int64)
    tri = v[f[rs.integers(0, len(f), n)]]
    b = 0.15 + 0.55 * rs.dirichlet(np.ones(3), n)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    return (b[:, :, None] * tri).sum(1) + rs.uniform(-reach, reach, (n, 1)) * fn


def mano_faces_closed():
    """The reference's closed MANO topology [1552, 3] (``tests/golden/mano_topology.npz``)."""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mano_topology.npz"))["faces_closed"]


def scene(kind="mixed", n=1031, seed=3, subdiv=1, color=True, pose=False, mano_faces=None, live=True, empty_right=False):
    """A scene for ``fuse``: points, body values, hands, nets.  ``kind``:
    ``mixed``     specials first (a live vertex of each hand: dist = 0; y exactly at the centre and one ulp below it, near each hand),
                  then body-box points (most of them inactive) and points about either hand, shuffled after the specials;
    ``inactive``  body points between the hands and points about the hands BELOW the centre y;
    ``active``    points about either hand, above the centre;
    ``left``      points about the left hand only (the right gate is exactly 0 there);
    ``clasped``   the hands 5 cm either side of x = 0 and points between them: wl + wr > 1;
    ``faces``     body points between the hands and points over the interior of a face of either hand: the closest face is the same
                  in float32 and float64 (a point whose closest point is an edge or a vertex has several faces at one distance, and the
                  two precisions then name different ones: the end-to-end comparison would have to leave it out)."""
    rs = np.random.default_rng(seed)
    hands = synthetic_hands(subdiv, 0.05 if kind == "clasped" else 0.75, mano_faces, live)
    if empty_right:                                   # one face with an index outside [0, V): it is skipped, every face_id is -1
        hands["right"]["f"] = np.array([[0, 1, len(hands["right"]["v"]) + 5]], np.int32)
    L, R = hands["left"], hands["right"]
    full = synthetic_hands(subdiv, 0.05 if kind == "clasped" else 0.75, mano_faces, live)       # faces for sampling even when a hand is emptied
    if kind == "mixed":
        special_c = [L["cano_v"][5], R["cano_v"][7]]
        special_p = [L["v"][5], R["v"][7]]
        for hnd in (L, R):
            c = hnd["cano_v"][3].astype(np.float64) + np.array([0.0, 0.0, 0.07])
            for y in (CENTRE[1], np.nextafter(CENTRE[1], np.float32(-1.0))):
                special_c.append(np.array([c[0], y, c[2]]))
                special_p.append(None)
        n_body = max(0, (n - 6) * 4 // 10)
        n_hand = max(0, n - 6 - n_body)
        body = rs.uniform([-0.95, -0.2, -0.15], [0.95, 0.6, 0.15], (n_body, 3))
        near = np.concatenate([_near_hand(rs, full["left"], n_hand - n_hand // 2, 0.02), _near_hand(rs, full["right"], n_hand // 2, 0.02)], 0)
        rest = np.concatenate([body, near], 0)
        rest = rest[rs.permutation(len(rest))]
        cano = np.concatenate([np.asarray(special_c, np.float64), rest], 0)[:n].astype(np.float32)
        p = to_live(cano) if live else cano.copy()
        for i, sp in enumerate(special_p[:n]):
            if sp is not None:
                p[i] = sp
    else:
        if kind == "inactive":
            a = rs.uniform([-0.3, -0.2, -0.15], [0.3, 0.6, 0.15], (n - n // 2, 3))
            b = np.concatenate([_near_hand(rs, full["left"], n // 2 - n // 4, 0.02), _near_hand(rs, full["right"], n // 4, 0.02)], 0)
            b[:, 1] = CENTRE[1] - 0.01 - np.abs(b[:, 1] - 0.3)
            cano = np.concatenate([a, b], 0)
        elif kind == "active":
            cano = np.concatenate([_near_hand(rs, full["left"], n - n // 2, 0.02), _near_hand(rs, full["right"], n // 2, 0.02)], 0)
        elif kind == "left":
            cano = _near_hand(rs, full["left"], n, 0.02)
        elif kind == "faces":
            m = n * 4 // 10
            cano = np.concatenate([rs.uniform([-0.3, -0.2, -0.15], [0.3, 0.6, 0.15], (m, 3)), _over_faces(rs, full["left"], n - m - (n - m) // 2),
                                   _over_faces(rs, full["right"], (n - m) // 2)], 0)
        elif kind == "clasped":
            cano = rs.uniform([-0.12, 0.24, -0.07], [0.12, 0.36, 0.07], (n, 3))
        else:
            raise ValueError(kind)
        if kind in ("active", "left"):
            cano[:, 1] = np.maximum(cano[:, 1], CENTRE[1] + 0.01)
        cano = cano[rs.permutation(len(cano))].astype(np.float32)
        p = to_live(cano) if live else cano.copy()
    sdf_b = (0.03 * np.sin(7.0 * cano[:, 0] + 1.0) * np.cos(5.0 * cano[:, 1]) + 0.01 * np.sin(31.0 * cano[:, 2])).astype(np.float32).reshape(-1, 1)
    sc = dict(p=np.ascontiguousarray(p), cano_xyz=np.ascontiguousarray(cano), sdf_b=sdf_b, density_b_in=body_density(sdf_b),
              color_b=rs.uniform(0, 1, (len(cano), 3)).astype(np.float32) if color else None, centre=CENTRE, density_beta=DENSITY_BETA,
              hands=hands, nets={"left": make_hand_net(101), "right": make_hand_net(202)}, multires=4,
              hand_pose=rs.uniform(-0.6, 0.6, 45).astype(np.float32) if pose else None)
    return sc


@functools.lru_cache(maxsize=None)
def case(kind="mixed", n=1031, color=True, pose=False, own_closest=False, empty_right=False, mano=False, subdiv=1):
    """A scene with both oracle runs, computed once per process and shared (read-only) by the tests: ``(scene, closest points fed to
    the kernel (the float32 search), o32, o64, keep)``.  ``own_closest``: each oracle searches the closest point in its own precision (the
    end-to-end comparison); else both are fed the float32 search's result, like the kernel.  ``mano``: the 1552-face MANO topology on
    synthetic vertices instead of the icospheres; ``subdiv``: the icospheres' subdivision (1: 80 faces, 2: 320)."""
    sc = scene(kind, n, color=color, pose=pose, empty_right=empty_right, mano_faces=mano_faces_closed() if mano else None, subdiv=subdiv)
    cp32 = closest(sc, torch.float32)
    o32 = fuse(sc, torch.float32, cp32)
    o64 = fuse(sc, torch.float64, None if own_closest else cp32)
    keep = ~disagree(o32, o64, own_closest)
    return sc, cp32, o32, o64, keep
