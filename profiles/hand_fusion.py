"""Times of the hand fusion (``hand_fusion.fuse_hands``, ``include/ag_hand_fusion.h``) on the GPU: device events after a warm-up, every
figure taken twice.  Not a test; nobody fixed a bar in advance.

    python profiles/hand_fusion.py [--out profiles/hand_fusion.txt]

Shapes: one training step's samples (1024 rays x 64) and one 262 144-point chunk of a view, drawn about a body-shaped surface in T-pose
(torso, head, arms to x = +-0.70, legs; closed MANO-sized hands of 1552 faces at x = +-0.78), canonical = render space.  The share of
active samples (a non-zero gate) is reported, not assumed.

Compared: ``fuse_hands`` with the compaction on and off; its stages one by one (gate + compaction, the two closest-point queries, the
fused kernel, the scatter); the fused kernel against the same chain as torch ops on the device (float32, TF32 off, fed the same closest
points); ``template_render.render`` with and without ``hands`` at equal rays.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import hand_fusion as hf  # noqa: E402
from animatablegaussians_amd import template_render as tr  # noqa: E402
from animatablegaussians_amd.mesh_query import closest_point  # noqa: E402
from animatablegaussians_amd.template_field import TemplateField  # noqa: E402

HAND_X, HAND_RADII, CENTRE = 0.78, np.array([0.09, 0.03, 0.05]), np.float32([0.0, -0.05, 0.0])
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def sphere_mesh(n_lat, n_lon):
    """Closed latitude / longitude sphere with two pole fans, counter-clockwise from outside: 2 n_lon (n_lat - 1) faces."""
    t = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    p = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(t, p, indexing="ij")
    v = np.concatenate([[[0, 1, 0]], np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1).reshape(-1, 3), [[0, -1, 0]]])
    idx = lambda i, j: 1 + i * n_lon + j % n_lon  # noqa: E731
    f = []
    for j in range(n_lon):
        f.append((0, idx(0, j + 1), idx(0, j)))
        f.append((len(v) - 1, idx(n_lat - 2, j), idx(n_lat - 2, j + 1)))
        for i in range(n_lat - 2):
            f += [(idx(i, j), idx(i, j + 1), idx(i + 1, j)), (idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1))]
    return v, np.asarray(f, np.int64)


def hands_on_device(dev):
    u, f = sphere_mesh(25, 32)                                     # 1536 faces, 770 vertices: the MANO hand's size (1552, 778)
    out = {}
    for side, sx in (("left", 1.0), ("right", -1.0)):
        v = (u * HAND_RADII + np.array([-HAND_X, 0.45, 0.0])) * np.array([-sx, 1.0, 1.0])
        ff = f[:, ::-1] if side == "left" else f
        vt, ft = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(ff).astype(np.int32)).to(dev)
        from animatablegaussians_amd.subject_maps import vertex_normals
        out[side] = dict(v=vt, n=vertex_normals(vt, ft), f=ft, cano_v=vt)
    return out


def body_samples(n, seed):
    """Points within a few centimetres of a T-pose body's surface, by area: torso, head, two arms, two hands, two legs."""
    rs = np.random.default_rng(seed)

    def ellipsoid(c, r, m):
        d = rs.normal(size=(m, 3))
        return np.asarray(c) + d / np.linalg.norm(d, axis=1, keepdims=True) * np.asarray(r)

    def cylinder(a, b, r, m):
        a, b = np.asarray(a, float), np.asarray(b, float)
        axis = (b - a) / np.linalg.norm(b - a)
        e1 = np.cross(axis, [0.0, 0.0, 1.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(axis, e1)
        t, ang = rs.uniform(0, 1, (m, 1)), rs.uniform(0, 2 * np.pi, (m, 1))
        return a + t * (b - a) + r * (np.cos(ang) * e1 + np.sin(ang) * e2)
    parts = [(0.52, lambda m: ellipsoid((0, 0.25, 0), (0.18, 0.30, 0.11), m)), (0.13, lambda m: ellipsoid((0, 0.68, 0), (0.1, 0.1, 0.1), m)),
             (0.15, lambda m: cylinder((0.18, 0.45, 0), (0.70, 0.45, 0), 0.045, m)), (0.15, lambda m: cylinder((-0.18, 0.45, 0), (-0.70, 0.45, 0), 0.045, m)),
             (0.03, lambda m: ellipsoid((HAND_X, 0.45, 0), HAND_RADII, m)), (0.03, lambda m: ellipsoid((-HAND_X, 0.45, 0), HAND_RADII, m)),
             (0.35, lambda m: cylinder((0.1, -0.85, 0), (0.1, -0.05, 0), 0.07, m)), (0.35, lambda m: cylinder((-0.1, -0.85, 0), (-0.1, -0.05, 0), 0.07, m))]
    total = sum(w for w, _ in parts)                                # weights: areas in m^2, rounded
    counts = [int(round(n * w / total)) for w, _ in parts]
    counts[0] += n - sum(counts)
    pts = np.concatenate([fn(m) for (_, fn), m in zip(parts, counts)], 0) + rs.normal(0, 0.03, (n, 3))
    return pts[rs.permutation(n)].astype(np.float32)


def hand_net(seed):
    rs = np.random.RandomState(seed)
    chans = [88, 64, 64, 64, 64, 64, 3]
    return [((rs.uniform(-1, 1, (chans[i + 1], chans[i])) / np.sqrt(chans[i])).astype(np.float32), rs.uniform(-0.1, 0.1, chans[i + 1]).astype(np.float32))
            for i in range(6)]


def narrow_field():
    """A small body field (multires 2, 64 + 5 x 32 + 33, colour 32 + 3): the render comparison measures what ``hands`` ADDS."""
    rs = np.random.RandomState(1)
    e = 15
    chans, geo = [e, 64, 32, 32, 32, 32, 32, 33], []
    for l in range(7):
        k = chans[l] + (e if l == 4 else 0)
        geo.append((rs.normal(0, np.sqrt(2.0 / chans[l + 1]), (chans[l + 1], k)).astype(np.float32), np.zeros(chans[l + 1], np.float32)))
    geo[-1] = ((np.full((33, 32), np.sqrt(np.pi / 32)) + rs.normal(0, 1e-3, (33, 32))).astype(np.float32), np.full(33, -0.4, np.float32))
    color = [(rs.uniform(-0.17, 0.17, (32, 32)).astype(np.float32), np.zeros(32, np.float32)), (rs.uniform(-0.17, 0.17, (3, 32)).astype(np.float32), np.zeros(3, np.float32))]
    return TemplateField(geo, color, multires=2)


def timed(fn, reps):
    """Mean ms per call over ``reps`` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def twice(name, fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t = [timed(fn, reps) for _ in range(2)]
    say(f"  {name:<58s} {t[0]:9.3f} ms  {t[1]:9.3f} ms")
    return min(t)


def torch_chain(pts, cano, sdf, color, hands, queries, fields, centre_y, b):
    """The fused kernel's chain as torch ops on the device, float32, on the same closest points."""
    def norm(cv, x):
        mn, mx = cv.min(0, keepdim=True)[0], cv.max(0, keepdim=True)[0]
        return 2 * (x - 0.5 * (mx + mn)) / (mx - mn)
    vals = []
    for side, (d2, fid, bary), field in zip(hf.SIDES, queries, fields):
        h = hands[side]
        ids = h["f"].long()[fid.long()]
        x = (bary[..., None] * norm(h["cano_v"], h["cano_v"])[ids]).sum(1)
        q = (bary[..., None] * h["v"][ids]).sum(1)
        nr = (bary[..., None] * h["n"][ids]).sum(1)
        s = (-torch.sign((nr * (pts - q)).sum(-1)) * torch.sqrt(d2))[:, None]
        feat = [x]
        for k in range(4):
            feat += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
        z = torch.cat(feat + [s], -1)
        for i, (w, bias) in enumerate(field):
            z = torch.nn.functional.linear(z, w, bias)
            z = torch.relu(z) if i < len(field) - 1 else torch.sigmoid(z)
        vals.append((s, z))
    wl = torch.sigmoid(25 * (norm(hands["left"]["cano_v"], cano)[:, 0:1] + 0.8))
    wr = torch.sigmoid(-25 * (norm(hands["right"]["cano_v"], cano)[:, 0:1] - 0.8))
    low = cano[:, 1] < centre_y
    wl[low] = 0.
    wr[low] = 0.
    t = torch.maximum(wl + wr, torch.ones_like(wl))
    wl, wr = wl / t, wr / t
    w = wl + wr
    out_sdf = wl * vals[0][0] + wr * vals[1][0] + (1.0 - w) * sdf
    out_col = wl * vals[0][1] + wr * vals[1][1] + (1.0 - w) * color
    raw = -out_sdf
    return out_sdf, (1 / b) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / b)), out_col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/hand_fusion.py needs a GPU"
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    hands = hands_on_device(dev)
    nets = [hand_net(1), hand_net(2)]
    left, right = hf.HandField(nets[0]), hf.HandField(nets[1])
    dev_nets = [[(torch.from_numpy(np.ascontiguousarray(w[:, :28] if i == 0 else w)).to(dev), torch.from_numpy(f.folded_bias() if i == 0 else bb).to(dev))
                 for i, (w, bb) in enumerate(net)] for net, f in zip(nets, (left, right))]
    b = 0.0101
    prepared = hf.PreparedHands(hands, dev)
    for n, what in ((1024 * 64, "one training step: 1024 rays x 64 samples"), (262144, "one chunk of a view: 262 144 samples")):
        pts = torch.from_numpy(body_samples(n, 7)).to(dev)
        sdf = (0.05 * torch.sin(9 * pts[:, 0:1]) * torch.cos(7 * pts[:, 1:2])).contiguous()
        raw = -sdf
        density = (1 / b) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / b))
        color = torch.rand(n, 3, device=dev)
        body = dict(sdf=sdf, density=density, color=color, cano_xyz=pts)
        kw = dict(cano_smpl_center=CENTRE, density_b=b)
        mask = hf.active_mask(pts, prepared.left.box[:, 0], prepared.right.box[:, 0], float(CENTRE[1]))
        idx = torch.nonzero(mask).reshape(-1)
        m = int(idx.numel())
        say(f"\n{what}; active (a non-zero gate): {m} of {n} = {m / n:.3f}")
        say(f"  {'':<58s} {'run 1':>12s} {'run 2':>12s}")
        on = twice("fuse_hands, compact=True", lambda: hf.fuse_hands(body, pts, prepared, left, right, **kw))
        off = twice("fuse_hands, compact=False", lambda: hf.fuse_hands(body, pts, prepared, left, right, compact=False, **kw), reps=5)
        a, c = hf.fuse_hands(body, pts, prepared, left, right, **kw), hf.fuse_hands(body, pts, prepared, left, right, compact=False, **kw)
        same = all(torch.equal(a[k].view(torch.int32), c[k].view(torch.int32)) for k in ("sdf", "density", "color"))
        say(f"  compact=True == compact=False bit for bit: {same}; compaction saves {off / on:.2f} x")
        # the stages of the compacted path
        state = {}

        def gate():
            mk = hf.active_mask(pts, prepared.left.box[:, 0], prepared.right.box[:, 0], float(CENTRE[1]))
            ix = torch.nonzero(mk).reshape(-1)
            state.update(ix=ix, p=pts[ix], s=sdf[ix].view(-1), d=density[ix].view(-1), c=color[ix])

        def query():
            state["q"] = tuple(closest_point(state["p"], h.v, h.f, walk=hf.QUERY_WALK) for h in (prepared.left, prepared.right))

        def kernel():
            hf.fuse_kernel(state["p"], state["p"], state["s"], state["d"], state["c"], prepared, state["q"], left, right, float(CENTRE[1]), b)

        def scatter():
            for full, part in ((sdf, state["s"][:, None]), (density, state["d"][:, None]), (color, state["c"])):
                full.clone().index_copy_(0, state["ix"], part)
        gate(), query()
        twice("  gate + nonzero + gathers (one host sync)", gate)
        twice(f"  two closest-point queries ({hf.QUERY_WALK}), {m} points x 1536 faces", query)
        for walk in ("default", "uniform", "tiled"):
            twice(f"    one query (left hand), walk = {walk!r}", lambda: closest_point(state["p"], prepared.left.v, prepared.left.f, walk=walk))
        k_ms = twice(f"  fused kernel, {m} points", kernel)
        twice("  clones + scatter", scatter)
        q = state["q"]
        t_ms = twice(f"  the kernel's chain as torch ops, {m} points", lambda: torch_chain(state["p"], state["p"], sdf[state["ix"]], state["c"], hands, q, dev_nets,
                                                                                       float(CENTRE[1]), b))
        ref = torch_chain(state["p"], state["p"], sdf[state["ix"]], color[state["ix"]], hands, q, dev_nets, float(CENTRE[1]), b)
        s2, d2, c2 = sdf[state["ix"]].view(-1).clone(), density[state["ix"]].view(-1).clone(), color[state["ix"]].clone()
        hf.fuse_kernel(state["p"], state["p"], s2, d2, c2, prepared, q, left, right, float(CENTRE[1]), b)
        say(f"  fused kernel vs torch chain: {t_ms / k_ms:.2f} x faster; max |difference| sdf {float((s2[:, None] - ref[0]).abs().max()):.2e}, "
            f"colour {float((c2 - ref[2]).abs().max()):.2e}")
        flops = 2.0 * m * 2 * (32 * 64 + 4 * 64 * 64 + 64 * 32)
        say(f"  fused kernel: {flops / k_ms / 1e9:.2f} TFLOP/s of padded MLP work ({flops / 1e9:.2f} GFLOP)")
        qa = tuple(closest_point(pts, h.v, h.f) for h in (prepared.left, prepared.right))
        for walk in ("default", "tiled"):
            twice(f"  one query (left hand), all {n} points, walk = {walk!r}", lambda: closest_point(pts, prepared.left.v, prepared.left.f, walk=walk), reps=5)
        sa, da, ca = sdf.view(-1).clone(), density.view(-1).clone(), color.clone()
        twice(f"  fused kernel, all {n} points", lambda: hf.fuse_kernel(pts, pts, sa, da, ca, prepared, qa, left, right, float(CENTRE[1]), b))
        # the same points in a coherent order (sorted along x, as samples along neighbouring rays are): tiles without weight skip the MLPs
        ps = pts[torch.argsort(pts[:, 0])].contiguous()
        qs = tuple(closest_point(ps, h.v, h.f) for h in (prepared.left, prepared.right))
        twice(f"  fused kernel, all {n} points, sorted along x", lambda: hf.fuse_kernel(ps, ps, sa, da, ca, prepared, qs, left, right, float(CENTRE[1]), b))

    # render with and without hands, 1024 rays x 64 samples through the body's box
    field = narrow_field()
    R = 1024
    rs = np.random.default_rng(3)
    o = np.concatenate([rs.uniform([-0.9, -0.9], [0.9, 0.8], (R, 2)), np.full((R, 1), -2.5)], 1).astype(np.float32)
    d = np.tile(np.float32([0, 0, 1]), (R, 1))
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    near, far = torch.full((R,), 2.2, device=dev), torch.full((R,), 2.8, device=dev)
    rh = dict(hands, left_field=left, right_field=right, cano_smpl_center=CENTRE)
    say(f"\nrender, {R} rays x 64 samples, uniform sampling, canonical space, a narrow body field")
    say(f"  {'':<58s} {'run 1':>12s} {'run 2':>12s}")
    plain = twice("render without hands", lambda: tr.render(field, o, d, near, far, sampling="uniform"))
    fused = twice("render with hands", lambda: tr.render(field, o, d, near, far, sampling="uniform", hands=rh))
    say(f"  hands add {fused - plain:.3f} ms per {R} rays")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
