"""Cases and float64 references of the kernels of csrc/ag_avatar.hip -- the map gather with its activations, linear-blend skinning forward and
backward, the joint-matrix gradient and hand fusion -- at which tests/test_avatar_kernels_edges_gpu.py runs them.  Not a test module.

References: ``oracle/avatar_oracle.py``'s ``gather_activate``, ``transform_cano2live`` and ``hand_fuse``, evaluated in float64 and in float32 on the same
fp32-representable inputs, with autograd for the gradients.  Every case is built in float32 and cast, so both types read the same numbers.

The bar (a copy of ``_bar`` of tests/test_pose_grad_gpu.py): a result passes when it is within 4 x the float32 oracle's own deviation from float64 + 2e-6 of
the float64 value's scale, in the max norm and in the L2 norm.  It is applied per output tensor and per case, and where one tensor mixes magnitude classes
(the channel groups of the other map, the zero-quaternion rows beside ordinary ones) per class, so that the scale term means something.

Two branches of the skinning kernels that a case might be built for cannot be reached by finite inputs, and tests/test_avatar_kernels_oracle_cpu.py asserts
that instead of counting rows on them: the four radicands of ``matrix_to_quaternion`` always sum to 4, so the largest is at least 1 -- the selected ``q_abs``
never falls to the 0.1 floor, and the radicand of the selected candidate is never <= 0.  What a negative or shrunk blend does reach is the positive-part
branch of the OTHER candidates (``x4[c] > 0 ? sqrt : 0``); the branch case counts those rows."""
import functools
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import avatar_oracle as ao  # noqa: E402

F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the bar
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def bar_ratio(got, f64, f32, name, floor=0.0):
    """Worst ratio of ``got``'s error to the bar (max norm and L2 norm); asserts shape and finiteness only.  ``floor``: an absolute term added to the
    max-norm limit (and, times sqrt(numel), to the L2 limit) for values below fp32's normal range."""
    got, f64, f32 = (t.detach().cpu().double() for t in (got, f64, f32))
    assert got.shape == f64.shape, f"{name}: shape {tuple(got.shape)} != {tuple(f64.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert torch.isfinite(f64).all() and torch.isfinite(f32).all(), f"{name}: non-finite reference"
    if got.numel() == 0:
        return 0.0
    e_max, e_l2 = float((got - f64).abs().max()), float((got - f64).norm())
    d_max, d_l2 = float((f32 - f64).abs().max()), float((f32 - f64).norm())
    lim_max = 4 * d_max + 2e-6 * float(f64.abs().max()) + floor
    lim_l2 = 4 * d_l2 + 2e-6 * float(f64.norm()) + floor * got.numel() ** 0.5
    r_max = e_max / lim_max if lim_max > 0 else (0.0 if e_max == 0 else float("inf"))
    r_l2 = e_l2 / lim_l2 if lim_l2 > 0 else (0.0 if e_l2 == 0 else float("inf"))
    return max(r_max, r_l2)


def bar(got, f64, f32, name, floor=0.0):
    """Assert the bar; returns the worst ratio (<= 1)."""
    r = bar_ratio(got, f64, f32, name, floor)
    assert r <= 1.0, f"{name}: error is {r:.3f} x the bar (4 x the fp32 oracle's deviation from fp64 + 2e-6 of the fp64 scale)"
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# gather + activations
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _mask_of(S, pixels):
    m = torch.zeros(S * 2 * S, dtype=torch.bool)
    m[torch.as_tensor(sorted(pixels))] = True
    return m.reshape(S, 2 * S)


def _mask_n(S, N, seed):
    """Exactly N pixels of the [S, 2S] canvas: pixel 0, the last pixel (S-1, 2S-1), both sides of the front|back seam (u = S-1, u = S) on row S/2,
    the rest drawn at random."""
    last = 2 * S * S - 1
    row = (S // 2) * 2 * S
    forced = [last, 0, row + S - 1, row + S][:N] if N < 4 else [0, last, row + S - 1, row + S]
    g = torch.Generator().manual_seed(seed)
    rest = [int(p) for p in torch.randperm(2 * S * S, generator=g) if int(p) not in forced]
    return _mask_of(S, forced + rest[:N - len(forced)])


# name -> (S, mask builder, kind).  kind: "plain" | "zero_quat" | a saturated class of SATURATED
GATHER_CASES = {
    "s8_full": (8, lambda: torch.ones(8, 16, dtype=torch.bool), "plain"),        # N = 128: every offset of map_offset, both halves, the seam
    "s16_n1_first": (16, lambda: _mask_of(16, [0]), "plain"),                     # N = 1 cannot hold both corner pixels: one case each
    "s16_n1_last": (16, lambda: _mask_of(16, [2 * 16 * 16 - 1]), "plain"),
    "s16_n255": (16, lambda: _mask_n(16, 255, 1), "plain"),                       # one ragged workgroup
    "s16_n256": (16, lambda: _mask_n(16, 256, 2), "plain"),                       # one full workgroup
    "s16_n257": (16, lambda: _mask_n(16, 257, 3), "plain"),                       # a second workgroup of one thread
    "zero_quat": (16, lambda: _mask_n(16, 257, 4), "zero_quat"),                  # norm <= 1e-12: forward 0, backward g * 1e12
    "opacity_pos": (16, lambda: _mask_n(16, 255, 5), "opacity_pos"),
    "opacity_neg": (16, lambda: _mask_n(16, 255, 6), "opacity_neg"),
    "scale_big": (16, lambda: _mask_n(16, 255, 7), "scale_big"),
    "scale_small": (16, lambda: _mask_n(16, 255, 8), "scale_small"),
}
# saturated class -> (which logits, lo, hi) of map + raw; one magnitude class per case
SATURATED = {
    "opacity_pos": ("opacity", 20.0, 100.0),       # sigmoid rounds to 1, its derivative to 0
    "opacity_neg": ("opacity", -100.0, -20.0),     # sigmoid down to 3.7e-44: below fp32's normal range from -87.3 on
    "scale_big": ("scale", 60.0, 80.0),            # exp up to 5.5e34
    "scale_small": ("scale", -100.0, -60.0),       # exp down to 3.7e-44
}
SUBNORMAL_FLOOR = 1e-37                            # absolute floor of the comparisons below fp32's normal range (1.18e-38)
GATHER_OUTPUTS = ("positions", "opacity", "scales", "rotations", "colors")
# gradient maps and the channel groups (per side, C channels each) that are compared on their own
GRAD_GROUPS = (("position_map", 3, ((0, 3, "positions"),)),
               ("other_map", 8, ((0, 1, "opacity"), (1, 4, "scales"), (4, 8, "rotations"))),
               ("color_map", 3, ((0, 3, "colors"),)))


@functools.lru_cache(maxsize=None)
def gather_case(name):
    """Float32 CPU inputs of one gather case: mask [S, 2S] bool, the three maps, the canonical parameters, the five upstream gradients, and
    ``zero_rows`` [N] bool (the rows whose rotation sum is exactly 0)."""
    S, build, kind = GATHER_CASES[name]
    mask = build()
    N = int(mask.sum())
    g = torch.Generator().manual_seed(100 + sorted(GATHER_CASES).index(name))
    d = dict(S=S, N=N, kind=kind, mask=mask,
             position_map=torch.randn(1, 6, S, S, generator=g),
             other_map=torch.randn(1, 16, S, S, generator=g) * 0.5,
             color_map=torch.rand(1, 6, S, S, generator=g),
             xyz=torch.randn(N, 3, generator=g) * 0.5,
             opacity_raw=torch.randn(N, 1, generator=g),
             scaling_raw=torch.randn(N, 3, generator=g) * 0.3 - 5.0,
             rotation_raw=torch.nn.functional.normalize(torch.randn(N, 4, generator=g)))
    d["zero_rows"] = torch.zeros(N, dtype=torch.bool)
    if kind == "zero_quat":
        zero = torch.arange(N) % 2 == 0
        gathered = ao.canvas(d["other_map"], 8)[mask][:, 4:8]
        d["rotation_raw"] = torch.where(zero[:, None], -gathered, d["rotation_raw"])      # x + (-x) is exactly 0 in every type
        d["zero_rows"] = zero
    elif kind in SATURATED:
        which, lo, hi = SATURATED[kind]
        ch, raw, width = {"opacity": ((0, 1), "opacity_raw", 1), "scale": ((1, 4), "scaling_raw", 3)}[which]
        # half of the logit in the map and half in the canonical parameter; the sum is rounded once, in fp32 as in fp64 (|sum| <= 100: exact or
        # one rounding, the same in the kernel and in the fp32 oracle)
        for side in (0, 8):
            d["other_map"][0, side + ch[0]:side + ch[1]] = (lo + (hi - lo) * torch.rand(ch[1] - ch[0], S, S, generator=g)) * 0.5
        d[raw] = (lo + (hi - lo) * torch.rand(N, width, generator=g)) * 0.5
    d["ups"] = tuple(torch.randn(N, c, generator=g) for c in (3, 1, 3, 4, 3))
    return d


def gather_logits(d, dtype=F64):
    """(opacity logits [N,1], scale logits [N,3], rotation sums [N,4]) of a case, map + canonical parameter."""
    others = ao.canvas(d["other_map"].to(dtype), 8)[d["mask"]]
    return others[:, 0:1] + d["opacity_raw"].to(dtype), others[:, 1:4] + d["scaling_raw"].to(dtype), others[:, 4:8] + d["rotation_raw"].to(dtype)


def _gather_ref(name, dtype):
    d = gather_case(name)
    maps = [d[k].to(dtype).clone().requires_grad_(True) for k in ("position_map", "other_map", "color_map")]
    outs = ao.gather_activate(*maps, d["mask"], *(d[k].to(dtype) for k in ("xyz", "opacity_raw", "scaling_raw", "rotation_raw")))
    torch.autograd.backward(list(outs), [u.to(dtype) for u in d["ups"]])
    return tuple(o.detach() for o in outs), tuple(m.grad for m in maps)


@functools.lru_cache(maxsize=None)
def gather_reference(name):
    """((outputs, gradient maps) in float64, the same in float32)."""
    return _gather_ref(name, F64), _gather_ref(name, F32)


def canvas_rows(grad_map, C, mask):
    """A gradient map [1, 2C, S, S] -> its [N, C] rows on the mask (the order of the kernel's Gaussians) and the map with those zeroed."""
    cv = ao.canvas(grad_map, C)
    off = cv.clone()
    off[mask] = 0
    return cv[mask], off


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# linear-blend skinning
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def joints(J, seed, max_shift=0.05):
    """Random rigid joint transforms: rotations <= 30 deg, translations <= ``max_shift``; row 3 is noise (the kernels never read it)."""
    g = torch.Generator().manual_seed(seed)
    ax = torch.nn.functional.normalize(torch.randn(J, 3, generator=g))
    ang = torch.rand(J, generator=g) * (np.pi / 6)
    K = torch.zeros(J, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    A = torch.eye(4)[None].repeat(J, 1, 1)
    A[:, :3, :3] = torch.eye(3)[None] + torch.sin(ang)[:, None, None] * K + (1 - torch.cos(ang))[:, None, None] * (K @ K)
    A[:, :3, 3] = (torch.rand(J, 3, generator=g) - 0.5) * 2 * max_shift
    A[:, 3, :3] = torch.randn(J, 3, generator=g)
    return A


# (N, J) of the dense + sparse parity cases: every N at J = 55 (odd) and 64 (even, a power of two: LDS rows on one bank), and the J ladder at a ragged last
# wave (65 = 64 + 1) and a second workgroup of one lane (257); N = 63 / 255 / 1000 leave whole waves past N (first >= N)
LBS_NJ = [(N, J) for J in (55, 64) for N in (1, 63, 64, 65, 255, 256, 257, 1000)] + [(N, J) for J in (1, 2, 24, 140, 160) for N in (65, 257)]
LBS_SPARSE_ONLY = [("j256_k1", 257, 256, 1), ("j256_k16", 257, 256, 16)]           # sparse only (dense J = 256 does not fit LDS): indices 250..255 in use
JOINT_GRAD_NJ = [(65, 140), (257, 140)]                                           # the joint gradient at its LDS limit
# the joint gradient through the shared backward chain: every arg-max candidate and the positive-part branch, a single weight column, one Gaussian beside
# three idle waves, the product's J with one Gaussian in the second workgroup, J at the edge of one column per lane.  dL/dA is compared over all rows, so
# none of them may be fragile (tests/test_avatar_kernels_oracle_cpu.py)
JOINT_GRAD_EDGE = ["branches", "n65_j1", "n1_j55", "n257_j55", "n1000_j64"]


def lbs_name(N, J):
    return f"n{N}_j{J}"


def _lbs_random(N, J, K, seed, cols=None):
    """K-sparse rows with sums in [0.5, 1.5] (unnormalised), quaternions of length in [0.5, 2] (not unit), both upstream gradients."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, J, generator=g)
    if cols is not None:
        w[cols[0], cols[1]] += 2.0                                                   # these columns are among every row's top K
    top = torch.topk(w, K, dim=1)
    lbs = torch.zeros(N, J).scatter_(1, top.indices, torch.rand(N, K, generator=g) + 0.05)
    lbs = lbs / lbs.sum(1, keepdim=True) * (0.5 + torch.rand(N, 1, generator=g))
    pos = torch.randn(N, 3, generator=g) * 0.5
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g)) * (0.5 + 1.5 * torch.rand(N, 1, generator=g))
    ups = (torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g))
    return dict(N=N, J=J, K=K, lbs=lbs.contiguous(), pos=pos, rot=rot, A=joints(J, seed + 1), ups=ups, exact_rows=torch.zeros(N, dtype=torch.bool))


@functools.lru_cache(maxsize=None)
def lbs_case(name):
    """Float32 CPU inputs of one skinning case: lbs [N, J], pos, rot, A [J, 4, 4], ups = (dL/dlive positions, dL/dlive rotations), K = non-zeros per row,
    ``exact_rows`` [N] bool: rows whose outputs the test asserts exactly instead of against the bar."""
    if name == "branches":
        return _branch_case()
    if name == "zero_row":
        d = _lbs_random(257, 55, 4, 7001)
        d["lbs"][64] = 0.0                                                            # first lane of the second wave
        d["exact_rows"][64] = True
        return d
    for nm, N, J, K in LBS_SPARSE_ONLY:
        if nm == name:
            rows = torch.arange(N)
            if K == 1:
                cols = (rows, torch.where(rows % 2 == 0, 250 + (rows // 2) % 6, (rows * 37) % 250))      # every second row on one of 250..255
            else:
                r = rows[rows % 2 == 0]
                cols = (r[:, None].expand(-1, 6), torch.arange(250, 256)[None].expand(len(r), -1))  # every second row uses all of 250..255
            return _lbs_random(N, J, K, 7100 + K, cols)
    N, J = (int(s[1:]) for s in name.split("_"))
    return _lbs_random(N, J, min(4, J), 7 * N + J)


# rows per class of the branch case
BRANCH_ROWS = 16


def _branch_case():
    """The construction of tests/test_avatar_gpu.py:101 -- quaternions near (1,0,0,0), (0,1,0,0), (0,0,1,0), (0,0,0,1) under an identity joint, which select
    the four arg-max candidates of matrix_to_quaternion, once at blend weight 1 and once at 0.004 (a strongly shrunk blend) -- extended by the same rows
    under a blend scaled by -0.5, where the candidate a positive blend selects has a radicand <= 0 (the positive-part branch of the sqrt).  The
    off-components are large enough that no two candidates come near a tie."""
    base = torch.tensor([[1.0, 0.30, 0.10, 0.20], [0.20, 1.0, 0.30, 0.10], [0.10, 0.20, 1.0, 0.30], [0.30, 0.10, 0.20, 1.0]])
    near = torch.tensor([[1.0, 0.02, 0.01, 0.03], [0.02, 1.0, 0.03, 0.01], [0.01, 0.02, 1.0, 0.03], [0.03, 0.01, 0.02, 1.0]])
    g = torch.Generator().manual_seed(7200)
    blocks, weights = [], []
    for q, w in ((near, 1.0), (near, 0.004), (base, 1.0), (base, 0.004), (base, -0.5)):
        qs = torch.nn.functional.normalize(q).repeat(BRANCH_ROWS // 4 * 4, 1)
        blocks.append(qs * (0.5 + 1.5 * torch.rand(qs.shape[0], 1, generator=g)))
        weights.append(torch.full((qs.shape[0],), w))
    rot = torch.cat(blocks)
    N = rot.shape[0]
    lbs = torch.zeros(N, 3)
    lbs[:, 0] = torch.cat(weights)
    A = torch.eye(4)[None].repeat(3, 1, 1)
    pos = torch.randn(N, 3, generator=g)
    ups = (torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g))
    return dict(N=N, J=3, K=1, lbs=lbs, pos=pos, rot=rot, A=A, ups=ups, exact_rows=torch.zeros(N, dtype=torch.bool))


def _lbs_ref(name, dtype, joint_grad):
    d = lbs_case(name)
    A = d["A"].to(dtype).clone().requires_grad_(joint_grad)
    p = d["pos"].to(dtype).clone().requires_grad_(True)
    r = d["rot"].to(dtype).clone().requires_grad_(True)
    lp, lr = ao.transform_cano2live(p, r, d["lbs"].to(dtype), A)
    torch.autograd.backward([lp, lr], [u.to(dtype) for u in d["ups"]])
    return lp.detach(), lr.detach(), p.grad, r.grad, (A.grad if joint_grad else None)


@functools.lru_cache(maxsize=None)
def lbs_reference(name, joint_grad=False):
    """(float64, float32) tuples of (live positions, live rotations, dL/dpositions, dL/drotations, dL/dA or None)."""
    return _lbs_ref(name, F64, joint_grad), _lbs_ref(name, F32, joint_grad)


def m2q_quantities(name):
    """Float64, per row of a skinning case: the four radicands x4 [N, 4] of matrix_to_quaternion applied to (blend[:3, :3] R(q)) and their positive-part
    roots q_abs [N, 4]."""
    d = lbs_case(name)
    M = torch.einsum('nj,jxy->nxy', d["lbs"].double(), d["A"].double())[:, :3, :3]
    m = M @ ao.quaternion_to_matrix(d["rot"].double())
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    x4 = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], 1)
    return x4, x4.clamp_min(0).sqrt()


FRAGILE_REL = 1e-4
FRAGILE_CAP = 2e-3            # at most this share of a case's rows; none at N <= 1000


@functools.lru_cache(maxsize=None)
def fragile_rows(name):
    """[N] bool, from the float64 inputs alone: rows whose arg-max candidate may legitimately differ between fp32 and fp64 -- the two largest q_abs differ by
    less than 1e-4 of the larger, or the largest is within 1e-4 of the 0.1 floor.  Left out of the rotation comparisons only."""
    _, qa = m2q_quantities(name)
    top = torch.topk(qa, 2, dim=1).values
    return ((top[:, 0] - top[:, 1]) < FRAGILE_REL * top[:, 0]) | ((top[:, 0] - 0.1).abs() < FRAGILE_REL)


def all_lbs_cases():
    return [lbs_name(N, J) for N, J in LBS_NJ] + [c[0] for c in LBS_SPARSE_ONLY] + ["zero_row", "branches"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hand fusion
# ---------------------------------------------------------------------------------------------------------------------------------------------------
HAND_N = (1, 255, 257, 5000)
HAND_RTOL, HAND_ATOL = 1e-5, 2e-6        # those of tests/test_avatar_gpu.py::test_hand_fuse_matches_reference_blend, here against float64
HAND_CENTRE = (0.0, 0.125, 0.0)
# x extents of the (left, right) hand boxes and the x ranges of the rows "on the left slope" / "on the right slope".
#   apart  : the hands of a body (left at +x).  wl rises around x = 0.52, wr around x = -0.52, w = wl + wr runs over all of (0, 1) and wl + wr < 1.
#   overlap: boxes that reach across each other, so that wl + wr > 1 between them and the max(wl + wr, 1) branch divides; the left box is half as wide
#            as the right one, which leaves wl + wr < 1 for x < -0.3.
HAND_BOXES = {
    "apart": ((0.62, 0.82), (-0.82, -0.62), (0.37, 0.67), (-0.67, -0.37)),
    "overlap": ((0.1, 0.5), (-0.9, -0.1), (-0.25, 0.3), (-0.6, -0.3)),
}


@functools.lru_cache(maxsize=None)
def hand_case(N, boxes):
    """Float32 CPU inputs of the hand-fusion case with N rows and the box layout ``boxes``.  Row i is of class i % 8:
       0  y == centre_y, x on the left slope                        4  far out at +x: the exponent of wl is below -88, that of wr above 88
       1  ordinary, y above the centre                              5  far out at -x: the reverse
       2  y < centre_y (weights forced to 0)                        6  y == centre_y, x on the right slope
       3  x on either slope, y above the centre                     7  y just below centre_y (the next float down), x on the left slope"""
    lx, rx, ls, rs = HAND_BOXES[boxes]
    g = torch.Generator().manual_seed(7300 + N + (0 if boxes == "apart" else 1))
    cls = torch.arange(N) % 8
    cy = torch.tensor(HAND_CENTRE[1])
    u = lambda: torch.rand(N, generator=g)  # noqa: E731
    left_slope, right_slope = ls[0] + (ls[1] - ls[0]) * u(), rs[0] + (rs[1] - rs[0]) * u()
    x = (u() - 0.5) * 4.0
    y = cy + 0.01 + u()
    x = torch.where((cls == 0) | (cls == 7), left_slope, x)
    x = torch.where(cls == 6, right_slope, x)
    x = torch.where(cls == 3, torch.where(u() < 0.5, left_slope, right_slope), x)
    x = torch.where(cls == 4, 20.0 + 20.0 * u(), x)
    x = torch.where(cls == 5, -20.0 - 20.0 * u(), x)
    y = torch.where((cls == 0) | (cls == 6), cy, y)
    y = torch.where(cls == 2, cy - 0.01 - u(), y)
    y = torch.where(cls == 7, torch.nextafter(cy, torch.tensor(-1.0)), y)
    xyz = torch.stack([x, y, torch.randn(N, generator=g) * 0.1], 1)

    def verts(lo, hi):
        v = torch.rand(778, 3, generator=g)
        v[:, 0] = lo + (hi - lo) * v[:, 0]
        v[0, 0], v[1, 0] = lo, hi
        return v

    cur = {'positions': torch.randn(N, 3, generator=g), 'opacity': torch.rand(N, 1, generator=g),
           'scales': torch.rand(N, 3, generator=g) * 0.01, 'rotations': torch.randn(N, 4, generator=g)}
    hand = {k: torch.randn(v.shape, generator=g) for k, v in cur.items()}
    return dict(N=N, cls=cls, xyz=xyz, left=verts(*lx), right=verts(*rx), centre=torch.tensor(HAND_CENTRE), cur=cur, hand=hand)


def hand_weights(d, dtype=F64):
    """(wl, wr before the y cut and the normalisation, exponent arguments of the two sigmoids) in ``dtype`` -- what the case-validity test counts."""
    xyz = d["xyz"].to(dtype)
    nl = ao.normalize_vert_bbox(d["left"].to(dtype), attris=xyz, dim=0, per_axis=True)[..., 0]
    nr = ao.normalize_vert_bbox(d["right"].to(dtype), attris=xyz, dim=0, per_axis=True)[..., 0]
    al, ar = -2.5 * (nl + 2.0), 2.5 * (nr - 2.0)             # the kernel evaluates 1 / (1 + exp(al)) and 1 / (1 + exp(ar))
    return torch.sigmoid(-al), torch.sigmoid(-ar), al, ar


@functools.lru_cache(maxsize=None)
def hand_reference(N, boxes):
    """The four fused attribute arrays in float64 (a dict) and the blend weight w [N, 1]."""
    d = hand_case(N, boxes)
    c = lambda t: t.to(F64).clone()  # noqa: E731
    out, w = ao.hand_fuse({k: c(v) for k, v in d["cur"].items()}, c(d["xyz"]), c(d["left"]), c(d["right"]), c(d["centre"]),
                          {k: c(v) for k, v in d["hand"].items()})
    return out, w
