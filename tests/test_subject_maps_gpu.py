"""Canonical maps from a mesh on the GPU (``include/ag_subject_maps.h``) against the float64 restatement in
``subject_maps_oracle.py``: face ids, barycentrics and resolved attributes, the exact grid k-NN, determinism, and the path from a mesh
to a rendering, training ``AvatarNet``.

Bounds of the barycentrics / attributes (check 6): not derivable in closed form for sliver faces, so they are taken from the oracle
itself -- the same restatement run in float32 against float64 on the same mesh, worst deviation relative to the output's largest
magnitude, times 4 (a different but equally legitimate fp32 evaluation order can be off by about as much again in either direction).
Measured on the MI355X, worst deviation from float64 relative to max |output| on non-fragile pixels.  The GPU's figure equals the
float32 oracle's in every cell (the kernels are compiled without contraction and follow the header's operation order, which is the
order the float32 oracle uses), so one number is given:

    mesh, S       fragile / covered    bary       position   normal     skinning w.  x, y vs pixel centre   |row sum - 1| (bound 4.0e-7)
    body, 1024    658 / 735 100        1.10e-6    1.28e-7    2.12e-7    1.91e-7      1.23e-7                1.56e-7
    body, 256     169 / 45 952         3.93e-7    1.08e-7    1.30e-7    1.93e-7      1.24e-7                1.49e-7
    soup, 256     70 / 32 864          3.42e-6    5.14e-6    4.71e-6    2.33e-6      4.40e-6                1.15e-7

Face ids: 0 differing pixels on all three, fragile pixels included.  Product-size k-NN (N = 268 348): max |log scale - host k-d tree|
9.5e-7 against the bound 2.9e-6.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_maps_oracle as smo  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = [("body", 1024), ("body", 256), ("soup", 256)]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    import torch
    from animatablegaussians_amd import subject_maps as sm, synth
    if name == "body":
        m = synth.body_mesh()
        v, f, w = m["vertices"], m["faces"], m["lbs_weights"]
    else:
        m = synth.smplx_model_arrays()
        v, f, w = m["v_template"].astype(np.float32), m["f"].astype(np.int32), m["weights"].astype(np.float32)
    n = sm.vertex_normals(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()).cpu().numpy()
    return v, f, n, w


@functools.lru_cache(maxsize=None)
def _gpu(name, S):
    import torch
    from animatablegaussians_amd import subject_maps as sm
    v, f, n, w = _mesh(name)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    maps = sm.canonical_maps(t(v), t(f), t(n), t(w), size=S)
    torch.cuda.synchronize()
    return maps


@functools.lru_cache(maxsize=None)
def _oracle(name, S, dtype):
    v, f, n, w = _mesh(name)
    r = smo.canonical_raster(v, f, S, dtype=dtype)
    r["pos"] = smo.resolve(r["face_id"], r["bary"], f, v, dtype)
    r["nml"] = smo.resolve(r["face_id"], r["bary"], f, n, dtype)
    r["lbs"] = smo.resolve(r["face_id"], r["bary"], f, w, dtype)
    return r


@pytest.mark.parametrize("name,S", CASES)
def test_face_ids_equal_the_oracle_on_every_non_fragile_pixel(name, S):
    want = _oracle(name, S, np.float64)
    got = _gpu(name, S)["face_id"].cpu().numpy()
    keep = ~want["fragile"]
    wrong = int((got[keep] != want["face_id"][keep]).sum())
    print(f"{name} S={S}: {int((want['face_id'] >= 0).sum())} covered, {int(want['fragile'].sum())} fragile, {wrong} differing ids outside them, "
          f"{int((got != want['face_id']).sum())} differing ids in all")
    assert wrong == 0
    assert int((got[keep] >= 0).sum()) == int((want["face_id"][keep] >= 0).sum())


def test_lattice_on_pixel_centres_equals_the_oracle_on_every_pixel():
    import torch
    from animatablegaussians_amd import subject_maps as sm
    for S in (32, 128):
        v, f = smo.lattice_mesh(S, n=6 if S == 32 else 30)
        view = smo.lattice_view(S)
        for cull in (True, False):
            ff = f if cull else f[:, [0, 2, 1]]                                   # clockwise faces, culling off: corners exchanged
            want = smo.rasterize(v, ff, view, S, S, cull=cull)
            fid, bary = sm.rasterize_ortho(torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(ff)).cuda(), view, S, cull=cull)
            assert np.array_equal(fid.cpu().numpy(), want["face_id"])
            assert (want["face_id"] >= 0).sum() > 0.2 * S * S
            assert np.abs(bary.cpu().numpy() - want["bary"]).max() <= 4 * U
        fid, _ = sm.rasterize_ortho(torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(f[:, [0, 2, 1]])).cuda(), view, S)
        assert int((fid >= 0).sum()) == 0                                         # all clockwise, culling on


@pytest.mark.parametrize("name,S", CASES)
def test_barycentrics_and_attributes_within_four_times_the_float32_oracle(name, S):
    o64, o32 = _oracle(name, S, np.float64), _oracle(name, S, np.float32)
    g = _gpu(name, S)
    keep = ~o64["fragile"] & (o64["face_id"] >= 0)
    assert np.array_equal(o32["face_id"][keep], o64["face_id"][keep]), "the float32 restatement must agree on non-fragile pixels"
    got = {"bary": g["bary"], "pos": g["cano_smpl_pos_map"], "nml": g["cano_smpl_nml_map"]}
    got = {k: a.cpu().numpy().astype(np.float64) for k, a in got.items()}
    lbs = np.zeros(o64["lbs"].shape)
    mask = g["mask"].cpu().numpy()
    lbs[mask] = g["init_pts_lbs"].cpu().numpy()
    got["lbs"] = lbs
    X, Y = smo.pixel_centre_xy(S, o64["cano_center"])
    report, failed = [], []
    for k in ("bary", "pos", "nml", "lbs"):
        scale = np.abs(o64[k][keep]).max()
        ref = np.abs(o32[k][keep].astype(np.float64) - o64[k][keep]).max() / scale
        dev = np.abs(got[k][keep] - o64[k][keep]).max() / scale
        report.append(f"{k}: float32 oracle {ref:.3e}, GPU {dev:.3e}")
        if not dev <= 4 * ref:
            failed.append(k)
    # independent of any oracle: the interpolated position lands on the sample point, on EVERY pixel the GPU covered (whichever of
    # two legitimate faces won a fragile pixel); the bound comes from the float32 oracle over ITS covered pixels
    xy_scale = max(np.abs(X).max(), np.abs(Y).max())
    c32, cg = o32["face_id"] >= 0, g["face_id"].cpu().numpy() >= 0
    ref = max(np.abs(o32["pos"][..., 0].astype(np.float64) - X)[c32].max(), np.abs(o32["pos"][..., 1].astype(np.float64) - Y)[c32].max()) / xy_scale
    dev = max(np.abs(got["pos"][..., 0] - X)[cg].max(), np.abs(got["pos"][..., 1] - Y)[cg].max()) / xy_scale
    report.append(f"x, y vs pixel centre (all covered pixels): float32 oracle {ref:.3e}, GPU {dev:.3e}")
    if not dev <= 4 * ref:
        failed.append("xy")
    print(f"{name} S={S}: " + "; ".join(report))
    assert not failed, failed
    # empty pixels exactly 0; N = mask count; canvas order
    empty = g["face_id"].cpu().numpy() < 0
    assert not got["pos"][empty].any() and not got["nml"][empty].any() and not got["bary"][empty].any()
    assert g["init_pts_lbs"].shape[0] == int(mask.sum()) == g["log_scale"].shape[0]
    assert np.array_equal(mask, np.linalg.norm(g["cano_smpl_pos_map"].cpu().numpy(), axis=-1) > 0)
    # rows of init_pts_lbs: sum_c out_c = sum_i b_i s_i with s_i the vertex rows' own sums; each out_c carries <= 3 roundings of
    # non-negative terms (3 u in the sum), b2 = (1 - b0) - b1 makes b0 + b1 + b2 = 1 within 2 u, one more u for slightly negative
    # barycentrics on an edge: 6 u + the input rows' own deviation from 1.  (Non-fragile pixels: there 0 <= b_i <= 1 + O(u).)
    w_rows = np.abs(_mesh(name)[3].astype(np.float64).sum(1) - 1).max()
    rows = np.abs(got["lbs"][keep].sum(-1) - 1).max()
    print(f"{name} S={S}: |row sum - 1| of init_pts_lbs {rows:.3e}, bound {6 * U + w_rows:.3e}")
    assert rows <= 6 * U + w_rows


def _knn_check(points, tol=8 * U, cell=None):
    import torch
    from animatablegaussians_amd import subject_maps as sm
    mean, d3 = sm.knn_dist2(torch.from_numpy(points).cuda(), cell=cell)
    raw = d3
    want = smo.knn3_dist2(points)
    d3 = d3.cpu().numpy().astype(np.float64)
    assert (np.diff(d3, axis=1) >= 0).all()
    err = np.abs(d3 - want)
    assert (err <= tol * want).all(), float((err / np.maximum(want, 1e-300)).max())      # distance VALUES, never indices
    m = mean.cpu().numpy().astype(np.float64)
    assert (np.abs(m - want.mean(1)) <= (tol + 3 * U) * want.mean(1)).all()
    return raw


def test_knn_distances_equal_float64_brute_force():
    """3 subtractions, 3 squares and 2 additions in fp32: the difference x_i - x_j of two fp32 numbers is exact up to one rounding
    RELATIVE TO ITSELF, so d carries at most (2 + 1 + 2) u < 8 u relative error -- there is no cancellation floor."""
    import torch
    from animatablegaussians_amd import subject_maps as sm
    g = _gpu("body", 256)
    pts = g["cano_smpl_pos_map"][g["mask"]].cpu().numpy()
    assert 20000 < len(pts) < 60000
    _knn_check(pts)
    rs = np.random.RandomState(5)
    dup = np.concatenate([pts[:3000], pts[:1500], pts[:700], rs.uniform(-1, 1, (100, 3)).astype(np.float32)])     # exact duplicates: up to three zeros kept
    _knn_check(dup)
    one = (rs.uniform(0, 1e-3, (2000, 3)) + 0.5).astype(np.float32)                                                # every point in one cell
    d_one_cell = _knn_check(one, cell=10.0)                                                                         # the same elementwise relative bound
    d_default = _knn_check(one)
    assert torch.equal(d_one_cell, d_default)                                                                       # the cell size never matters
    # a grid of 10^6 cells along one axis, far from the origin: the cell assignment and the block planes round by a good fraction of a
    # cell there, which the closing distance's safety term has to cover
    line = np.zeros((5000, 3), np.float32)
    line[:, 0] = rs.uniform(500, 600, 5000)
    _knn_check(line, cell=1e-4)
    four = pts[:4].copy()
    _knn_check(four)
    with pytest.raises(ValueError, match="at least 4"):
        sm.knn_log_scale(torch.from_numpy(pts[:3]).cuda())


def test_knn_log_scale_equals_the_host_kd_tree_at_product_size():
    import torch
    from animatablegaussians_amd import subject_maps as sm, synth
    from animatablegaussians_amd.avatar import _knn3_log_scale
    pts = synth.avatar_map_gaussians(1024)["means3D"].astype(np.float32)
    assert len(pts) > 200000
    want = _knn3_log_scale(pts).astype(np.float64)
    got = sm.knn_log_scale(torch.from_numpy(pts).cuda()).cpu().numpy().astype(np.float64)
    # log sqrt(m) = 0.5 log m: a relative error e of m moves it by e / 2, e <= (8 + 3) u from the mean of three distances; the fp32
    # sqrt (1 ulp = 2 u, relative: 2 u in the log), the fp32 log (2 ulp = 4 u of |log| <= 8.1 here) and the host result's own
    # rounding to fp32 (u of |log|)
    bound = 0.5 * 11 * U + 2 * U + 8.1 * 5 * U
    print(f"N = {len(pts)}: max |log scale - host| {np.abs(got - want).max():.3e}, bound {bound:.3e}")
    assert np.abs(got - want).max() <= bound


def test_two_runs_are_bit_identical():
    import torch
    from animatablegaussians_amd import subject_maps as sm
    v, f, n, w = _mesh("body")
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    a = _gpu("body", 1024)
    b = sm.canonical_maps(t(v), t(f), t(n), t(w), size=1024)
    for k in ("cano_smpl_pos_map", "cano_smpl_nml_map", "init_pts_lbs", "log_scale", "face_id", "bary"):
        assert torch.equal(a[k], b[k]), k


def _items(net, S=512, seed=3):
    import torch
    from animatablegaussians_amd import camera
    g = torch.Generator().manual_seed(seed)
    J = net.lbs.shape[1]
    A = torch.eye(4)[None].repeat(J, 1, 1)
    A[:, :3, 3] = (torch.rand(J, 3, generator=g) - 0.5) * 0.02
    extr = torch.from_numpy(camera.calc_front_mv(np.zeros(3, np.float32), tar_pos=(0.0, 0.0, 2.5)))
    intr = torch.tensor([[550.0, 0, S / 2], [0, 550.0, S / 2], [0, 0, 1]])
    return {'cano2live_jnt_mats': A.cuda(), 'cano2live_jnt_mats_woRoot': A.cuda(), 'extr': extr.cuda(), 'intr': intr.cuda(),
            'img_w': S, 'img_h': S}


def test_from_mesh_renders_trains_and_round_trips_through_the_subject_directory(tmp_path):
    import torch
    from animatablegaussians_amd import subject_maps as sm, synth
    from animatablegaussians_amd.avatar import AvatarNet
    torch.manual_seed(31359)
    m = synth.body_mesh()
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    net = AvatarNet.from_mesh({'with_viewdirs': True}, t(m["vertices"]), t(m["faces"]), t(m["lbs_weights"]))
    N = int(net.cano_smpl_mask.sum())
    assert N == net.init_points.shape[0] == net.lbs.shape[0] > 100000 and net.with_viewdirs
    assert torch.equal(net.core.scaling_raw, net.subject_maps["log_scale"][:, None].repeat(1, 3))
    items = _items(net)
    net.get_pose_map(items)
    net.eval()
    with torch.no_grad():
        out = net.render(items, bg_color=(1., 1., 1.))
    assert torch.isfinite(out['rgb_map']).all() and torch.isfinite(out['mask_map']).all() and float(out['mask_map'].max()) > 0.5
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    out = net.render(items, bg_color=(1., 1., 1.))
    loss = (out['rgb_map'] - 0.5).abs().mean() + out['offset'].square().mean()
    loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in net.parameters()) and any(p.grad is not None for p in net.parameters())
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    # the files gen_pos_maps.py writes, read back by the constructor the reference's assets go through
    sm.write_subject_dir(str(tmp_path), net.subject_maps)
    back = AvatarNet.from_data_dir({'with_viewdirs': True}, str(tmp_path))
    assert torch.equal(back.cano_smpl_mask, net.cano_smpl_mask)
    assert torch.equal(back.init_points, net.init_points) and torch.equal(back.lbs, net.lbs)
    assert torch.equal(back.cano_nmls, net.cano_nmls)


def test_from_smplx_on_the_synthetic_model_constructs():
    import torch
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.avatar import AvatarNet
    from animatablegaussians_amd.smplx import SMPLX
    model = SMPLX(synth.smplx_model_arrays(), use_pca=False, flat_hand_mean=True)
    betas = torch.from_numpy(synth.smplx_pose_params()['betas']).cuda()
    nets = [AvatarNet.from_smplx({'with_viewdirs': True}, model, betas, size=256) for _ in range(2)]
    a, b = nets
    N = int(a.cano_smpl_mask.sum())
    assert tuple(a.cano_smpl_mask.shape) == (256, 512) and a.init_points.shape == (N, 3) and a.lbs.shape == (N, 55) and N > 1000
    assert a.core.scaling_raw.shape == (N, 3) and torch.isfinite(a.core.scaling_raw).all()
    for k in ("cano_smpl_pos_map", "cano_smpl_nml_map", "init_pts_lbs", "log_scale"):
        assert torch.equal(a.subject_maps[k], b.subject_maps[k]), k
    with pytest.raises(ValueError, match="host path"):
        AvatarNet.from_smplx({'with_viewdirs': True}, model, betas.cpu(), size=256)


def test_host_tensors_raise_on_the_gpu_box_too():
    import torch
    from animatablegaussians_amd import subject_maps as sm, synth
    m = synth.body_mesh()
    with pytest.raises(ValueError, match="GPU"):
        sm.canonical_maps(torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]).cuda(), torch.from_numpy(m["vertices"]).cuda(),
                          torch.from_numpy(m["lbs_weights"]).cuda())
