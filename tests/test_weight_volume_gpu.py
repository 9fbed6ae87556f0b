"""The blend-weight volume sampler on the GPU (``include/ag_weight_volume.h``) against the float64 restatement in
``weight_volume_oracle.py`` and against outputs of the reference's own ``CanoBlendWeightVolume`` (``golden/weight_volume_ref.npz``);
``canonical_maps`` with a volume; and the path from a directory holding ``template.ply`` and ``cano_weight_volume.npz`` to a rendering,
training ``AvatarNet``.

Bar of every comparison with float64 (the rule of ``test_subject_maps_gpu.py``): 4 x the worst |float32 oracle - float64 oracle| on the
same inputs (a different but equally legitimate fp32 evaluation order can be off by about as much again in either direction) plus
2^-22 (outputs are convex combinations of values <= 1 in magnitude; the term keeps the bar above zero where the float32 oracle
happens to be exact, as for N = 1).  Never derived from the kernel's output.

NOT MEASURED on the MI355X yet: no GPU run of this file exists (the figures belong here once one does; every test prints its own).
Known without a GPU: the kernel's source, compiled for the host with the same no-contraction flag and run thread by thread, equals
the float32 oracle bit for bit on the three shapes below (worst |float32 oracle - float64| 6.4e-7, 1.7e-6 and 2.0e-7), and the
float64 oracle equals the reference's own float64 outputs on the fixture exactly.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_volume_oracle as wvo  # noqa: E402
from weight_volume_oracle import FIXTURE_CASES, GOLDEN, fixture_case  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(9, 7, 5, 6), (16, 16, 16, 55), (5, 4, 3, 1)]
N_POINTS = 4099


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(arrays of a volume file, points [4099, 3] with the special ones, WeightVolume) -- built once, never modified."""
    from animatablegaussians_amd.weight_volume import WeightVolume
    rng = np.random.RandomState(1000 + shape[3])
    res = shape[:3]
    w = rng.uniform(0, 1, shape) ** 3
    diff = (w / w.sum(-1, keepdims=True)).astype(np.float32) if shape[3] > 1 else rng.normal(0, 0.3, shape).astype(np.float32)
    ori = rng.uniform(0, 1, shape).astype(np.float32)
    centre = np.array([0.013, -0.21, 0.017], np.float32)
    bounds = np.stack([centre - np.float32([0.99, 1.1, 0.7]), centre + np.float32([0.99, 0.9, 0.8])]).astype(np.float32)
    sdf = rng.normal(0, 0.1, res).astype(np.float32)
    n_nodes = min(int(np.prod(res)), 512)
    pts = wvo.special_points(bounds, res, rng, N_POINTS - n_nodes - 9)
    assert pts.shape == (N_POINTS, 3)
    a = {"diff_weight_volume": diff, "ori_weight_volume": ori, "sdf_volume": sdf, "volume_bounds": bounds, "center": centre,
         "smpl_bounds": bounds}
    vol = WeightVolume(_t(diff), _t(ori), _t(bounds), _t(centre), _t(bounds), sdf_volume=_t(sdf))
    return a, pts, vol


def _compare(tag, got, volume, pts, bounds):
    o64, o32 = wvo.sample(volume, pts, bounds, np.float64), wvo.sample(volume, pts, bounds, np.float32)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == o64.shape
    own = float(np.abs(o32.astype(np.float64) - o64).max()) if o64.size else 0.0
    dev = float(np.abs(got.astype(np.float64) - o64).max()) if o64.size else 0.0
    bar = 4 * own + 2.0 ** -22
    print(f"{tag}: worst |GPU - float64| {dev:.3e}, float32 oracle {own:.3e}, bar {bar:.3e}, equals the float32 oracle bit for bit: "
          f"{np.array_equal(got, o32)}")
    assert np.isfinite(got).all() and dev <= bar


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [N_POINTS, 1, 0])
def test_parity_with_the_float64_oracle(shape, n):
    a, pts, vol = _case(shape)
    p = pts[:n] if n != 1 else pts[777:778]
    assert (vol.res_x, vol.res_y, vol.res_z, vol.joint_num) == shape
    _compare(f"{shape} N={n} diff", vol.forward_weight(_t(p)), a["diff_weight_volume"], p, a["volume_bounds"])
    _compare(f"{shape} N={n} ori", vol.forward_weight(_t(p), volume_type="ori"), a["ori_weight_volume"], p, a["volume_bounds"])
    lo, hi = a["volume_bounds"].astype(np.float64)
    unit = ((p.astype(np.float64) - lo) / (hi - lo)).astype(np.float32)
    _compare(f"{shape} N={n} requires_scale=False", vol.forward_weight(_t(unit), requires_scale=False), a["diff_weight_volume"], unit, None)


def test_grid_nodes_return_the_stored_rows_bit_for_bit():
    """lo = 0, hi = R - 1 with R - 1 = (8, 4, 2): u = k / (R - 1), 2 u - 1, (g + 1) / 2 and its product with R - 1 are all exact, so
    x = k, f = 0 and the output is 1 * row + seven exact zeros -- on the last node of an axis too, where the upper corners are skipped."""
    import torch
    from animatablegaussians_amd.weight_volume import WeightVolume
    R, C = (9, 5, 3), 6
    rng = np.random.RandomState(7)
    v = rng.normal(0, 1, R + (C,)).astype(np.float32)
    bounds = np.array([[0, 0, 0], [R[0] - 1, R[1] - 1, R[2] - 1]], np.float32)
    vol = WeightVolume(_t(v), _t(v), _t(bounds), _t(np.zeros(3, np.float32)), _t(bounds))
    nodes = np.stack(np.meshgrid(*[np.arange(r, dtype=np.float32) for r in R], indexing="ij"), -1).reshape(-1, 3)
    got = vol.forward_weight(_t(nodes), requires_scale=True)
    assert torch.equal(got, _t(v.reshape(-1, C)))


@pytest.mark.parametrize("out,vol,pts,scaled", FIXTURE_CASES)
def test_reference_fixture(out, vol, pts, scaled):
    """Against what the reference's own class returned in float64; the bar is the oracle's, as above."""
    from animatablegaussians_amd.weight_volume import WeightVolume
    d = np.load(GOLDEN)
    assert out + "_f64" in d.files, "the fixture carries no float64 copy of the reference's outputs"
    w = WeightVolume(_t(d["diff_weight_volume"]), _t(d["ori_weight_volume"]), _t(d["volume_bounds"]), _t(d["center"]), _t(d["smpl_bounds"]),
                     sdf_volume=_t(d["sdf_volume"]))
    p = _t(d[pts])[None]                                                           # [1, N, 3], as the reference is called
    got = {"w_diff": lambda: w.forward_weight(p), "w_ori": lambda: w.forward_weight(p, volume_type="ori"),
           "w_unit": lambda: w.forward_weight(p, requires_scale=False), "sdf": lambda: w.forward_sdf(p)}[out]()
    assert got.shape[:2] == (1, d[pts].shape[0])
    got = got[0].cpu().numpy()
    v, pp, b = fixture_case(d, vol, pts, scaled)
    o64, o32 = wvo.sample(v, pp, b, np.float64), wvo.sample(v, pp, b, np.float32)
    bar = 4 * float(np.abs(o32.astype(np.float64) - o64).max()) + 2.0 ** -22
    dev = float(np.abs(got.astype(np.float64) - d[out + "_f64"]).max())
    print(f"{out}: worst |GPU - reference float64| {dev:.3e}, bar {bar:.3e}, equals the reference's float32 output bit for bit: "
          f"{np.array_equal(got, d[out + '_f32'])}")
    assert dev <= bar


def test_batched_points_equal_single_calls_and_a_repeat_is_bit_identical():
    import torch
    a, pts, vol = _case(SHAPES[1])
    p = _t(pts)
    q = torch.flip(p, (0,)).contiguous()
    both = vol.forward_weight(torch.stack([p, q]))
    assert both.shape == (2, N_POINTS, 55)
    one, two = vol.forward_weight(p), vol.forward_weight(q)
    assert torch.equal(both[0], one) and torch.equal(both[1], two)
    assert torch.equal(vol.forward_weight(torch.stack([p, q])), both) and torch.equal(vol.forward_weight(p), one)
    assert not one.requires_grad and not vol.forward_weight(p.clone().requires_grad_(True)).requires_grad      # no gradient, documented


def test_forward_sdf_with_a_three_dimensional_sdf_volume():
    a, pts, vol = _case(SHAPES[0])
    assert a["sdf_volume"].ndim == 3
    got = vol.forward_sdf(_t(pts))
    assert tuple(got.shape) == (N_POINTS, 1)
    _compare("sdf [N, 3]", got, a["sdf_volume"][..., None], pts, a["volume_bounds"])
    got = vol.forward_sdf(_t(pts)[None], requires_scale=False)
    assert tuple(got.shape) == (1, N_POINTS, 1)
    _compare("sdf [1, N, 3] unscaled", got[0], a["sdf_volume"][..., None], pts, None)


def test_constructor_and_argument_errors():
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.weight_volume import WeightVolume
    a, pts, vol = _case(SHAPES[2])
    b, c = _t(a["volume_bounds"]), _t(a["center"])
    for shape in ((1, 4, 3, 2), (5, 1, 3, 2), (5, 4, 1, 2)):
        with pytest.raises(ValueError, match=">= 2"):
            WeightVolume(torch.zeros(shape).cuda(), torch.zeros(shape).cuda(), b, c, b)
    with pytest.raises(ValueError, match="GPU"):
        vol.forward_weight(torch.from_numpy(pts))
    with pytest.raises(ValueError, match="GPU"):
        WeightVolume(torch.zeros(5, 4, 3, 2), torch.zeros(5, 4, 3, 2), b.cpu(), c.cpu(), b.cpu())
    for bad in (torch.zeros(10, 2), torch.zeros(3), torch.zeros(2, 2, 5, 3)):
        with pytest.raises(ValueError, match="pts must be"):
            vol.forward_weight(bad.cuda())
    with pytest.raises(ValueError, match="sdf_volume"):
        WeightVolume(_t(a["diff_weight_volume"]), _t(a["ori_weight_volume"]), b, c, b).forward_sdf(_t(pts))
    # the C ABI's own refusal of a resolution below 2 (the Python class never lets one through)
    z = torch.zeros(64).cuda()
    rc = _lib.lib().ag_weight_volume_sample(z.data_ptr(), 1, 4, 4, 2, z.data_ptr(), 4, None, z.data_ptr(), None)
    assert rc != 0 and b"at least 2" in _lib.lib().ag_last_error()


def test_rows_past_two_to_the_31_elements_are_addressed():
    """A [129, 257, 257, 253] volume has 2.156e9 elements (8.6 GB): an element index kept in 32 bits wraps for the upper half of the
    last x slab, a byte offset kept in 32 bits for every node past the first half.  Grid nodes with lo = 0, hi = R - 1 (all powers of
    two) return their stored rows bit for bit (see the exact-nodes test), so the check needs no host copy of the volume."""
    import torch
    from animatablegaussians_amd.weight_volume import WeightVolume
    R, C = (129, 257, 257), 253
    assert R[0] * R[1] * R[2] * C > 2 ** 31
    g = torch.Generator().manual_seed(3)
    nodes = torch.stack([torch.randint(0, r, (3000,), generator=g) for r in R], 1)
    nodes[:1500, 0] = R[0] - 1                                                      # past 2^31 elements: x = 128 and y >= 132
    nodes[:1500, 1] = torch.randint(132, R[1], (1500,), generator=g)
    flat = torch.unique((nodes[:, 0] * R[1] + nodes[:, 1]) * R[2] + nodes[:, 2])
    nodes = torch.stack([flat // (R[1] * R[2]), (flat // R[2]) % R[1], flat % R[2]], 1)
    assert int((flat * C >= 2 ** 31).sum()) > 1000
    rows = torch.randn(flat.numel(), C, generator=g).cuda()
    v = torch.zeros(R + (C,), device="cuda")
    v.view(-1, C)[flat.cuda()] = rows
    bounds = torch.tensor([[0., 0., 0.], [R[0] - 1., R[1] - 1., R[2] - 1.]]).cuda()
    vol = WeightVolume(v, v, bounds, torch.zeros(3).cuda(), bounds)
    got = vol.forward_weight(nodes.to(torch.float32).cuda())
    assert torch.equal(got, rows)


@functools.lru_cache(maxsize=None)
def _body_volume(res=(33, 33, 33)):
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.weight_volume import WeightVolume
    m = synth.body_mesh()
    a = synth.weight_volume_arrays(m, res, 55)
    vol = WeightVolume(*[_t(a[k]) for k in ("diff_weight_volume", "ori_weight_volume", "volume_bounds", "center", "smpl_bounds")],
                       sdf_volume=_t(a["sdf_volume"]))
    return m, a, vol


def test_canonical_maps_with_a_volume():
    import torch
    from animatablegaussians_amd import subject_maps as sm
    m, a, vol = _body_volume()
    v, f = _t(m["vertices"]), _t(m["faces"])
    n = sm.vertex_normals(v, f)
    maps = sm.canonical_maps(v, f, n, weight_volume=vol, size=256)
    pts = maps["cano_smpl_pos_map"][maps["mask"]]
    assert 20000 < pts.shape[0] == maps["init_pts_lbs"].shape[0] and maps["init_pts_lbs"].shape[1] == 55
    assert torch.equal(maps["init_pts_lbs"], vol.forward_weight(pts))
    assert torch.equal(maps["cano_center"], vol.center)
    rows = float((maps["init_pts_lbs"].double().sum(1) - 1).abs().max())
    print(f"|row sum - 1| of the sampled weights (not renormalised): {rows:.3e}")
    assert rows < 1e-5
    per_vertex = sm.canonical_maps(v, f, n, _t(m["lbs_weights"]), size=256, center=vol.center)
    for k in ("cano_smpl_pos_map", "cano_smpl_nml_map", "mask", "face_id", "bary", "log_scale"):
        assert torch.equal(maps[k], per_vertex[k]), k
    assert not torch.equal(maps["init_pts_lbs"], per_vertex["init_pts_lbs"])
    # another centre moves the views: the keyword is not ignored
    moved = sm.canonical_maps(v, f, n, weight_volume=vol, size=256, center=vol.center + 0.05)
    assert not torch.equal(moved["mask"], maps["mask"])


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


def test_from_template_dir_renders_trains_and_round_trips_through_the_subject_directory(tmp_path):
    """A directory holding only template.ply and cano_weight_volume.npz -> a rendering, training avatar.  size = 1024: the StyleUNets'
    output maps are 1024^2, which is also what the from_mesh test of this kind runs at."""
    import torch
    from animatablegaussians_amd import obj_io, subject_maps as sm
    from animatablegaussians_amd.avatar import AvatarNet
    torch.manual_seed(31359)
    m, a, vol = _body_volume()
    src = tmp_path / "subject"
    obj_io.save_mesh_ply(str(src / "template.ply"), m["vertices"], m["faces"])
    np.savez(str(src / "cano_weight_volume.npz"), **a)
    assert sorted(os.listdir(src)) == ["cano_weight_volume.npz", "template.ply"]
    net = AvatarNet.from_template_dir({'with_viewdirs': True}, str(src))
    N = int(net.cano_smpl_mask.sum())
    assert N == net.init_points.shape[0] == net.lbs.shape[0] > 100000 and net.with_viewdirs and net.lbs.shape[1] == 55
    assert torch.equal(net.lbs, vol.forward_weight(net.init_points))
    assert net.core.lbs_sparse is None                                              # dense rows: the diffused volume has no zeros
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
    sm.write_subject_dir(str(tmp_path / "written"), net.subject_maps)
    back = AvatarNet.from_data_dir({'with_viewdirs': True}, str(tmp_path / "written"))
    assert torch.equal(back.cano_smpl_mask, net.cano_smpl_mask)
    assert torch.equal(back.init_points, net.init_points) and torch.equal(back.lbs, net.lbs)
