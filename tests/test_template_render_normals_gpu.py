"""``template_render.render_normals`` against a torch restatement: the samples of ``template_render_oracle.sample`` (which the kernel gives
bit for bit), the gradient and the density of ``template_field_grad_oracle`` / ``template_field_oracle`` at them, the unit normals
composited by ``template_render_oracle.composite`` in the colour's place -- once in float64, once in float32.

Bars as everywhere in the template stage: |gpu - float64 chain| <= 4 x max|float32 chain - float64 chain| + 2^-22 x max|float64 chain|, per
output, maxima over the case's whole ray set.  ``acc_map`` must moreover be ``render``'s bit for bit, and nothing may depend on
``chunk_size``.  Every test prints measured deviation and bar.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_grad_oracle as tgo  # noqa: E402
import template_field_oracle as tfo  # noqa: E402
import template_render_oracle as tro  # noqa: E402

pytestmark = pytest.mark.gpu
NEAR_SUR_DIST = 0.05


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


@functools.lru_cache(maxsize=None)
def _sphere_net():
    from animatablegaussians_amd.template_field import TemplateField
    net = tfo.make_net(tfo.NARROW, 4, trained=False)        # geometric initialisation: an approximate sphere of radius 0.7
    arch = net["arch"]
    return net, TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=False, multires_viewdir=arch["multires_viewdir"])


@functools.lru_cache(maxsize=None)
def _rays(R):
    """``R`` rays of a 12 x 12 camera at the sphere, the box near / far and a depth per ray (0: none)."""
    o, d = tro.pinhole_rays(12, half_width=0.3)
    idx = np.arange(144)[::4][:R] if R <= 36 else np.arange(R)
    o, d = o[idx], d[idx]
    near, far = np.full(R, 1.3, np.float32), np.full(R, 3.7, np.float32)
    # the depth of a ray: its first of 64 uniform samples inside the body by the float64 oracle (the surface is less than one step of
    # 0.038 in front of it, inside the window of NEAR_SUR_DIST); 0 for a ray that stays outside, and for every third ray
    import torch
    z, pts = tro.sample(o, d, near, far, 64)
    inside = tfo.forward(_sphere_net()[0], pts.reshape(-1, 3), None, torch.float64)["raw"].reshape(R, 64) < 0
    dist = np.where(inside.any(1), z[np.arange(R), inside.argmax(1)], 0).astype(np.float32)
    dist[::3] = 0.0
    assert (dist > 1e-6).sum() >= R // 4
    for a in (o, d, near, far, dist):
        a.setflags(write=False)
    return o, d, near, far, dist


@functools.lru_cache(maxsize=None)
def _chain(R, sampling, S):
    """The restatement in float64 and float32 -- built once, never modified."""
    import torch
    net, _ = _sphere_net()
    o, d, near, far, dist = _rays(R)
    if sampling == "depth":
        valid = dist > 1e-6
        near = np.where(valid, dist - np.float32(NEAR_SUR_DIST), near).astype(np.float32)
        far = np.where(valid, dist + np.float32(NEAR_SUR_DIST), far).astype(np.float32)
    z, pts = tro.sample(o, d, near, far, S)
    chains = []
    for dtype in (torch.float64, torch.float32):
        g = tgo.autograd(net, pts.reshape(-1, 3), dtype)
        density = tfo.forward(net, pts.reshape(-1, 3), None, dtype)["density"]
        maps = tro.composite(density, tgo.unit(g["normal"]), z, False, dtype)
        chains.append(dict(normal=g["normal"].reshape(R, S, 3), normal_map=maps["rgb_map"], acc_map=maps["acc_map"], depth_map=maps["depth_map"],
                           weights=maps["weights"]))
    for c in chains:
        for a in c.values():
            a.setflags(write=False)
    return chains


def _compare(name, got, o64, o32, keys):
    for k in keys:
        w64, w32 = o64[k], o32[k].astype(np.float64)
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert g.shape == w64.shape, (k, g.shape, w64.shape)
        own = float(np.abs(w32 - w64).max())
        bar = 4 * own + 2.0 ** -22 * float(np.abs(w64).max())
        dev = float(np.abs(g - w64).max())
        print(f"{name} {k}: |gpu - float64 chain| {dev:.3e}, the float32 chain's own {own:.3e}, bar {bar:.3e}")
        assert np.isfinite(g).all() and dev <= bar, f"{name} {k}: {dev:.3e} > {bar:.3e}"


ALL = ("normal", "normal_map", "acc_map", "depth_map", "weights")


@pytest.mark.parametrize("R", [33, 130])
@pytest.mark.parametrize("sampling,S", [("uniform", 64), ("depth", 2), ("depth", 64)])
def test_render_normals_against_the_chain(R, sampling, S):
    from animatablegaussians_amd import template_render as tr
    net, field = _sphere_net()
    o64, o32 = _chain(R, sampling, S)
    o, d, near, far, dist = (_t(a) for a in _rays(R))
    kw = dict(sampling=sampling)
    if sampling == "depth":
        kw.update(dist=dist, near_sur_dist=NEAR_SUR_DIST, n_samples=S)
    got = tr.render_normals(field, o, d, near, far, want=ALL, **kw)
    assert set(got) == set(ALL) and got["normal"].shape == (R, S, 3) and got["normal_map"].shape == (R, 3) and got["acc_map"].shape == (R,)
    assert got["depth_map"].shape == (R,) and got["weights"].shape == (R, S)
    assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in got.values())
    assert set(tr.render_normals(field, o, d, near, far, **kw)) == {"normal_map", "acc_map"}
    _compare(f"render_normals R = {R}, {sampling}, S = {S}", got, o64, o32, ALL)
    acc = got["acc_map"].cpu().numpy()
    length = np.linalg.norm(got["normal_map"].cpu().numpy().astype(np.float64), axis=1)
    print(f"acc {acc.min():.4f} .. {acc.max():.4f}; |normal_map| up to {length.max():.4f}")
    assert acc.max() > 0.5 and (length <= acc + 1e-5).all(), "a sum of unit vectors with weights of sum acc is at most acc long"
    # acc_map, depth_map and weights are render's, bit for bit
    maps = tr.render(field, o, d, near, far, want=("acc_map", "depth_map", "weights"), **kw)
    assert _same(maps, {k: got[k] for k in maps}), "acc_map / depth_map / weights differ from render's"
    # the chain of the public calls
    n2, f2 = near, far
    if sampling == "depth":
        import torch
        valid = dist > 1e-6
        n2, f2 = torch.where(valid, dist - NEAR_SUR_DIST, near), torch.where(valid, dist + NEAR_SUR_DIST, far)
    pts, z = tr.sample_pts_on_rays(o, d, n2, f2, S)
    ret = field.sdf_normal(pts.view(-1, 3), want=("sdf", "normal", "density"))
    assert np.array_equal(_bits(got["normal"]).reshape(-1, 3), _bits(ret["normal"])), "normal is not sdf_normal's at the samples"
    by_hand = tr.composite(ret["density"], field.surface_normals(pts.view(-1, 3)), z, want=("rgb_map", "acc_map"))
    assert np.array_equal(_bits(by_hand["rgb_map"]), _bits(got["normal_map"])) and np.array_equal(_bits(by_hand["acc_map"]), _bits(got["acc_map"]))
    for chunk in (1, 7, R):
        assert _same(got, tr.render_normals(field, o, d, near, far, want=ALL, chunk_size=chunk, **kw)), f"chunk_size = {chunk} changes the outputs"
    batched = tr.render_normals(field, o[None], d[None], near[None], far[None], want=ALL,
                                **dict(kw, dist=dist[None]) if sampling == "depth" else kw)
    assert batched["normal"].shape == (1, R, S, 3) and _same(got, {k: v[0] for k, v in batched.items()})


def test_render_normals_posed_space_is_the_chain_by_hand():
    import inverse_skinning_oracle as iso
    import mesh_query_oracle as mqo
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd import template_render as tr
    from animatablegaussians_amd.weight_volume import WeightVolume
    net, field = _sphere_net()
    case = iso.smooth_case((16, 16, 16, 55), n=1, B=1, offset=0.05)
    vol = WeightVolume(_t(case["volume"]), _t(case["volume"]), case["bounds"], np.zeros(3, np.float32), case["bounds"])
    v, f = mqo.lattice_mesh(8, 10)
    live = dict(cano2live_jnt_mats=_t(case["jnt_mats"]), volume=vol, live_mesh_v=_t(v[None]), live_mesh_f=_t(f[None]),
                live_mesh_lbs=_t(mqo.sparse_weights(v, 55)[None]), near_thres=0.05, use_root_finding=True, with_hand=False)
    o, d = tro.pinhole_rays(8, eye=(0.1, -0.2, -2.5), target=(0.0, -0.2, 0.0), half_width=0.3)
    o, d = _t(o), _t(d)
    near, far = _t(np.full(64, 1.8, np.float32)), _t(np.full(64, 3.2, np.float32))
    want = ("normal", "normal_map", "acc_map")
    got = tr.render_normals(field, o, d, near, far, space="live", sampling="uniform", live=live, chunk_size=24, want=want)
    pts, z = tr.sample_pts_on_rays(o, d, near, far, 64)
    cano, _ = inv.transform_live2cano(pts.view(1, -1, 3), **live)
    assert not np.array_equal(_bits(cano[0]), _bits(pts.view(-1, 3))), "the samples were not moved"
    ret = field.sdf_normal(cano[0], want=("sdf", "normal", "density"))
    assert np.array_equal(_bits(got["normal"]).reshape(-1, 3), _bits(ret["normal"])), "normal is not the gradient at the canonical points"
    by_hand = tr.composite(ret["density"], field.surface_normals(cano[0]), z, want=("rgb_map", "acc_map"))
    assert np.array_equal(_bits(by_hand["rgb_map"]), _bits(got["normal_map"])) and np.array_equal(_bits(by_hand["acc_map"]), _bits(got["acc_map"]))
    posed = tr.render(field, o, d, near, far, space="live", sampling="uniform", live=live, want=("acc_map",))
    assert np.array_equal(_bits(posed["acc_map"]), _bits(got["acc_map"]))
    cano_maps = tr.render_normals(field, o, d, near, far, sampling="uniform", want=want)
    assert not _same(got, cano_maps)
    # the canonical gradient against the float64 oracle at the canonical points the kernels found
    import torch
    c = cano[0].cpu().numpy()
    o64, o32 = tgo.autograd(net, c, torch.float64), tgo.autograd(net, c, torch.float32)
    _compare("posed render", {"normal": got["normal"].view(-1, 3)}, o64, o32, ("normal",))
    acc = got["acc_map"].cpu().numpy()
    assert np.isfinite(acc).all() and acc.max() > 0.5


def test_refusals_and_empty_ray_sets():
    import torch
    from animatablegaussians_amd import template_render as tr
    net, field = _sphere_net()
    o, d, near, far, dist = (_t(a[:10]) for a in _rays(33))
    bad = [
        lambda: tr.render_normals(None, o, d, near, far, sampling="uniform"), lambda: tr.render_normals(field, o, d, near, far, sampling="importance"),
        lambda: tr.render_normals(field, o, d, near, far, sampling="smpl"), lambda: tr.render_normals(field, o, d, near, far, sampling="depth"),
        lambda: tr.render_normals(field, o, d, near, far, sampling="depth", dist=dist),
        lambda: tr.render_normals(field, o, d, near, far, sampling="depth", dist=dist, near_sur_dist=0.05, n_samples=1),
        lambda: tr.render_normals(field, o, d, near, far, sampling="depth", dist=dist, near_sur_dist=0.05, n_samples=1025),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", space="world"),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", space="live"),
        lambda: tr.render_normals(field, o.cpu(), d, near, far, sampling="uniform"), lambda: tr.render_normals(field, o, d[:5], near, far, sampling="uniform"),
        lambda: tr.render_normals(field, o, d, near.double(), far, sampling="uniform"),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", chunk_size=0),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", want=("rgb_map",)),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", want=("disp_map",)),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", want=("normals",)),
        lambda: tr.render_normals(field, o, d, near, far, sampling="uniform", u=torch.rand(10, 63, device="cuda")),
        lambda: tr.render(field, o, d, near, far, sampling="uniform", want=("normal",)),
        lambda: tr.render(field, o, d, near, far, sampling="uniform", want=("normal_map",)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    e3, e1 = torch.empty((0, 3), device="cuda"), torch.empty((0,), device="cuda")
    for sampling, kw, S in (("uniform", {}, 64), ("depth", dict(dist=e1, near_sur_dist=0.05, n_samples=9), 9)):
        r0 = tr.render_normals(field, e3, e3, e1, e1, sampling=sampling, want=ALL, **kw)
        assert r0["normal"].shape == (0, S, 3) and r0["normal_map"].shape == (0, 3) and r0["acc_map"].shape == (0,) and r0["weights"].shape == (0, S)
        assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in r0.values())
    # a perturbed sampling gives other samples, and the same ones for the same u
    u = torch.rand(10, 64, device="cuda")
    a = tr.render_normals(field, o, d, near, far, sampling="uniform", u=u, want=ALL)
    b = tr.render_normals(field, o, d, near, far, sampling="uniform", u=u, want=ALL, chunk_size=3)
    assert _same(a, b) and not _same(a, tr.render_normals(field, o, d, near, far, sampling="uniform", want=ALL))
