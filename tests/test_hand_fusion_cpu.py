"""Host-side checks of the hand fusion (``hand_fusion.py``, ``include/ag_hand_fusion.h``): the oracle against the reference's own modules
(``tests/golden/hand_fusion_ref.npz``, written by ``make_golden_hand_fusion.py``), state-dict loading, the pose fold, the packed blob, the
MANO topology, the binding table, the entry points' refusals that run before any device call, and the exclusion cap of the GPU tests
evaluated on the two oracle runs alone.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hand_fusion_oracle as hfo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hand_fusion_ref.npz")
TOPOLOGY = os.path.join(ROOT, "tests", "golden", "mano_topology.npz")
HEADER = os.path.join(ROOT, "include", "ag_hand_fusion.h")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def _fixture_scene(fx, posed):
    """The scene of the fixture from its STORED inputs; only the weights come from the recipe."""
    sc = hfo.scene("mixed", len(fx["p"]), pose=True)
    for k in ("p", "cano_xyz", "sdf_b", "color_b"):
        assert np.array_equal(sc[k], fx[k]), f"the recipe's {k} is not the fixture's: regenerate the fixture"
        sc[k] = fx[k]
    for side in hfo.SIDES:
        sc["hands"][side] = {k: fx[f"{side}_{k}"] for k in ("v", "n", "f", "cano_v")}
    sc["hand_pose"] = fx["hand_pose"] if posed else None
    sc["density_b_in"] = None                      # the reference recomputes the density at every point
    cp = {side: dict(dist2=fx[f"{side}_dist2"], face=fx[f"{side}_face"], bary=fx[f"{side}_bary"]) for side in hfo.SIDES}
    return sc, cp


@pytest.mark.parametrize("pose", ["zero", "posed"])
def test_oracle_equals_the_reference_modules(pose):
    fx = np.load(FIXTURE)
    sc, cp = _fixture_scene(fx, pose == "posed")
    o64, o32 = hfo.fuse(sc, torch.float64, cp), hfo.fuse(sc, torch.float32, cp)
    for k in ("sdf", "density", "color"):
        f64, f32 = fx[f"{pose}_{k}64"], fx[f"{pose}_{k}32"]
        assert f64.dtype == np.float64 and f32.dtype == np.float32 and o64[k].shape == f64.shape
        rel = float(np.abs(o64[k] - f64).max() / np.abs(f64).max())
        own = float(np.abs(f32.astype(np.float64) - f64).max())
        d32 = float(np.abs(o32[k].astype(np.float64) - f32).max())
        print(f"{pose} {k}: float64 oracle - fixture {rel:.2e} of the largest value; float32 oracle - fixture {d32:.3e}, the fixture's own {own:.3e}")
        assert rel <= 1e-12
        assert own > 0 and d32 <= 4 * own
    w = o64["wl"] + o64["wr"]
    assert (w > 0.99).sum() > 50 and (w < 1e-30).sum() > 50 and ((w > 0.01) & (w < 0.99)).sum() >= 1, "the fixture does not cover body, hands and the fade"
    assert float(np.abs(fx["posed_color64"] - fx["zero_color64"]).max()) > 1e-3, "the pose columns carry no weight"
    assert (fx["left_face"] >= 0).all() and fx["left_dist2"].min() == 0.0, "the point on the surface is gone"


def test_the_sdf_column_carries_weight():
    """Zeroing column 27 of layer 0 (``sdf_h``) must move the colour: a kernel that dropped the column would not pass the bars."""
    sc, cp, _, o64, _ = hfo.case("active", 257)
    cut = dict(sc, nets={s: [(w.copy(), b) for w, b in sc["nets"][s]] for s in hfo.SIDES})
    for s in hfo.SIDES:
        cut["nets"][s][0][0][:, 27] = 0
    assert float(np.abs(hfo.fuse(cut, torch.float64, cp)["color"] - o64["color"]).max()) > 1e-2


@pytest.mark.parametrize("kind,n,kw", [(k, 1031, {}) for k in ("mixed", "inactive", "active", "left", "clasped")]
                         + [("mixed", n, {}) for n in hfo.SIZES[:-1]] + [("faces", 1031, dict(own_closest=True)), ("faces", 1031, dict(own_closest=True, subdiv=2)),
                                                                        ("mixed", 257, dict(pose=True)), ("mixed", 257, dict(mano=True)),
                                                                        ("mixed", 257, dict(empty_right=True)), ("faces", 257, dict(empty_right=True, own_closest=True)),
                                                                        ("mixed", 257, dict(color=False))])
def test_the_oracles_alone_stay_under_the_exclusion_cap(kind, n, kw):
    """The GPU tests may leave out a point only where the float32 and float64 oracles take different discrete decisions, at most 1 % of
    a case.  Evaluated here on the oracle alone, for every point set the GPU tests use."""
    sc, _, o32, o64, keep = hfo.case(kind, n, **kw)
    out = int((~keep).sum())
    print(f"{kind} n = {n}: {out} of {n} points left out; inactive in float32: {int(o32['inactive'].sum())}")
    assert out <= hfo.EXCLUSION_CAP * n
    if kind == "inactive":
        assert o32["inactive"].all()
    if kind in ("active", "left", "clasped"):
        assert not o32["inactive"].any()
    if kind == "left":
        assert (o32["wr"] == 0).all() and (o32["wl"] > 0).all()
    if kind == "clasped":
        assert ((o64["wl"] + o64["wr"]) > 0.999).sum() > n // 2 and (np.minimum(o64["wl"], o64["wr"]) > 0.3).sum() > n // 8, "too few points have wl + wr > 1"
    if kw.get("empty_right"):
        assert (o32["wr"] == 0).all() and (o32["face_right"] == -1).all() and (o32["wl"] > 0).sum() > n // 4
    if kind == "mixed" and n >= 6:
        kept = [2] if kw.get("empty_right") else [2, 4]                       # point 4 sits by the right hand
        assert o32["inactive"][[3, 5]].all() and not o32["inactive"][kept].any(), "y at the centre is kept, one ulp below it is zeroed"


# ---- state dict, fold, blob ---------------------------------------------------------------------------------------------------------------
def _fields():
    from animatablegaussians_amd.hand_fusion import HandField
    left, right = hfo.make_hand_net(101), hfo.make_hand_net(202)
    sd = hfo.state_dict(left, right)
    return sd, HandField.from_state_dict(sd, "left"), HandField.from_state_dict(sd, "right"), left, right


def test_from_state_dict_reads_both_hands():
    sd, fl, fr, left, right = _fields()
    for f, layers in ((fl, left), (fr, right)):
        assert f.multires == 4 and f.n_joints == 15 and f.k_point == 28 and len(f.layers) == 6
        for (w, b), (ww, bw) in zip(f.layers, layers):
            assert w.dtype == np.float32 and np.array_equal(w, ww) and np.array_equal(b, bw)
    assert [w.shape for w, _ in fl.layers] == [(64, 88)] + [(64, 64)] * 4 + [(3, 64)]


def test_from_state_dict_refuses_by_key():
    from animatablegaussians_amd.hand_fusion import HandField
    sd, *_ = _fields()
    with pytest.raises(ValueError, match="side"):
        HandField.from_state_dict(sd, "middle")
    for key in ("left_hand.tex_mlp.fc_list.0.0.weight", "left_hand.tex_mlp.fc_list.3.0.bias", "left_hand.tex_mlp.fc_list.5.weight"):
        cut = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(KeyError, match=re.escape(key)):
            HandField.from_state_dict(cut, "left")
    HandField.from_state_dict({k: v for k, v in sd.items() if not k.startswith("left")}, "right")          # the other hand is not needed
    for key, shape, what in (("right_hand.tex_mlp.fc_list.0.0.weight", (64, 87), "88"), ("right_hand.tex_mlp.fc_list.2.0.weight", (64, 48), "64"),
                             ("right_hand.tex_mlp.fc_list.1.0.weight", (48, 64), "32 or 64"), ("right_hand.tex_mlp.fc_list.5.weight", (4, 64), "3"),
                             ("right_hand.tex_mlp.fc_list.4.0.bias", (63,), "64")):
        bad = dict(sd)
        bad[key] = torch.zeros(shape)
        if key.endswith("1.0.weight"):
            bad["right_hand.tex_mlp.fc_list.1.0.bias"] = torch.zeros(48)
        if key.endswith("5.weight"):
            bad["right_hand.tex_mlp.fc_list.5.bias"] = torch.zeros(4)
        with pytest.raises(ValueError, match=re.escape(key.rsplit(".", 1)[0])) as e:
            HandField.from_state_dict(bad, "right")
        assert what in str(e.value), (key, str(e.value))
    with pytest.raises(ValueError, match="multires"):
        HandField.from_state_dict(sd, "left", multires=11)


def test_general_multires_and_widths():
    from animatablegaussians_amd.hand_fusion import HandField
    net = hfo.make_hand_net(5, multires=2, widths=(32, 64, 32), n_joints=3)
    f = HandField(net, multires=2)
    assert f.k_point == 16 and f.n_joints == 3 and f.desc().n_layers == 4 and list(f.desc().width)[:4] == [32, 64, 32, 3]
    with pytest.raises(ValueError, match="2 .. 8"):
        HandField(net[-1:], multires=2)


def test_bias_fold_is_the_float64_product_rounded_once():
    _, fl, _, left, _ = _fields()
    w0, b0 = left[0]
    zero = fl.folded_bias()
    quat0 = np.tile([1.0, 0.0, 0.0, 0.0], 15)
    assert np.array_equal(zero, (b0.astype(np.float64) + w0[:, 28:].astype(np.float64) @ quat0).astype(np.float32))
    assert np.array_equal(zero, (b0.astype(np.float64) + w0[:, 28::4].astype(np.float64).sum(1)).astype(np.float32))
    pose = np.random.RandomState(4).uniform(-0.8, 0.8, 45).astype(np.float32)
    pose[3:6] = 0                                                   # one joint at rest: the small-angle branch
    quat = hfo.axis_angle_to_quaternion(torch.from_numpy(pose).double().reshape(-1, 3)).reshape(-1).numpy()
    assert np.allclose(np.linalg.norm(quat.reshape(-1, 4), axis=1), 1.0, atol=1e-15) and np.array_equal(quat[4:8], [1, 0, 0, 0])
    got = fl.folded_bias(pose)
    assert np.array_equal(got, (b0.astype(np.float64) + w0[:, 28:].astype(np.float64) @ quat).astype(np.float32))
    assert np.array_equal(got, fl.folded_bias(torch.from_numpy(pose))) and not np.array_equal(got, zero)
    # the fold against the unfolded layer in float64: W0 @ [u, quat] + b0 == W0[:, :28] @ u + bias0' up to the one rounding of bias0'
    u = np.random.RandomState(5).uniform(-1, 1, 28)
    full = w0.astype(np.float64) @ np.concatenate([u, quat]) + b0
    assert np.abs(full - (w0[:, :28].astype(np.float64) @ u + got)).max() <= 2.0 ** -24 * np.abs(full - w0[:, :28].astype(np.float64) @ u).max()
    with pytest.raises(ValueError, match="45"):
        fl.folded_bias(np.zeros(44))


@pytest.mark.parametrize("pose", [False, True])
def test_pack_unpack_round_trip_with_zero_padding(pose):
    _, fl, _, left, _ = _fields()
    hp = np.random.RandomState(6).uniform(-0.5, 0.5, 45) if pose else None
    blob = fl.pack(hp)
    assert blob.dtype == np.float32 and blob.shape == (20832,)
    layers, padding = fl.unpack(blob)
    assert padding.size == 20832 - (28 * 64 + 64 + 4 * (64 * 64 + 64) + 64 * 3 + 3) and not padding.any()
    for i, ((w, b), (ww, bw)) in enumerate(zip(layers, left)):
        assert np.array_equal(w, ww[:, :28] if i == 0 else ww)
        assert np.array_equal(b, fl.folded_bias(hp) if i == 0 else bw)
    # the layout the header states: element [g][n][j] of layer 1 is W[n][4 g + j]
    off = 32 * 64 + 64
    w1 = blob[off:off + 64 * 64].reshape(16, 64, 4)
    assert w1[3, 7, 2] == left[1][0][7, 14] and blob[off + 64 * 64 + 9] == left[1][1][9]
    w0 = blob[:32 * 64].reshape(8, 64, 4)
    assert w0[6, 11, 3] == left[0][0][11, 27] and not w0[7].any()                # column 27 is sdf_h; rows 28 .. 31 are padding
    with pytest.raises(ValueError, match="20832"):
        fl.unpack(blob[:-1])


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_table_agree():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"ag_hand_field_fuse_args_bytes", "ag_hand_fusion_blob_floats", "ag_hand_field_gate", "ag_hand_field_fuse"}
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert declared <= set(table)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert L.ag_hand_field_fuse_args_bytes() == ctypes.sizeof(_lib.AgHandFieldFuseArgs) == 320
    assert ctypes.sizeof(_lib.AgHandSide) == 96 and ctypes.sizeof(_lib.AgHandFusionDesc) == 40
    assert int(re.search(r"#define AG_HAND_MAX_LAYERS (\d+)", hdr).group(1)) == _lib.AG_HAND_MAX_LAYERS == 8


def test_blob_floats_equals_the_python_layout():
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.hand_fusion import HandField
    L = _lib.lib()
    _, fl, *_ = _fields()
    assert L.ag_hand_fusion_blob_floats(ctypes.byref(fl.desc())) == fl.pack().size == fl._layout()[1] == 20832
    for multires, widths in ((0, (32,)), (2, (32, 64, 32)), (10, (64,) * 7)):
        f = HandField(hfo.make_hand_net(1, multires=multires, widths=widths, n_joints=2), multires=multires)
        assert L.ag_hand_fusion_blob_floats(ctypes.byref(f.desc())) == f.pack().size
    for change, word in ((dict(multires=11), "multires"), (dict(n_layers=1), "n_layers"), (dict(n_layers=9), "n_layers"), (dict(w0=48), "width"),
                         (dict(w5=4), "width")):
        d = fl.desc()
        if "multires" in change:
            d.multires = change["multires"]
        if "n_layers" in change:
            d.n_layers = change["n_layers"]
        if "w0" in change:
            d.width[0] = change["w0"]
        if "w5" in change:
            d.width[5] = change["w5"]
        assert L.ag_hand_fusion_blob_floats(ctypes.byref(d)) == 0 and word in L.ag_last_error().decode()


def _args(_lib, fl):
    a = _lib.AgHandFieldFuseArgs()
    a.N, a.desc, a.centre_y, a.density_b, a.blob_floats = 0, fl.desc(), 0.1, 0.0101, 20832
    for side in (a.left, a.right):
        for c in range(3):
            side.bbox_min[c], side.bbox_max[c] = -1.0, 1.0
        side.face_id = 16                       # never read: every refusal below comes before a launch, and N = 0 launches nothing
    return a


def test_the_entry_points_refuse_before_any_device_call():
    from animatablegaussians_amd import _lib
    L = _lib.lib()
    _, fl, *_ = _fields()
    assert L.ag_hand_field_fuse(ctypes.byref(_args(_lib, fl)), None) == 0                  # N = 0: nothing to do
    assert L.ag_hand_field_fuse(None, None) != 0 and "NULL" in L.ag_last_error().decode()
    for change, word in ((lambda a: setattr(a, "N", -1), "N = -1"), (lambda a: setattr(a, "N", 2 ** 31), "N = "),
                         (lambda a: setattr(a, "blob_floats", 20831), "20832 expected"), (lambda a: setattr(a, "density_b", 0.0), "density_b"),
                         (lambda a: setattr(a, "centre_y", float("nan")), "centre_y"), (lambda a: setattr(a.desc, "n_layers", 1), "n_layers"),
                         (lambda a: a.left.bbox_max.__setitem__(1, -1.0), "left hand"), (lambda a: a.right.bbox_min.__setitem__(2, float("inf")), "right hand"),
                         (lambda a: setattr(a.right, "F", -2), "right hand"), (lambda a: setattr(a.left, "face_id", None), "face_id"),
                         (lambda a: setattr(a.left, "F", 3), "null pointer among"), (lambda a: setattr(a, "color", 16), "color and color_in"),
                         (lambda a: (setattr(a, "color", 16), setattr(a, "color_in", 16)), "blob is NULL"),
                         (lambda a: (setattr(a, "color", 16), setattr(a, "color_in", 16), setattr(a.left, "blob", 8)), "16-byte aligned"),
                         (lambda a: setattr(a, "N", 5), "null pointer in ag_hand_field_fuse")):
        a = _args(_lib, fl)
        change(a)
        assert L.ag_hand_field_fuse(ctypes.byref(a), None) != 0, word
        assert word in L.ag_last_error().decode(), (word, L.ag_last_error().decode())
    box, bad = (ctypes.c_float * 2)(-1.0, 1.0), (ctypes.c_float * 2)(1.0, 1.0)
    assert L.ag_hand_field_gate(None, 0, box, box, 0.0, None, None) == 0
    for call, word in (((None, -1, box, box, 0.0, None, None), "N = -1"), ((None, 0, bad, box, 0.0, None, None), "left box"),
                       ((None, 0, box, None, 0.0, None, None), "right box"), ((None, 0, box, box, float("inf"), None, None), "centre_y"),
                       ((None, 4, box, box, 0.0, None, None), "null pointer")):
        assert L.ag_hand_field_gate(*call) != 0 and word in L.ag_last_error().decode(), word


def test_host_wrappers_refuse_host_tensors_and_bad_arguments():
    from animatablegaussians_amd import hand_fusion as hf
    _, fl, fr, *_ = _fields()
    sc = hfo.scene("mixed", 8)
    body = {"sdf": torch.from_numpy(sc["sdf_b"]), "density": torch.from_numpy(sc["density_b_in"]), "cano_xyz": torch.from_numpy(sc["cano_xyz"])}
    with pytest.raises(ValueError, match="GPU"):
        hf.fuse_hands(body, torch.from_numpy(sc["p"]), {}, fl, fr, cano_smpl_center=sc["centre"], density_b=0.0101)
    with pytest.raises(ValueError, match="sdf, density and cano_xyz"):
        hf.fuse_hands({"sdf": body["sdf"]}, torch.from_numpy(sc["p"]), {}, fl, fr, cano_smpl_center=sc["centre"], density_b=0.0101)
    with pytest.raises(ValueError, match="HandFields"):
        hf.fuse_hands(body, torch.from_numpy(sc["p"]), {}, fl, None, cano_smpl_center=sc["centre"], density_b=0.0101)
    with pytest.raises(ValueError, match="GPU"):
        hf.hand_meshes(torch.zeros(10, 3), [0, 1, 2], [3, 4, 5], [[0, 1, 2]])


def test_render_refuses_malformed_hands_before_anything_runs():
    import inspect
    import template_field_oracle as tfo
    from animatablegaussians_amd import template_render
    from animatablegaussians_amd.template_field import TemplateField
    assert inspect.signature(template_render.render).parameters["hands"].default is None
    field = TemplateField.from_state_dict(tfo.state_dict(tfo.make_net(tfo.NARROW, 1)), multires=2)
    for hands in ({"left": 1}, [1], {"left": 1, "right": 1, "left_field": 1, "right_field": 1, "cano_smpl_center": 1, "pose": 1}):
        with pytest.raises(ValueError, match="hands must be"):
            template_render.render(field, None, None, None, None, hands=hands)
    # the two nets and the pose are refused before the march is set up (the rays here are None: reaching it would raise something else)
    _, fl, fr, *_ = _fields()
    from animatablegaussians_amd.hand_fusion import HandField
    narrow = HandField(hfo.make_hand_net(5, multires=2, widths=(32, 64, 32), n_joints=15), multires=2)
    ok = {"left": 1, "right": 1, "cano_smpl_center": 1}
    for extra, word in ((dict(left_field=fl, right_field=None), "HandFields"), (dict(left_field=fl, right_field=narrow), "one multires"),
                        (dict(left_field=fl, right_field=fr, hand_pose=np.zeros(44)), "45 values")):
        with pytest.raises(ValueError, match=word):
            template_render.render(field, None, None, None, None, hands=dict(ok, **extra))


def test_the_device_blobs_do_not_grow_with_the_poses():
    """One blob for the zero pose and one for the last other pose per device, whatever the number of poses seen."""
    _, fl, *_ = _fields()
    cpu = torch.device("cpu")
    zero = fl._blob_on(cpu)
    assert fl._blob_on(cpu, np.zeros(45)) is zero and np.array_equal(zero.numpy(), fl.pack())
    rs = np.random.RandomState(8)
    for _ in range(5):
        pose = rs.uniform(-0.5, 0.5, 45)
        blob = fl._blob_on(cpu, pose)
        assert fl._blob_on(cpu, torch.from_numpy(pose)) is blob and np.array_equal(blob.numpy(), fl.pack(pose))
        assert fl._blob_on(cpu) is zero
    slots = list(fl._device_blobs.values())
    assert len(slots) == 1 and set(slots[0]) == {"zero", "posed"}


def test_package_exports():
    import animatablegaussians_amd as ag
    from animatablegaussians_amd import hand_fusion
    assert {"HandField", "hand_meshes", "fuse_hands", "hand_fields_from_checkpoint"} <= set(ag.__all__)
    assert ag.fuse_hands is hand_fusion.fuse_hands and ag.HandField is hand_fusion.HandField


def test_hand_fields_from_checkpoint(tmp_path):
    from animatablegaussians_amd.hand_fusion import hand_fields_from_checkpoint
    sd, fl, fr, *_ = _fields()
    path = tmp_path / "net.pt"
    torch.save({"network": sd}, path)
    a, b = hand_fields_from_checkpoint(path)
    assert np.array_equal(a.pack(), fl.pack()) and np.array_equal(b.pack(), fr.pack()) and not np.array_equal(a.pack(), b.pack())
    torch.save({"net": sd}, path)
    with pytest.raises(KeyError, match="network"):
        hand_fields_from_checkpoint(path)


# ---- the MANO topology ----------------------------------------------------------------------------------------------------------------------
def _directed_edges(f):
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def test_hand_topology_winding_and_indexing():
    """The reference's closed MANO topology (778 vertices, 1552 faces): closed and consistently wound (every directed edge once, its
    reverse once), the left hand's faces are the right hand's reversed, and the ids pick 778 distinct SMPL-X vertices per hand."""
    from animatablegaussians_amd.hand_fusion import hand_topology
    t = np.load(TOPOLOGY)
    li, ri, lf, rf = hand_topology(t["left_ids"], t["right_ids"], t["faces_closed"])
    assert lf.dtype == rf.dtype == np.int32 and lf.shape == rf.shape == (1552, 3) and li.shape == ri.shape == (778,)
    assert np.array_equal(rf, t["faces_closed"]) and np.array_equal(lf, rf[:, ::-1]) and lf.flags["C_CONTIGUOUS"]
    for f in (lf, rf):
        e = _directed_edges(f.astype(np.int64))
        keys = e[:, 0] * 778 + e[:, 1]
        assert len(np.unique(keys)) == len(keys) == 3 * 1552, "a directed edge occurs twice: the winding is not consistent"
        assert np.array_equal(np.sort(keys), np.sort(e[:, 1] * 778 + e[:, 0])), "an edge without its reverse: the mesh is not closed"
        assert 778 - len(e) // 2 + 1552 == 2, "Euler characteristic of a sphere"
        assert set(np.unique(f)) == set(range(778))
    assert len(set(li)) == len(set(ri)) == 778 and not set(li) & set(ri) and 0 <= min(li.min(), ri.min()) and max(li.max(), ri.max()) < 10475
    # mirrored vertices + reversed faces enclose the same positive volume as the originals: what the reversal is for
    v = np.random.RandomState(778).normal(size=(778, 3))
    vol = lambda v, f: (v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0  # noqa: E731
    assert np.isclose(vol(v * [-1, 1, 1], lf), vol(v, rf), rtol=1e-12)
    with pytest.raises(ValueError, match="faces_closed"):
        hand_topology(t["left_ids"][:700], t["right_ids"][:700], t["faces_closed"])
    with pytest.raises(ValueError, match="one length"):
        hand_topology(t["left_ids"], t["right_ids"][:700], t["faces_closed"])
