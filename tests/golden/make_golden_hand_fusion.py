"""Writes ``hand_fusion_ref.npz`` and ``mano_topology.npz``.

``hand_fusion_ref.npz``: the reference's own ``MLPLinear``, ``get_embedder``, ``geo_util.normalize_vert_bbox`` and ``LaplaceDensity``, run on
the host in float32 and float64 and chained the way ``TemplateNet.fuse_hands`` (``network/template.py:146-202``) and ``HandAvatar.forward``
(``network/hand_avatar.py:28-36``) chain them, for one batch element with batch axis 1, on the scene and the weights of
``tests/hand_fusion_oracle`` (``scene('mixed', 300)``, ``make_hand_net``), once with a zero ``hand_pose`` (the reference's only call site) and
once with the scene's non-zero one.  What the reference takes from pytorch3d is not run: the nearest face of every point
(``nearest_face_pytorch3d``) is a STORED INPUT, the float32 search of ``tests/mesh_query_oracle``, and ``axis_angle_to_quaternion`` is
restated here, because ``network/hand_avatar.py`` itself imports pytorch3d and cannot be imported without it.

``mano_topology.npz``: the reference's MANO topology data as it is, ``faces_closed`` (``smpl_files/mano/mano_face_close.txt``) and the two
``smpl_vert_id_to_mano`` arrays (``smplx_{l,r}hand_to_mano_rhand.npz``) as int32.

Generation time only: it needs a checkout of the reference (first argument, or ``AG_REFERENCE_DIR``).  The fixture holds the points, the
inputs and the outputs; the weights are NOT stored, they come from the recipe.

    python tests/golden/make_golden_hand_fusion.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hand_fusion_oracle as hfo  # noqa: E402

N_POINTS = 300


def quaternions(axis_angle):
    """pytorch3d.transforms.axis_angle_to_quaternion, restated."""
    angle = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    tiny = angle.abs() < 1e-6
    ratio = torch.where(tiny, 0.5 - angle * angle / 48, torch.sin(0.5 * angle) / torch.where(tiny, torch.ones_like(angle), angle))
    return torch.cat([torch.cos(0.5 * angle), axis_angle * ratio], -1)


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    import config
    config.device = torch.device("cpu")                       # LaplaceDensity moves its beta_min there
    from network.density import LaplaceDensity
    from network.mlp import MLPLinear
    from utils import geo_util
    from utils.embedder import get_embedder
    from utils.knn import knn_gather

    mano = os.path.join(ref_dir, "smpl_files", "mano")
    topo = {"faces_closed": np.loadtxt(os.path.join(mano, "mano_face_close.txt")).astype(np.int32)}
    for side, name in (("left", "smplx_lhand_to_mano_rhand.npz"), ("right", "smplx_rhand_to_mano_rhand.npz")):
        topo[side + "_ids"] = np.load(os.path.join(mano, name), allow_pickle=True)["smpl_vert_id_to_mano"].astype(np.int32)
    path = os.path.join(HERE, "mano_topology.npz")
    np.savez_compressed(path, **topo)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")

    sc = hfo.scene("mixed", N_POINTS, pose=True)
    cp = hfo.closest(sc, torch.float32)
    out = {"p": sc["p"], "cano_xyz": sc["cano_xyz"], "sdf_b": sc["sdf_b"], "color_b": sc["color_b"], "hand_pose": sc["hand_pose"]}
    for side in hfo.SIDES:
        for k in ("v", "n", "f", "cano_v"):
            out[f"{side}_{k}"] = sc["hands"][side][k]
        out[f"{side}_dist2"], out[f"{side}_face"] = cp[side]["dist2"].astype(np.float32), cp[side]["face"].astype(np.int32)
        out[f"{side}_bary"] = cp[side]["bary"].astype(np.float32)

    embedder, pos_dim = get_embedder(sc["multires"], 3)
    nets = {}
    for side in hfo.SIDES:
        nets[side] = MLPLinear(in_channels=pos_dim + 1 + 60, inter_channels=[64, 64, 64, 64, 64], out_channels=3, last_op=nn.Sigmoid())
        sd = hfo.state_dict(sc["nets"]["left"], sc["nets"]["right"])
        prefix = f"{side}_hand.tex_mlp."
        nets[side].load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    density = LaplaceDensity(params_init={"beta": hfo.DENSITY_BETA})

    for pose_name, pose_np in (("zero", np.zeros(45, np.float32)), ("posed", sc["hand_pose"])):
        for dtype, name in ((torch.float32, "32"), (torch.float64, "64")):
            density.to(dtype)
            one = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)[None]  # noqa: E731
            with torch.no_grad():
                posed, cano = one(sc["p"]), one(sc["cano_xyz"])
                pose = one(pose_np)                                                                   # [1, 45]
                hand_out = {}
                for side in hfo.SIDES:
                    nets[side].to(dtype)
                    h = sc["hands"][side]
                    faces = torch.from_numpy(h["f"].astype(np.int64))
                    face = torch.from_numpy(cp[side]["face"].astype(np.int64))[None]
                    dist = torch.sqrt(one(cp[side]["dist2"]))
                    bary = one(cp[side]["bary"])
                    corner_ids = faces[face[0]][None]                                                # [1, N, 3]
                    unit_cano = geo_util.normalize_vert_bbox(one(h["cano_v"]), dim=1, per_axis=True)
                    x = (bary[..., None] * knn_gather(unit_cano, corner_ids)).sum(2)
                    q = (bary[..., None] * knn_gather(one(h["v"]), corner_ids)).sum(2)
                    nrm = (bary[..., None] * knn_gather(one(h["n"]), corner_ids)).sum(2)
                    hand_sdf = (-torch.sign(torch.einsum("bni,bni->bn", nrm, posed - q)) * dist).unsqueeze(-1)
                    quat = quaternions(pose.reshape(1, -1, 3)).reshape(1, -1)
                    feat = torch.cat([embedder(x), hand_sdf, quat[:, None].expand(-1, x.shape[1], -1)], -1)
                    hand_out[side] = (hand_sdf, nets[side](feat))
                wl = torch.sigmoid(25 * (geo_util.normalize_vert_bbox(one(sc["hands"]["left"]["cano_v"]), attris=cano, dim=1, per_axis=True)[..., 0:1] + 0.8))
                wr = torch.sigmoid(-25 * (geo_util.normalize_vert_bbox(one(sc["hands"]["right"]["cano_v"]), attris=cano, dim=1, per_axis=True)[..., 0:1] - 0.8))
                low = cano[..., 1] < one(sc["centre"])[0, 1]
                wl[low] = 0.
                wr[low] = 0.
                total = torch.maximum(wl + wr, torch.ones_like(wl))
                wl, wr = wl / total, wr / total
                w = wl + wr
                sdf = wl * hand_out["left"][0] + wr * hand_out["right"][0] + (1.0 - w) * one(sc["sdf_b"])
                color = wl * hand_out["left"][1] + wr * hand_out["right"][1] + (1.0 - w) * one(sc["color_b"])
                dens = density(-sdf)
            out[f"{pose_name}_sdf{name}"], out[f"{pose_name}_density{name}"], out[f"{pose_name}_color{name}"] = sdf[0].numpy(), dens[0].numpy(), color[0].numpy()
    path = os.path.join(HERE, "hand_fusion_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["AG_REFERENCE_DIR"])
