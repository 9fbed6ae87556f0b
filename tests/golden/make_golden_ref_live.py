#!/usr/bin/env python
"""Golden fixtures of the reference rasterizer's CPU build (oracle/_ref, built by oracle/ref_build.py in the build container) on the two
larger scenes of tests/test_oracle_cpu.py (tests/helpers.live_scene): ``config1`` and ``long_lists``.

What the tests compare bit for bit is stored as SHA-256 digests (tests/helpers.bits_digest): every forward state and, for config1, every
gradient.  For long_lists the blend-backward gradients themselves are stored (the test holds them to the fp64 oracle within the spread of
admissible summation orders, then feeds them to the oracle's preprocess backward), and so is mark_visible.

    OMP_NUM_THREADS=1 python tests/golden/make_golden_ref_live.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import helpers as h  # noqa: E402
from oracle import ref_raster  # noqa: E402

STATE_ALL = ("radii", "tiles_touched", "point_offsets", "keys_sorted", "point_list", "ranges", "n_contrib", "color", "depth", "alpha")
STATE_VISIBLE = ("depths", "means2D", "cov3D", "conic_opacity")


def run(name):
    sc, cam = h.live_scene(name)
    r = ref_raster.RefRasterizer()
    rs = r.forward(sc["means3D"], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"], sc["bg"], cam["viewmatrix"],
                   cam["projmatrix"], cam["campos"], cam["tanfovx"], cam["tanfovy"], sc["img_w"], sc["img_h"])
    vis = rs["radii"] > 0
    out = {"num_rendered": np.array([rs["num_rendered"]], np.int64)}
    for k in STATE_ALL:
        out["st_" + k] = np.array(h.bits_digest(rs[k]))
    for k in STATE_VISIBLE:
        out["st_" + k] = np.array(h.bits_digest(rs[k][vis]))
    gr = r.backward(sc["dL_dcolor"], sc["dL_ddepth"], sc["dL_dalpha"])
    for k, v in gr.items():
        if name == "long_lists":
            out["g_" + k] = np.ascontiguousarray(v)
        else:
            out["gd_" + k] = np.array(h.bits_digest(v))
    if name == "long_lists":
        out["mark_visible"] = ref_raster.mark_visible(sc["means3D"], cam["viewmatrix"], cam["projmatrix"])
    path = os.path.join(HERE, f"ref_live_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: R={rs['num_rendered']} visible={int(vis.sum())} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    assert ref_raster.available(), "build oracle/_ref first: python oracle/ref_build.py"
    for n in ("config1", "long_lists"):
        run(n)
