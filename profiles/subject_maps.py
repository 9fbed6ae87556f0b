"""Time ``subject_maps.canonical_maps`` for ``synth.body_mesh()`` at S = 1024 and, beside it, the host k-d tree it replaces.

Wall time (host clock around a device synchronise, warmed up):      python profiles/subject_maps.py
Per-kernel times (a run of its own; the kernels are mesh_depth_kernel, mesh_resolve_ids_kernel, resolve_attribute_kernel and
knn_{count,tile_sums,scan_sums,tile_scan,scatter,search}_kernel):
    rocprofv3 --kernel-trace --stats -d <out> -- python profiles/subject_maps.py --once
Prints one JSON line; algorithmic bytes per kernel are computed from the shapes (DESIGN.md section 4 states the bounds)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import subject_maps as sm, synth  # noqa: E402
from animatablegaussians_amd.avatar import _knn3_log_scale  # noqa: E402


def main():
    once = "--once" in sys.argv
    S = 1024
    m = synth.body_mesh()
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    v, f, w = t(m["vertices"]), t(m["faces"]), t(m["lbs_weights"])
    n = sm.vertex_normals(v, f)
    maps = sm.canonical_maps(v, f, n, w, size=S)
    torch.cuda.synchronize()
    N, J, F = maps["init_pts_lbs"].shape[0], w.shape[1], f.shape[0]
    out = {"S": S, "faces": F, "N": N}
    if not once:
        pts = maps["cano_smpl_pos_map"][maps["mask"]]
        times = {}
        for name, fn in (("canonical_maps", lambda: sm.canonical_maps(v, f, n, w, size=S)), ("knn_log_scale", lambda: sm.knn_log_scale(pts)),
                         ("rasterize_both_views", lambda: [sm.rasterize_ortho(v, f, m_, S) for m_ in sm.view_matrices((0, 0, 0))])):
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            times[name + "_ms"] = [round(x, 3) for x in sorted(ts)]
        host = pts.cpu().numpy()
        t0 = time.perf_counter()
        _knn3_log_scale(host)
        times["host_kd_tree_log_scale_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out.update(times)
    # algorithmic bytes (what each kernel must move at least once)
    px = 2 * S * S
    out["bytes"] = {"mesh_depth_kernel": F * 2 * (12 + 36) + 8 * N, "mesh_resolve_ids_kernel": px * (8 + 4 + 12) + N * 48,
                    "resolve_attribute_dense_C3": px * (4 + 12 + 12) + N * 36, "resolve_attribute_lbs": N * (4 + 4 + 12 + 4 * J),
                    "knn_search_kernel": N * (16 + 4 + 12) + N * 27 * 8}
    cells = sm.knn_grid(maps["cano_smpl_pos_map"][maps["mask"]])[2].prod()
    out["knn_cells"] = int(cells)
    out["bytes"].update({"knn_count_kernel": N * 12, "knn_scatter_kernel": N * (12 + 16), "knn_tile_sums_kernel": int(cells) * 4,
                         "knn_tile_scan_kernel": int(cells) * 12})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
