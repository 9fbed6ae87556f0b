"""bench.py's one-line JSON contract (driver-facing): keys, types, the roofline and cpu_baseline objects, and that the reported
HIP-event duration of the dominant kernel is consistent with the step time.  Short run (the driver's defaults are 2000 / 200)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
# the legs beyond the headline (rooflines, full_step, stress, CPU baselines, the N > 1 exchange records) run under --full only
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "20", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict),
                 ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 60 and d["warmup"] == 20 and d["scaling"] == "weak"
    assert d["unit"] == "views/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] * d["ms_per_step"] - 1000.0) < 5.0                       # value = steps / elapsed at N = 1
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["launches_timed"] == 60
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and 0.01 < r["frac"] < 1.0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 0.02 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] > 0.5 * r["algorithmic_bytes_per_launch"]
    assert 20.0 < r["avg_launch_us"] < 1000.0 * d["ms_per_step"] * 2               # the kernel fits into (two overlapped) steps
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "views/s" and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    assert d["value"] > 100 * c["value"]
    # the dependent-step rate on one stream is reported next to the pipelined headline and cannot beat it by much
    assert d["sequential"]["views_per_s"] > 0 and d["sequential"]["views_per_s"] < 1.2 * d["value"]
    # ... and so is the reference's operator path (GaussianRasterizer + public torch.autograd.backward): same kernels, more host time
    assert 0 < d["operator_path"]["views_per_s"] < 1.2 * d["value"] and "library-owned step" in d["config"]["workload"]
    # BASELINE configs[2] (whole training iteration) and the MFMA roofline of the convolutions, measured in the same process
    f = d["full_step"]
    assert abs(f["views_per_s_1view_per_step"] * f["ms_per_step_1view"] - 1000.0) < 5.0
    assert abs(f["views_per_s_4views_per_step"] * f["ms_per_step_4views"] - 4000.0) < 20.0
    assert f["views_per_s_4views_per_step"] > f["views_per_s_1view_per_step"] > 1.0 and f["parameters"] > 2.2e8
    # the other two arithmetic modes are measured beside the default (interleaved blocks of a few steps each: the comparison is a sanity
    # band, not a ranking -- a single slow block moves a median by 10 %)
    assert f["conv_math"] == "split_f16" and f["conv_math_fp32"]["views_per_s_1view_per_step"] < f["views_per_s_1view_per_step"] * 1.2
    assert f["conv_math_split_bf16"]["views_per_s_1view_per_step"] < f["views_per_s_1view_per_step"] * 1.1        # the six-product form (default before round 4)
    assert f["conv_math_split_bf16x3_opt_in_not_fp32_grade"]["views_per_s_1view_per_step"] > f["views_per_s_1view_per_step"] * 0.7
    for k in ("conv_math_fp32", "conv_math_split_bf16", "conv_math_split_bf16x3_opt_in_not_fp32_grade"):
        assert abs(f[k]["views_per_s_1view_per_step"] * f[k]["ms_per_step_1view"] - 1000.0) < 5.0
    m = d["roofline_mfma"]
    # the product's arithmetic: three fp16 products per fp32 product, priced (executed = 3 x algorithmic) against the dense 16-bit MFMA peak
    assert m["bound"] == "mfma" and m["unit"] == "TFLOP/s" and m["math"] == "split_f16" and m["peak"] == 2500.0
    assert abs(m["executed"] - 3 * m["achieved"]) < 0.5 and abs(m["frac"] - m["executed"] / m["peak"]) < 1e-3 and 0.05 < m["frac"] < 1.0
    assert abs(m["frac_of_fp32_mfma_peak"] - m["achieved"] / 157.3) < 1e-3
    for k in ("gather_conv_kernel", "wgrad_kernel"):
        assert m[k]["launches_timed"] > 0 and 1.0 < m[k]["TFLOPs"] < 2500.0 / 3
    # ... and the fp32-MFMA mode beside it, against its own peak
    q = m["fp32_mfma_mode"]
    assert q["peak"] == 157.3 and abs(q["frac"] - q["achieved"] / q["peak"]) < 1e-3 and 0.05 < q["frac"] < 1.0
    assert q["whole_network_frac"] <= q["frac"] + 0.05 and q["achieved"] < 1.1 * m["achieved"]
    for k in ("gather_conv_kernel", "wgrad_kernel"):
        assert q[k]["launches_timed"] > 0 and 1.0 < q[k]["TFLOPs"] < 157.3
    # every convolution FLOP of the three networks' forward + backward is accounted for: 3 x 586 GFLOP x 3 (forward, input gradient,
    # weight gradient); the pose map needs no gradient and the grouped chain runs the branch-independent parts of the comb convolutions
    # (the whole first one, the encoder-level half of the others) once per network instead of once per branch: 11 % less than 9 x 586
    total = m["gather_conv_kernel"]["GFLOP_per_pass_of_the_three_networks"] + m["wgrad_kernel"]["GFLOP_per_pass_of_the_three_networks"]
    assert 0.85 * 9 * 585.8 < total < 1.01 * 9 * 585.8, total          # 4700 of 5272 GFLOP: the comb convolutions' level halves run once per network
    # the per-Gaussian assembly / skinning kernels against HBM (north_star's third hand-written stage)
    a = d["roofline_avatar_kernels"]
    for k in ("gather_forward", "gather_backward", "lbs_forward", "lbs_backward"):
        assert a[k]["bound"] == "hbm" and a[k]["peak"] == 8000.0 and 1.0 < a[k]["avg_launch_us"] < 500.0
        assert abs(a[k]["achieved"] - a[k]["algorithmic_bytes_per_launch"] / (a[k]["avg_launch_us"] * 1e-6) / 1e9) < 0.02 * a[k]["achieved"]
        assert abs(a[k]["frac"] - a[k]["achieved"] / 8000.0) < 1e-3 and 0.01 < a[k]["frac"] < 1.0
    # the short-region stability evidence, BASELINE configs[3] at N = 1 and the step with the reference's whole loss
    vb = d["value_blocks"]["views_per_s"]
    assert len(vb) == 5 and all(v > 0 for v in vb)
    assert "extra_legs_error" not in f, f.get("extra_legs_error")
    v16 = f["views16_one_pose_configs3_n1"]
    assert abs(v16["views_per_s"] * v16["ms_per_step"] - 16000.0) < 100.0 and v16["views_per_s"] > f["views_per_s_4views_per_step"] * 0.8
    inf = f["inference_1view"]
    assert inf["views_per_s"] > 2 * f["views_per_s_1view_per_step"] and inf["views_per_s_hip_graphs"] > 0.8 * inf["views_per_s"]
    lp = f["with_the_references_full_loss"]
    assert 1.0 < lp["views_per_s_1view_per_step"] <= f["views_per_s_1view_per_step"] * 1.1


HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                 "data", "config", "headline"}


def test_plain_bench_line_is_the_headline_alone(tmp_path):
    """Without --full the run sets up, warms up, times its steps, writes --dump-outputs and prints the line: the headline fields with the
    same meaning as under --full, and none of the other legs."""
    dump = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "20", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert set(d) == HEADLINE_KEYS | {"dumped_outputs"}, sorted(d)
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["metric"] == "rendered views/sec (fwd+bwd) @1024^2, ~250k Gaussians" and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 60 and d["warmup"] == 20 and d["scaling"] == "weak"
    assert d["unit"] == "views/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and "library-owned step" in d["config"]["workload"]
    assert abs(d["value"] * d["ms_per_step"] - 1000.0) < 5.0                       # value = steps / elapsed at N = 1
    assert d["headline"] == {"value_views_per_s": d["value"], "n_gpus": 1}
    du = d["dumped_outputs"]
    assert du["view"] == (20 + 60 - 1) % d["config"]["views"] and du["dtype"] == "float32"
    assert sorted(os.listdir(dump)) == sorted(f"{k}.npy" for k in du["arrays"]) and len(du["arrays"]) == 10


def test_bench_breakdown_needs_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--breakdown"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--full" in p.stderr, p.stderr[-2000:]


def test_bench_dump_outputs_are_the_last_steps_own(tmp_path):
    """--dump-outputs writes what the LAST timed step computed: one view's images, radii and per-Gaussian gradients, float32, within 64 MB.
    20 + 62 - 1 = 81 puts that step on stream slot 0 of three, the slot whose gradient buffers FusedRasterStep.join() sums the other
    slots into at the end of the timed region; the dump must hold the view's own gradients all the same.  Checked against a fresh
    one-view FusedRasterStep.view() of the same view and inputs: images and radii to 1e-6, gradients to 1e-4 of their largest magnitude
    (float-atomic sums in another order; the sum over three views would be off by its own magnitude)."""
    import numpy as np
    import torch

    from animatablegaussians_amd import camera, synth
    from animatablegaussians_amd.rasterizer import FusedRasterStep, GaussianRasterizationSettings
    dump, warmup, steps = tmp_path / "outputs", 20, 62
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--full", "--no-full-step", "--no-stress", "--no-cpu-baseline", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["roofline"]["launches_timed"] == steps and d["config"]["streams"] == 3
    assert (warmup + steps - 1) % d["config"]["streams"] == 0                     # the last step ran on slot 0
    du = d["dumped_outputs"]
    view = (warmup + steps - 1) % d["config"]["views"]
    P, side = d["config"]["gaussians"], 1024
    want = {"color": [3, side, side], "depth": [1, side, side], "alpha": [1, side, side], "radii": [P], "dL_dmeans2D": [P, 3],
            "dL_dmeans3D": [P, 3], "dL_dscales": [P, 3], "dL_drotations": [P, 4], "dL_dopacity": [P, 1], "dL_dcolors": [P, 3]}
    assert du["view"] == view and du["arrays"] == want and du["bytes"] <= 64 << 20
    assert sorted(os.listdir(dump)) == sorted(f"{k}.npy" for k in want)
    a = {k: np.load(dump / f"{k}.npy") for k in want}
    for k, v in a.items():
        assert v.dtype == np.float32 and list(v.shape) == want[k] and np.isfinite(v).all(), k

    # the same view through a fresh one-slot step, with bench.py's seeded inputs
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    av = synth.avatar_map_gaussians()
    c = synth.free_view_cameras(8, img=side)[view]
    cm = camera.camera_from_intr_extr(c["extr"], c["intr"], side, side)
    rs = GaussianRasterizationSettings(image_height=side, image_width=side, tanfovx=cm["tanfovx"], tanfovy=cm["tanfovy"], bg=t(av["bg"]),
                                       scale_modifier=1.0, viewmatrix=t(cm["viewmatrix"]), projmatrix=t(cm["projmatrix"]), sh_degree=0,
                                       campos=t(cm["campos"]), prefiltered=False, debug=False)
    up = synth.upstream_grads(side, side, 12345)
    one = FusedRasterStep(P, side, side, dev, n_streams=1)
    color, depth, alpha, radii, g = one.view(rs, t(av["means3D"]), t(av["colors"]), t(av["opacities"]), t(av["scales"]), t(av["rotations"]),
                                             t(up["dL_dcolor"]), t(up["dL_ddepth"]), t(up["dL_dalpha"]))
    torch.cuda.synchronize(dev)
    ref = {"color": color, "depth": depth, "alpha": alpha, "radii": radii, **{k: g[k] for k in want if k.startswith("dL_")}}
    ref = {k: v.float().cpu().numpy().reshape(want[k]) for k, v in ref.items()}
    assert (ref["radii"] > 0).any() and np.abs(ref["color"]).max() > 0
    for k in ("color", "depth", "alpha", "radii"):
        np.testing.assert_allclose(a[k], ref[k], rtol=0, atol=1e-6, err_msg=k)
    for k in want:
        if k.startswith("dL_"):
            m = float(np.abs(ref[k]).max())
            assert m > 0 and float(np.abs(a[k].astype(np.float64) - ref[k]).max()) <= 1e-4 * m, k


def test_bench_two_ranks_control_flow_on_one_gpu():
    """The N > 1 launch exactly as the driver issues it (python -m torch.distributed.run, one rank per process), with the gloo
    transport so that both ranks can share this box's single GPU: a functional check of the sharded path, the max-over-ranks timing
    and the extra exchange record -- never a measurement."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    # no AG_DIST_BACKEND: with fewer GPUs than ranks the launch must pick the shared-device gloo run by itself (and say so), not hang in RCCL
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("AG_DIST_BACKEND", None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "30", "--warmup", "10",
                        "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 30 and d["scaling"] == "weak" and "view-sharded x2" in d["config"]["parallelism"]
    assert abs(d["value"] * d["ms_per_step"] - 2000.0) < 20.0                      # whole-job aggregate: 2 ranks x steps / time
    assert "cpu_baseline" not in d and "full_step" not in d and "stress_1m_2048" not in d      # N = 1 only
    import torch
    if torch.cuda.device_count() < 2:
        assert d["config"]["backend"].startswith("gloo") and "NOT a measurement" in d["config"]["backend"]
    x = d["exchange_styleunet"]
    assert x["bytes"] == 4 * 223648936 and x["ms"] > 0 and x["bus_GBps"] > 0
    # the per-Gaussian gradient exchange of the headline loop (round 5: packed on the view's stream, summed over the rank's views on the
    # communication stream, one all-reduce per 16 // N steps under the next views' kernels): one untimed iteration checked by linearity
    assert d["config"]["exchange_every_steps"] == 8
    c = d["exchange_check"]
    assert c["ok"] is True and c["views_per_rank_checked"] == 8 and c["sum_of_magnitudes"] > 0, c


def test_training_replicas_stay_identical_over_two_adam_steps_two_ranks_one_gpu():
    """`bench_avatar.py --gpus 2` as the driver would launch it, ranks sharing this box's GPU over gloo: two full training iterations
    (view-sharded render, six-stream backward, bucketed all-reduce on the communication stream, fused Adam); afterwards every rank must
    hold bit-identical parameters -- the property data parallelism rests on.  Functional only; no RCCL execution exists on this pool."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench_avatar.py"), "--gpus", "2", "--steps", "2", "--warmup", "0"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["replicas_identical_after_run"] is True, d["config"]


def test_pose_per_rank_mode_keeps_replicas_identical_two_ranks_one_gpu():
    """DESIGN.md section 6 mode (b), `bench_avatar.py --gpus 2 --pose-per-rank --views 2`: every rank renders two cameras of ITS OWN pose (different joint
    transforms per rank, so different pose maps, Gaussians and gradients), the bucketed exchange averages the gradients, fused Adam steps: after two
    iterations both ranks hold bit-identical parameters, and the line says which scaling mode it reports.  Functional only (ranks share this GPU over gloo)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench_avatar.py"), "--gpus", "2", "--steps", "2", "--warmup", "0", "--views", "2",
                        "--pose-per-rank"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["views_per_step"] == 2
    assert d["config"]["replicas_identical_after_run"] is True, d["config"]
    assert d["config"]["scaling_mode"].startswith("(b)") and "one pose per rank x2" in d["config"]["parallelism"]
    assert abs(d["value"] * d["ms_per_step"] - 2 * 2 * 1000.0) < 40.0          # whole-job aggregate: 2 ranks x 2 views per step
