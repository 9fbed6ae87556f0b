#!/usr/bin/env python
"""Writes tests/golden/inverse_skinning_ref.npz: what the REFERENCE's own code computes on the inputs of
``tests/inverse_skinning_oracle.py`` -- its ``compute_gradient_volume`` (``network/volume.py``, run on the CPU) and its root-finding kernel
(``utils/root_finding/root_finding.cu``), compiled for the host.  Needs the reference checkout; the tests need only the file.

The kernel is built in a temporary directory and nowhere else: the source is read where it lies, its one launch is rewritten by
``oracle/ref_build.rewrite`` (chevrons -> ``cuemu::launch``), and it is compiled with g++ -ffp-contract=off against ``oracle/cuda_cpu/`` and
four stub headers of a few lines each, written below (the rewritten translation unit must lie beside the stub ``utils.h`` for its
``#include "utils.h"`` to find it).  Only inputs and outputs are recorded, for B = 1:

* ``small_*``: the (9, 7, 5, 6) volume, initial guesses off by up to 2 cm; the whole gradient volume;
* ``big_*``: the (16, 16, 16, 55) volume, initial guesses off by up to 2 cm and (``big5_*``) 5 cm; the gradient at GRAD_NODES nodes (the
  eight corners, edge and face nodes among them): the whole [16, 16, 16, 55, 3] array alone would be 2.7 MB.

    python tests/golden/make_golden_inverse_skinning.py <reference checkout>      (or AG_REFERENCE_DIR)
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import inverse_skinning_oracle as iso  # noqa: E402
from oracle import ref_build  # noqa: E402

GRAD_NODES = 160

STUBS = {
    "ATen/ATen.h": """#pragma once
namespace at { struct Tensor { void* p; long long dims[8];
  long long size(int i) const { return dims[i]; }
  template <class T> T* data() const { return static_cast<T*>(p); } }; }
""",
    "thrust/tuple.h": "#pragma once\n",
    "vector_functions.h": """#pragma once
#include <cuda_runtime.h>
struct int3 { int x, y, z; };
inline float3 make_float3(float x, float y, float z) { float3 v; v.x = x; v.y = y; v.z = z; return v; }
inline float4 make_float4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
inline int3 make_int3(int x, int y, int z) { int3 v; v.x = x; v.y = y; v.z = z; return v; }
""",
    "utils.h": """#pragma once
#define CHECK_CONTIGUOUS_CUDA(x)
#define CHECK_IS_FLOAT(x)
#define CHECK_IS_INT(x)
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
""",
}

DRIVER = """
extern "C" void golden_root_finding(float* volume, float* grad, float* xt, float* xc_init, float* jnt_mats, float* bounds, int* res, float* xc_opt,
                                    int B, int N, int J, float lambda, int iterations)
{
    at::Tensor v{volume, {res[0], res[1], res[2], J}}, g{grad, {res[0], res[1], res[2], 3 * J}}, t{xt, {B, N, 3}}, c{xc_init, {B, N, 3}};
    at::Tensor m{jnt_mats, {B, J, 4, 4}}, b{bounds, {2, 3}}, r{res, {3}}, o{xc_opt, {B, N, 3}};
    root_finding(v, g, t, c, m, b, r, o, lambda, iterations);
}
"""


def build_reference_kernel(ref, tmp):
    src = os.path.join(ref, "utils", "root_finding")
    with open(os.path.join(src, "root_finding.cu")) as fh:
        text, n = ref_build.rewrite(fh.read())
    assert n == 1, f"expected one kernel launch in root_finding.cu, rewrote {n}"
    for name, body in STUBS.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, name)), exist_ok=True)
        with open(os.path.join(tmp, name), "w") as fh:
            fh.write(body)
    unit = os.path.join(tmp, "root_finding_cpu.cpp")
    with open(unit, "w") as fh:
        fh.write(text + DRIVER)
    lib = os.path.join(tmp, "libgolden_root_finding.so")
    cuda_cpu = os.path.join(ROOT, "oracle", "cuda_cpu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", "-I", tmp, "-I", cuda_cpu,
                           "-I", src, "-o", lib, unit, os.path.join(cuda_cpu, "cuemu.cpp")])
    return ctypes.CDLL(lib)


def reference_gradient(ref, volume, spacing):
    """[X, Y, Z, J, 3] float32 from the reference's compute_gradient_volume ([J, 3, X, Y, Z]) on the CPU."""
    import torch
    sys.path.insert(0, ref)
    import config
    config.device = torch.device("cpu")
    from network.volume import compute_gradient_volume
    with torch.no_grad():
        g = compute_gradient_volume(torch.from_numpy(volume).permute(3, 0, 1, 2).contiguous(), torch.from_numpy(spacing))
    return g.permute(2, 3, 4, 0, 1).contiguous().numpy()


def reference_root_find(lib, case, grad, lam=0.1, iterations=10):
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    vol, g, xt, xc, mats, bounds = (f(case[k]) if isinstance(k, str) else f(k) for k in ("volume", grad, "xt", "xc_init", "jnt_mats", "bounds"))
    res = np.ascontiguousarray(vol.shape[:3], np.int32)
    out = np.full_like(xc, np.nan)
    B, N, _ = xc.shape
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.golden_root_finding.restype = None
    lib.golden_root_finding.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int]
    lib.golden_root_finding(ptr(vol), ptr(g), ptr(xt), ptr(xc), ptr(mats), ptr(bounds), ptr(res), ptr(out), B, N, vol.shape[3], lam, iterations)
    assert np.isfinite(out).all()
    return out


def gradient_nodes(shape, n, seed=11):
    """[n, 3] node indices: the eight corners, then random nodes of which half are pushed onto a face, an edge or a corner."""
    rng = np.random.RandomState(seed)
    res = np.array(shape[:3])
    corners = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]) * (res - 1)
    nodes = np.stack([rng.randint(0, r, n - 8) for r in res], -1)
    push = rng.randint(0, 4, nodes.shape)                      # 0: to the low face, 1: to the high face, else stay
    nodes = np.where(push == 0, 0, np.where(push == 1, res - 1, nodes))
    nodes[n // 2:] = np.stack([rng.randint(0, r, n - 8 - n // 2) for r in res], -1)
    return np.concatenate([corners, nodes], 0).astype(np.int32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AG_REFERENCE_DIR")
    if not ref or not os.path.isdir(os.path.join(ref, "utils", "root_finding")):
        sys.exit("usage: make_golden_inverse_skinning.py <reference checkout>")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference_kernel(ref, tmp)
        for tag, shape, offset in (("small", iso.SHAPES[0], 0.02), ("big", iso.SHAPES[1], 0.02), ("big5", iso.SHAPES[1], 0.05)):
            case = iso.smooth_case(shape, offset=offset)
            grad = reference_gradient(ref, case["volume"], case["spacing"])
            xc = reference_root_find(lib, case, grad.reshape(shape[:3] + (3 * shape[3],)))
            worst = float(np.abs(xc - case["x_true"]).max())
            print(f"{tag}: {shape}, offset {offset}: reference ends {worst:.3e} from the constructed root at worst")
            if tag == "big5":
                assert np.array_equal(case["volume"], out["big_volume"]) and np.array_equal(case["xt"], out["big_xt"])
                out["big5_xc_init"], out["big5_ref_xc"] = case["xc_init"], xc
                continue
            for k in ("volume", "bounds", "spacing", "jnt_mats", "xt", "xc_init"):
                out[f"{tag}_{k}"] = case[k]
            out[f"{tag}_ref_xc"] = xc
            if tag == "small":
                out["small_ref_grad"] = grad
            else:
                nodes = gradient_nodes(shape, GRAD_NODES)
                out["big_grad_nodes"] = nodes
                out["big_ref_grad"] = grad[nodes[:, 0], nodes[:, 1], nodes[:, 2]]
    path = os.path.join(HERE, "inverse_skinning_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
