"""Host-side checks of the pose-gradient surface (no GPU): the additive C ABI and its Python bindings."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ag_lbs_backward_joints", "ag_lbs_backward_joints_workspace_bytes", "ag_smplx_backward", "ag_mat4_mul_inverse_backward")


def test_backward_entry_points_are_declared_bound_and_exported():
    import ctypes
    from animatablegaussians_amd import _lib
    hdr = ""
    for name in ("ag_avatar.h", "ag_smplx.h"):
        hdr += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(ag_[a-z0-9_]+)\s*\(", hdr))
    bound = {s[0] for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in bound and hasattr(L, name), name
    assert "ag_lbs_backward" in declared                # the plain backward stays
    L.ag_abi_version.restype = ctypes.c_int
    assert L.ag_abi_version() == 1


def test_joint_gradient_workspace_is_one_slab_per_workgroup():
    import ctypes
    from animatablegaussians_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    f = L.ag_lbs_backward_joints_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]
    assert f(268348, 55) == 1049 * 55 * 12 * 4
    assert f(256, 24) == 24 * 12 * 4 and f(257, 24) == 2 * 24 * 12 * 4 and f(0, 55) == 0


def test_backward_without_a_gpu_tensor_is_refused():
    """The autograd entry points validate their inputs on the host before any launch."""
    import pytest
    import torch
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    with pytest.raises(RuntimeError, match="float32 GPU tensors"):
        mat4_mul_inverse(torch.eye(4)[None].requires_grad_(True), torch.eye(4)[None])
