"""The SMPL-X chain backward (csrc/ag_smplx.hip: smplx_chain_backward_kernel<false> and <true>, fed by ag_smplx_vertex_backward) off the
standard skeleton: the eight models of smplx_forward_oracle.GRID_SMALL -- J = 1, 2, 24, 40, 55, 64 on a chain, a star, the SMPL-X tree and
a random tree, NB = 0, 1, 20, 300, 401 (the `l += 64` loop of dcomps runs 0, 1 and 7 times) -- through the C interface, against torch
autograd in float64 and float32 through `forward_generic(..., differentiable=True)`.

Per row, with dL_dtransl asked for (and a transl in the forward) and without:
  ag_smplx_backward        seeded dL_dA and dL_djoints                                          -> dpose, dcomps, dtransl
  ag_smplx_forward_keep -> ag_smplx_vertex_backward -> ag_smplx_backward_full, seeded dL_dvertices added  -> the same three
Bar: `smplx_forward_oracle.bar`, the rule of test_pose_grad_gpu._bar (4 x the float32 oracle's own deviation from float64 + 2e-6 of the
float64 gradient's scale, max and L2 norm); tests/test_smplx_forward_edges_cpu.py shows the deviation is non-zero on every row.  Every
output lies in a guarded buffer (all of it written, nothing behind it), two calls give the same bits, a NULL dL_dtransl changes no bit of
the other two outputs, and ag_smplx_backward_full with nothing handed over is ag_smplx_backward.

Measured on the MI355X, the worst of the 69 comparisons per output as GPU error / float32 oracle's deviation / limit (max norm):
  dpose    1.67e-3 / 1.67e-3 / 6.7e-3   (0.25 of the limit; V = 97, J = 64, NB = 401, random tree, B = 7, chain loss)
  dcomps   4.1e-8 / 2.5e-8 / 2.6e-7     (0.16; V = 31, J = 24, NB = 20, SMPL-X tree, B = 2)
  dtransl  6.7e-6 / 1.2e-6 / 5.7e-5     (0.12; V = 95, J = 64, 63-deep chain, B = 3)
Every bit comparison holds.  Wall time of the file: 2.8 s, 0.3 s for the slowest row.
"""
import ctypes

import pytest

import smplx_forward_oracle as fo
from test_smplx_forward_edges_gpu import SENTINEL, _CModel, _guarded, _p, _untouched, _written

pytestmark = pytest.mark.gpu


def _chain_backward(cm, B, comps, pose, gA, gJ, want_tr, ext=None):
    """ag_smplx_backward, or ag_smplx_backward_full when `ext` = (dAs, dfeat, dtr_add, dcomps_add) is given -> (dpose, dcomps, dtransl)."""
    J, NB = cm.J, cm.NB
    dpose, dcomps, dtr = _guarded(3 * B * J), _guarded(B * NB), _guarded(3 * B)
    head = [ctypes.byref(cm.m), B, _p(comps), _p(pose), _p(gA), _p(gJ)]
    tail = [_p(dpose), _p(dtr) if want_tr else None, _p(dcomps) if NB > 0 else None, cm.stream]
    if ext is None:
        rc = cm.L.ag_smplx_backward(*head, *tail)
    else:
        rc = cm.L.ag_smplx_backward_full(*head, *[_p(t) for t in ext], *tail)
    assert rc == 0, cm.L.ag_last_error().decode()
    if not want_tr:
        _untouched(dtr, 3 * B, "dtransl (not asked for)")
    return (_written(dpose, 3 * B * J, "dpose").view(B, J, 3), _written(dcomps, B * NB, "dcomps").view(B, NB),
            _written(dtr, 3 * B, "dtransl").view(B, 3) if want_tr else None)


def _vertex_backward(cm, B, saved, gV):
    """ag_smplx_vertex_backward -> (dAs, dfeat or None, dtr_add, dcomps_add or None), as smplx.py hands them to ag_smplx_backward_full."""
    V, J, NB = cm.V, cm.J, cm.NB
    P = 9 * (J - 1)
    nws = int(cm.L.ag_smplx_vertex_backward_workspace_floats(ctypes.byref(cm.m), B))
    dAs, dfeat, dtr, dcomps, ws = _guarded(12 * B * J), _guarded(B * P), _guarded(3 * B), _guarded(B * NB), _guarded(nws)
    rc = cm.L.ag_smplx_vertex_backward(ctypes.byref(cm.m), B, _p(saved), _p(gV), _p(dAs), _p(dfeat) if P > 0 else None, _p(dtr),
                                       _p(dcomps) if NB > 0 else None, _p(ws), nws, cm.stream)
    assert rc == 0, cm.L.ag_last_error().decode()
    assert bool((ws[nws:] == SENTINEL).all()),"ag_smplx_vertex_backward wrote behind its workspace"
    return (_written(dAs, 12 * B * J, "dAs"), _written(dfeat, B * P, "dfeat") if P > 0 else None, _written(dtr, 3 * B, "dtr_add"),
            _written(dcomps, B * NB, "dcomps_add") if NB > 0 else None)


@pytest.mark.parametrize("row", fo.GRID_SMALL, ids=lambda c: "-".join(str(x) for x in c))
def test_chain_backward_on_the_small_models(row):
    import torch
    V, J, NB, tree, B = row
    c = fo.small_case(*row)
    cm = _CModel(c['arrays'])
    comps, pose = c['comps'].cuda().contiguous(), c['pose'].cuda().contiguous()
    for with_transl in (True, False):
        ref = fo.small_case_gradients(*row, with_transl)
        tag = f"V={V} J={J} NB={NB} {tree} B={B} transl={with_transl}"
        gA, gJ, gV = ref['wA'].cuda().contiguous(), ref['wJ'].cuda().contiguous(), ref['wV'].cuda().contiguous()
        transl = ref['transl'].cuda().contiguous() if with_transl else None

        def check(loss, got, again):
            for name, a, b in zip(("pose", "comps", "transl"), got, again):
                if name == "transl" and not with_transl:
                    continue
                assert torch.equal(a, b), f"{tag} {loss}: d{name} of two calls differs in its bits"
                if name == "comps" and NB == 0:
                    continue
                fo.bar(a, ref[loss]['64'][name].reshape(a.shape), ref[loss]['32'][name].reshape(a.shape), f"{tag} {loss}: d{name}")

        chain = _chain_backward(cm, B, comps, pose, gA, gJ, with_transl)
        check("chain", chain, _chain_backward(cm, B, comps, pose, gA, gJ, with_transl))
        nothing = _chain_backward(cm, B, comps, pose, gA, gJ, with_transl, ext=(None, None, None, None))
        for name, a, b in zip(("pose", "comps", "transl"), chain, nothing):
            assert (a is None and b is None) or torch.equal(a, b),f"{tag}: d{name} of ag_smplx_backward_full with nothing handed over differs from ag_smplx_backward"

        o = cm.outputs(B)
        assert cm.forward(B, comps, pose, transl, o, keep=True) == 0, cm.L.ag_last_error().decode()
        saved = _written(o['saved'], cm.sizes(B)[1], "saved")
        ext = _vertex_backward(cm, B, saved, gV)
        for a, b in zip(ext, _vertex_backward(cm, B, saved, gV)):
            assert (a is None and b is None) or torch.equal(a, b), f"{tag}: two calls of ag_smplx_vertex_backward differ in their bits"
        full = _chain_backward(cm, B, comps, pose, gA, gJ, with_transl, ext=ext)
        check("full", full, _chain_backward(cm, B, comps, pose, gA, gJ, with_transl, ext=ext))
        if with_transl:
            with_tr = {"chain": chain, "full": full}
        else:       # dL_dtransl = NULL takes nothing from the other two; `saved` does not depend on transl (it holds the un-translated A)
            for loss, got in (("chain", chain), ("full", full)):
                for name, a, b in zip(("pose", "comps"), got, with_tr[loss]):
                    assert torch.equal(a, b), f"{tag} {loss}: d{name} changes with dL_dtransl = NULL"
