"""Every case of tests/avatar_kernels_oracle.py reaches what its comment claims: the record of WHY tests/test_avatar_kernels_edges_gpu.py runs those shapes.
Conditions on the inputs, counted on the float64 oracle.  Needs no GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avatar_kernels_oracle as ako  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_gather_masks_hold_the_seam_the_corners_and_the_workgroup_tails():
    counts = {name: ako.gather_case(name)["N"] for name in ako.GATHER_CASES}
    assert counts["s8_full"] == 128 and counts["s16_n1_first"] == 1 and counts["s16_n1_last"] == 1
    assert [counts[f"s16_n{n}"] for n in (255, 256, 257)] == [255, 256, 257]          # below, at and one past the 256 threads of a workgroup
    for name, N in counts.items():
        d = ako.gather_case(name)
        S, mask = d["S"], d["mask"]
        assert tuple(mask.shape) == (S, 2 * S) and N == int(mask.sum())
        if N == 1:
            continue
        # u = S-1 (last front column) and u = S (first back column) on one row, pixel 0 and the last canvas pixel (S-1, 2S-1)
        assert bool((mask[:, S - 1] & mask[:, S]).any()), f"{name}: no row crosses the front|back seam"
        assert bool(mask[0, 0]) and bool(mask[S - 1, 2 * S - 1]), f"{name}: a corner pixel is missing"
    assert bool(ako.gather_case("s16_n1_first")["mask"][0, 0]) and bool(ako.gather_case("s16_n1_last")["mask"][15, 31])
    assert bool(ako.gather_case("s8_full")["mask"].all())


def test_zero_quaternion_rows_sum_to_exactly_zero_in_fp32():
    d = ako.gather_case("zero_quat")
    z = d["zero_rows"]
    assert int(z.sum()) >= 100 and int((~z).sum()) >= 100
    for dtype in (ako.F32, ako.F64):
        q = ako.gather_logits(d, dtype)[2]
        assert bool((q[z] == 0).all()), "a zero-quaternion row does not sum to exactly 0"
        assert float(q[~z].norm(dim=1).min()) > 0.1                                   # the other rows are far off the eps branch
    # what the references do there, in both types: output 0, gradient g * 1e12 (F.normalize divides by max(|x|, 1e-12))
    mask, g = d["mask"], d["ups"][3]
    for (outs, grads), rel in zip(ako.gather_reference("zero_quat"), (1e-12, 1e-6)):
        assert bool((outs[3][z] == 0).all())
        rows = ako.canvas_rows(grads[1], 8, mask)[0][:, 4:8]
        assert float((rows[z].double() - g[z].double() * 1e12).abs().max()) <= rel * 1e12 * float(g[z].abs().max())


@pytest.mark.parametrize("kind", sorted(ako.SATURATED))
def test_saturated_classes_lie_in_their_logit_range(kind):
    which, lo, hi = ako.SATURATED[kind]
    d = ako.gather_case(kind)
    opacity, scale, _ = ako.gather_logits(d)
    sat, other = (opacity, scale) if which == "opacity" else (scale, opacity)
    assert float(sat.min()) >= lo and float(sat.max()) <= hi, f"{kind}: logits in [{float(sat.min()):.1f}, {float(sat.max()):.1f}]"
    assert float(sat.max()) - float(sat.min()) > 0.8 * (hi - lo)                      # and they fill it
    assert float(other.abs().max()) < 10                                              # the other activation stays ordinary
    if kind in ("opacity_neg", "scale_small"):                                        # some values below fp32's normal range, some above
        assert bool((sat < -87.4).any()) and bool((sat > -87.3).any())
    (o64, _), (o32, _) = ako.gather_reference(kind)
    assert all(bool(torch.isfinite(t).all()) for t in o64 + o32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# skinning
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dict.fromkeys(ako.all_lbs_cases() + [ako.lbs_name(N, J) for N, J in ako.JOINT_GRAD_NJ] + ako.JOINT_GRAD_EDGE)))
def test_fragile_rows_stay_under_their_cap(name):
    d = ako.lbs_case(name)
    frag = ako.fragile_rows(name)
    assert tuple(frag.shape) == (d["N"],)
    # rows the test asserts exactly (the all-zero weight row: a four-way tie by construction) are not measured against the bar at all
    loose = frag & ~d["exact_rows"]
    assert int(loose.sum()) <= ako.FRAGILE_CAP * d["N"], f"{name}: {int(loose.sum())} fragile rows of {d['N']}"
    if d["N"] <= 1000:
        assert int(loose.sum()) == 0, f"{name}: fragile rows {loose.nonzero().flatten().tolist()} (choose another seed in lbs_case)"
    if name in ako.JOINT_GRAD_EDGE:                                                   # dL/dA is compared over all rows: none may be fragile at all
        assert not bool(frag.any()), f"{name}: fragile rows {frag.nonzero().flatten().tolist()}"


@pytest.mark.parametrize("name", [n for n in ako.all_lbs_cases() if n not in ("branches", "zero_row")])
def test_skinning_rows_are_unnormalised_sparse_and_not_unit(name):
    d = ako.lbs_case(name)
    lbs, rot = d["lbs"], d["rot"]
    sums, lens = lbs.sum(1), rot.norm(dim=1)
    assert float(sums.min()) >= 0.49 and float(sums.max()) <= 1.51
    assert float(lens.min()) >= 0.49 and float(lens.max()) <= 2.01
    if d["N"] >= 63:
        assert float(sums.max() - sums.min()) > 0.5 and float(lens.max() - lens.min()) > 0.8
    assert int((lbs != 0).sum(1).max()) == d["K"] <= 16                               # SparseLbs.build has a form
    assert bool((lbs >= 0).all())


def test_sparse_only_cases_use_the_last_joint_indices():
    for name, N, J, K in ako.LBS_SPARSE_ONLY:
        lbs = ako.lbs_case(name)["lbs"]
        assert tuple(lbs.shape) == (N, 256)
        used = (lbs != 0).sum(0)
        assert bool((used[250:256] >= 8).all()), f"{name}: joints 250..255 used by {used[250:256].tolist()} rows"
        assert bool((used[:250] > 0).any())


def test_zero_row_case():
    d = ako.lbs_case("zero_row")
    row = int(d["exact_rows"].nonzero())
    assert row == 64 and float(d["lbs"][row].abs().max()) == 0.0 and int(d["exact_rows"].sum()) == 1
    for ref in ako.lbs_reference("zero_row"):                                          # float64 and float32 agree on the values the kernel must give
        assert ref[0][row].tolist() == [0.0, 0.0, 0.0] and ref[1][row].tolist() == [0.5, 0.0, 0.0, 0.0]
        assert ref[3][row].tolist() == [0.0, 0.0, 0.0, 0.0] and ref[2][row].abs().max() == 0


def test_branch_case_reaches_every_reachable_branch():
    """At least 8 rows on each of the four arg-max candidates and on the positive-part branch of the square root (a radicand <= 0), none near a tie.  The
    0.1 floor and a radicand <= 0 of the SELECTED candidate cannot be reached: the radicands sum to 4, so the largest is >= 1 -- asserted here for every
    row of every case, shrunk (0.004) and negative (-0.5) blends included."""
    d = ako.lbs_case("branches")
    x4, qa = ako.m2q_quantities("branches")
    best = qa.argmax(1)
    assert torch.bincount(best, minlength=4).min() >= 8, torch.bincount(best, minlength=4).tolist()
    assert int((x4 <= 0).any(1).sum()) >= 8
    neg = d["lbs"][:, 0] < 0
    assert int(neg.sum()) >= 8 and bool((x4[neg] <= 0).any(1).all())                     # every row of the -0.5 blend takes it
    assert torch.bincount(best[neg], minlength=4).min() >= 1
    shrunk = d["lbs"][:, 0] == 0.004
    assert int(shrunk.sum()) >= 8 and torch.bincount(best[shrunk], minlength=4).min() >= 8
    assert not bool(ako.fragile_rows("branches").any())
    top = torch.topk(qa, 2, dim=1).values
    assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 50 * ako.FRAGILE_REL
    for name in ako.all_lbs_cases():
        x4, qa = ako.m2q_quantities(name)
        assert float((x4.sum(1) - 4).abs().max()) < 1e-12
        assert float(qa.max(1).values.min()) >= 1.0 - 1e-12, f"{name}: a selected q_abs below 1"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hand fusion
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [n for n in ako.HAND_N if n > 1])
def test_hand_cases_hold_the_rows_they_name(N):
    for boxes in ako.HAND_BOXES:
        d = ako.hand_case(N, boxes)
        y, cy = d["xyz"][:, 1], d["centre"][1]
        wl, wr, al, ar = ako.hand_weights(d)
        out, w = ako.hand_reference(N, boxes)
        w = w[:, 0]
        on, above, below = y == cy, y > cy, y < cy
        assert int(on.sum()) >= 32 and int(below.sum()) >= 32 and int(above.sum()) >= 32
        assert float(w[below].abs().max()) == 0.0
        assert int((y == torch.nextafter(cy, torch.tensor(-1.0))).sum()) >= 16              # one float below the centre: cut
        # y == centre_y rows keep a weight that matters: cutting them (y <= centre_y) would move the result
        assert int((on & (w > 0.1)).sum()) >= 16, f"{boxes}: y == centre_y rows carry no weight"
        # the fast exponential's argument beyond +-88 (it overflows to inf or underflows to 0), on rows that are not cut
        for a in (al, ar):
            assert int(((a > 88) & ~below).sum()) >= 16 and int(((a < -88) & ~below).sum()) >= 16
        if boxes == "overlap":
            assert int(((wl + wr > 1.01) & ~below).sum()) >= 32                           # max(wl + wr, 1) divides
            assert int(((wl + wr < 1) & ~below).sum()) >= 16                              # ... and does not, in the same launch
        else:
            mid = (w > 0.05) & (w < 0.95)
            assert int(mid.sum()) >= 32 and int((mid & on).sum()) >= 8                    # the blend weight runs over (0, 1)
            assert float((wl + wr)[~below].max()) <= 1.0
        assert all(bool(torch.isfinite(t).all()) for t in out.values())
    assert N % 256 != 0


def test_single_row_hand_case_sits_on_the_centre_line():
    for boxes in ako.HAND_BOXES:
        d = ako.hand_case(1, boxes)
        assert d["N"] == 1 and float(d["xyz"][0, 1]) == float(d["centre"][1])
        assert float(ako.hand_reference(1, boxes)[1][0, 0]) > 0.1
