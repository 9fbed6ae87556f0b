"""A/B of the kernels of csrc/ag_avatar.hip between two builds of the library (AG_LIB_PATH selects one; default: the tree's own).
    python profiles/avatar_kernels_ab.py dump OUT.pt         every result the bits comparison of profiles/avatar_kernels_ab.txt covers
    python profiles/avatar_kernels_ab.py compare A.pt B.pt   arrays / elements / differing elements, bitwise
    python profiles/avatar_kernels_ab.py time [dense]        one JSON line: avatar_kernel_rooflines of bench_avatar.py (with `dense`: the
                                                             synthetic subject without its sparse rows) and the joint-gradient backward,
                                                             dense and sparse, timed the way its graph_us times (20 launches per replay)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import avatar_kernels_oracle as ako
    from animatablegaussians_amd import avatar_ops as ops
    out = {}
    joint = [ako.lbs_name(N, J) for N, J in ako.JOINT_GRAD_NJ] + ako.JOINT_GRAD_EDGE
    for name, joint_grad in [(n, False) for n in ako.all_lbs_cases()] + [(n, True) for n in joint]:
        d = ako.lbs_case(name)
        sparse = ops.SparseLbs.build(d["lbs"].cuda())
        forms = ([("dense", None)] if d["J"] <= 160 else []) + ([("sparse", sparse)] if sparse is not None else [])
        for form, sp in forms:
            p, r = (d[k].cuda().requires_grad_(True) for k in ("pos", "rot"))
            A = d["A"].cuda().requires_grad_(joint_grad)
            lp, lr = ops.lbs_transform(p, r, d["lbs"].cuda(), A, sp)
            torch.autograd.backward([lp, lr], [u.cuda() for u in d["ups"]])
            for what, t in zip(("lp", "lr", "dp", "dr", "dA"), (lp, lr, p.grad, r.grad, A.grad)):
                if t is not None:
                    out[f"lbs/{name}/{'joint' if joint_grad else 'plain'}/{form}/{what}"] = t.detach().cpu()
    for name in ako.GATHER_CASES:
        d = ako.gather_case(name)
        maps = [d[k].cuda().requires_grad_(True) for k in ("position_map", "other_map", "color_map")]
        outs = ops.gather_activate(*maps, ops.mask_to_pix(d["mask"].cuda()), *(d[k].cuda() for k in ("xyz", "opacity_raw", "scaling_raw", "rotation_raw")))
        torch.autograd.backward(list(outs), [u.cuda() for u in d["ups"]])
        for i, t in enumerate(list(outs) + [m.grad for m in maps]):
            out[f"gather/{name}/{i}"] = t.detach().cpu()
    torch.save(out, path)
    print(f"{path}: {len(out)} arrays, {sum(t.numel() for t in out.values())} elements")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert list(a) == list(b)
    bits = lambda t: t.contiguous().view(torch.int32)
    bad = {k: int((bits(a[k]) != bits(b[k])).sum()) for k in a if a[k].shape != b[k].shape or not torch.equal(bits(a[k]), bits(b[k]))}
    print(f"{pa} != {pb}: {len(a)} arrays, {sum(t.numel() for t in a.values())} elements; differing in {len(bad)} arrays {bad}")
    for group in ("lbs", "gather"):
        ks = [k for k in a if k.startswith(group)]
        print(f"  {group}: {len(ks)} arrays, {sum(a[k].numel() for k in ks)} elements, {sum(bad.get(k, 0) for k in ks)} elements differ")
    return 1 if bad else 0


def graph_us(fn, dev, reps=20):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / reps)
    return float(sorted(us)[len(us) // 2])


def time_kernels(dense):
    import bench_avatar
    from animatablegaussians_amd import avatar_ops as ops
    from animatablegaussians_amd.avatar import AvatarRenderCore
    dev = torch.device("cuda", 0)
    build = ops.SparseLbs.build
    if dense:
        ops.SparseLbs.build = staticmethod(lambda lbs, max_k=16: None)
    roof = bench_avatar.avatar_kernel_rooflines(dev)
    ops.SparseLbs.build = build
    res = {"form": "dense" if dense else "default", "K": roof["sparse_lbs_pairs_per_gaussian"]}
    res.update({k: roof[k]["avg_launch_us"] for k in ("gather_forward", "gather_backward", "lbs_forward", "lbs_backward")})

    class Ctx:                                             # stands in for autograd's ctx, as in avatar_kernel_rooflines
        def __init__(self, needs):
            self.needs_input_grad = needs

        def save_for_backward(self, *ts):
            self.saved_tensors = ts

    core = AvatarRenderCore.synthetic(device=dev)
    N = int(core.xyz.shape[0])
    gen = torch.Generator().manual_seed(7)
    pos, rot = (torch.randn(N, c, generator=gen).to(dev) for c in (3, 4))
    gpr = [torch.randn(N, c, generator=gen).to(dev) for c in (3, 4)]
    A = bench_avatar.joint_transforms(core.lbs.shape[1], dev)
    # dL/dA alone (the joint kernel + the slab reducer), and with dL/dpositions and dL/drotations (lbs_backward_kernel's launch as well)
    for form, sp in (("dense", None), ("sparse", core.lbs_sparse)):
        for tag, needs in (("joints", (False, False, False, True, False)), ("joints_and_inputs", (True, True, False, True, False))):
            ctx = Ctx(needs)
            ops._LbsTransform.forward(ctx, pos, rot, core.lbs, A, sp)
            res[f"{tag}_{form}"] = round(graph_us(lambda: ops._LbsTransform.backward(ctx, *gpr), dev), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        time_kernels(len(sys.argv) > 2 and sys.argv[2] == "dense")
