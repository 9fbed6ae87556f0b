"""A/B of two builds of libag_hip.so around a change to csrc/ag_conv.hip; took what profiles/conv_engine_ab.txt records.
    python profiles/conv_engine_ab.py resources PARENT.hip NEW.hip    registers / scratch / LDS / instruction lines of every kernel (no GPU)
    AG_LIB_PATH=LIB python profiles/conv_engine_ab.py time MODE       one process: us per launch of the three shapes, one `TIME` line
    AG_LIB_PATH=LIB python profiles/conv_engine_ab.py results OUT.pt  one process: the 46 result entries, saved
    python profiles/conv_engine_ab.py equal A.pt B.pt                 torch.equal over every tensor of two such files
    python profiles/conv_engine_ab.py bar LOG                         per shape, family and mode: means, the parent's spread, the bar
The caller runs one process per library and measurement, serially, alternating parent, new, new, parent, ...; a `time` process is labelled
by AG_AB_LABEL (parent / new)."""
import os
import re
import subprocess
import sys

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-ffp-contract=fast"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# TIME_SHAPES: (name, Cin, Cout, H = W), 3 x 3 stride 1 padding 1; RESULT_SHAPES: (kind, Cin, Cout, H, W, k, stride, padding); both sets are
# those of profiles/conv_cleanup_ab.txt
TIME_SHAPES = [("256_256", 256, 256, 256), ("64_512", 64, 64, 512), ("512_32", 512, 512, 32)]
RESULT_SHAPES = [("conv", 256, 256, 64, 64, 3, 1, 1), ("conv", 128, 128, 96, 96, 3, 1, 1), ("conv", 64, 128, 64, 64, 3, 2, 1), ("conv", 512, 256, 32, 32, 3, 1, 1),
                 ("convT", 64, 32, 24, 24, 3, 2, 0), ("conv", 48, 80, 40, 36, 3, 1, 1), ("conv", 12, 64, 66, 62, 4, 2, 1), ("conv", 64, 64, 256, 256, 3, 1, 1),
                 ("conv", 512, 512, 8, 8, 3, 1, 1)]
MODES = ["split_f16", "fp32", "split_bf16", "split_bf16x3", "f16"]


def demangle(names):
    return subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")[:len(names)]


def kernel_table(src):
    """{kernel: (VGPRs, scratch bytes per lane, occupancy, LDS bytes, instruction lines)}"""
    err = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    asm = subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True).stdout
    lines, cur = {}, None
    for line in asm.splitlines():           # instruction lines: neither labels, directives nor comments, between a kernel's label and its end
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            lines[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and line.strip() and not line.strip().startswith((";", ".", "//")) and not line.strip().endswith(":"):
            lines[cur] += 1
    names = list(res)
    return {d.strip(): (res[n].get("VGPRs", -1), res[n].get("ScratchSize [bytes/lane]", -1), res[n].get("Occupancy [waves/SIMD]", -1),
                        res[n].get("LDS Size [bytes/block]", -1), lines.get(n, -1)) for n, d in zip(names, demangle(names))}


def resources(parent_src, new_src):
    a, b = kernel_table(parent_src), kernel_table(new_src)
    print(f"kernels: parent {len(a)}, new {len(b)}, same names: {set(a) == set(b)}")
    print(f"{'VGPRs':>9s} {'scratch':>9s} {'occ':>5s} {'LDS':>13s} {'instr. lines':>13s}  kernel   (parent -> new; one number: equal)")
    for k in a:
        x, y = a[k], b.get(k, (-1,) * 5)
        cell = lambda i, w: f"{(str(x[i]) if x[i] == y[i] else f'{x[i]}->{y[i]}'):>{w}s}"
        print(f"{cell(0, 9)} {cell(1, 9)} {cell(2, 5)} {cell(3, 13)} {cell(4, 13)}  {k.replace('ag::', '').replace('void ', '').split('(')[0]}")
    bad = [k for k in a if k in b and (a[k][2] != b[k][2] or a[k][3] != b[k][3])]
    two = [k for k in a if k in b and re.search(r", 2>\(|, 2, (true|false)>\(", k) and b[k][1] > a[k][1]]
    print(f"occupancy or LDS differ: {bad or 'none'}; NTERMS = 2 kernels with more scratch than the parent: {two or 'none'}")


def timed(mode):
    import torch
    from animatablegaussians_amd import _lib, conv
    conv.set_math(mode)
    out = []
    for name, cin, cout, hw in TIME_SHAPES:
        g = torch.Generator().manual_seed(3)
        x = torch.randn(1, cin, hw, hw, generator=g).cuda()
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda().requires_grad_(True)
        for _ in range(30):
            y = conv.conv2d(x, w, padding=1)
        torch.cuda.synchronize()
        _lib.prof_enable([_lib.AG_K_GATHER_CONV])
        _lib.prof_collect()
        for _ in range(150):
            y = conv.conv2d(x, w, padding=1)
        torch.cuda.synchronize()
        n, ms = next(v for v in _lib.prof_collect().values() if v[0])
        assert n == 150, n
        gather_us = 1e3 * ms / n
        gy = torch.randn(y.shape, generator=g).cuda()
        _lib.prof_enable([])
        for _ in range(10):
            torch.autograd.grad(y, w, gy, retain_graph=True)
        torch.cuda.synchronize()
        _lib.prof_enable([_lib.AG_K_WGRAD])
        _lib.prof_collect()
        for _ in range(50):
            torch.autograd.grad(y, w, gy, retain_graph=True)
        torch.cuda.synchronize()
        n, ms = next(v for v in _lib.prof_collect().values() if v[0])
        assert n == 50, n
        _lib.prof_enable([])
        out.append(f"g{name} {gather_us:.2f} w{name} {1e3 * ms / n:.2f}")
    print(f"TIME {os.environ.get('AG_AB_LABEL', '?')} {mode} " + " ".join(out), flush=True)


def results(path):
    import torch
    from animatablegaussians_amd import conv, grouped
    saved = {}
    for mode in MODES:
        conv.set_math(mode)
        for kind, cin, cout, h, w_, k, stride, padding in RESULT_SHAPES:
            g = torch.Generator().manual_seed(cin * 7 + cout)
            x = torch.randn(1, cin, h, w_, generator=g).cuda().requires_grad_(True)
            w = (torch.randn(*((cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)), generator=g) / (cin * k * k) ** 0.5).cuda().requires_grad_(True)
            y = conv.conv2d(x, w, None, stride=stride, padding=padding) if kind == "conv" else conv.conv_transpose2d(x, w, None, stride=2)
            gy = torch.randn(y.shape, generator=g).cuda()
            dx, dw = torch.autograd.grad(y, (x, w), gy)
            saved[f"{mode} {kind} {cin} {cout} {h} {w_} {k} {stride} {padding}"] = [t.detach().cpu() for t in (y, dx, dw)]
    conv.set_math("split_f16")
    G, ci, co, hs = 6, 64, 64, 32
    g = torch.Generator().manual_seed(5)
    xs = torch.randn(G, ci, hs, hs, generator=g).cuda().requires_grad_(True)
    ws = [torch.randn(1, co, ci, 3, 3, generator=g).cuda().requires_grad_(True) for _ in range(G)]
    sts = [(torch.randn(1, ci, generator=g) + 1).cuda().requires_grad_(True) for _ in range(G)]
    nzs = [torch.randn(1, 1, hs, hs, generator=g).cuda() for _ in range(G)]
    nws = [torch.randn(1, generator=g).cuda().requires_grad_(True) for _ in range(G)]
    bss = [(torch.randn(co, generator=g) * 0.1).cuda().requires_grad_(True) for _ in range(G)]
    y = grouped.grouped_styled_conv(xs, ws, sts, nzs, nws, bss, None, 1 / (ci * 9) ** 0.5, False)
    grads = torch.autograd.grad(y, [xs] + ws + sts + nws + bss, torch.randn(y.shape, generator=g).cuda())
    saved["grouped StyledConv G=6"] = [t.detach().cpu() for t in (y,) + tuple(grads)]
    torch.save(saved, path)
    print(f"RESULTS {len(saved)} entries -> {path}")


def equal(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert a.keys() == b.keys()
    diff = []
    for k in a:
        for i, (s, t) in enumerate(zip(a[k], b[k])):
            if not torch.equal(s, t):
                diff.append((k, i, int((s != t).sum()), float((s - t).abs().max())))
    print(f"EQUAL {len(a)} entries, {sum(len(v) for v in a.values())} tensors: " + ("every tensor bit-identical" if not diff else f"DIFFERENT {diff}"))
    sys.exit(1 if diff else 0)


def bar(log):
    rows = {}
    for line in open(log):
        f = line.split()
        if f[:1] == ["TIME"]:
            for name, v in zip(f[3::2], f[4::2]):
                rows.setdefault((f[2], name), {}).setdefault(f[1], []).append(float(v))
    ok = True
    for (mode, name), d in rows.items():
        p, n = d["parent"], d["new"]
        pm, nm, spread = sum(p) / len(p), sum(n) / len(n), max(p) - min(p)
        met = nm <= pm + spread
        ok = ok and met
        print(f"{mode:10s} {name:9s} parent {pm:8.2f} ({len(p)} runs, spread {spread:5.2f})  new {nm:8.2f} ({len(n)} runs)  {100 * (nm / pm - 1):+5.2f} %  {'within' if met else 'OVER'} the bar")
    print("per-kernel bar (new mean <= parent mean + parent spread): " + ("met everywhere" if ok else "MISSED"))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    {"resources": resources, "time": timed, "results": results, "equal": equal, "bar": bar}[sys.argv[1]](*sys.argv[2:])
