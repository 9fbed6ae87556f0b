"""Plain-torch restatement of the template stage's field (``include/ag_template_field.h``, ``template_field.TemplateField``): positional
embedding -> weight-normalised geometry MLP (the embedding concatenated AFTER the activations at the skip layer) -> colour MLP ->
Laplace density.  It runs in float32 and float64 on the host and returns every layer's pre-activation, so that a missed bar can be
traced to its layer.

``make_net`` is a deterministic numpy recipe (``RandomState``; no torch RNG): the shapes of the geometric initialisation, then -- for a
"trained-like" net -- every weight, bias and ``weight_g`` perturbed, so that the high-frequency embedding columns of layer 0 and the
embedding columns of the skip layer, both zero at initialisation, carry weight.  Fixtures store points and outputs only; the weights are
always regenerated from this recipe.  ``state_dict`` writes the keys of the reference's ``TemplateNet``.
"""
import numpy as np
import torch
import torch.nn.functional as F

REFERENCE = dict(multires=6, widths=(512, 256, 256, 256, 256, 256), out=257, skip=(4,), color=(256, 256, 256), multires_viewdir=3)
NARROW = dict(multires=2, widths=(64, 32, 32, 32, 32, 32), out=33, skip=(4,), color=(32,), multires_viewdir=3)
SOFTPLUS_BETA = 100.0
BETA_MIN = np.float32(1e-4)          # LaplaceDensity's beta_min: an fp32 constant in every precision


def embed_dim(multires):
    return 3 + 6 * multires


def make_net(arch=REFERENCE, seed=0, use_viewdir=False, trained=True, sphere_bias=None, scale=1.0, geo_activation="softplus", density_beta=0.01, noise=0.05):
    """Raw parameters: ``geo`` = [(v [out, in], g [out, 1], bias [out])], ``color`` = [(W, bias)], all float32 numpy.  ``scale``
    multiplies every hidden geometry layer's ``weight_g`` (so the folded weights): it moves the pre-activations across softplus' branches.
    ``noise``: the perturbation of a trained-like net's weights, in units of the layer's initialisation spread."""
    if sphere_bias is None:          # the perturbed cosine columns act as a bias of about 0.4: 1.1 keeps the zero level near radius 0.7
        sphere_bias = 1.1 if trained else 0.7
    rs = np.random.RandomState(seed)
    e_pos = embed_dim(arch["multires"])
    chans = [e_pos] + list(arch["widths"]) + [arch["out"]]
    geo = []
    for l in range(len(chans) - 1):
        out_dim = chans[l + 1]
        in_dim = chans[l] + (e_pos if l in arch["skip"] else 0)
        last = l == len(chans) - 2
        std = np.sqrt(2) / np.sqrt(out_dim)
        if last:
            v = rs.normal(np.sqrt(np.pi) / np.sqrt(in_dim), 1e-4, (out_dim, in_dim))
            b = np.full(out_dim, -sphere_bias)
        else:
            v = rs.normal(0.0, std, (out_dim, in_dim))
            b = np.zeros(out_dim)
            if l == 0:
                v[:, 3:] = 0.0
            elif l in arch["skip"]:
                v[:, -(e_pos - 3):] = 0.0
        g = np.sqrt((v * v).sum(1, keepdims=True))
        if trained:
            v = v + rs.normal(0.0, noise * (1e-2 if last else std), v.shape)
            b = b + rs.normal(0.0, 0.02, b.shape)
            g = g * (1.0 + 0.1 * rs.normal(size=g.shape))
        if not last:
            g = g * scale
        geo.append((v.astype(np.float32), g.astype(np.float32), b.astype(np.float32)))
    e_view = embed_dim(arch["multires_viewdir"]) if use_viewdir else 0
    cch = [arch["out"] - 1 + e_view] + list(arch["color"]) + [3]
    color = []
    for l in range(len(cch) - 1):
        bound = 1.0 / np.sqrt(cch[l])
        color.append((rs.uniform(-bound, bound, (cch[l + 1], cch[l])).astype(np.float32), rs.uniform(-bound, bound, cch[l + 1]).astype(np.float32)))
    return dict(arch=arch, use_viewdir=use_viewdir, geo=geo, color=color, beta=np.float32(density_beta), geo_activation=geo_activation)


def state_dict(net, spelling="weight_g"):
    """The reference's keys.  ``spelling``: ``"weight_g"`` (``nn.utils.weight_norm``) or ``"parametrizations"``
    (``nn.utils.parametrizations.weight_norm``)."""
    gk, vk = ("weight_g", "weight_v") if spelling == "weight_g" else ("parametrizations.weight.original0", "parametrizations.weight.original1")
    sd = {}
    for i, (v, g, b) in enumerate(net["geo"]):
        p = f"geo_mlp.fc_list.{i}." + ("" if i == len(net["geo"]) - 1 else "0.")
        sd[p + gk], sd[p + vk], sd[p + "bias"] = torch.from_numpy(g.copy()), torch.from_numpy(v.copy()), torch.from_numpy(b.copy())
    for i, (w, b) in enumerate(net["color"]):
        p = f"tex_mlp.fc_list.{i}." + ("" if i == len(net["color"]) - 1 else "0.")
        sd[p + "weight"], sd[p + "bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    sd["density_func.beta"] = torch.tensor(float(net["beta"]), dtype=torch.float32)
    return sd


def embed(x, multires):
    """Column order of ``Embedder.embed``: x, then per frequency 1, 2, .., 2^(L-1): sin(x f), cos(x f)."""
    cols = [x]
    for k in range(multires):
        f = float(2 ** k)
        cols += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(cols, -1)


def fold(v, g, dtype):
    """torch's weight_norm forward, in ``dtype``: v * (g / ||v||_row)."""
    v, g = torch.from_numpy(v).to(dtype), torch.from_numpy(g).to(dtype)
    return v * (g / v.norm(dim=1, keepdim=True))


def forward(net, xyz, viewdirs=None, dtype=torch.float64):
    """``xyz`` [N, 3] numpy float32 -> dict of numpy arrays in ``dtype``: ``sdf`` [N, 1] (negated raw output), ``raw`` [N, 1],
    ``density`` [N, 1], ``color`` [N, 3], ``pre_geo`` / ``pre_color``: the pre-activation of every layer."""
    arch = net["arch"]
    x = torch.from_numpy(np.asarray(xyz, np.float32)).to(dtype)
    e = embed(x, arch["multires"])
    act = (lambda t: F.softplus(t, beta=SOFTPLUS_BETA, threshold=20)) if net["geo_activation"] == "softplus" else torch.relu
    h, pre_geo = e, []
    for l, (v, g, b) in enumerate(net["geo"]):
        if l in arch["skip"]:
            h = torch.cat([h, e], -1)
        z = F.linear(h, fold(v, g, dtype), torch.from_numpy(b).to(dtype))
        pre_geo.append(z)
        h = z if l == len(net["geo"]) - 1 else act(z)
    raw, feat = h[:, :1], h[:, 1:]
    if net["use_viewdir"]:
        d = torch.zeros_like(x) if viewdirs is None else torch.from_numpy(np.asarray(viewdirs, np.float32)).to(dtype)
        feat = torch.cat([feat, embed(d, arch["multires_viewdir"])], -1)
    c, pre_color = feat, []
    for l, (w, b) in enumerate(net["color"]):
        z = F.linear(c, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype))
        pre_color.append(z)
        c = torch.sigmoid(z) if l == len(net["color"]) - 1 else torch.relu(z)
    beta = torch.tensor(float(net["beta"]), dtype=torch.float32).to(dtype).abs() + torch.tensor(BETA_MIN).to(dtype)
    density = (1 / beta) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / beta))
    n = lambda t: t.numpy()  # noqa: E731
    return dict(sdf=n(-raw), raw=n(raw), density=n(density), color=n(c), pre_geo=[n(z) for z in pre_geo], pre_color=[n(z) for z in pre_color])


def folded_layers(net):
    """What ``TemplateField`` takes: the geometry weights folded in float64 and rounded once, the colour layers as they are."""
    geo = []
    for v, g, b in net["geo"]:
        v64 = v.astype(np.float64)
        geo.append(((g.astype(np.float64) * v64 / np.sqrt((v64 * v64).sum(1, keepdims=True))).astype(np.float32), b))
    return geo, list(net["color"])


def box_points(n, seed, half=1.2):
    """``n`` points uniform in a subject-sized box, float32."""
    return np.random.RandomState(seed).uniform(-half, half, (n, 3)).astype(np.float32)


def unit_dirs(n, seed):
    d = np.random.RandomState(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def volume_points(bounds, res):
    """``net_util.generate_volume_points``' formula on the host: [X * Y * Z, 3] float32."""
    b = torch.from_numpy(np.asarray(bounds, np.float32))
    axes = [torch.linspace(0, 1, steps=int(r), dtype=torch.float32) for r in res]
    xv, yv, zv = torch.meshgrid(*axes, indexing="ij")
    pts = torch.cat([xv.reshape(-1, 1), yv.reshape(-1, 1), zv.reshape(-1, 1)], -1)
    return (pts * (b[1] - b[0]) + b[0]).numpy()
