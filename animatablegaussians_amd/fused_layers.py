"""The layer-level autograd nodes of the StyleUNet, one ``torch.autograd.Function`` per layer of dual_styleunet.py:

  * ``_LayerCall``: ConvLayer (:326-371) and StyledConv (:570-604) as ONE native call each way (include/ag_layers.h ``AgLayerArgs``): the
    kernel sequence is issued from C, so the host pays one Python -> ctypes transition, one output allocation and one argument check per
    layer and direction instead of one per kernel (3-5 per layer, 13-32 us each; profiles/README.md has the host issue times).
  * ``_ToRGB`` (:607-633): the per-kernel Functions of ``styleunet_ops`` / ``conv`` composed in Python.  It calls their ``forward`` /
    ``backward`` static methods as plain functions with a stand-in for autograd's ``ctx`` (``_Sub``), it does not duplicate them; the wavelet
    skip iwt -> Upsample -> dwt is the one composed kernel ``skip_chain``.

``styleunet.set_fused_layers(False)`` runs the chain of per-kernel Functions instead; tests/test_styleunet_net.py pins the two against
each other.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import conv as agc
from ._lib import scratch as _scratch, stream as _stream
from .styleunet_ops import _flipped, _ModulateWeight, skip_chain_backward, skip_chain_forward_

_SQRT2 = 2 ** 0.5


class _Sub:
    """Stands in for the ``ctx`` of a custom Function whose forward / backward is called directly inside a fused node."""
    __slots__ = ("saved_tensors", "cfg", "needs_input_grad")

    def __init__(self, needs_input_grad=()):
        self.saved_tensors = ()
        self.cfg = None
        self.needs_input_grad = needs_input_grad

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _stash(ctx, subs):
    """Hand every tensor the sub-steps saved to autograd's own save_for_backward (an OUTPUT of the node kept as a plain attribute would
    form a reference cycle node -> output -> node and its memory would wait for the garbage collector)."""
    flat, layout = [], []
    for s in subs:
        n = len(s.saved_tensors) if s is not None else 0
        layout.append(n)
        if n:
            flat.extend(s.saved_tensors)
            s.saved_tensors = ()
    ctx.save_for_backward(*flat)
    ctx.subs, ctx.layout = subs, layout


def _unstash(ctx):
    saved, i = ctx.saved_tensors, 0
    for s, n in zip(ctx.subs, ctx.layout):
        if n:
            s.saved_tensors = tuple(saved[i:i + n])
            i += n
    return ctx.subs


def _release(ctx):
    """Drop the sub-steps' references again when the backward is done: they include the node's own output (the activation kernel's
    backward reads it), and a reference from the node to its output that autograd does not know about is a cycle only the garbage
    collector breaks -- gigabytes of activations per step would pile up until it runs."""
    for s in ctx.subs:
        if s is not None:
            s.saved_tensors = ()


def _releasing(backward):
    def wrapped(ctx, *grads):
        try:
            return backward(ctx, *grads)
        finally:
            _release(ctx)
    return wrapped


class _ToRGB(torch.autograd.Function):
    """ToRGB: modulated 1 x 1 convolution (no demodulation) + bias [+ wavelet-domain upsampled skip: iwt -> Upsample -> dwt]."""

    @staticmethod
    def forward(ctx, x, w, style, bias, skip, k_blur_up, mod_scale):
        s_mod = _Sub()
        wm = _ModulateWeight.forward(s_mod, w, style, mod_scale, False, False)
        s_conv = _Sub()
        out = agc._Conv.forward(s_conv, x, wm, bias, None, agc.AG_CONV, 1, 0, 1.0)
        ctx.skip_k = None
        if skip is not None:                                  # one kernel: the composed linear map, accumulated into the layer's output
            skip_chain_forward_(out, skip, k_blur_up, accumulate=True)
            ctx.skip_k = k_blur_up                            # a module buffer, not an output of this node: a plain attribute is safe
        _stash(ctx, (s_mod, s_conv))
        return out

    @staticmethod
    @_releasing
    def backward(ctx, g):
        s_mod, s_conv = _unstash(ctx)
        nx, nw, ns, nb, nskip = ctx.needs_input_grad[:5]
        g = g.contiguous()
        gskip = None
        if ctx.skip_k is not None and nskip:                 # the skip path's adjoint: one kernel
            gskip = skip_chain_backward(g, ctx.skip_k)
        s_conv.needs_input_grad = (nx, nw or ns)
        s_conv.cfg = s_conv.cfg[:3] + (bool(nb),) + s_conv.cfg[4:]          # bias gradient only when the bias wants one
        gx, gwm, gb = agc._Conv.backward(s_conv, g)[:3]
        gw = gs = None
        if gwm is not None:
            gw, gs = _ModulateWeight.backward(s_mod, gwm)[:2]
        return gx, gw, gs, gb, gskip, None, None


_SIZES = {}          # layer shape -> (OH, OW, forward scratch floats, backward scratch floats, conv workspace bytes)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _layer_sizes(a):
    key = (a.Cin, a.Cout, a.H, a.W, a.k, a.resample, a.modulated)
    v = _SIZES.get(key)
    if v is None:
        L = _lib.lib()
        oh, ow = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(L.ag_layer_output_size(ctypes.byref(a), ctypes.byref(oh), ctypes.byref(ow)), "ag_layer_output_size")
        # the convolution workspace: the library maps the layer to its convolution (ag_layers.hip geometry()); the single-layer call is G = 1
        g = _lib.AgGroupedLayerArgs()
        g.G, g.Cin, g.Cout, g.H, g.W, g.k, g.resample, g.modulated = 1, a.Cin, a.Cout, a.H, a.W, a.k, a.resample, a.modulated
        v = _SIZES[key] = (oh.value, ow.value, int(L.ag_layer_scratch_floats(ctypes.byref(a), 0)), int(L.ag_layer_scratch_floats(ctypes.byref(a), 1)),
                           int(L.ag_grouped_layer_workspace_bytes(ctypes.byref(g))))
    return v


def _describe(x, w, k_blur, scale, resample, modulated):
    if x.dim() != 4 or x.shape[0] != 1 or not x.is_cuda or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise RuntimeError("layer call: float32 GPU tensors, batch 1")
    a = _lib.AgLayerArgs()
    a.Cout, a.Cin, a.k = int(w.shape[-4]), int(w.shape[-3]), int(w.shape[-1])
    a.H, a.W = int(x.shape[2]), int(x.shape[3])
    if int(x.shape[1]) != a.Cin:
        raise RuntimeError("weight shape does not match the input channels")
    a.resample, a.modulated = int(bool(resample)), int(bool(modulated))
    a.scale, a.slope, a.act_scale = float(scale), 0.2, _SQRT2
    if resample and (k_blur is None or tuple(k_blur.shape) != (4, 4)):
        raise RuntimeError("resampling layers use the 4 x 4 FIR kernel")
    return a


class _LayerCall(torch.autograd.Function):
    """ConvLayer (modulated = False: style / noise / noise_weight are None) or StyledConv as ONE native call each way."""

    @staticmethod
    def forward(ctx, x, w, style, noise, noise_weight, bias, k_blur, scale, resample, modulated):
        x, w = x.contiguous(), w.contiguous()
        a = _describe(x, w, k_blur, scale, resample, modulated)
        oh, ow, f_fwd, _, a.workspace_bytes = _layer_sizes(a)
        dev = x.device
        out = torch.empty((1, a.Cout, oh, ow), dtype=torch.float32, device=dev)
        keep = None                                       # what the backward needs besides the inputs and the output
        if modulated:
            style = style.contiguous()
            if style.numel() != a.Cin:
                raise RuntimeError("style must have one entry per input channel")
            keep = torch.empty(w.numel() + a.Cout, dtype=torch.float32, device=dev)      # modulated weight, then the demodulation coefficients
            a.w_mod, a.demod, a.style = keep.data_ptr(), keep.data_ptr() + 4 * w.numel(), style.data_ptr()
            if noise is not None and noise_weight is not None:
                noise = noise.contiguous()
                if noise.numel() != oh * ow:
                    raise RuntimeError("noise must be [1, 1, OH, OW]")
                a.noise, a.noise_weight = noise.data_ptr(), noise_weight.data_ptr()
            else:
                noise = noise_weight = None
        elif resample:
            keep = torch.empty((1, a.Cin, a.H + 1, a.W + 1), dtype=torch.float32, device=dev)    # the blurred input (the weight gradient's operand)
            a.x_blur = keep.data_ptr()
        a.x, a.weight, a.out, a.act_bias = x.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias)
        a.k_blur = _ptr(k_blur) if resample else None
        buf, a.scratch, a.workspace = _scratch(f_fwd, a.workspace_bytes, dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ag_layer_forward(ctypes.byref(a), _stream(dev)), "ag_layer_forward")
        ctx.save_for_backward(x, w, style, noise, noise_weight, bias, out, keep, _flipped(k_blur) if resample else None)
        ctx.cfg = (float(scale), bool(resample), bool(modulated))
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, style, noise, noise_weight, bias, out, keep, k_flip = ctx.saved_tensors
        scale, resample, modulated = ctx.cfg
        nx, nw, ns, _, nnw, nb = ctx.needs_input_grad[:6]
        a = _describe(x, w, k_flip, scale, resample, modulated)
        dev = x.device
        g = g.contiguous()
        a.x, a.weight, a.out, a.g_out, a.act_bias = x.data_ptr(), w.data_ptr(), out.data_ptr(), g.data_ptr(), _ptr(bias)
        a.k_blur = _ptr(k_flip)
        gx = torch.empty_like(x) if nx else None
        want_w = nw or (modulated and ns)
        gw = torch.empty_like(w) if want_w else None
        gs = gnw = gb = gbn = None
        if modulated:
            a.style, a.w_mod, a.demod = style.data_ptr(), keep.data_ptr(), keep.data_ptr() + 4 * w.numel()
            if noise is not None:
                a.noise, a.noise_weight = noise.data_ptr(), noise_weight.data_ptr()
            if want_w:
                gs = torch.empty_like(style)
        elif resample:
            a.x_blur = keep.data_ptr()
        a.want_bias = int(bool(nb and bias is not None))
        a.want_noise_weight = int(bool(modulated and nnw and noise is not None))
        if a.want_bias or a.want_noise_weight:
            gbn = torch.empty(a.Cout + 1, dtype=torch.float32, device=dev)
            gb = gbn[:a.Cout] if a.want_bias else None
            gnw = gbn[a.Cout:] if a.want_noise_weight else None
        a.g_x, a.g_weight, a.g_style, a.g_bias_noise = _ptr(gx), _ptr(gw), _ptr(gs), _ptr(gbn)
        _, _, _, f_bwd, a.workspace_bytes = _layer_sizes(a)
        buf, a.scratch, a.workspace = _scratch(f_bwd, a.workspace_bytes, dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ag_layer_backward(ctypes.byref(a), _stream(dev)), "ag_layer_backward")
        if gnw is not None and noise_weight is not None:
            gnw = gnw.view(noise_weight.shape)
        return gx, gw, gs, None, gnw, gb, None, None, None, None


def conv_layer(x, w, bias, k_blur, scale, downsample):
    return _LayerCall.apply(x, w, None, None, None, bias, k_blur if downsample else None, float(scale), bool(downsample), False)


def styled_conv(x, w, style, noise, noise_weight, act_bias, k_blur, mod_scale, upsample):
    return _LayerCall.apply(x, w, style, noise, noise_weight, act_bias, k_blur if upsample else None, float(mod_scale), bool(upsample), True)


def to_rgb(x, w, style, bias, skip, k_blur_up, mod_scale):
    return _ToRGB.apply(x, w, style, bias, skip, k_blur_up, float(mod_scale))
