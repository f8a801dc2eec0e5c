"""StarGAN v2 networks (methods/GAN-based/StarGANv2AdvCon/core/model.py), HIP-backed: forward and first-order
backward of the AdaIN generator, the mapping network, the style encoder and the ResBlk discriminator, with the
reference's module trees and state_dict keys, ``build_model``, ``moving_average``, ``CheckpointIO``
(core/checkpoint.py) and style-guided inference for the Sintel harness (core/solver.py:325-347).

The networks are chains of small autograd nodes over NHWC fp32 tensors (channel counts are multiples of 4 beyond the
image / logit ends):
  * convs on the implicit-GEMM kernels (zero padding); ``Linear`` layers are 1x1 convs over [B, 1, 1, K] on the
    same path (the AdaIN ``fc``, the mapping network, the heads), with the ReLU / LeakyReLU that follows a layer
    in its epilogue;
  * ``InstanceNorm2d(affine=True)`` + LeakyReLU (vst_instnorm_affine_*) and AdaIN + LeakyReLU (vst_adain_*), both
    over the statistics pass vst_instnorm_stats;
  * ``avg_pool2d(2)`` (vst_avgpool2_*), nearest 2x upsampling (vst_upsample2x_*) and the block's
    ``(shortcut + residual) / sqrt(2)`` with the identity shortcut's resampling folded in (vst_merge_*).
The learned shortcut's 1x1 conv runs on the low-resolution side of its resampling (ResBlk: pool, then conv;
AdainResBlk: conv, then upsample in the merge), a quarter of the reference order's work; see DESIGN.md.

The discriminator half of the solver (core/solver.py:167-176, :360-382, :459-476) is here too: ``adv_loss``, ``r1_reg``,
``compute_d_loss`` / ``d_losses``, ``he_init`` and ``DiscriminatorTrainer`` (torch.optim.Adam with the reference's
weight decay, ``d_step``).  The R1 penalty differentiates ||dD/dx_real||^2 with respect to D's weights, so every node
under the discriminator is differentiable twice (see the note above ``_INPUT_GRAD_ONLY``); the penalty itself and the
adversarial term (BCE with logits fused with the domain gather) are the kernels vst_loss_r1 / vst_loss_bce_logits.

Still missing: ``compute_g_loss`` (the generator half of the step) and the EMA train loop around both halves.
``w_hpf > 0`` (HighPass / FAN) and ``masks`` are not on the HIP path and raise NotImplementedError.
"""
import copy
import math
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from .faststyle import InstanceNormAffine
from .fc2 import _AttrDict
from .networks import Conv2d, _Marker, _ToNCHW, _ToNHWC
from .ops import cpad

SLOPE = 0.2
RSQRT2 = 1.0 / math.sqrt(2.0)


# ------------------------------------------------------------------------------------ autograd nodes (NHWC)
def _packs(mod):
    """(forward pack, data-gradient pack, padded bias) of a Conv2d / Linear holder, rebuilt when its weights change
    (in-place updates and loads bump the parameters' versions; moving the module changes the storage)."""
    w, b = mod.weight, mod.bias
    key = (w._version, w.data_ptr(), None if b is None else (b._version, b.data_ptr()))
    ent = getattr(mod, "_vst_packs", None)
    if ent is None or ent[0] != key:
        w4 = w.detach().reshape(w.shape[0], w.shape[1], *(w.shape[2:] if w.dim() == 4 else (1, 1))).contiguous()
        bp = None
        if b is not None:
            bp = torch.zeros(cpad(b.numel()), device=b.device)
            bp[:b.numel()] = b.detach()
        ent = (key, (ops.weight_pack(w4, ops.PACK_FWD), ops.weight_pack(w4, ops.PACK_DGRAD), bp))
        mod._vst_packs = ent
    return ent[1]


# The nodes under the discriminator (conv, LeakyReLU, pooling, merge, the layout conversions) are differentiable
# twice: each backward is itself made of autograd Functions over the same kernels, so the R1 penalty's
# autograd.grad(create_graph=True) leaves a graph that loss.backward() walks down to D's weights.  A conv's three
# bilinear kernels are each other's derivatives (forward <-> data gradient, both -> weight gradient); the activation
# mask, the pooling backward and the merge backward are linear maps whose adjoints are kernels the forward already has.
# The norm and upsampling nodes (generator only) stay first-order and say so (once_differentiable).
#
# Set by _input_grad around the penalty's autograd.grad (a module global: the engine runs the backward on its device
# thread): that sweep asks for the image gradient alone, and the weight / bias gradients are no part of its graph.
_INPUT_GRAD_ONLY = [False]


class _MaskFn(torch.autograd.Function):
    """g * act'(y) through the activation's output y: linear in g and its own adjoint; d/dy = 0 almost everywhere."""

    @staticmethod
    def forward(ctx, g, y, act):
        ctx.save_for_backward(y)
        ctx.act = act
        return ops.act_bwd(g, y, act, SLOPE)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        (y,) = ctx.saved_tensors
        return ops.act_bwd(gg.contiguous(), y, ctx.act, SLOPE), None, None


def _wgrad(x, gz, weight, has_bias, k, stride, pad):
    """(dw, db) of a conv from its input and its output's gradient: one vst_conv2d_wgrad launch."""
    co, ci = weight.shape[0], weight.shape[1]
    dw = torch.zeros_like(weight)
    db = torch.zeros(co, device=x.device) if has_bias else None
    ops.conv2d_wgrad(x, gz, dw, db, k, k, stride, pad, "zero", co, ci, ci * k * k, k * k, accumulate=False)
    return dw, db


class _DgradFn(torch.autograd.Function):
    """dx = conv^T(gz; W), bilinear in (gz, W): its backward is the forward conv of ggx (for gz) and the weight
    gradient of (ggx, gz) (for W)."""

    @staticmethod
    def forward(ctx, gz, weight, mod, ck, k, stride, pad, xshape):
        ctx.save_for_backward(gz)
        ctx.conf = (weight, mod, k, stride, pad)
        _, H, W, C = xshape
        return ops.conv2d_tfwd(gz, ck, None, H, W, C, k, k, stride, pad)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        (gz,) = ctx.saved_tensors
        weight, mod, k, stride, pad = ctx.conf
        ggx = ggx.contiguous()
        d_gz = d_w = None
        if ctx.needs_input_grad[0]:
            d_gz = ops.conv2d_fwd(ggx, _packs(mod)[0], None, cpad(weight.shape[0]), k, k, stride, pad, "zero",
                                  role="bwd")
        if ctx.needs_input_grad[1]:
            d_w, _ = _wgrad(ggx, gz, weight, False, k, stride, pad)
        return d_gz, d_w, None, None, None, None, None, None


class _WgradFn(torch.autograd.Function):
    """(dw, db) of a conv.  First-order: the R1 penalty never differentiates it (its sweep computes no weight
    gradient, and the masks have zero derivative), and anything that tries is refused."""

    @staticmethod
    def forward(ctx, x, gz, weight, has_bias, k, stride, pad):
        return _wgrad(x, gz, weight, has_bias, k, stride, pad)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggw, ggb):
        raise RuntimeError("the weight gradient of a StarGAN v2 conv is first-order only")


class _ConvFn(torch.autograd.Function):
    """act(conv(x, weight) + bias), zero padding; weight [Co, Ci, k, k] or a Linear's [Co, Ci] (k = 1).
    backward: activation mask -> data gradient -> weight and bias gradient, each a Function."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, k, stride, pad, act):
        kc, ck, bp = _packs(mod)
        role = "fwd" if any(ctx.needs_input_grad[:3]) else "infer"
        y = ops.conv2d_fwd(x, kc, bp, cpad(weight.shape[0]), k, k, stride, pad, "zero", act=act, slope=SLOPE, role=role)
        ctx.save_for_backward(x, y if act != "none" else None)
        ctx.conf = (weight, bias is not None, mod, ck, k, stride, pad, act)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        weight, has_bias, mod, ck, k, stride, pad, act = ctx.conf
        gz = gy.contiguous()
        if act != "none":
            gz = _MaskFn.apply(gz, y, act)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _DgradFn.apply(gz, weight, mod, ck, k, stride, pad, x.shape)
        if not _INPUT_GRAD_ONLY[0] and (ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])):
            dw, db = _WgradFn.apply(x, gz, weight.detach(), has_bias, k, stride, pad)
        return dx, dw, db, None, None, None, None, None


def _conv(x, mod, act="none"):
    return _ConvFn.apply(x, mod.weight, mod.bias, mod, mod.kernel_size, mod.stride, mod.padding, act)


def _linear(x, mod, act="none"):
    """x [B, K] (K % 4 == 0) -> [B, out_features] through the 1x1 conv over [B, 1, 1, K]."""
    B, K = x.shape
    if K % 4:
        raise NotImplementedError("Linear on the HIP path needs in_features %% 4 == 0, got %d" % K)
    y = _ConvFn.apply(x.contiguous().view(B, 1, 1, K), mod.weight, mod.bias, mod, 1, 1, 0, act)
    return y.view(B, -1)[:, :mod.out_features]


class _AffineNormActFn(torch.autograd.Function):
    """LeakyReLU(InstanceNorm2d(affine=True)(x))."""

    @staticmethod
    def forward(ctx, x, gamma, beta):
        st = ops.instnorm_stats(x)
        ctx.save_for_backward(x, st, gamma, beta)
        return ops.instnorm_affine_fwd(x, st, gamma.detach(), beta.detach(), "lrelu", slope=SLOPE)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, st, gamma, beta = ctx.saved_tensors
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        dx = ops.instnorm_affine_bwd(g.contiguous(), x, st, gamma.detach(), beta.detach(), "lrelu", dgamma=dg,
                                     dbeta=db, accumulate=False, slope=SLOPE)
        return dx, dg, db


class _AdaINActFn(torch.autograd.Function):
    """LeakyReLU((1 + gamma) * InstanceNorm2d(x) + beta), {gamma, beta} = h.chunk(2, 1); h [N, 2*C]."""

    @staticmethod
    def forward(ctx, x, h):
        st = ops.instnorm_stats(x)
        ctx.save_for_backward(x, st, h)
        return ops.adain_fwd(x, st, h, "lrelu", SLOPE)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, st, h = ctx.saved_tensors
        dh = torch.empty_like(h) if ctx.needs_input_grad[1] else None
        dx = ops.adain_bwd(g.contiguous(), x, st, h, "lrelu", SLOPE, dh=dh)
        return dx, dh


class _LReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.act_fwd(x, "lrelu", SLOPE)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return _MaskFn.apply(g.contiguous(), y, "lrelu")


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.avgpool2(x)

    @staticmethod
    def backward(ctx, g):
        return _PoolBwdFn.apply(g.contiguous())


class _PoolBwdFn(torch.autograd.Function):
    """g / 4 spread over each 2x2 window; its adjoint is the pooling itself."""

    @staticmethod
    def forward(ctx, g):
        return ops.avgpool2_bwd(g)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        return ops.avgpool2(gg.contiguous())


class _Up2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.upsample2x(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.upsample2x_bwd(g.contiguous())


class _MergeFn(torch.autograd.Function):
    """(a + f(b)) / sqrt(2), f by mode ('same' | 'pool' | 'up')."""

    @staticmethod
    def forward(ctx, a, b, mode):
        ctx.mode = mode
        return ops.merge(a, b, mode, RSQRT2)

    @staticmethod
    def backward(ctx, g):
        ga, gb = _MergeBwdFn.apply(g.contiguous(), ctx.mode)
        return ga, gb, None


class _MergeBwdFn(torch.autograd.Function):
    """g -> (g, f^T(g)) / sqrt(2); its adjoint (gga, ggb) -> (gga + f(ggb)) / sqrt(2) is the merge itself."""

    @staticmethod
    def forward(ctx, g, mode):
        ctx.mode = mode
        return ops.merge_bwd(g, mode, RSQRT2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gga, ggb):
        return ops.merge(gga.contiguous(), ggb.contiguous(), ctx.mode, RSQRT2), None


class _ToNHWC2(torch.autograd.Function):
    """NCHW -> NHWC with channel stride cs; the pair below is each other's backward, so an image gradient taken
    through it can be differentiated again."""

    @staticmethod
    def forward(ctx, x, cs):
        ctx.c = x.shape[1]
        return ops.nchw_to_nhwc(x.contiguous(), cs)

    @staticmethod
    def backward(ctx, g):
        return _ToNCHW2.apply(g.contiguous(), ctx.c), None


class _ToNCHW2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, c):
        ctx.cs = y.shape[-1]
        return ops.nhwc_to_nchw(y.contiguous(), c)

    @staticmethod
    def backward(ctx, g):
        return _ToNHWC2.apply(g.contiguous(), ctx.cs), None


class _R1Fn(torch.autograd.Function):
    """r1_reg of the NHWC-4 image gradient g (vst_loss_r1); its backward is a Function too, so create_graph runs
    through it."""

    @staticmethod
    def forward(ctx, g):
        ctx.save_for_backward(g)
        return ops.r1(g)

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return _R1BwdFn.apply(gout.contiguous(), g)


class _R1BwdFn(torch.autograd.Function):
    """u = gout * g / B with lane 3 zeroed: bilinear in (gout, g)."""

    @staticmethod
    def forward(ctx, gout, g):
        ctx.save_for_backward(gout, g)
        return ops.r1_bwd(g, gout)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggu):
        gout, g = ctx.saved_tensors
        ggu = ggu.contiguous()
        d_gout = d_g = None
        if ctx.needs_input_grad[0]:   # only a third-order use gets here: the penalty's gout is a constant
            d_gout = (ggu[..., :3] * g[..., :3]).sum() / g.shape[0]
        if ctx.needs_input_grad[1]:
            d_g = ops.r1_bwd(ggu, gout)
        return d_gout, d_g


class _BCEFn(torch.autograd.Function):
    """adv_loss of the head's output z [B, cpad(num_domains)] at the columns y (vst_loss_bce_logits): the gather,
    the constant target and the mean in one launch each way; the other columns get exact zeros."""

    @staticmethod
    def forward(ctx, z, y, nd, target):
        ctx.save_for_backward(z, y)
        ctx.conf = (nd, target)
        return ops.bce_logits(z, y, nd, target)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, y = ctx.saved_tensors
        return ops.bce_logits_bwd(z, y, *ctx.conf, gout.contiguous()), None, None, None


# ------------------------------------------------------------------------------------------- parameter holders
class Linear(nn.Module):
    """Parameter holder with nn.Linear's state (weight [out, in], bias [out]) and default init."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        nn.init.uniform_(self.bias, -1 / in_features ** 0.5, 1 / in_features ** 0.5)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias=True"


def _conv2d(cin, cout, k, stride=1, padding=0, bias=True):
    """networks.Conv2d with nn.Conv2d's default init."""
    m = Conv2d(cin, cout, k, stride=stride, padding=padding, bias=bias)
    nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
    if bias:
        fan_in = cin * k * k
        nn.init.uniform_(m.bias, -1 / fan_in ** 0.5, 1 / fan_in ** 0.5)
    return m


def _check_c4(*dims):
    for d in dims:
        if d % 4:
            raise NotImplementedError("channel counts must be multiples of 4 on the HIP path (NHWC float4 lanes), "
                                      "got %d" % d)


# ------------------------------------------------------------------------------------------------------ blocks
class ResBlk(nn.Module):
    """core/model.py:23-64: pre-activation residual block, LeakyReLU(0.2), optional affine IN and avg_pool2d(2).
    forward_nhwc takes and returns NHWC tensors."""

    def __init__(self, dim_in, dim_out, actv=None, normalize=False, downsample=False):
        super().__init__()
        _check_c4(dim_in, dim_out)
        self.actv = _Marker("LeakyReLU(0.2)")
        self.normalize, self.downsample = normalize, downsample
        self.learned_sc = dim_in != dim_out
        self.conv1 = _conv2d(dim_in, dim_in, 3, 1, 1)
        self.conv2 = _conv2d(dim_in, dim_out, 3, 1, 1)
        if normalize:
            self.norm1 = InstanceNormAffine(dim_in)
            self.norm2 = InstanceNormAffine(dim_in)
        if self.learned_sc:
            self.conv1x1 = _conv2d(dim_in, dim_out, 1, 1, 0, bias=False)

    def _act(self, x, norm):
        return _AffineNormActFn.apply(x, norm.weight, norm.bias) if self.normalize else _LReluFn.apply(x)

    def forward_nhwc(self, x):
        if self.downsample and (x.shape[1] % 2 or x.shape[2] % 2):
            raise ValueError("ResBlk(downsample=True) needs even H and W, got %d x %d" % (x.shape[1], x.shape[2]))
        r = _conv(self._act(x, getattr(self, "norm1", None)), self.conv1)
        if self.downsample:
            r = _PoolFn.apply(r)
        r = _conv(self._act(r, getattr(self, "norm2", None)), self.conv2)
        if self.learned_sc:  # the 1x1 conv commutes with the pooling: pool first, a quarter of the pixels
            sc = _conv(_PoolFn.apply(x) if self.downsample else x, self.conv1x1)
            return _MergeFn.apply(r, sc, "same")
        return _MergeFn.apply(r, x, "pool" if self.downsample else "same")


class AdaIN(nn.Module):
    """core/model.py:67-77: (1 + gamma) * InstanceNorm2d(x) + beta, {gamma, beta} = fc(s).chunk(2, 1).  ``norm`` is
    the stateless InstanceNorm2d(affine=False).  Applied with the LeakyReLU that follows it in AdainResBlk."""

    def __init__(self, style_dim, num_features):
        super().__init__()
        _check_c4(style_dim, num_features)
        self.norm = _Marker("InstanceNorm2d(%d, affine=False)" % num_features)
        self.fc = Linear(style_dim, num_features * 2)

    def forward_act_nhwc(self, x, s):
        return _AdaINActFn.apply(x, _linear(s, self.fc).contiguous())


class AdainResBlk(nn.Module):
    """core/model.py:80-120 with w_hpf = 0."""

    def __init__(self, dim_in, dim_out, style_dim=64, w_hpf=0, actv=None, upsample=False):
        super().__init__()
        if w_hpf != 0:
            raise NotImplementedError("w_hpf > 0 (HighPass / FAN masks) is not on the HIP path")
        _check_c4(dim_in, dim_out)
        self.w_hpf, self.upsample = w_hpf, upsample
        self.actv = _Marker("LeakyReLU(0.2)")
        self.learned_sc = dim_in != dim_out
        self.conv1 = _conv2d(dim_in, dim_out, 3, 1, 1)
        self.conv2 = _conv2d(dim_out, dim_out, 3, 1, 1)
        self.norm1 = AdaIN(style_dim, dim_in)
        self.norm2 = AdaIN(style_dim, dim_out)
        if self.learned_sc:
            self.conv1x1 = _conv2d(dim_in, dim_out, 1, 1, 0, bias=False)

    def forward_nhwc(self, x, s):
        r = self.norm1.forward_act_nhwc(x, s)
        if self.upsample:
            r = _Up2Fn.apply(r)
        r = _conv(r, self.conv1)
        r = _conv(self.norm2.forward_act_nhwc(r, s), self.conv2)
        # the 1x1 conv commutes with nearest upsampling: conv at the low resolution, upsample in the merge
        sc = _conv(x, self.conv1x1) if self.learned_sc else x
        return _MergeFn.apply(r, sc, "up" if self.upsample else "same")


def _style(s, style_dim, B):
    if s.dim() != 2 or s.shape[0] != B or s.shape[1] != style_dim:
        raise ValueError("style code must be [%d, %d], got %s" % (B, style_dim, tuple(s.shape)))
    return s.float().contiguous()


# ---------------------------------------------------------------------------------------------------- networks
class Generator(nn.Module):
    """core/model.py:135-186 with w_hpf = 0: from_rgb, log2(img_size) - 4 down / up levels and two bottleneck
    blocks each way, to_rgb (IN(affine) + LeakyReLU + 1x1 conv).  Fully convolutional: H and W need only be
    multiples of 2^levels.  forward(x, s) -> NCHW image."""

    def __init__(self, img_size=256, style_dim=64, max_conv_dim=512, w_hpf=0):
        super().__init__()
        if w_hpf != 0:
            raise NotImplementedError("w_hpf > 0 (HighPass / FAN masks) is not on the HIP path; the reference "
                                      "default is w_hpf = 0")
        dim_in = 2 ** 14 // img_size
        self.img_size, self.style_dim = img_size, style_dim
        self.from_rgb = _conv2d(3, dim_in, 3, 1, 1)
        self.encode = nn.ModuleList()
        self.decode = nn.ModuleList()
        self.to_rgb = nn.Sequential(InstanceNormAffine(dim_in), _Marker("LeakyReLU(0.2)"), _conv2d(dim_in, 3, 1, 1, 0))
        self.levels = int(math.log2(img_size)) - 4
        dim_out = dim_in
        for _ in range(self.levels):
            dim_out = min(dim_in * 2, max_conv_dim)
            self.encode.append(ResBlk(dim_in, dim_out, normalize=True, downsample=True))
            self.decode.insert(0, AdainResBlk(dim_out, dim_in, style_dim, w_hpf=w_hpf, upsample=True))
            dim_in = dim_out
        for _ in range(2):
            self.encode.append(ResBlk(dim_out, dim_out, normalize=True))
            self.decode.insert(0, AdainResBlk(dim_out, dim_out, style_dim, w_hpf=w_hpf))

    def _check(self, H, W, s, B):
        m = 2 ** self.levels
        if H % m or W % m:
            raise ValueError("Generator with %d downsamplings needs H and W to be multiples of %d, got %d x %d"
                             % (self.levels, m, H, W))
        return _style(s, self.style_dim, B)

    def forward_nhwc(self, x, s):
        s = self._check(x.shape[1], x.shape[2], s, x.shape[0])
        h = _conv(x, self.from_rgb)
        for blk in self.encode:
            h = blk.forward_nhwc(h)
        for blk in self.decode:
            h = blk.forward_nhwc(h, s)
        norm = self.to_rgb[0]
        return _conv(_AffineNormActFn.apply(h, norm.weight, norm.bias), self.to_rgb[2])

    def forward(self, x, s, masks=None):
        if masks is not None:
            raise NotImplementedError("masks (the w_hpf > 0 path) are not on the HIP path")
        self._check(x.shape[2], x.shape[3], s, x.shape[0])
        return _ToNCHW.apply(self.forward_nhwc(_ToNHWC.apply(x.float(), 4), s), 3)


def _gather_domain(out, y):
    """out [B, D, ...] -> out[b, y[b]]: plain indexing, so the heads of the domains not selected get dense zero
    gradients (as the reference's ``out[idx, y]``)."""
    idx = torch.arange(y.shape[0], device=out.device)
    return out[idx, y.to(out.device).long()]


class MappingNetwork(nn.Module):
    """core/model.py:189-218: four shared Linear + ReLU, then per domain three Linear + ReLU and a Linear to the
    style code; forward(z, y) -> s [B, style_dim], row b from domain y[b]."""

    def __init__(self, latent_dim=16, style_dim=64, num_domains=2):
        super().__init__()
        _check_c4(latent_dim)
        self.latent_dim, self.style_dim, self.num_domains = latent_dim, style_dim, num_domains
        layers = [Linear(latent_dim, 512), _Marker("ReLU")]
        for _ in range(3):
            layers += [Linear(512, 512), _Marker("ReLU")]
        self.shared = nn.Sequential(*layers)
        self.unshared = nn.ModuleList()
        for _ in range(num_domains):
            self.unshared.append(nn.Sequential(Linear(512, 512), _Marker("ReLU"), Linear(512, 512), _Marker("ReLU"),
                                               Linear(512, 512), _Marker("ReLU"), Linear(512, style_dim)))

    def forward(self, z, y):
        if z.dim() != 2 or z.shape[1] != self.latent_dim:
            raise ValueError("latent code must be [B, %d], got %s" % (self.latent_dim, tuple(z.shape)))
        h = z.float().contiguous()
        for i in (0, 2, 4, 6):
            h = _linear(h, self.shared[i], "relu")
        out = []
        for seq in self.unshared:
            t = h
            for i in (0, 2, 4):
                t = _linear(t, seq[i], "relu")
            out.append(_linear(t, seq[6]))
        return _gather_domain(torch.stack(out, dim=1), y)


def _trunk(img_size, max_conv_dim):
    """The shared trunk of the style encoder and the discriminator (core/model.py:224-236, :258-270): 3x3 conv,
    log2(img_size) - 2 downsampling ResBlks, LeakyReLU, 4x4 valid conv, LeakyReLU.  Returns (modules, dim_out)."""
    dim_in = 2 ** 14 // img_size
    blocks = [_conv2d(3, dim_in, 3, 1, 1)]
    dim_out = dim_in
    for _ in range(int(math.log2(img_size)) - 2):
        dim_out = min(dim_in * 2, max_conv_dim)
        blocks.append(ResBlk(dim_in, dim_out, downsample=True))
        dim_in = dim_out
    blocks += [_Marker("LeakyReLU(0.2)"), _conv2d(dim_out, dim_out, 4, 1, 0), _Marker("LeakyReLU(0.2)")]
    return blocks, dim_out


def _check_trunk_input(img_size, shape, ax):
    """shape[ax], shape[ax + 1]: the image's height and width."""
    if len(shape) != 4 or shape[ax] != img_size or shape[ax + 1] != img_size:
        raise ValueError("this network takes %d x %d images (its 4x4 conv must end at 1x1), got %s"
                         % (img_size, img_size, tuple(shape)))


def _run_trunk_nhwc(seq, n_res, x4):
    """x4 NHWC [B, img_size, img_size, 4] -> [B, dim_out] (the 4x4 conv's 1x1 output, LeakyReLU applied)."""
    h = _conv(x4, seq[0])
    for i in range(1, n_res + 1):
        h = seq[i].forward_nhwc(h)
    h = _conv(_LReluFn.apply(h), seq[n_res + 2], "lrelu")
    return h.view(h.shape[0], h.shape[-1])


def _run_trunk(seq, n_res, img_size, x):
    """x NCHW [B, 3, img_size, img_size] -> [B, dim_out]."""
    _check_trunk_input(img_size, x.shape, 2)
    return _run_trunk_nhwc(seq, n_res, _ToNHWC2.apply(x.float(), 4))


class StyleEncoder(nn.Module):
    """core/model.py:221-252: forward(x, y) -> s [B, style_dim] from the head of domain y[b]."""

    def __init__(self, img_size=256, style_dim=64, num_domains=2, max_conv_dim=512):
        super().__init__()
        blocks, dim_out = _trunk(img_size, max_conv_dim)
        self.img_size, self.n_res = img_size, len(blocks) - 4
        self.shared = nn.Sequential(*blocks)
        self.unshared = nn.ModuleList([Linear(dim_out, style_dim) for _ in range(num_domains)])

    def forward(self, x, y):
        h = _run_trunk(self.shared, self.n_res, self.img_size, x)
        return _gather_domain(torch.stack([_linear(h, layer) for layer in self.unshared], dim=1), y)


class Discriminator(nn.Module):
    """core/model.py:255-279: forward(x, y) -> logits [B], the output channel of domain y[b]."""

    def __init__(self, img_size=256, num_domains=2, max_conv_dim=512):
        super().__init__()
        blocks, dim_out = _trunk(img_size, max_conv_dim)
        self.img_size, self.n_res, self.num_domains = img_size, len(blocks) - 4, num_domains
        blocks.append(_conv2d(dim_out, num_domains, 1, 1, 0))
        self.main = nn.Sequential(*blocks)

    def head_nhwc(self, x4):
        """x4 NHWC [B, img_size, img_size, 4] -> every domain's logit [B, cpad(num_domains)] (padding columns 0):
        what vst_loss_bce_logits gathers from."""
        _check_trunk_input(self.img_size, x4.shape, 1)
        if x4.shape[3] != 4:
            raise ValueError("the NHWC image has 4 lanes (3 channels + padding), got %s" % (tuple(x4.shape),))
        h = _run_trunk_nhwc(self.main, self.n_res, x4)
        out = _conv(h.view(h.shape[0], 1, 1, h.shape[1]), self.main[self.n_res + 4])
        return out.view(out.shape[0], -1)

    def forward_nhwc(self, x4, y):
        """forward on the NHWC-4 image: the R1 penalty differentiates with respect to x4, so the image gradient
        never goes back through NCHW."""
        return _gather_domain(self.head_nhwc(x4)[:, :self.num_domains], y)

    def forward(self, x, y):
        _check_trunk_input(self.img_size, x.shape, 2)
        return self.forward_nhwc(_ToNHWC2.apply(x.float(), 4), y)


# ------------------------------------------------------------------------------------- model set, EMA, checkpoints
def build_model(args):
    """core/model.py:282-304: (nets, nets_ema) attribute dicts; the EMA set holds deep copies of the generator, the
    mapping network and the style encoder.  args: img_size, style_dim, latent_dim, num_domains, w_hpf."""
    if getattr(args, "w_hpf", 0) > 0:
        raise NotImplementedError("w_hpf > 0 (HighPass / FAN) is not on the HIP path; the reference default is 0")
    generator = Generator(args.img_size, args.style_dim, w_hpf=args.w_hpf)
    mapping_network = MappingNetwork(args.latent_dim, args.style_dim, args.num_domains)
    style_encoder = StyleEncoder(args.img_size, args.style_dim, args.num_domains)
    discriminator = Discriminator(args.img_size, args.num_domains)
    nets = _AttrDict(generator=generator, mapping_network=mapping_network, style_encoder=style_encoder,
                     discriminator=discriminator)
    nets_ema = _AttrDict(generator=copy.deepcopy(generator), mapping_network=copy.deepcopy(mapping_network),
                         style_encoder=copy.deepcopy(style_encoder))
    return nets, nets_ema


def moving_average(model, model_test, beta=0.999):
    """core/solver.py:297-299: model_test <- lerp(model, model_test, beta), parameter by parameter."""
    with torch.no_grad():
        for param, param_test in zip(model.parameters(), model_test.parameters()):
            param_test.copy_(torch.lerp(param.detach(), param_test.detach(), beta))


class CheckpointIO(object):
    """core/checkpoint.py: ``{name: state_dict}`` per registered module in one file, fname_template.format(step)
    (e.g. '{:06d}_nets_ema.ckpt')."""

    def __init__(self, fname_template, **kwargs):
        os.makedirs(os.path.dirname(fname_template) or ".", exist_ok=True)
        self.fname_template = fname_template
        self.module_dict = kwargs

    def register(self, **kwargs):
        self.module_dict.update(kwargs)

    def save(self, step):
        fname = self.fname_template.format(step)
        torch.save({name: module.state_dict() for name, module in self.module_dict.items()}, fname)
        return fname

    def load(self, step):
        fname = self.fname_template.format(step)
        assert os.path.exists(fname), fname + ' does not exist!'
        module_dict = torch.load(fname, map_location="cpu", weights_only=True)
        for name, module in self.module_dict.items():
            module.load_state_dict(module_dict[name])
        return fname


# --------------------------------------------------------------------------------------- style-guided inference
class StyleGuided:
    """A generator with a fixed target style for the Sintel harness (core/solver.py:325-347):
    forward_eval(img) = nets.generator(img, s_trg) without gradients, so sintel_eval.evaluate_video and computeTCL
    take it as they take any model.  s_trg [1, style_dim] (repeated over the batch) or [B, style_dim]."""

    def __init__(self, nets, s_trg):
        self.nets, self.s_trg = nets, s_trg.detach()

    @classmethod
    def from_latent(cls, nets, z, y):
        """Latent-guided: s_trg = mapping_network(z, y)."""
        with torch.no_grad():
            return cls(nets, nets.mapping_network(z, y))

    @classmethod
    def from_reference(cls, nets, x_ref, y):
        """Reference-guided: s_trg = style_encoder(x_ref, y)."""
        with torch.no_grad():
            return cls(nets, nets.style_encoder(x_ref, y))

    @torch.no_grad()
    def forward_eval(self, img):
        s = self.s_trg
        if s.shape[0] != img.shape[0]:
            if s.shape[0] != 1:
                raise ValueError("StyleGuided: %d style codes for a batch of %d" % (s.shape[0], img.shape[0]))
            s = s.expand(img.shape[0], -1)
        return self.nets.generator(img, s.contiguous())


# --------------------------------------------------------------------- the solver's discriminator half
def he_init(module):
    """core/utils.py:41-49 on the parameter holders: kaiming-normal (fan_in, relu) weights and zero biases for every
    conv and Linear; ``net.apply(he_init)``."""
    if isinstance(module, (Conv2d, Linear)):
        nn.init.kaiming_normal_(module.weight, mode="fan_in", nonlinearity="relu")
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)


def _input_grad(out, x, grad_out):
    """d<out, grad_out>/dx with a graph (create_graph), data gradients only: no weight-gradient kernel runs."""
    _INPUT_GRAD_ONLY[0] = True
    try:
        return torch.autograd.grad(outputs=out, inputs=x, grad_outputs=grad_out, create_graph=True, retain_graph=True,
                                   only_inputs=True)[0]
    finally:
        _INPUT_GRAD_ONLY[0] = False


def adv_loss(logits, target):
    """core/solver.py:459-463: binary_cross_entropy_with_logits against the constant target, mean over all logits."""
    assert target in [1, 0]
    z = torch.nn.functional.pad(logits.float().reshape(-1, 1), (0, 3))    # one "domain" per row, padded to a float4
    return _BCEFn.apply(z, torch.zeros(z.shape[0], dtype=torch.long, device=z.device), 1, target)


def r1_reg(d_out, x_in):
    """core/solver.py:466-476: the zero-centred gradient penalty 0.5 * mean_b ||d sum(d_out) / d x_in[b]||^2 of real
    images x_in [B, C <= 3, H, W], differentiable with respect to the discriminator's weights."""
    if x_in.dim() != 4 or x_in.shape[1] > 3:
        raise NotImplementedError("r1_reg on the HIP path takes images [B, C <= 3, H, W], got %s" % (tuple(x_in.shape),))
    grad_dout = _input_grad(d_out, x_in, torch.ones_like(d_out))
    assert grad_dout.size() == x_in.size()
    return _R1Fn.apply(_ToNHWC2.apply(grad_dout, 4))


def _nhwc4(x):
    return ops.nchw_to_nhwc(x.detach().float().contiguous(), 4)


def d_losses(discriminator, x_real, y_org, x_fake, y_trg, lambda_reg):
    """The arithmetic of compute_d_loss (core/solver.py:360-382) from x_fake on:
    loss = adv_loss(D(x_real, y_org), 1) + adv_loss(D(x_fake, y_trg), 0) + lambda_reg * r1_reg(D(x_real, y_org), x_real).
    Returns (loss, attribute dict of the three detached device scalars real / fake / reg).  The images are read, never
    marked: the penalty differentiates with respect to an NHWC-4 copy of x_real, so x_real.grad stays unset and the
    image gradient never goes back through NCHW; the domain gather, the target and the mean of each adversarial term
    are one launch (vst_loss_bce_logits)."""
    D = discriminator
    dev = x_real.device
    y_org, y_trg = (y.to(dev).long().contiguous() for y in (y_org, y_trg))
    x4 = _nhwc4(x_real).requires_grad_()
    z = D.head_nhwc(x4)
    loss_real = _BCEFn.apply(z, y_org, D.num_domains, 1)
    # d sum_b z[b, y_org[b]] / d x4: the selected logits by comparison, not by index (an id outside the head selects
    # nothing here and turns the adversarial term into NaN there)
    sel = (torch.arange(z.shape[1], device=dev)[None] == y_org[:, None]).to(z.dtype)
    loss_reg = _R1Fn.apply(_input_grad(z, x4, sel).contiguous())
    loss_fake = _BCEFn.apply(D.head_nhwc(_nhwc4(x_fake)), y_trg, D.num_domains, 0)
    loss = loss_real + loss_fake + lambda_reg * loss_reg
    return loss, _AttrDict(real=loss_real.detach(), fake=loss_fake.detach(), reg=loss_reg.detach())


def compute_d_loss(nets, args, x_real, y_org, y_trg, z_trg=None, x_ref=None, masks=None):
    """core/solver.py:360-382: x_fake from the mapping network (z_trg) or the style encoder (x_ref) without gradients,
    then d_losses.  Returns (loss, attribute dict of the floats real / fake / reg) — one host sync for the three."""
    assert (z_trg is None) != (x_ref is None)
    if masks is not None:
        raise NotImplementedError("masks (the w_hpf > 0 path) are not on the HIP path")
    with torch.no_grad():
        s_trg = nets.mapping_network(z_trg, y_trg) if z_trg is not None else nets.style_encoder(x_ref, y_trg)
        x_fake = nets.generator(x_real, s_trg)
    loss, parts = d_losses(nets.discriminator, x_real, y_org, x_fake, y_trg, args.lambda_reg)
    real, fake, reg = torch.stack([parts.real, parts.fake, parts.reg]).tolist()
    return loss, _AttrDict(real=real, fake=fake, reg=reg)


class DiscriminatorTrainer:
    """The discriminator's side of Solver (core/solver.py:52-61, :167-176): its Adam and the update.  One iteration's
    D half is ``d_step(..., z_trg=z_trg)`` then ``d_step(..., x_ref=x_ref)``.  args: lr, beta1, beta2, weight_decay,
    lambda_reg."""

    def __init__(self, nets, args):
        self.nets, self.args = nets, args
        self.optimizer = torch.optim.Adam(params=nets.discriminator.parameters(), lr=args.lr,
                                          betas=[args.beta1, args.beta2], weight_decay=args.weight_decay)

    def d_step(self, x_real, y_org, y_trg, z_trg=None, x_ref=None):
        """Zero grads, compute_d_loss, backward, step; returns the loss dict.  The backward is asked for D's
        parameters alone, so nothing is spent on the gradient of the penalty's image copy."""
        loss, losses = compute_d_loss(self.nets, self.args, x_real, y_org, y_trg, z_trg=z_trg, x_ref=x_ref)
        self.optimizer.zero_grad()
        loss.backward(inputs=list(self.nets.discriminator.parameters()))
        self.optimizer.step()
        return losses
