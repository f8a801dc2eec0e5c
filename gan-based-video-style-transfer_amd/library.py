"""``torch.library`` registration of the C-ABI entries as ``vst::*`` operators (SURVEY §8b "Callers").

The module facades (networks.py, perceptual.py, flowtools.py) call libvst_hip through ctypes inside
their own autograd Functions; this module exposes the same kernels as first-class PyTorch operators,
so they are visible to ``torch.ops``, FX / ``torch.compile`` tracing (each op has a fake-tensor
implementation for shape propagation) and ``torch.library.opcheck``.  Every op takes and returns the
reference's NCHW fp32 tensors — the semantics of the PyTorch call it replaces — and converts to the
library's NHWC layout on the device.  Backward passes are themselves ``vst::`` ops.

  vst::conv2d(x, weight, bias?, stride, padding, pad_mode)          nn.Conv2d (+ ReflectionPad2d)
        networks.py:340-367 (reflect 3x3 ResnetBlock convs), :404-426 (s2 down convs), :556-578 (D)
  vst::conv_transpose2d(x, weight, bias?, stride, padding, output_padding)   nn.ConvTranspose2d
        networks.py:408-416 (up-sampling layers)
  vst::instance_norm_act(x, act, slope)        InstanceNorm2d(affine=False) + ReLU / LeakyReLU / none
  vst::cond_instance_norm(x, sid, embed, bn_weight, bn_bias, act)   learning-based network.py:120-145
        ConditionalBatchNorm2d (+ ReLU); sid a device int32 [N], the embedding rows gathered by the kernel
  vst::instance_norm_skip(y, normalize, slope) GAN-based networks.py:468-535, the U-Net skip connection under its
        in-place activations: (lrelu(z), relu(z)), z = InstanceNorm2d(affine=False)(y) or y (normalize=False)
  vst::adain_act(x, h, act, slope)             StarGANv2AdvCon core/model.py:67-77 AdaIN (+ LeakyReLU); h = fc(s) [N, 2C]
        (the fc itself, like every nn.Linear of these nets, is vst::conv2d over [B, K, 1, 1])
  vst::avg_pool2(x)                            F.avg_pool2d(x, 2), core/model.py:45-55
  vst::merge(a, b, mode, scale)                core/model.py:62-64, :116-120: (a + f(b)) * scale, f = identity | pool | up
  vst::r1_penalty(grad)                        core/solver.py:473-475, the R1 penalty of an image gradient; its backward
        op is differentiable too, so create_graph runs through it
  vst::bce_logits(logits, y, target)           core/solver.py:459-463 adv_loss of logits[arange(B), y], y a device int64 [B]
  vst::warp_bilinear(x, flow)                  utils/flowtools.py:18-32 (F.grid_sample, zeros)
  vst::fbcheck(flow_fw, flow_bw)               utils/flowtools.py:34-58 (fbcCheckTorch)
  vst::temporal_loss(a, b, flow, mask, lam)    CycleGANCon cycle_gan_model.py:191-204
  vst::temporal_sqdiff(a, b, flow, mask, scale, ab_scale, i1?, i2?)   learning-based fs_huang.py:55-56,
        fs_reconet.py:61-69 (fs_lib.warp validity, optional luminance input term)
  vst::resize_bilinear(x, out_h, out_w, mult?) F.interpolate(mode='bilinear'), fs_reconet.py:57-60
  vst::ruder_stack(y_prev, img, flow, mask, scale)      learning-based fs_ruder.py:50-52, the recurrent input
  vst::ruder_temporal(w, y, mask, scale, ab_scale)      fs_ruder.py:97, the temporal loss on the last frame
  vst::gram(f)                                 learning-based fast_style_transfer.py:813-817
  vst::adam_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step)   torch.optim.Adam step

All ops require contiguous float32 CUDA tensors and raise on CPU inputs (no fallback).
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops

_ACTS = ("none", "relu", "lrelu")


def _nhwc(x):
    return ops.nchw_to_nhwc(x.contiguous())


def _bias_padded(bias, co):
    if bias is None:
        return None
    b = torch.zeros(ops.cpad(co), device=bias.device)
    b[:co] = bias.detach()
    return b


def _check_pad(pad_mode):
    if pad_mode not in ops.PAD:
        raise ValueError("vst: pad_mode must be 'zero' or 'reflect', got %r" % pad_mode)


# ----------------------------------------------------------------------------------- conv2d
@torch.library.custom_op("vst::conv2d", mutates_args=())
def conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, padding: int,
           pad_mode: str) -> Tensor:
    """y = conv2d(pad(x, padding, pad_mode), weight, bias, stride): the reference's
    [ReflectionPad2d(p)] + Conv2d(k, stride, padding=0 | p) pair as one op."""
    _check_pad(pad_mode)
    ops._dev_check(x, weight)
    Co, Ci, R, S = weight.shape
    if x.shape[1] != Ci:
        raise ValueError("vst::conv2d: x has %d channels, weight expects %d" % (x.shape[1], Ci))
    wp = ops.weight_pack(weight.detach().contiguous(), ops.PACK_FWD)
    y = ops.conv2d_fwd(_nhwc(x), wp, _bias_padded(bias, Co), ops.cpad(Co), R, S, stride, padding, pad_mode)
    return ops.nhwc_to_nchw(y, Co)


@conv2d.register_fake
def _(x, weight, bias, stride, padding, pad_mode):
    N, _, H, W = x.shape
    Co, _, R, S = weight.shape
    return x.new_empty((N, Co, (H + 2 * padding - R) // stride + 1, (W + 2 * padding - S) // stride + 1))


@torch.library.custom_op("vst::conv2d_backward", mutates_args=())
def conv2d_backward(grad: Tensor, x: Tensor, weight: Tensor, stride: int, padding: int,
                    pad_mode: str, need_input: bool = True, need_weight: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dweight, dbias) of vst::conv2d.  dx: the transposed conv (reflect, stride 1: mirrored
    contributions gathered in-kernel; reflect, stride > 1: the transposed conv onto the padded frame,
    then the reflect fold); dweight: the split-K weight-gradient GEMM; dbias: the per-channel sum of
    grad.  need_input / need_weight = False skip that GEMM (its output is returned as zeros)."""
    _check_pad(pad_mode)
    ops._dev_check(grad, x, weight)
    N, Ci, H, W = x.shape
    Co, _, R, S = weight.shape
    gy = _nhwc(grad)
    if need_input:
        ik = ops.weight_pack(weight.detach().contiguous(), ops.PACK_DGRAD)
        if pad_mode == "reflect" and stride != 1:
            dxp = ops.conv2d_tfwd(gy, ik, None, H + 2 * padding, W + 2 * padding, ops.cpad(Ci), R, S, stride, 0)
            dx = ops.nhwc_to_nchw(ops.reflect_fold(dxp, padding), Ci)
        else:
            dxn = ops.conv2d_tfwd(gy, ik, None, H, W, ops.cpad(Ci), R, S, stride, padding, pad_mode=pad_mode)
            dx = ops.nhwc_to_nchw(dxn, Ci)
    else:
        dx = torch.zeros_like(x)
    dw = torch.zeros_like(weight)
    db = torch.zeros(Co, device=x.device)
    if need_weight:
        ops.conv2d_wgrad(_nhwc(x), gy, dw, db, R, S, stride, padding, pad_mode, Co, Ci, Ci * R * S, R * S,
                         accumulate=False)
    else:
        ops.channel_sum(gy, db, Co, accumulate=False)
    return dx, dw, db


@conv2d_backward.register_fake
def _(grad, x, weight, stride, padding, pad_mode, need_input=True, need_weight=True):
    return torch.empty_like(x), torch.empty_like(weight), weight.new_empty((weight.shape[0],))


def _conv2d_setup(ctx, inputs, output):
    x, weight, bias, stride, padding, pad_mode = inputs
    ctx.save_for_backward(x, weight)
    ctx.conf = (stride, padding, pad_mode, bias is not None)


def _conv2d_bwd(ctx, grad):
    x, weight = ctx.saved_tensors
    stride, padding, pad_mode, has_bias = ctx.conf
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dx, dw, db = torch.ops.vst.conv2d_backward(grad.contiguous(), x, weight, stride, padding, pad_mode,
                                               need_x, need_w)
    return (dx if need_x else None), (dw if need_w else None), (db if has_bias else None), None, None, None


conv2d.register_autograd(_conv2d_bwd, setup_context=_conv2d_setup)


# -------------------------------------------------------------------------- conv_transpose2d
def _convT_out(n, stride, padding, k, output_padding):
    return (n - 1) * stride - 2 * padding + k + output_padding


@torch.library.custom_op("vst::conv_transpose2d", mutates_args=())
def conv_transpose2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, padding: int,
                     output_padding: int) -> Tensor:
    """nn.ConvTranspose2d(Ci, Co, k, stride, padding, output_padding) with weight [Ci][Co][k][k]:
    the gather-form transposed conv (vst_conv2d_tfwd) with the weight read as O = Ci, I = Co."""
    ops._dev_check(x, weight)
    N, Ci, H, W = x.shape
    _, Co, R, S = weight.shape
    Ho, Wo = _convT_out(H, stride, padding, R, output_padding), _convT_out(W, stride, padding, S, output_padding)
    ik = ops.weight_pack(weight.detach().contiguous(), ops.PACK_DGRAD)
    y = ops.conv2d_tfwd(_nhwc(x), ik, _bias_padded(bias, Co), Ho, Wo, ops.cpad(Co), R, S, stride, padding,
                        role="fwd")
    return ops.nhwc_to_nchw(y, Co)


@conv_transpose2d.register_fake
def _(x, weight, bias, stride, padding, output_padding):
    N, _, H, W = x.shape
    _, Co, R, S = weight.shape
    return x.new_empty((N, Co, _convT_out(H, stride, padding, R, output_padding),
                        _convT_out(W, stride, padding, S, output_padding)))


@torch.library.custom_op("vst::conv_transpose2d_backward", mutates_args=())
def conv_transpose2d_backward(grad: Tensor, x: Tensor, weight: Tensor, stride: int,
                              padding: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dweight, dbias) of vst::conv_transpose2d: dx is the forward conv of grad with the same
    weight (O = Ci, I = Co); dweight is the weight gradient of that conv with x := grad,
    dy := x (include/vst_hip.h, vst_conv2d_wgrad)."""
    ops._dev_check(grad, x, weight)
    N, Ci, H, W = x.shape
    _, Co, R, S = weight.shape
    gy = _nhwc(grad)
    ok = ops.weight_pack(weight.detach().contiguous(), ops.PACK_FWD)
    dx = ops.conv2d_fwd(gy, ok, None, ops.cpad(Ci), R, S, stride, padding, role="bwd")
    if dx.shape[1] != H or dx.shape[2] != W:
        raise ValueError("vst::conv_transpose2d_backward: inconsistent output_padding")
    dw = torch.zeros_like(weight)
    ops.conv2d_wgrad(gy, _nhwc(x), dw, None, R, S, stride, padding, "zero", Ci, Co, Co * R * S, R * S,
                     accumulate=False)
    db = torch.zeros(Co, device=x.device)
    ops.channel_sum(gy, db, Co, accumulate=False)
    return ops.nhwc_to_nchw(dx, Ci), dw, db


@conv_transpose2d_backward.register_fake
def _(grad, x, weight, stride, padding):
    return torch.empty_like(x), torch.empty_like(weight), weight.new_empty((weight.shape[1],))


def _convT_setup(ctx, inputs, output):
    x, weight, bias, stride, padding, _ = inputs
    ctx.save_for_backward(x, weight)
    ctx.conf = (stride, padding, bias is not None)


def _convT_bwd(ctx, grad):
    x, weight = ctx.saved_tensors
    stride, padding, has_bias = ctx.conf
    dx, dw, db = torch.ops.vst.conv_transpose2d_backward(grad.contiguous(), x, weight, stride, padding)
    return dx, dw, (db if has_bias else None), None, None, None


conv_transpose2d.register_autograd(_convT_bwd, setup_context=_convT_setup)


# ------------------------------------------------------------------------ instance_norm_act
@torch.library.custom_op("vst::instance_norm_act", mutates_args=())
def instance_norm_act(x: Tensor, act: str, slope: float) -> Tensor:
    """act(InstanceNorm2d(affine=False, eps=1e-5)(x)); act in none | relu | lrelu (fp64 statistics)."""
    if act not in _ACTS:
        raise ValueError("vst::instance_norm_act: act must be one of %s" % (_ACTS,))
    C = x.shape[1]
    y = _nhwc(x)
    a = ops.instnorm_act_fwd(y, ops.instnorm_stats(y), act, slope)
    return ops.nhwc_to_nchw(a, C)


@instance_norm_act.register_fake
def _(x, act, slope):
    return torch.empty_like(x)


@torch.library.custom_op("vst::instance_norm_act_backward", mutates_args=())
def instance_norm_act_backward(grad: Tensor, x: Tensor, act: str, slope: float) -> Tensor:
    C = x.shape[1]
    y = _nhwc(x)
    dy = ops.instnorm_act_bwd(_nhwc(grad), y, ops.instnorm_stats(y), act, slope)
    return ops.nhwc_to_nchw(dy, C)


@instance_norm_act_backward.register_fake
def _(grad, x, act, slope):
    return torch.empty_like(x)


def _in_setup(ctx, inputs, output):
    x, act, slope = inputs
    ctx.save_for_backward(x)
    ctx.conf = (act, slope)


def _in_bwd(ctx, grad):
    (x,) = ctx.saved_tensors
    return torch.ops.vst.instance_norm_act_backward(grad.contiguous(), x, *ctx.conf), None, None


instance_norm_act.register_autograd(_in_bwd, setup_context=_in_setup)


# ------------------------------------------------------------------------ cond_instance_norm
def _cond_args(x, sid, embed, bn_weight, bn_bias, act):
    if act not in ("none", "relu"):
        raise ValueError("vst::cond_instance_norm: act must be 'none' or 'relu'")
    ops._dev_check(x, embed, bn_weight, bn_bias)
    C = x.shape[1]
    if bn_weight.numel() != C or bn_bias.numel() != C or tuple(embed.shape[1:]) != (2 * C,):
        raise ValueError("vst::cond_instance_norm: bn_weight / bn_bias [C] and embed [S, 2*C] for x [N, C, H, W]")
    y = _nhwc(x)
    return y, ops.instnorm_stats(y), embed.detach().contiguous(), bn_weight.detach().contiguous(), \
        bn_bias.detach().contiguous()


@torch.library.custom_op("vst::cond_instance_norm", mutates_args=())
def cond_instance_norm(x: Tensor, sid: Tensor, embed: Tensor, bn_weight: Tensor, bn_bias: Tensor,
                       act: str) -> Tensor:
    """network.py:120-145 ConditionalBatchNorm2d (+ ReLU): act(ge * InstanceNorm2d(affine=True)(x) + be) with
    {ge, be} = embed[sid[n]].chunk(2); sid a device int32 [N] (one style per sample; the reference's 0-dim id is
    that id N times), embed [S, 2*C].  act in none | relu."""
    y, st, e, w, b = _cond_args(x, sid, embed, bn_weight, bn_bias, act)
    return ops.nhwc_to_nchw(ops.cond_instnorm_fwd(y, st, sid, e, w, b, act), x.shape[1])


@cond_instance_norm.register_fake
def _(x, sid, embed, bn_weight, bn_bias, act):
    return torch.empty_like(x)


@torch.library.custom_op("vst::cond_instance_norm_backward", mutates_args=())
def cond_instance_norm_backward(grad: Tensor, x: Tensor, sid: Tensor, embed: Tensor, bn_weight: Tensor,
                                bn_bias: Tensor, act: str) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dx, dembed, dbn_weight, dbn_bias) of vst::cond_instance_norm; dembed is dense: rows of styles absent
    from sid are zero."""
    y, st, e, w, b = _cond_args(x, sid, embed, bn_weight, bn_bias, act)
    de, dw, db = torch.empty_like(e), torch.empty_like(w), torch.empty_like(b)
    dx = ops.cond_instnorm_bwd(_nhwc(grad), y, st, sid, e, w, b, act, dembed=de, dbn_w=dw, dbn_b=db,
                               accumulate=False)
    return ops.nhwc_to_nchw(dx, x.shape[1]), de, dw, db


@cond_instance_norm_backward.register_fake
def _(grad, x, sid, embed, bn_weight, bn_bias, act):
    return torch.empty_like(x), torch.empty_like(embed), torch.empty_like(bn_weight), torch.empty_like(bn_bias)


def _cin_setup(ctx, inputs, output):
    x, sid, embed, bn_weight, bn_bias, act = inputs
    ctx.save_for_backward(x, sid, embed, bn_weight, bn_bias)
    ctx.act = act


def _cin_bwd(ctx, grad):
    x, sid, embed, bn_weight, bn_bias = ctx.saved_tensors
    dx, de, dw, db = torch.ops.vst.cond_instance_norm_backward(grad.contiguous(), x, sid, embed, bn_weight, bn_bias,
                                                               ctx.act)
    return dx, None, de, dw, db, None


cond_instance_norm.register_autograd(_cin_bwd, setup_context=_cin_setup)


# ------------------------------------------------------------------------ instance_norm_skip
@torch.library.custom_op("vst::instance_norm_skip", mutates_args=())
def instance_norm_skip(y: Tensor, normalize: bool, slope: float) -> Tuple[Tensor, Tensor]:
    """networks.py:468-535 UnetSkipConnectionBlock's skip connection as its readers see it: with z =
    InstanceNorm2d(affine=False, eps=1e-5)(y) (normalize=False: z = y), returns (d, skip) = (LeakyReLU(slope)(z) —
    the child's in-place activation, the next down conv's input —, ReLU(z) — the skip half of the concatenation
    after the parent's in-place ReLU).  One pass over y (vst_instnorm_skip_fwd)."""
    ops._dev_check(y)
    C = y.shape[1]
    yn = _nhwc(y)
    skip = torch.empty_like(yn)
    d = ops.instnorm_skip_fwd(yn, ops.instnorm_stats(yn) if normalize else None, skip, 0, slope=slope)
    return ops.nhwc_to_nchw(d, C), ops.nhwc_to_nchw(skip, C)


@instance_norm_skip.register_fake
def _(y, normalize, slope):
    return torch.empty_like(y), torch.empty_like(y)


@torch.library.custom_op("vst::instance_norm_skip_backward", mutates_args=())
def instance_norm_skip_backward(g_d: Tensor, g_skip: Tensor, y: Tensor, normalize: bool, slope: float) -> Tensor:
    """dy of vst::instance_norm_skip from both output gradients: g = g_d * lrelu'(z) + g_skip * relu'(z), then the
    InstanceNorm backward (vst_instnorm_skip_bwd)."""
    ops._dev_check(g_d, g_skip, y)
    yn = _nhwc(y)
    dy = ops.instnorm_skip_bwd(_nhwc(g_d), _nhwc(g_skip), 0, yn, ops.instnorm_stats(yn) if normalize else None,
                               slope=slope)
    return ops.nhwc_to_nchw(dy, y.shape[1])


@instance_norm_skip_backward.register_fake
def _(g_d, g_skip, y, normalize, slope):
    return torch.empty_like(y)


def _ins_setup(ctx, inputs, output):
    y, normalize, slope = inputs
    ctx.save_for_backward(y)
    ctx.conf = (normalize, slope)


def _ins_bwd(ctx, g_d, g_skip):
    (y,) = ctx.saved_tensors
    return torch.ops.vst.instance_norm_skip_backward(g_d.contiguous(), g_skip.contiguous(), y, *ctx.conf), None, None


instance_norm_skip.register_autograd(_ins_bwd, setup_context=_ins_setup)


# ---------------------------------------------------------------------------------- adain_act
def _adain_args(x, h, act):
    if act not in ("none", "lrelu"):
        raise ValueError("vst::adain_act: act must be 'none' or 'lrelu'")
    ops._dev_check(x, h)
    if h.dim() != 2 or h.shape[0] != x.shape[0] or h.shape[1] != 2 * x.shape[1] or x.shape[1] % 4:
        raise ValueError("vst::adain_act: h [N, 2*C] for x [N, C, H, W] with C %% 4 == 0, got %s and %s"
                         % (tuple(h.shape), tuple(x.shape)))
    y = _nhwc(x)
    return y, ops.instnorm_stats(y), h.detach().contiguous()


@torch.library.custom_op("vst::adain_act", mutates_args=())
def adain_act(x: Tensor, h: Tensor, act: str, slope: float) -> Tensor:
    """StarGAN v2 core/model.py:67-77 AdaIN (+ LeakyReLU): act((1 + gamma) * InstanceNorm2d(x) + beta) with
    {gamma, beta} = h.chunk(2, 1), h [N, 2*C] the style projection fc(s).  act in none | lrelu."""
    y, st, hh = _adain_args(x, h, act)
    return ops.nhwc_to_nchw(ops.adain_fwd(y, st, hh, act, slope), x.shape[1])


@adain_act.register_fake
def _(x, h, act, slope):
    return torch.empty_like(x)


@torch.library.custom_op("vst::adain_act_backward", mutates_args=())
def adain_act_backward(grad: Tensor, x: Tensor, h: Tensor, act: str, slope: float) -> Tuple[Tensor, Tensor]:
    """(dx, dh) of vst::adain_act."""
    y, st, hh = _adain_args(x, h, act)
    dh = torch.empty_like(hh)
    dx = ops.adain_bwd(_nhwc(grad), y, st, hh, act, slope, dh=dh)
    return ops.nhwc_to_nchw(dx, x.shape[1]), dh


@adain_act_backward.register_fake
def _(grad, x, h, act, slope):
    return torch.empty_like(x), torch.empty_like(h)


def _adain_setup(ctx, inputs, output):
    x, h, act, slope = inputs
    ctx.save_for_backward(x, h)
    ctx.conf = (act, slope)


def _adain_bwd(ctx, grad):
    x, h = ctx.saved_tensors
    dx, dh = torch.ops.vst.adain_act_backward(grad.contiguous(), x, h, *ctx.conf)
    return dx, dh, None, None


adain_act.register_autograd(_adain_bwd, setup_context=_adain_setup)


# ------------------------------------------------------------------------- avg_pool2 / merge
def _c4(x, what):
    ops._dev_check(x)
    if x.dim() != 4 or x.shape[1] % 4:
        raise ValueError("vst::%s: [N, C, H, W] with C %% 4 == 0, got %s" % (what, tuple(x.shape)))


@torch.library.custom_op("vst::avg_pool2", mutates_args=())
def avg_pool2(x: Tensor) -> Tensor:
    """F.avg_pool2d(x, 2) of [N, C, H, W] with even H and W (core/model.py:45-55)."""
    _c4(x, "avg_pool2")
    return ops.nhwc_to_nchw(ops.avgpool2(_nhwc(x)), x.shape[1])


@avg_pool2.register_fake
def _(x):
    return x.new_empty((x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))


@torch.library.custom_op("vst::avg_pool2_backward", mutates_args=())
def avg_pool2_backward(grad: Tensor) -> Tensor:
    _c4(grad, "avg_pool2_backward")
    return ops.nhwc_to_nchw(ops.avgpool2_bwd(_nhwc(grad)), grad.shape[1])


@avg_pool2_backward.register_fake
def _(grad):
    return grad.new_empty((grad.shape[0], grad.shape[1], 2 * grad.shape[2], 2 * grad.shape[3]))


def _ap_bwd(ctx, grad):
    return torch.ops.vst.avg_pool2_backward(grad.contiguous())


avg_pool2.register_autograd(_ap_bwd, setup_context=lambda ctx, inputs, output: None)


def _merge_b_nchw(shape, mode):
    N, C, H, W = shape
    if mode not in ops.MERGE:
        raise ValueError("vst::merge: mode must be one of %s" % sorted(ops.MERGE))
    return {"same": (N, C, H, W), "pool": (N, C, 2 * H, 2 * W), "up": (N, C, H // 2, W // 2)}[mode]


@torch.library.custom_op("vst::merge", mutates_args=())
def merge(a: Tensor, b: Tensor, mode: str, scale: float) -> Tensor:
    """(a + f(b)) * scale: the residual merge of ResBlk / AdainResBlk (core/model.py:62-64, :116-120) with the
    shortcut's resampling folded in; mode 'same' (f = identity), 'pool' (f = avg_pool2d(., 2), b at twice a's
    resolution) or 'up' (f = nearest 2x upsampling, b at half a's resolution)."""
    _c4(a, "merge")
    _c4(b, "merge")
    if tuple(b.shape) != _merge_b_nchw(a.shape, mode):
        raise ValueError("vst::merge %r: a %s and b %s do not fit" % (mode, tuple(a.shape), tuple(b.shape)))
    return ops.nhwc_to_nchw(ops.merge(_nhwc(a), _nhwc(b), mode, scale), a.shape[1])


@merge.register_fake
def _(a, b, mode, scale):
    return torch.empty_like(a)


@torch.library.custom_op("vst::merge_backward", mutates_args=())
def merge_backward(grad: Tensor, mode: str, scale: float) -> Tuple[Tensor, Tensor]:
    """(da, db) of vst::merge from one pass over grad."""
    _c4(grad, "merge_backward")
    ga, gb = ops.merge_bwd(_nhwc(grad), mode, scale)
    return ops.nhwc_to_nchw(ga, grad.shape[1]), ops.nhwc_to_nchw(gb, grad.shape[1])


@merge_backward.register_fake
def _(grad, mode, scale):
    return torch.empty_like(grad), grad.new_empty(_merge_b_nchw(grad.shape, mode))


def _merge_setup(ctx, inputs, output):
    ctx.conf = (inputs[2], inputs[3])


def _merge_bwd(ctx, grad):
    ga, gb = torch.ops.vst.merge_backward(grad.contiguous(), *ctx.conf)
    return ga, gb, None, None


merge.register_autograd(_merge_bwd, setup_context=_merge_setup)


# ------------------------------------------------------------------- r1_penalty / bce_logits
def _img_grad(g, what):
    ops._dev_check(g)
    if g.dim() != 4 or g.shape[1] > 3:
        raise ValueError("vst::%s: an image gradient [B, C <= 3, H, W], got %s" % (what, tuple(g.shape)))


@torch.library.custom_op("vst::r1_penalty", mutates_args=())
def r1_penalty(grad: Tensor) -> Tensor:
    """0.5 * grad.pow(2).view(B, -1).sum(1).mean(0) of the image gradient [B, 3, H, W] (core/solver.py:473-475)."""
    _img_grad(grad, "r1_penalty")
    return ops.r1(ops.nchw_to_nhwc(grad.contiguous(), 4))


@r1_penalty.register_fake
def _(grad):
    return grad.new_empty(())


@torch.library.custom_op("vst::r1_penalty_backward", mutates_args=())
def r1_penalty_backward(gout: Tensor, grad: Tensor) -> Tensor:
    """gout * grad / B: the gradient of vst::r1_penalty, linear in grad."""
    _img_grad(grad, "r1_penalty_backward")
    return ops.nhwc_to_nchw(ops.r1_bwd(ops.nchw_to_nhwc(grad.contiguous(), 4), gout.contiguous()), grad.shape[1])


@r1_penalty_backward.register_fake
def _(gout, grad):
    return torch.empty_like(grad)


def _r1_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _r1_bwd(ctx, gout):
    return torch.ops.vst.r1_penalty_backward(gout, ctx.saved_tensors[0])


def _r1b_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _r1b_bwd(ctx, ggu):
    """The double backward: d/d grad is the same kernel applied to ggu; d/d gout = <ggu, grad> / B."""
    gout, grad = ctx.saved_tensors
    d_gout = (ggu * grad).sum() / grad.shape[0] if ctx.needs_input_grad[0] else None
    d_grad = torch.ops.vst.r1_penalty_backward(gout, ggu.contiguous()) if ctx.needs_input_grad[1] else None
    return d_gout, d_grad


r1_penalty.register_autograd(_r1_bwd, setup_context=_r1_setup)
r1_penalty_backward.register_autograd(_r1b_bwd, setup_context=_r1b_setup)


def _padded_logits(logits, y, what):
    ops._dev_check(logits)
    if logits.dim() != 2 or y.dim() != 1 or y.shape[0] != logits.shape[0]:
        raise ValueError("vst::%s: logits [B, num_domains] and y [B], got %s and %s"
                         % (what, tuple(logits.shape), tuple(y.shape)))
    z = logits.new_zeros((logits.shape[0], ops.cpad(logits.shape[1])))
    z[:, :logits.shape[1]] = logits
    return z, y.long().contiguous()


@torch.library.custom_op("vst::bce_logits", mutates_args=())
def bce_logits(logits: Tensor, y: Tensor, target: float) -> Tensor:
    """adv_loss(logits[arange(B), y], target) (core/solver.py:459-463), target 0 or 1."""
    z, yl = _padded_logits(logits, y, "bce_logits")
    return ops.bce_logits(z, yl, logits.shape[1], target)


@bce_logits.register_fake
def _(logits, y, target):
    return logits.new_empty(())


@torch.library.custom_op("vst::bce_logits_backward", mutates_args=())
def bce_logits_backward(gout: Tensor, logits: Tensor, y: Tensor, target: float) -> Tensor:
    z, yl = _padded_logits(logits, y, "bce_logits_backward")
    return ops.bce_logits_bwd(z, yl, logits.shape[1], target, gout.contiguous())[:, :logits.shape[1]].contiguous()


@bce_logits_backward.register_fake
def _(gout, logits, y, target):
    return torch.empty_like(logits)


def _bce_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.target = inputs[2]


def _bce_bwd(ctx, gout):
    logits, y = ctx.saved_tensors
    return torch.ops.vst.bce_logits_backward(gout, logits, y, ctx.target), None, None


bce_logits.register_autograd(_bce_bwd, setup_context=_bce_setup)


# ------------------------------------------------------------------------------------ flow
@torch.library.custom_op("vst::warp_bilinear", mutates_args=())
def warp_bilinear(x: Tensor, flow: Tensor) -> Tensor:
    """utils/flowtools.py:18-32: backward bilinear warp of x [B,C,H,W] by flow [B,2,H,W] (pixels,
    channel 0 = x displacement), zeros outside, align_corners=False."""
    ops._dev_check(flow)
    C = x.shape[1]
    return ops.nhwc_to_nchw(ops.warp_nhwc(_nhwc(x), flow.contiguous()), C)


@warp_bilinear.register_fake
def _(x, flow):
    return torch.empty_like(x)


@torch.library.custom_op("vst::warp_bilinear_backward", mutates_args=())
def warp_bilinear_backward(grad: Tensor, flow: Tensor) -> Tensor:
    """Gradient w.r.t. x of vst::warp_bilinear (the bilinear scatter; the flow gets none, as in every
    training path of the reference)."""
    C = grad.shape[1]
    return ops.nhwc_to_nchw(ops.warp_bwd_nhwc(_nhwc(grad), flow.contiguous()), C)


@warp_bilinear_backward.register_fake
def _(grad, flow):
    return torch.empty_like(grad)


def _warp_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _warp_bwd(ctx, grad):
    (flow,) = ctx.saved_tensors
    return torch.ops.vst.warp_bilinear_backward(grad.contiguous(), flow), None


warp_bilinear.register_autograd(_warp_bwd, setup_context=_warp_setup)


@torch.library.custom_op("vst::fbcheck", mutates_args=())
def fbcheck(flow_fw: Tensor, flow_bw: Tensor) -> Tensor:
    """utils/flowtools.py:34-58 fbcCheckTorch: occlusion / motion-boundary mask [B,1,H,W]."""
    return ops.fbcheck(flow_fw.contiguous(), flow_bw.contiguous())


@fbcheck.register_fake
def _(flow_fw, flow_bw):
    B, _, H, W = flow_bw.shape
    return flow_bw.new_empty((B, 1, H, W))


# ---------------------------------------------------------------------------------- losses
@torch.library.custom_op("vst::temporal_loss", mutates_args=())
def temporal_loss(a: Tensor, b: Tensor, flow: Tensor, mask: Tensor, lam: float) -> Tensor:
    """lam * mean((mask * (b - warp(a, flow)))^2) over [B,3,H,W] frames (CycleGANCon
    cycle_gan_model.py:191-204, a = fake_B, b = fake_B2)."""
    C = a.shape[1]
    return ops.loss_temporal(_nhwc(a), _nhwc(b), flow.contiguous(), mask.contiguous(), lam, cl=C)


@temporal_loss.register_fake
def _(a, b, flow, mask, lam):
    return a.new_empty(())


@torch.library.custom_op("vst::temporal_loss_backward", mutates_args=())
def temporal_loss_backward(grad: Tensor, a: Tensor, b: Tensor, flow: Tensor, mask: Tensor,
                           lam: float) -> Tuple[Tensor, Tensor]:
    C = a.shape[1]
    an, bn = _nhwc(a), _nhwc(b)
    ga, gb = torch.zeros_like(an), torch.empty_like(bn)
    ops.loss_temporal_bwd(an, bn, flow.contiguous(), mask.contiguous(), grad.contiguous(), ga, gb, lam, cl=C)
    return ops.nhwc_to_nchw(ga, C), ops.nhwc_to_nchw(gb, C)


@temporal_loss_backward.register_fake
def _(grad, a, b, flow, mask, lam):
    return torch.empty_like(a), torch.empty_like(b)


def _tl_setup(ctx, inputs, output):
    a, b, flow, mask, lam = inputs
    ctx.save_for_backward(a, b, flow, mask)
    ctx.lam = lam


def _tl_bwd(ctx, grad):
    a, b, flow, mask = ctx.saved_tensors
    ga, gb = torch.ops.vst.temporal_loss_backward(grad, a, b, flow, mask, ctx.lam)
    return ga, gb, None, None, None


temporal_loss.register_autograd(_tl_bwd, setup_context=_tl_setup)


@torch.library.custom_op("vst::temporal_sqdiff", mutates_args=())
def temporal_sqdiff(a: Tensor, b: Tensor, flow: Tensor, mask: Tensor, scale: float, ab_scale: float,
                    i1: Optional[Tensor], i2: Optional[Tensor]) -> Tensor:
    """scale * mean((mask * (s*b - fs_lib.warp(s*a, flow) - r))^2) over [B,C,H,W] a, b (C = 3 or a multiple
    of 4), s = ab_scale (fs_huang.py:55-56, fs_reconet.py:61-69).  i1, i2 (both or neither; [B,3,H,W] input
    frames, a and b then 3-channel images): r = 0.2126 d0 + 0.7152 d1 + 0.0722 d2, d = i2 - warp(i1, flow)."""
    C = a.shape[1]
    inputs = None if i1 is None else (_nhwc(i1), _nhwc(i2))
    return ops.temporal_sqdiff(_nhwc(a), _nhwc(b), flow.contiguous(), mask.contiguous(), scale, C, ab_scale, inputs)


@temporal_sqdiff.register_fake
def _(a, b, flow, mask, scale, ab_scale, i1, i2):
    return a.new_empty(())


@torch.library.custom_op("vst::temporal_sqdiff_backward", mutates_args=())
def temporal_sqdiff_backward(grad: Tensor, a: Tensor, b: Tensor, flow: Tensor, mask: Tensor, scale: float,
                             ab_scale: float, i1: Optional[Tensor], i2: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    C = a.shape[1]
    an, bn = _nhwc(a), _nhwc(b)
    inputs = None if i1 is None else (_nhwc(i1), _nhwc(i2))
    ga, gb = torch.zeros_like(an), torch.empty_like(bn)
    ops.temporal_sqdiff_bwd(an, bn, flow.contiguous(), mask.contiguous(), grad.contiguous(), ga, gb, scale, C,
                            ab_scale, inputs)
    return ops.nhwc_to_nchw(ga, C), ops.nhwc_to_nchw(gb, C)


@temporal_sqdiff_backward.register_fake
def _(grad, a, b, flow, mask, scale, ab_scale, i1, i2):
    return torch.empty_like(a), torch.empty_like(b)


def _tsq_setup(ctx, inputs, output):
    a, b, flow, mask, scale, ab_scale, i1, i2 = inputs
    ctx.save_for_backward(a, b, flow, mask, i1, i2)
    ctx.conf = (scale, ab_scale)


def _tsq_bwd(ctx, grad):
    a, b, flow, mask, i1, i2 = ctx.saved_tensors
    ga, gb = torch.ops.vst.temporal_sqdiff_backward(grad, a, b, flow, mask, *ctx.conf, i1, i2)
    return ga, gb, None, None, None, None, None, None


temporal_sqdiff.register_autograd(_tsq_bwd, setup_context=_tsq_setup)


@torch.library.custom_op("vst::resize_bilinear", mutates_args=())
def resize_bilinear(x: Tensor, out_h: int, out_w: int, mult: Optional[List[float]]) -> Tensor:
    """F.interpolate(x, size=(out_h, out_w), mode='bilinear', align_corners=False) of [B,C,H,W] planes, channel c
    times mult[c] (fs_reconet.py:57-60: the flow and mask at feature-map resolution)."""
    return ops.resize_bilinear(x.contiguous(), (out_h, out_w), mult)


@resize_bilinear.register_fake
def _(x, out_h, out_w, mult):
    return x.new_empty((x.shape[0], x.shape[1], out_h, out_w))


@torch.library.custom_op("vst::ruder_stack", mutates_args=())
def ruder_stack(y_prev: Tensor, img: Tensor, flow: Tensor, mask: Tensor, scale: float) -> Tuple[Tensor, Tensor]:
    """fs_ruder.py:50-52: (cat(img, mask, w), w) with w = fs_lib.warp(scale * y_prev, flow).  y_prev, img
    [B,3,H,W]; flow [B,2,H,W]; mask [B,1,H,W] -> ([B,7,H,W], [B,3,H,W]).  Differentiable in y_prev."""
    x, w = ops.ruder_stack(_nhwc(y_prev), _nhwc(img), flow.contiguous(), mask.contiguous(), scale)
    return ops.nhwc_to_nchw(x, 7), ops.nhwc_to_nchw(w, 3)


@ruder_stack.register_fake
def _(y_prev, img, flow, mask, scale):
    B, _, H, W = img.shape
    return img.new_empty((B, 7, H, W)), img.new_empty((B, 3, H, W))


@torch.library.custom_op("vst::ruder_stack_backward", mutates_args=())
def ruder_stack_backward(gx: Tensor, gw: Tensor, flow: Tensor, scale: float) -> Tensor:
    """d/dy_prev of vst::ruder_stack from both output gradients (gx [B,7,H,W], gw [B,3,H,W]) in one scatter."""
    B, _, H, W = flow.shape
    gy = torch.zeros((B, H, W, 4), device=flow.device, dtype=torch.float32)
    ops.ruder_stack_bwd(_nhwc(gx), _nhwc(gw), flow.contiguous(), gy, scale)
    return ops.nhwc_to_nchw(gy, 3)


@ruder_stack_backward.register_fake
def _(gx, gw, flow, scale):
    return torch.empty_like(gw)


def _rs_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[2])
    ctx.scale = inputs[4]


def _rs_bwd(ctx, gx, gw):
    (flow,) = ctx.saved_tensors
    return torch.ops.vst.ruder_stack_backward(gx.contiguous(), gw.contiguous(), flow, ctx.scale), None, None, None, None


ruder_stack.register_autograd(_rs_bwd, setup_context=_rs_setup)


@torch.library.custom_op("vst::ruder_temporal", mutates_args=())
def ruder_temporal(w: Tensor, y: Tensor, mask: Tensor, scale: float, ab_scale: float) -> Tensor:
    """fs_ruder.py:97: scale * mean((mask * (w - ab_scale * y))^2) over [B,3,H,W] w (the warped previous frame)
    and y (the styled frame, 0..255); mask [B,1,H,W]."""
    return ops.ruder_temporal(_nhwc(w), _nhwc(y), mask.contiguous(), scale, ab_scale)


@ruder_temporal.register_fake
def _(w, y, mask, scale, ab_scale):
    return w.new_empty(())


@torch.library.custom_op("vst::ruder_temporal_backward", mutates_args=())
def ruder_temporal_backward(grad: Tensor, w: Tensor, y: Tensor, mask: Tensor, scale: float,
                            ab_scale: float) -> Tuple[Tensor, Tensor]:
    gw, gy = ops.ruder_temporal_bwd(_nhwc(w), _nhwc(y), mask.contiguous(), grad.contiguous(), scale, ab_scale)
    return ops.nhwc_to_nchw(gw, 3), ops.nhwc_to_nchw(gy, 3)


@ruder_temporal_backward.register_fake
def _(grad, w, y, mask, scale, ab_scale):
    return torch.empty_like(w), torch.empty_like(y)


def _rt_setup(ctx, inputs, output):
    w, y, mask, scale, ab_scale = inputs
    ctx.save_for_backward(w, y, mask)
    ctx.conf = (scale, ab_scale)


def _rt_bwd(ctx, grad):
    w, y, mask = ctx.saved_tensors
    gw, gy = torch.ops.vst.ruder_temporal_backward(grad, w, y, mask, *ctx.conf)
    return gw, gy, None, None, None


ruder_temporal.register_autograd(_rt_bwd, setup_context=_rt_setup)


@torch.library.custom_op("vst::gram", mutates_args=())
def gram(f: Tensor) -> Tensor:
    """fast_style_transfer.py:813-817 gram_matrix of [B,C,H,W] features: bmm(F, F^T) / (h*w) per
    sample (C % 4 == 0), on the split-K weight-gradient GEMM (ops.gram)."""
    if f.shape[1] % 4:
        raise NotImplementedError("vst::gram: channel count must be a multiple of 4")
    return ops.gram(_nhwc(f))


@gram.register_fake
def _(f):
    B, C = f.shape[0], f.shape[1]
    return f.new_empty((B, C, C))


@torch.library.custom_op("vst::gram_backward", mutates_args=())
def gram_backward(grad: Tensor, f: Tensor) -> Tensor:
    """dF_b = (dG_b + dG_b^T) F_b / (h*w) (ops.gram_bwd: a 1x1 conv with the symmetrised weight)."""
    return ops.nhwc_to_nchw(ops.gram_bwd(_nhwc(f), grad.contiguous()), f.shape[1])


@gram_backward.register_fake
def _(grad, f):
    return torch.empty_like(f)


def _gram_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _gram_bwd(ctx, grad):
    (f,) = ctx.saved_tensors
    return torch.ops.vst.gram_backward(grad.contiguous(), f)


gram.register_autograd(_gram_bwd, setup_context=_gram_setup)


# ----------------------------------------------------------------------------------- Adam
@torch.library.custom_op("vst::adam_", mutates_args=("param", "exp_avg", "exp_avg_sq"))
def adam_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
          beta2: float, eps: float, step: int) -> None:
    """One torch.optim.Adam step (weight_decay 0, amsgrad off, bias-corrected) over flat fp32
    buffers, in place (adam_k)."""
    ops.adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step)


@adam_.register_fake
def _(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    return None


OPS: List[str] = ["conv2d", "conv2d_backward", "conv_transpose2d", "conv_transpose2d_backward",
                  "instance_norm_act", "instance_norm_act_backward", "warp_bilinear", "warp_bilinear_backward",
                  "fbcheck", "temporal_loss", "temporal_loss_backward", "temporal_sqdiff", "temporal_sqdiff_backward",
                  "resize_bilinear", "gram", "gram_backward", "adam_", "ruder_stack", "ruder_stack_backward",
                  "ruder_temporal", "ruder_temporal_backward", "cond_instance_norm", "cond_instance_norm_backward",
                  "instance_norm_skip", "instance_norm_skip_backward", "adain_act", "adain_act_backward",
                  "avg_pool2", "avg_pool2_backward", "merge", "merge_backward", "r1_penalty", "r1_penalty_backward",
                  "bce_logits", "bce_logits_backward"]
