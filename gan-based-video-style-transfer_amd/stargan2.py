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

Left to the training pull request: the solver's losses, the R1 penalty (a double backward) and the EMA loop.
``w_hpf > 0`` (HighPass / FAN) and ``masks`` are not on the HIP path and raise NotImplementedError.
"""
import copy
import math
import os

import torch
import torch.nn as nn

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


class _ConvFn(torch.autograd.Function):
    """act(conv(x, weight) + bias), zero padding; weight [Co, Ci, k, k] or a Linear's [Co, Ci] (k = 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, k, stride, pad, act):
        kc, ck, bp = _packs(mod)
        role = "fwd" if any(ctx.needs_input_grad[:3]) else "infer"
        y = ops.conv2d_fwd(x, kc, bp, cpad(weight.shape[0]), k, k, stride, pad, "zero", act=act, slope=SLOPE, role=role)
        ctx.save_for_backward(x, y if act != "none" else None)
        ctx.conf = (weight, bias is not None, ck, k, stride, pad, act)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        weight, has_bias, ck, k, stride, pad, act = ctx.conf
        gy = gy.contiguous()
        if act != "none":
            gy = ops.act_bwd(gy, y, act, SLOPE)
        co, ci = weight.shape[0], weight.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            N, H, W, C = x.shape
            dx = ops.conv2d_tfwd(gy, ck, None, H, W, C, k, k, stride, pad)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dw = torch.zeros_like(weight)
            db = torch.zeros(co, device=x.device) if has_bias else None
            ops.conv2d_wgrad(x, gy, dw, db, k, k, stride, pad, "zero", co, ci, ci * k * k, k * k, accumulate=False)
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
        return ops.act_bwd(g.contiguous(), y, "lrelu", SLOPE)


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.avgpool2(x)

    @staticmethod
    def backward(ctx, g):
        return ops.avgpool2_bwd(g.contiguous())


class _Up2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.upsample2x(x)

    @staticmethod
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
        ga, gb = ops.merge_bwd(g.contiguous(), ctx.mode, RSQRT2)
        return ga, gb, None


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


def _run_trunk(seq, n_res, img_size, x):
    """x NCHW [B, 3, img_size, img_size] -> [B, dim_out] (the 4x4 conv's 1x1 output, LeakyReLU applied)."""
    if x.dim() != 4 or x.shape[2] != img_size or x.shape[3] != img_size:
        raise ValueError("this network takes %d x %d images (its 4x4 conv must end at 1x1), got %s"
                         % (img_size, img_size, tuple(x.shape)))
    h = _conv(_ToNHWC.apply(x.float(), 4), seq[0])
    for i in range(1, n_res + 1):
        h = seq[i].forward_nhwc(h)
    h = _conv(_LReluFn.apply(h), seq[n_res + 2], "lrelu")
    return h.view(h.shape[0], h.shape[-1])


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

    def forward(self, x, y):
        h = _run_trunk(self.main, self.n_res, self.img_size, x)
        out = _conv(h.view(h.shape[0], 1, 1, h.shape[1]), self.main[self.n_res + 4])
        return _gather_domain(out.view(out.shape[0], -1)[:, :self.num_domains], y)


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
