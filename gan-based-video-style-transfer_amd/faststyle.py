"""Johnson fast-style transformer net and its perceptual-loss train step, HIP-backed.

Drop-in for methods/learning-based/network.py:80-298 (``FastStyleNet`` with ``ConvLayer``,
``ConvInstRelu``, ``UpsampleConvInstRelu``, ``ResidualBlock``, ``ConvTanh``; identical module tree
and state_dict keys, ``SelectiveLoadModule`` loading) and fs_johnson.py:5-52 (``Johnson`` train /
infer methods) on top of fast_style_transfer.py's loss helpers (perceptual.py).

MI355X design: the whole net is one autograd node over NHWC fp32 tensors —
  * reflect-padded convs (9x9, 3x3 s2, 3x3) on the implicit-GEMM MFMA kernels with the padding
    folded into the operand gather; stride-2 reflect data-gradients go through a padded buffer and
    the reflect-fold kernel;
  * affine InstanceNorm (+ReLU) with fp64 statistics, and the ResidualBlock's ``layer_strength``
    gate 2|s*l|/(1+|s*l|) and residual add fused into the normalise pass (gate gradient reduced in
    the same backward pass);
  * nearest 2x upsampling materialised by a streaming kernel (its backward sums 2x2 blocks);
  * ConvTanh's tanh(x/255)*150+127.5 as a streaming epilogue kernel.
``FastStyleNet`` is the single-style net (``n_styles == 1``, plain InstanceNorm2d(affine=True)).  The
reference's multi-style ``FastStyleNet(num_inp, n_styles > 1)`` is ``MultiStyleNet``: conv1..3 and
deconv1..2 carry the conditional norm (an embedding row per style scaling and shifting the affine
InstanceNorm, network.py:120-145), applied by the vst_cond_instnorm_* kernels from device-resident
style ids; ``make_net`` picks between the two, ``Dumoulin`` is its train step (fs_dumoulin.py).
"""
import torch
import torch.nn as nn

from . import fs_lib, ops, perceptual
from .networks import Conv2d, FlatNet, _Marker, _ToNCHW, _ToNHWC, _pad_channels, _padded_bias
from .ops import cpad
from .optim import FusedAdam

# The 3x3 stride-1 data gradients (residual blocks, upsampling convs) as forward convs over the rotated taps on the
# split-bf16 kernel with the reflect border GEMM (ops.conv2d_dgrad_s1, the generator's route) instead of the
# transposed conv on the fp32-operand kernel; False keeps the latter
FS_DGRAD_FPROP = True
# The 9x9 32 -> 3 output layer on the tap routes of the generator's 7x7 output layer: forward as the 1x1 conv into
# (tap, co) channels + the tap sum (ops.tap_conv_fwd), weight gradient as the swapped GEMM (tap_conv_wgrad_swap),
# data gradient as the forward conv of the 8-channel-padded dy over the rotated taps + reflect fold; instead of the
# VALU skinny kernels and the fp32-operand transposed conv.  False keeps those.
FS_TAP = True
# The loss network's two forwards (styled image, content image) as one batch (perceptual._VggMultiFn);
# False: two calls
VGG_BATCHED = True


class InstanceNormAffine(nn.Module):
    """Parameter holder with nn.InstanceNorm2d(affine=True)'s state (weight=1, bias=0)."""

    def __init__(self, c):
        super().__init__()
        self.num_features = c
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))

    def extra_repr(self):
        return f"{self.num_features}, eps=1e-05, affine=True"


class ConvLayer(nn.Module):
    """network.py:95-107: ReflectionPad2d(k//2) + Conv2d(stride)."""

    def __init__(self, cin, cout, kernel_size, stride, bias=True):
        super().__init__()
        k = kernel_size
        self.reflection_pad = _Marker("ReflectionPad2d(%d)" % (k // 2))
        self.conv2d = Conv2d(cin, cout, k, stride=stride, bias=bias)
        self.k, self.stride = k, stride


class ConvTanh(ConvLayer):
    """network.py:110-118: tanh(conv(x)/255)*150 + 255/2."""

    def __init__(self, cin, cout, kernel_size, stride):
        super().__init__(cin, cout, kernel_size, stride)
        self.tanh = _Marker("Tanh")


class _Embedding(nn.Module):
    """Parameter holder with nn.Embedding's state: weight [num_embeddings, embedding_dim]."""

    def __init__(self, n, dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = n, dim
        self.weight = nn.Parameter(torch.zeros(n, dim))

    def extra_repr(self):
        return f"{self.num_embeddings}, {self.embedding_dim}"


class ConditionalInstanceNorm(nn.Module):
    """network.py:120-145 ConditionalBatchNorm2d(C, S): parameter holder with children ``bn``
    (InstanceNorm2d(affine=True): weight 1, bias 0) and ``embed`` (Embedding(S, 2C): the scale half N(1, 0.02),
    the shift half 0).  Applied by vst_cond_instnorm_* (ops.cond_instnorm_fwd / _bwd)."""

    def __init__(self, c, n_styles):
        super().__init__()
        self.num_features, self.n_styles = c, n_styles
        self.bn = InstanceNormAffine(c)
        self.embed = _Embedding(n_styles, 2 * c)
        with torch.no_grad():
            self.embed.weight[:, :c].normal_(1, 0.02)


def _style_norm(cout, n_styles):
    return InstanceNormAffine(cout) if n_styles == 1 else ConditionalInstanceNorm(cout, n_styles)


class ConvInstRelu(ConvLayer):
    """network.py:146-170."""

    def __init__(self, cin, cout, kernel_size, stride, n_styles=1):
        super().__init__(cin, cout, kernel_size, stride)
        self.n_styles = n_styles
        self.instance = _style_norm(cout, n_styles)
        self.relu = _Marker("ReLU")


class UpsampleConvInstRelu(nn.Module):
    """network.py:173-217: nearest upsample x2, ReflectionPad2d(k//2), conv, IN(affine), ReLU."""

    def __init__(self, cin, cout, kernel_size, stride, upsample=None, n_styles=1):
        super().__init__()
        k = kernel_size
        if upsample not in (None, 2) or stride != 1:
            raise NotImplementedError("UpsampleConvInstRelu: upsample 2 / stride 1 only on the HIP path")
        self.upsample = upsample
        self.reflection_pad = _Marker("ReflectionPad2d(%d)" % (k // 2))
        self.conv2d = Conv2d(cin, cout, k, stride=stride)
        self.n_styles = n_styles
        self.instance = _style_norm(cout, n_styles)
        self.relu = _Marker("ReLU")
        self.k, self.stride = k, stride


class ResidualBlock(nn.Module):
    """network.py:219-261: x + strength * IN2(conv2(relu(IN1(conv1(x))))),
    strength = 2|s*layer_strength| / (1 + |s*layer_strength|)."""

    def __init__(self, cin, cout, kernel_size=3, stride=1, n_styles=1):
        super().__init__()
        self.conv1 = ConvLayer(cin, cout, kernel_size, stride)
        self.in1 = InstanceNormAffine(cout)
        self.in2 = InstanceNormAffine(cout)
        self.conv2 = ConvLayer(cout, cout, kernel_size, stride)
        self.relu = _Marker("ReLU")
        self.layer_strength = nn.Parameter(torch.tensor([1], dtype=torch.float32))


class FastStyleNet(FlatNet):
    """network.py:263-298.  forward(x, style_strength=1.0, s_id=0) -> (features, image), NCHW;
    x is the [0, 1] image (3 channels, or 7 for Ruder's stacked input: frame, mask, warped previous frame)."""

    def __init__(self, num_inp, n_styles=1):
        if n_styles != 1:
            raise NotImplementedError("FastStyleNet is the single-style net (plain InstanceNorm2d(affine=True)); "
                                      "MultiStyleNet(num_inp, n_styles) / make_net carry the conditional norm")
        self._build(num_inp, 1)

    def _build(self, num_inp, n_styles):
        FlatNet.__init__(self)
        self.input_nc, self.output_nc, self.n_styles = num_inp, 3, n_styles
        self.conv1 = ConvInstRelu(num_inp, 32, kernel_size=9, stride=1, n_styles=n_styles)
        self.conv2 = ConvInstRelu(32, 64, kernel_size=3, stride=2, n_styles=n_styles)
        self.conv3 = ConvInstRelu(64, 128, kernel_size=3, stride=2, n_styles=n_styles)
        self.res1 = ResidualBlock(128, 128, n_styles=n_styles)
        self.res2 = ResidualBlock(128, 128, n_styles=n_styles)
        self.res3 = ResidualBlock(128, 128, n_styles=n_styles)
        self.res4 = ResidualBlock(128, 128, n_styles=n_styles)
        self.res5 = ResidualBlock(128, 128, n_styles=n_styles)
        self.deconv1 = UpsampleConvInstRelu(128, 64, kernel_size=3, stride=1, upsample=2, n_styles=n_styles)
        self.deconv2 = UpsampleConvInstRelu(64, 32, kernel_size=3, stride=1, upsample=2, n_styles=n_styles)
        self.deconv3 = ConvTanh(32, 3, kernel_size=9, stride=1)
        self._init_torch_default()
        self._flatten()

    def _init_torch_default(self):
        """nn.Conv2d's default init (kaiming_uniform a=sqrt(5), bias U(+-1/sqrt(fan_in)))."""
        for m in self.modules():
            if isinstance(m, Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                nn.init.uniform_(m.bias, -1 / fan_in ** 0.5, 1 / fan_in ** 0.5)

    def load_state_dict(self, state_dict, strict=False):
        """SelectiveLoadModule.load_state_dict (network.py:82-92): copy only the names we own."""
        own = self.state_dict()
        with torch.no_grad():
            for name, param in state_dict.items():
                if name in own:
                    own[name].copy_(param)
        self.bump_version()

    def blocks(self):
        return [self.res1, self.res2, self.res3, self.res4, self.res5]

    def _make_packs(self):
        P = {}
        for name, m in self.named_modules():
            if isinstance(m, Conv2d):
                # + the rotated pack of the 3x3 stride-1 layers' data gradient as a forward conv (conv2d_dgrad_s1)
                s1 = m.kernel_size == 3 and m.stride == 1
                P[name] = (ops.weight_pack(m.weight, ops.PACK_FWD), ops.weight_pack(m.weight, ops.PACK_DGRAD),
                           _padded_bias(m), ops.weight_pack(m.weight, ops.PACK_IKF) if s1 else None)
        if FS_TAP:  # the output layer's (CK pack of the tap forward, 8-output IKF pack of its data gradient)
            w = self.deconv3.conv2d.weight
            P["deconv3.tap"] = (ops.weight_pack(w, ops.PACK_CK), ops.weight_pack(w, ops.PACK_IKF, Op=8))
        return P

    def forward_nhwc(self, x, style_strength=1.0):
        return _FastStyleFn.apply(x, self._anchor(), self, float(style_strength), _AFFINE_NORM)

    def forward(self, x, style_strength=1.0, s_id=0):
        feats, img = self.forward_nhwc(_ToNHWC.apply(x, cpad(self.input_nc)), style_strength)
        return _ToNCHW.apply(feats, 128), _ToNCHW.apply(img, 3)


class MultiStyleNet(FastStyleNet):
    """network.py:263-298 with n_styles > 1: FastStyleNet(num_inp, n_styles) whose conv1..3 / deconv1..2 norms are
    ConditionalInstanceNorm (the ResidualBlocks keep plain InstanceNorm2d(affine=True), network.py:224-236); same
    module tree and state_dict keys (``*.instance.bn.*``, ``*.instance.embed.weight``), SelectiveLoadModule
    loading; 1,679,240 + 640 * n_styles parameters for num_inp = 3.

    forward(x, style_strength=1.0, s_id=0) -> (features, image).  s_id: a Python int or a 0-dim tensor (long or
    float, truncated as ``.long()`` does) — the reference's one style for the whole batch — or, beyond what the
    reference can express, a length-N sequence / 1-D tensor with one style per sample: sample n is then computed
    as if run alone with the scalar id s_id[n].  Ids given as host values are range-checked (ValueError); a
    device tensor is never copied back, the kernels clamp it to [0, n_styles)."""

    def __init__(self, num_inp, n_styles):
        if int(n_styles) < 2:
            raise ValueError("MultiStyleNet: n_styles >= 2 (FastStyleNet is the single-style net; see make_net)")
        self._build(num_inp, int(n_styles))

    def forward_nhwc(self, x, style_strength=1.0, s_id=0):
        sid = ops.style_ids(s_id, x.shape[0], self.n_styles, x.device)
        return _FastStyleFn.apply(x, self._anchor(), self, float(style_strength), _CondNorm(sid))

    def forward(self, x, style_strength=1.0, s_id=0):
        feats, img = self.forward_nhwc(_ToNHWC.apply(x, cpad(self.input_nc)), style_strength, s_id)
        return _ToNCHW.apply(feats, 128), _ToNCHW.apply(img, 3)


def make_net(num_inp, n_styles=1):
    """The reference's ``FastStyleNet(num_inp, n_styles)`` constructor: FastStyleNet for one style, MultiStyleNet
    otherwise (the name INTEGRATION.md binds in reference code)."""
    return FastStyleNet(num_inp, 1) if int(n_styles) == 1 else MultiStyleNet(num_inp, n_styles)


def _aff(mod):
    return mod.weight.detach(), mod.bias.detach()


class _AffineNorm:
    """The norm + ReLU step of conv1..3 / deconv1..2 and its backward, as _FastStyleFn takes it: plain
    InstanceNorm2d(affine=True) (FastStyleNet)."""

    def fwd(self, y, s, inst):
        g, b = _aff(inst)
        return ops.instnorm_affine_fwd(y, s, g, b, "relu")

    def bwd(self, g, y, s, inst, conv_mod, train_w):
        gam, bet = _aff(inst)
        kw = dict(dgamma=inst.weight.grad, dbeta=inst.bias.grad, dbias=conv_mod.bias.grad) if train_w else {}
        return ops.instnorm_affine_bwd(g, y, s, gam, bet, "relu", accumulate=True, **kw)


class _CondNorm:
    """... the conditional norm of MultiStyleNet: ``sid`` is the batch's device int32 style ids (ops.style_ids)."""

    def __init__(self, sid):
        self.sid = sid

    @staticmethod
    def _params(inst):
        return inst.embed.weight.detach(), inst.bn.weight.detach(), inst.bn.bias.detach()

    def fwd(self, y, s, inst):
        return ops.cond_instnorm_fwd(y, s, self.sid, *self._params(inst), "relu")

    def bwd(self, g, y, s, inst, conv_mod, train_w):
        kw = {}
        if train_w:
            kw = dict(dembed=inst.embed.weight.grad, dbn_w=inst.bn.weight.grad, dbn_b=inst.bn.bias.grad,
                      dbias=conv_mod.bias.grad)
        return ops.cond_instnorm_bwd(g, y, s, self.sid, *self._params(inst), "relu", accumulate=True, **kw)


_AFFINE_NORM = _AffineNorm()


class _FastStyleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, net, strength, norm):
        ctx.set_materialize_grads(False)
        P = net.packs()
        role = "fwd" if any(ctx.needs_input_grad[:2]) else "infer"
        sv = {"x": x}

        def conv(inp, key, cout, k, st):
            kc, _, b, _ = P[key]
            return ops.conv2d_fwd(inp, kc, b, cpad(cout), k, k, st, k // 2, "reflect", role=role)

        def cir(inp, layer, key, cout, k, st):
            y = conv(inp, key, cout, k, st)
            s = ops.instnorm_stats(y)
            return y, s, norm.fwd(y, s, layer.instance)

        a = x
        for name, cout, k, st in (("conv1", 32, 9, 1), ("conv2", 64, 3, 2), ("conv3", 128, 3, 2)):
            y, s, an = cir(a, getattr(net, name), name + ".conv2d", cout, k, st)
            sv[name] = (a, y, s)
            a = an
        h = a
        for i, blk in enumerate(net.blocks()):
            key = "res%d" % (i + 1)
            t = conv(h, key + ".conv1.conv2d", 128, 3, 1)
            s1 = ops.instnorm_stats(t)
            g1, b1 = _aff(blk.in1)
            u = ops.instnorm_affine_fwd(t, s1, g1, b1, "relu")
            v = conv(u, key + ".conv2.conv2d", 128, 3, 1)
            s2 = ops.instnorm_stats(v)
            g2, b2 = _aff(blk.in2)
            hn = ops.instnorm_affine_fwd(v, s2, g2, b2, "none", gate=blk.layer_strength.detach(),
                                         gate_mult=strength, residual=h)
            sv[key] = (h, t, s1, u, v, s2)
            h = hn
        feats = h
        a = h
        for name, cout in (("deconv1", 64), ("deconv2", 32)):
            up = ops.upsample2x(a)
            y, s, an = cir(up, getattr(net, name), name + ".conv2d", cout, 3, 1)
            sv[name] = (up, y, s)
            a = an
        if "deconv3.tap" in P:
            y = ops.tap_conv_fwd(a, P["deconv3.tap"][0], P["deconv3.conv2d"][2], 9, 4, "reflect", role=role)
        else:
            y = conv(a, "deconv3.conv2d", 3, 9, 1)
        out = ops.scaled_tanh(y, 3)
        sv["deconv3"] = (a, y)
        ctx.sv, ctx.net, ctx.P, ctx.strength, ctx.norm = sv, net, P, strength, norm
        ctx.train_w = anchor.requires_grad
        return feats, out

    @staticmethod
    def backward(ctx, gfeat, gout):
        sv, net, P, strength, norm = ctx.sv, ctx.net, ctx.P, ctx.strength, ctx.norm
        train_w = ctx.train_w

        def wgrad(mod, inp, dy, k, st, db=False):
            if not train_w:
                return
            w = mod.weight
            co, ci = w.shape[0], w.shape[1]
            ops.conv2d_wgrad(inp, dy, w.grad, mod.bias.grad if db else None, k, k, st, k // 2, "reflect",
                             co, ci, ci * k * k, k * k, accumulate=True)

        def dgrad(dy, key, xin, k, st, addend=None):
            _, ck, _, ikf = P[key]
            N, H, W, C = xin.shape
            p = k // 2
            if st == 1 and ikf is not None and FS_DGRAD_FPROP:  # interior conv + border GEMM (the generator's route)
                return ops.conv2d_dgrad_s1(dy, ikf, H, W, C, k, p, "reflect", addend=addend)
            if st == 1:
                return ops.conv2d_tfwd(dy, ck, None, H, W, C, k, k, 1, p, pad_mode="reflect", addend=addend)
            # strided reflect conv: data gradient of the valid conv into the padded frame, then fold
            dxp = ops.conv2d_tfwd(dy, ck, None, H + 2 * p, W + 2 * p, C, k, k, st, 0)
            return ops.reflect_fold(dxp, p, addend)

        def in_bwd(g, y, s, layer, conv_mod, act, gate=None):
            gam, bet = _aff(layer)
            kw = {}
            if train_w:
                kw = dict(dgamma=layer.weight.grad, dbeta=layer.bias.grad, dbias=conv_mod.bias.grad)
                if gate is not None:
                    kw["dgate"] = gate.grad
            return ops.instnorm_affine_bwd(g, y, s, gam, bet, act, gate=None if gate is None else gate.detach(),
                                           gate_mult=strength, accumulate=True, **kw)

        g = None
        if gout is not None:
            a, y = sv["deconv3"]
            gy = ops.scaled_tanh_bwd(y, gout.contiguous(), 3)
            m = net.deconv3.conv2d
            tap = P.get("deconv3.tap")
            if tap is not None and train_w and ops.tap_conv_wgrad_swap_ok(a, 9, 4, "reflect", co=m.weight.shape[0]):
                ops.tap_conv_wgrad_swap(a, gy, m.weight.grad, 9, 4, "reflect", accumulate=True, db=m.bias.grad)
            else:
                wgrad(m, a, gy, 9, 1, db=True)
            if tap is not None:
                gp = _pad_channels(gy, 8)
                gp.vst_real_c = 3  # (tools/convflops: the MACs of the 3 real channels)
                g = ops.conv2d_dgrad_s1(gp, tap[1], a.shape[1], a.shape[2], a.shape[-1], 9, 4, "reflect")
            else:
                g = dgrad(gy, "deconv3.conv2d", a, 9, 1)
            for name in ("deconv2", "deconv1"):
                up, y, s = sv[name]
                layer = getattr(net, name)
                dy = norm.bwd(g, y, s, layer.instance, layer.conv2d, train_w)
                wgrad(layer.conv2d, up, dy, 3, 1)
                g = ops.upsample2x_bwd(dgrad(dy, name + ".conv2d", up, 3, 1))
        if gfeat is not None:
            gfeat = gfeat.contiguous()
            if g is None:
                g = gfeat.clone()
            else:
                ops.axpby(gfeat, g, 1.0, 1.0)
        if g is None:
            return None, None, None, None, None
        gh = g
        for i in reversed(range(5)):
            blk = net.blocks()[i]
            key = "res%d" % (i + 1)
            h, t, s1, u, v, s2 = sv[key]
            dv = in_bwd(gh, v, s2, blk.in2, blk.conv2.conv2d, "none", gate=blk.layer_strength)
            wgrad(blk.conv2.conv2d, u, dv, 3, 1)
            du = dgrad(dv, key + ".conv2.conv2d", u, 3, 1)
            dt = in_bwd(du, t, s1, blk.in1, blk.conv1.conv2d, "relu")
            wgrad(blk.conv1.conv2d, h, dt, 3, 1)
            gh = dgrad(dt, key + ".conv1.conv2d", h, 3, 1, addend=gh)
        g = gh
        gx = None
        for name, k, st in (("conv3", 3, 2), ("conv2", 3, 2), ("conv1", 9, 1)):
            a_in, y, s = sv[name]
            layer = getattr(net, name)
            dy = norm.bwd(g, y, s, layer.instance, layer.conv2d, train_w)
            wgrad(layer.conv2d, a_in, dy, k, st)
            if name != "conv1":
                g = dgrad(dy, name + ".conv2d", a_in, k, st)
            elif ctx.needs_input_grad[0]:
                gx = dgrad(dy, name + ".conv2d", a_in, k, st)
        ctx.sv = None
        return gx, None, None, None, None


class Johnson:
    """fs_johnson.py:5-52 Johnson method + the FastStyle training plumbing it relies on
    (fast_style_transfer.py:226-248 Adam loop, 762-793 prep_training/prep_adam, 741-756 style
    Grams), on device-resident batches.

    ``train_step(img)`` = prep_adam + train_method + adam.step for one [B,3,H,W] batch in [0,1];
    returns (loss, content, style, tv) as device scalars and the styled image (NHWC4, 0..255)."""

    def __init__(self, style_imgs, emphasis=(1.0, 1e5, 1e-6), lr=1e-3, batch_sz=16, device="cuda",
                 vgg=None, model=None):
        self.device = torch.device(device)
        self.model = model if model is not None else FastStyleNet(3, 1).to(self.device)
        self.vgg = vgg if vgg is not None else perceptual.Vgg16(self.device)
        self.adam = FusedAdam([self.model], lr=lr)
        self.batch_sz = batch_sz
        self.alpha, self.beta, self.delta = emphasis
        # loadStyles: normalize -> VGG -> gram per level, one style (n_styles == 1)
        self.styles = [perceptual.style_grams(self.vgg, s.to(self.device)) for s in style_imgs]
        self._gram_cache = {}
        self.itr = 0

    def _style_targets(self, B):
        if B not in self._gram_cache:
            # broadcast of the [1, C, C] style Gram against the batch's [B, C, C] (fs_johnson.py:41)
            self._gram_cache[B] = [g.expand(B, -1, -1).contiguous() for g in self.styles[0]]
        return self._gram_cache[B]

    def prep_adam(self, itr):
        """fast_style_transfer.py:788-793: zero grads; lr /= 1.2 every 500/batch_sz iterations."""
        self.adam.zero_grad()
        if (itr + 1) % int(500 / self.batch_sz) == 0:
            for pg in self.adam.param_groups:
                pg["lr"] = max(pg["lr"] / 1.2, 1e-4)

    def losses_nhwc(self, img_nhwc):
        """train_method's loss graph on an NHWC4 [0,1] image batch -> (loss, cl, sl, tv, styled)."""
        _, styled = self.model.forward_nhwc(img_nhwc)
        if VGG_BATCHED:  # styled (differentiated) and the content image through the VGG as one batch, the content
            # image through the slices its loss reads only (relu3_3)
            with torch.no_grad():
                xc = perceptual.normalize_nhwc(img_nhwc)
            styled_f, img_f = self.vgg.forward_multi_nhwc([perceptual.normalize_nhwc(styled, d0=255.0), xc],
                                                          [len(self.vgg.slices_idx), 3])
        else:
            styled_f = self.vgg.forward_nhwc(perceptual.normalize_nhwc(styled, d0=255.0))
            with torch.no_grad():
                img_f = self.vgg.forward_nhwc(perceptual.normalize_nhwc(img_nhwc))
        content = perceptual.mse_loss(styled_f[2], img_f[2], self.alpha)
        grams = self._style_targets(img_nhwc.shape[0])
        style = None
        for f, gs in zip(styled_f, grams):
            t = perceptual.mse_loss(perceptual.gram_nhwc(f), gs, self.beta)
            style = t if style is None else style + t
        # calc_tv_loss(styled / 255) == calc_tv_loss(styled) / 255 (positively homogeneous)
        tv = perceptual.tv_loss_nhwc(styled, self.delta / 255.0, 3)
        loss = content + style + tv
        return loss, content, style, tv, styled

    def train_step(self, img):
        self.prep_adam(self.itr)
        x = ops.nchw_to_nhwc(img.to(self.device).float().contiguous())
        loss, cl, sl, tv, styled = self.losses_nhwc(x)
        loss.backward()
        self.adam.step()
        self.itr += 1
        return (loss.detach(), cl.detach(), sl.detach(), tv.detach()), styled

    @torch.no_grad()
    def infer_method(self, frame):
        """fs_johnson.py:50-52: styled frame / 255."""
        _, styled = self.model(frame.to(self.device).float())
        return styled / 255.0


class Dumoulin(Johnson):
    """fs_dumoulin.py:6-58: one net for ``n_styles = len(style_imgs)`` styles.  Each step styles the batch with ONE
    style id (fast_style_transfer.py:230-246: a np.random.randint(0, n_styles) draw per iteration, 0 for a single
    style) and takes content = alpha * mse(relu3_3) and style = beta * sum_levels mean((Gram - styles[id][level])^2);
    no TV term, no temporal term.  Adam covers every parameter with dense gradients, so the embedding rows of the
    styles not drawn get a zero gradient (their Adam moments still decay).
    emphasis: one (alpha, beta) pair, or a list of one pair per style."""

    def __init__(self, style_imgs, emphasis=(1.0, 1e5), lr=1e-3, batch_sz=16, device="cuda", vgg=None, model=None):
        self.n_styles = len(style_imgs)
        if self.n_styles < 1:
            raise ValueError("Dumoulin: at least one style image")
        per_style = isinstance(emphasis[0], (tuple, list))
        self.emphasis = [tuple(e) for e in emphasis] if per_style else [tuple(emphasis)] * self.n_styles
        if len(self.emphasis) != self.n_styles or any(len(e) != 2 for e in self.emphasis):
            raise ValueError("Dumoulin: emphasis is one (alpha, beta) pair or one pair per style")
        if model is None:
            model = make_net(3, self.n_styles).to(torch.device(device))
        super().__init__(style_imgs, self.emphasis[0] + (0.0,), lr, batch_sz, device, vgg, model)

    def draw_style(self):
        """fast_style_transfer.py:237-240: one np.random.randint(0, n_styles) draw; no draw for a single style."""
        if self.n_styles == 1:
            return 0
        import numpy as np
        return int(np.random.randint(0, self.n_styles))

    def _check_style(self, style_id):
        style_id = int(style_id)
        if not 0 <= style_id < self.n_styles:
            raise ValueError("Dumoulin: style id %d outside [0, %d)" % (style_id, self.n_styles))
        return style_id

    def _style_targets(self, B, style_id=0):
        if (B, style_id) not in self._gram_cache:
            self._gram_cache[(B, style_id)] = [g.expand(B, -1, -1).contiguous() for g in self.styles[style_id]]
        return self._gram_cache[(B, style_id)]

    def _forward_nhwc(self, x, style_id):
        if isinstance(self.model, MultiStyleNet):
            return self.model.forward_nhwc(x, s_id=style_id)
        return self.model.forward_nhwc(x)

    def losses_nhwc(self, img_nhwc, style_id):
        """train_method's loss graph (fs_dumoulin.py:26-49) on an NHWC4 [0,1] image batch with the host style id
        -> (loss, content, style, styled), the reference's tuple order + the styled image (NHWC4, 0..255)."""
        style_id = self._check_style(style_id)
        alpha, beta = self.emphasis[style_id]
        _, styled = self._forward_nhwc(img_nhwc, style_id)
        with torch.no_grad():
            xc = perceptual.normalize_nhwc(img_nhwc)
        styled_f, img_f = self.vgg.forward_multi_nhwc([perceptual.normalize_nhwc(styled, d0=255.0), xc],
                                                      [len(self.vgg.slices_idx), 3])
        content = perceptual.mse_loss(styled_f[2], img_f[2], alpha)
        style = None
        for f, gs in zip(styled_f, self._style_targets(img_nhwc.shape[0], style_id)):
            t = perceptual.mse_loss(perceptual.gram_nhwc(f), gs, beta)
            style = t if style is None else style + t
        return content + style, content, style, styled

    def train_step(self, img, style_id=None):
        """prep_adam + train_method + adam.step for one [B,3,H,W] batch in [0,1].  style_id None: drawn as the
        reference's loop does (draw_style).  Returns ((total, content, style) as device scalars, styled NHWC4
        0..255)."""
        if style_id is None:
            style_id = self.draw_style()
        self.prep_adam(self.itr)
        x = ops.nchw_to_nhwc(img.to(self.device).float().contiguous())
        loss, cl, sl, styled = self.losses_nhwc(x, style_id)
        loss.backward()
        self.adam.step()
        self.itr += 1
        return (loss.detach(), cl.detach(), sl.detach()), styled

    @torch.no_grad()
    def infer_method(self, frame, style_id=0):
        """fs_dumoulin.py:56-58: styled frame / 255."""
        _, styled = self.model(frame.to(self.device).float(), s_id=style_id)
        return styled / 255.0


class _VideoFastStyle(Johnson):
    """The frame-pair train step Huang and ReCoNet share (fs_huang.py:28-67, fs_reconet.py:28-78) on
    Johnson's plumbing (FusedAdam, prep_adam, style-Gram cache, VGG handle, infer_method).

    Both frames run as ONE batch of 2B (frames 1, then frames 2) through FastStyleNet and the VGG:
    InstanceNorm, the Grams and every loss mean are per sample, so the arithmetic is the two separate
    passes' and the GEMMs see twice the rows.  With it
      content = (alpha/2) (mse_1 + mse_2) = alpha * mse over the 2B batch,
      style   = (beta/2) sum_levels (mse(G_1) + mse(G_2)) = beta * sum_levels mse over the 2B Grams,
    and the temporal terms are the fused masked-warp loss (fs_lib.temporal_loss_pair_nhwc)."""

    def _pair_features(self, x):
        """x: [2B,H,W,4] in [0,1] -> (feature map, styled 0..255, content loss, style loss)."""
        feats, styled = self.model.forward_nhwc(x)
        with torch.no_grad():
            xc = perceptual.normalize_nhwc(x)
        styled_f, img_f = self.vgg.forward_multi_nhwc([perceptual.normalize_nhwc(styled, d0=255.0), xc],
                                                      [len(self.vgg.slices_idx), 3])
        content = perceptual.mse_loss(styled_f[2], img_f[2], self.alpha)
        style = None
        for f, gs in zip(styled_f, self._style_targets(x.shape[0])):
            t = perceptual.mse_loss(perceptual.gram_nhwc(f), gs, self.beta)
            style = t if style is None else style + t
        return feats, styled, content, style

    def train_step(self, imgs, masks, flows):
        """imgs: list of [B,3,H,W] frames in [0,1] (the first two are used); masks [B,k,H,W]; flows
        [B,2k,H,W] (pair 0: masks[:, 0:1], flows[:, 0:2]).  prep_adam + train_method + adam.step;
        returns the losses in the reference's order (device scalars) and styled frame 2 (NHWC4, 0..255)."""
        self.prep_adam(self.itr)
        dev = self.device
        x = ops.nchw_to_nhwc(torch.cat([imgs[0].to(dev).float(), imgs[1].to(dev).float()]).contiguous())
        B = imgs[0].shape[0]
        flow = flows[:, 0:2].to(dev).float().contiguous()
        mask = masks[:, 0:1].to(dev).float().contiguous()
        out = self.losses_nhwc(x, flow, mask)
        out[0].backward()
        self.adam.step()
        self.itr += 1
        return tuple(v.detach() for v in out[:-1]), out[-1][B:]


class Huang(_VideoFastStyle):
    """fs_huang.py:8-71: Johnson's perceptual losses on two consecutive frames + the output temporal
    loss gamma * mean((mask * (styled2 - warp(styled1, flow)))^2); TV on styled frame 1 only.
    emphasis = (alpha, beta, gamma, delta); train_step returns ((total, content, style, temporal, tv),
    styled frame 2)."""

    def __init__(self, style_imgs, emphasis=(1.0, 1e5, 1e2, 1e-6), lr=1e-3, batch_sz=16, device="cuda",
                 vgg=None, model=None):
        alpha, beta, self.gamma, delta = emphasis
        super().__init__(style_imgs, (alpha, beta, delta), lr, batch_sz, device, vgg, model)

    def losses_nhwc(self, x, flow, mask):
        """train_method's loss graph on the NHWC4 [0,1] frames x ([2B,H,W,4]: frames 1, then frames 2), flow
        [B,2,H,W], mask [B,1,H,W] -> (loss, content, style, temporal, tv, styled [2B,H,W,4] 0..255)."""
        B = x.shape[0] // 2
        _, styled, content, style = self._pair_features(x)
        temporal = fs_lib.temporal_loss_pair_nhwc(styled, flow, mask, self.gamma, ab_scale=1.0 / 255.0, cl=3)
        # calc_tv_loss(styled1 / 255) == calc_tv_loss(styled1) / 255 (positively homogeneous)
        tv = perceptual.tv_loss_nhwc(styled[:B], self.delta / 255.0, 3)
        loss = content + style + temporal + tv
        return loss, content, style, temporal, tv, styled


class Reconet(_VideoFastStyle):
    """fs_reconet.py:8-82: the perceptual losses on two consecutive frames + the feature-map temporal
    loss at the residual blocks' output (flow and mask resized to it) + the output temporal loss with
    the luminance-weighted input term; TV averaged over both styled frames.
    emphasis = (alpha, beta, gamma_f, gamma_o, delta); train_step returns ((total, content, style,
    f_temporal, o_temporal, tv), styled frame 2)."""

    def __init__(self, style_imgs, emphasis=(1.0, 1e5, 1e2, 1e2, 1e-6), lr=1e-3, batch_sz=16, device="cuda",
                 vgg=None, model=None):
        alpha, beta, self.gamma_f, self.gamma_o, delta = emphasis
        super().__init__(style_imgs, (alpha, beta, delta), lr, batch_sz, device, vgg, model)

    def losses_nhwc(self, x, flow, mask):
        """As Huang.losses_nhwc -> (loss, content, style, f_temporal, o_temporal, tv, styled)."""
        B, H, W = x.shape[0] // 2, x.shape[1], x.shape[2]
        feats, styled, content, style = self._pair_features(x)
        Hf, Wf = feats.shape[1], feats.shape[2]
        # fs_reconet.py:58-59 scales flow channel 0 (x) by the HEIGHT ratio and channel 1 (y) by the WIDTH ratio;
        # passed as the reference computes them (at every size the net takes, H and W multiples of 4, both are 1/4)
        fflow = ops.resize_bilinear(flow, (Hf, Wf), (float(Hf) / H, float(Wf) / W))
        fmask = ops.resize_bilinear(mask, (Hf, Wf))
        f_temporal = fs_lib.temporal_loss_pair_nhwc(feats, fflow, fmask, self.gamma_f)
        o_temporal = fs_lib.temporal_loss_pair_nhwc(styled, flow, mask, self.gamma_o, inputs=(x[:B], x[B:]),
                                                    ab_scale=1.0 / 255.0, cl=3)
        # (delta/2) (tv_1 + tv_2): the TV sum over the 2B batch
        tv = perceptual.tv_loss_nhwc(styled, self.delta / 2.0 / 255.0, 3)
        loss = content + style + f_temporal + o_temporal + tv
        return loss, content, style, f_temporal, o_temporal, tv, styled


class Ruder(Johnson):
    """fs_ruder.py:10-121: the recurrent video method.  Frame k is styled by ``model`` (FastStyleNet(7, 1)) from
    cat(frame_k, mask_{k-1}, fs_lib.warp(styled_{k-1} / 255, flow_{k-1})); frame 1 by the frozen
    ``pre_style_model`` (FastStyleNet(3, 1), a trained Johnson net).  The recurrence runs for 2, 3 or 5 frames,
    the losses are taken on the last frame only, and their gradient runs back through every warp and every
    earlier application of ``model`` down to styled frame 1, where it stops: Adam covers ``model`` only
    (fast_style_transfer.py:226) and the pre-style net runs under no_grad.
    emphasis = (alpha, beta, gamma): content, style and temporal weights."""

    def __init__(self, style_imgs, emphasis=(1.0, 1e5, 1e2), lr=1e-3, batch_sz=16, device="cuda", vgg=None,
                 model=None, pre_style_model=None):
        alpha, beta, self.gamma = emphasis
        dev = torch.device(device)
        if model is None:
            model = FastStyleNet(7, 1).to(dev)
        super().__init__(style_imgs, (alpha, beta, 0.0), lr, batch_sz, device, vgg, model)
        self.pre_style_model = pre_style_model if pre_style_model is not None else FastStyleNet(3, 1).to(dev)

    @staticmethod
    def roll(p=0.5):
        """fs_ruder.py:18-19: one np.random.random() draw."""
        import numpy as np
        return bool(np.random.random() < p)

    @staticmethod
    def n_recurrent(n_imgs):
        """Index of the loss frame for ``n_imgs`` frames (fs_ruder.py:52-75): the ``len > 2`` and ``len > 4``
        branches make it 1, 2 or 4 (2, 3 or 5 frames used; 4 frames behave as 3)."""
        if n_imgs < 2:
            raise ValueError("Ruder: at least two frames, got %d" % n_imgs)
        return 4 if n_imgs > 4 else 2 if n_imgs > 2 else 1

    def losses_nhwc(self, frames, masks, flows, roll):
        """train_method's loss graph (fs_ruder.py:38-108).  frames: list of NHWC4 [0,1] batches; masks: list of
        [B,1,H,W] planes; flows: list of [B,2,H,W] planes (pair k-1 leads from frame k-1 to frame k).

        Returns (total, style, content, temporal, styled frame 2 as NHWC4 0..255): the REFERENCE's tuple order
        (fs_ruder.py:103 packs style before content although its labels name content first).  The temporal term
        is weighted by the LAST plane of ``masks`` (``masks[-1]``, fs_ruder.py:97) whichever frame the loss is
        taken on; without ``roll`` frame 2 is styled from the blank input (fs_ruder.py:78) and the temporal loss
        is a device zero."""
        if roll:
            last = self.n_recurrent(len(frames))
            if len(masks) < last or len(flows) < last:
                raise ValueError("Ruder: %d frames need %d mask / flow planes, got %d / %d" %
                                 (last + 1, last, len(masks), len(flows)))
            with torch.no_grad():
                _, y = self.pre_style_model.forward_nhwc(frames[0])
            styled2 = None
            for k in range(1, last + 1):
                x, w = fs_lib.ruder_stack_nhwc(y, frames[k], flows[k - 1], masks[k - 1])
                _, y = self.model.forward_nhwc(x)
                if k == 1:
                    styled2 = y
            loss_img = frames[last]
            temporal = fs_lib.ruder_temporal_nhwc(w, y, masks[-1], self.gamma)
        else:
            _, y = self.model.forward_nhwc(fs_lib.ruder_blank_nhwc(frames[1]))
            styled2, loss_img = y, frames[1]
            temporal = torch.zeros((), device=y.device)
        with torch.no_grad():
            xc = perceptual.normalize_nhwc(loss_img)
        styled_f, img_f = self.vgg.forward_multi_nhwc([perceptual.normalize_nhwc(y, d0=255.0), xc],
                                                      [len(self.vgg.slices_idx), 3])
        content = perceptual.mse_loss(styled_f[2], img_f[2], self.alpha)
        style = None
        for f, gs in zip(styled_f, self._style_targets(loss_img.shape[0])):
            t = perceptual.mse_loss(perceptual.gram_nhwc(f), gs, self.beta)
            style = t if style is None else style + t
        loss = content + style + temporal
        return loss, style, content, temporal, styled2

    def train_step(self, imgs, masks, flows, roll=None):
        """imgs: list of [B,3,H,W] frames in [0,1]; masks [B,k,H,W]; flows [B,2k,H,W] (the reference's layout).
        roll None: drawn as fs_ruder.py:44 does (np.random.random() < 0.5, one draw per step).  prep_adam +
        train_method + adam.step; returns ((total, style, content, temporal) as device scalars, in the reference's
        order) and styled frame 2 (NHWC4, 0..255)."""
        if roll is None:
            roll = self.roll(0.5)
        self.prep_adam(self.itr)
        dev = self.device
        frames = [ops.nchw_to_nhwc(i.to(dev).float().contiguous()) for i in imgs]
        masks = masks.to(dev).float()
        flows = flows.to(dev).float()
        mlist = [masks[:, k:k + 1].contiguous() for k in range(masks.shape[1])]
        flist = [flows[:, 2 * k:2 * k + 2].contiguous() for k in range(flows.shape[1] // 2)]
        out = self.losses_nhwc(frames, mlist, flist, roll)
        out[0].backward()
        self.adam.step()
        self.itr += 1
        return tuple(v.detach() for v in out[:-1]), out[-1].detach()

    @torch.no_grad()
    def infer_method(self, params):
        """fs_ruder.py:110-121 on NCHW tensors: params = (frame, mask, warped).  mask None: the pre-style net
        on the frame alone (first frame); else model(cat(frame, mask, warped)).  Styled frame / 255."""
        frame, mask, warped = (tuple(params) + (None, None))[:3]
        dev = self.device
        frame = frame.to(dev).float()
        if mask is None:
            _, styled = self.pre_style_model(frame)
        else:
            _, styled = self.model(torch.cat((frame, mask.to(dev).float(), warped.to(dev).float()), 1))
        return styled / 255.0

    @torch.no_grad()
    def stylize_next(self, prev_styled_nhwc, frame_nhwc, flow, mask):
        """One device-resident recurrence step of video inference: the previous styled frame (NHWC4, 0..255) is
        warped by ``flow``, stacked with the next frame (NHWC4, [0,1]) and ``mask`` by one kernel and styled;
        returns the styled frame (NHWC4, 0..255), ready to be the next call's ``prev_styled_nhwc``."""
        dev = self.device
        x, _ = ops.ruder_stack(prev_styled_nhwc.contiguous(), frame_nhwc.contiguous(),
                               flow.to(dev).float().contiguous(), mask.to(dev).float().contiguous(), want_w=False)
        _, styled = self.model.forward_nhwc(x)
        return styled


from . import _lib as _lib_routes  # noqa: E402
_lib_routes.apply_route_overrides(__name__, globals())
