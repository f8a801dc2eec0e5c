"""Network factory — drop-in for methods/GAN-based/CycleGAN/models/networks.py, HIP-backed.

Public API mirrors the reference (same names, argument meaning and errors):
  get_norm_layer (18-35), get_scheduler (38-64), init_weights (67-98), init_net (101-116),
  define_G (119-159), define_D (162-203), GANLoss (209-275), ResnetGenerator (315-373),
  ResnetBlock (376-433), UnetGenerator (436-465), UnetSkipConnectionBlock (468-535),
  NLayerDiscriminator (538-583).

MI355X design (not a translation):
  * Each network keeps the reference's nn.Sequential index structure so ``state_dict()`` keys and
    shapes are identical (``model.10.conv_block.1.weight`` …) and reference checkpoints load
    unmodified; the parameters themselves are views into ONE flat fp32 buffer per network (and the
    grads into one flat grad buffer) so the optimizer and the DP all-reduce are single fused calls.
  * ``forward`` runs the WHOLE network as one autograd node whose forward/backward are sequences
    of libvst_hip kernels: NHWC implicit-GEMM convs on fp32 MFMA with reflect padding / stride /
    transposition folded into address generation, fp64-reduced InstanceNorm fused with the
    activation and the residual add, deterministic split-K weight gradients written straight into
    the flat grad buffer (accumulating across the several passes of one train step).
  * Activations are NHWC with channel stride a multiple of 4; images are NHWC4.  ``forward`` takes
    and returns NCHW like the reference; ``forward_nhwc`` is the internal zero-copy entry.
"""
import functools
import os

import torch
import torch.nn as nn
from torch.nn import init
from torch.optim import lr_scheduler

from . import ops
from .ops import cpad


###############################################################################
# Helper Functions (reference networks.py:13-116)
###############################################################################
class Identity(nn.Module):
    def forward(self, x):
        return x


def get_norm_layer(norm_type='instance'):
    """networks.py:18-35.  Only 'instance' is on the HIP hot path (reference defaults)."""
    if norm_type == 'batch':
        return functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)
    elif norm_type == 'instance':
        return functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    elif norm_type == 'none':
        def norm_layer(x):
            return Identity()
        return norm_layer
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


def get_scheduler(optimizer, opt):
    """networks.py:38-64 (linear | step | plateau | cosine)."""
    if opt.lr_policy == 'linear':
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + opt.epoch_count - opt.n_epochs) / float(opt.n_epochs_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    elif opt.lr_policy == 'step':
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    elif opt.lr_policy == 'plateau':
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.2, threshold=0.01, patience=5)
    elif opt.lr_policy == 'cosine':
        return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.n_epochs, eta_min=0)
    return NotImplementedError('learning rate policy [%s] is not implemented', opt.lr_policy)


def init_weights(net, init_type='normal', init_gain=0.02):
    """networks.py:67-98: conv weights ~ init, conv biases = 0."""
    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, 'weight') and m.weight is not None and (classname.find('Conv') != -1):
            with torch.no_grad():
                if init_type == 'normal':
                    init.normal_(m.weight.data, 0.0, init_gain)
                elif init_type == 'xavier':
                    init.xavier_normal_(m.weight.data, gain=init_gain)
                elif init_type == 'kaiming':
                    init.kaiming_normal_(m.weight.data, a=0, mode='fan_in')
                elif init_type == 'orthogonal':
                    init.orthogonal_(m.weight.data, gain=init_gain)
                else:
                    raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
                if getattr(m, 'bias', None) is not None:
                    init.constant_(m.bias.data, 0.0)
    print('initialize network with %s' % init_type)
    net.apply(init_func)
    if isinstance(net, FlatNet):
        net.bump_version()


def _device_for(gpu_ids):
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        return torch.device('cuda:%d' % gpu_ids[0])
    if torch.cuda.is_available():
        return torch.device('cuda:%d' % torch.cuda.current_device())
    return torch.device('cpu')


def init_net(net, init_type='normal', init_gain=0.02, gpu_ids=[]):
    """networks.py:101-116.  Instead of nn.DataParallel (single-process multi-GPU), multi-GPU runs
    one process per GPU with torch.distributed (see dp.py); the net is placed on gpu_ids[0]."""
    net.to(_device_for(gpu_ids))
    init_weights(net, init_type, init_gain=init_gain)
    return net


###############################################################################
# Parameter holders: keep the reference module tree / state_dict keys
###############################################################################
class Conv2d(nn.Module):
    """Parameter holder with nn.Conv2d's state (weight [Co,Ci,k,k], bias [Co])."""

    def __init__(self, cin, cout, k, stride=1, padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.stride, self.padding = stride, padding
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}"


class ConvTranspose2d(nn.Module):
    """Parameter holder with nn.ConvTranspose2d's state (weight [Ci,Co,k,k], bias [Co])."""

    def __init__(self, cin, cout, k, stride=1, padding=0, output_padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.stride, self.padding, self.output_padding = stride, padding, output_padding
        self.weight = nn.Parameter(torch.empty(cin, cout, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}"


class _Marker(nn.Module):
    """Stateless placeholder for a fused layer (pad / norm / activation) — keeps indices & repr."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what


###############################################################################
# Flat parameter / gradient storage
###############################################################################
# The generator's image-side layers (c0: 3 -> ngf 7x7, and the data gradient of f: ngf -> 3 7x7) carry
# their 3-channel side padded to 8 channels, so the 7x7 implicit GEMMs run on the split-bf16 kernels
# (8-channel K chunks; half the K is zeros) instead of the fp32-image [row][k] kernels they otherwise
# need at 4 channels (~40 TF).
C8_EDGES = True
# The generator's first conv runs on the 4-channel image itself (conv_fprop_bf_k's 4-channel variant,
# K = 49*4 instead of 49*8); the 8-channel copy is still made for its weight gradient.  Likewise the
# data gradient of the last conv (a forward conv over its 4-channel output gradient).  (Module flags
# like this one are route selectors the tests flip in-process to compare routes; they are not read
# from the environment.)
C4_FWD = True
# ... and the first conv's weight gradient reads the 4-channel image too (the split-bf16 wgrad takes any
# channel count: K rows 49*4 instead of 49*8, and no 8-channel copy at all).
C4_WGRAD = C4_FWD


def _pad_channels(x, cs):
    """NHWC copy of x with its channel stride raised to cs (extra channels zero)."""
    y = torch.zeros(x.shape[:-1] + (cs,), device=x.device, dtype=x.dtype)
    ops.copy_channels(x, 0, y, 0, x.shape[-1])
    return y


# No-grad forwards replay captured HIP graphs (FlatNet.graphed_forward); VST_GRAPHS=0 runs them eagerly.
GRAPHS = os.environ.get("VST_GRAPHS", "1") != "0"
GRAPH_CACHE = 8  # captured input shapes kept per network


# Pack every layer of a network in one launch and refresh in place after updates (ops.PackBatch);
# False: one vst_weight_pack_split launch per pack, rebuilt per weight version.
PACK_BATCH = True


class FlatNet(nn.Module):
    """Base for HIP-backed networks: every parameter is a view into self.flat_param and its .grad a
    view into self.flat_grad.  Moving the module re-flattens on the new device."""

    def _flatten(self):
        params = list(self.parameters())
        dev = params[0].device
        n = sum(p.numel() for p in params)
        flat = torch.zeros(n, device=dev, dtype=torch.float32)
        gflat = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for p in params:
            k = p.numel()
            flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = flat[off:off + k].view_as(p)
            p.grad = gflat[off:off + k].view_as(p)
            off += k
        self.flat_param, self.flat_grad = flat, gflat
        self._wversion = getattr(self, "_wversion", 0) + 1
        self._packs = None
        self._graphs = {}  # captured forwards read the packs: recaptured after a rebuild

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._flatten()
        return self

    def bump_version(self):
        self._wversion += 1

    def _version_key(self):
        return (self._wversion, sum(p._version for p in self.parameters()))

    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()

    def weights_trainable(self):
        return any(p.requires_grad for p in self.parameters())

    def packs(self):
        """The layers' packed weights for the current weight version.  Built once (all packs in one
        ops.PackBatch launch); after a weight update the same batch re-packs every layer in place."""
        key = self._version_key()
        if not PACK_BATCH:
            if self._packs is None or self._packs[0] != key:
                self._packs = [key, self._make_packs(), None]
                self._graphs = {}
            return self._packs[1]
        if self._packs is None:
            with ops.PackBatch() as pb:
                P = self._make_packs()
            self._packs = [key, P, pb]
            self._graphs = {}
        elif self._packs[0] != key:
            self._packs[2].run()
            self._packs[0] = key
        return self._packs[1]

    def _anchor(self):
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != self.flat_param.device:
            a = torch.zeros((), device=self.flat_param.device, requires_grad=True)
            self._anchor_t = a
        return a if self.weights_trainable() and torch.is_grad_enabled() else a.detach()

    def forward(self, x):
        """Reference-compatible NCHW entry: [N, C, H, W] -> [N, C', H', W'].  Inference calls (no grad,
        GPU input) replay a HIP graph captured once per input shape (graphed_forward)."""
        if GRAPHS and not torch.is_grad_enabled() and x.is_cuda and not torch.cuda.is_current_stream_capturing():
            return self.graphed_forward(x)
        return self._forward_eager(x)

    def _forward_eager(self, x):
        cin = self.input_nc
        y = self.forward_nhwc(_ToNHWC.apply(x, cpad(cin)))
        return _ToNCHW.apply(y, self.output_nc)

    def graphed_forward(self, x):
        """No-grad forward replayed from a HIP graph captured once per (shape, device, conv policy,
        pack set, route switches — ops.route_flags(), so flipping e.g. ops.CONVT_DIRECT in-process
        captures a new graph instead of replaying the old route): the ~100 kernel launches of a generator forward (forward_eval,
        CycleGAN/models/cycle_gan_model.py:164-171) become one graph launch, so small batches are
        not bound by host launch latency.  The packs are refreshed in place before each replay
        (weight updates keep the captured buffers valid).  Returns a fresh output tensor."""
        P = self.packs()
        key = (tuple(x.shape), x.device, ops.get_conv_math(), id(P), ops.route_flags())
        cache = self._graphs
        ent = cache.get(key)
        if ent is None:
            if len(cache) >= GRAPH_CACHE:
                cache.clear()
            xs = x.detach().float().contiguous().clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up outside capture (allocator, first-touch)
                self._forward_eager(xs)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._forward_eager(xs)
            ent = (g, xs, out)
            cache[key] = ent
        g, xs, out = ent
        xs.copy_(x)
        g.replay()
        return out.clone()

    # ---- gradient readiness for the data-parallel exchange (dp.GradExchange.attach) ----------
    # Every training forward (trainable weights, grad enabled) adds one pending backward pass; the
    # backward pass that brings the count to zero is the last one of this optimizer phase, so each
    # layer's slice of flat_grad is final as soon as that pass has written it.  The pass then
    # reports, layer by layer in reverse parameter order, the lowest flat offset from which every
    # gradient is final; the exchange launches the RCCL all-reduce of every bucket at or above it
    # while the rest of the backward is still running.
    _grad_ready_cb = None
    _bwd_pending = 0

    def _note_forward(self, train_w):
        if train_w:
            self._bwd_pending += 1

    def _bwd_begin(self):
        """Call at the start of a backward pass; True if this is the phase's last pass and an
        exchange is attached (the pass must then call _grad_done after each layer)."""
        self._bwd_pending = max(0, self._bwd_pending - 1)
        return self._bwd_pending == 0 and self._grad_ready_cb is not None

    def _grad_done(self, mod):
        base = self.flat_param.data_ptr()
        off = min((p.data_ptr() - base) // p.element_size() for p in mod.parameters())
        self._grad_ready_cb(off)

    def _reset_pending(self):
        self._bwd_pending = 0


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cs):
        ctx.c = x.shape[1]
        return ops.nchw_to_nhwc(x.contiguous(), cs)

    @staticmethod
    def backward(ctx, g):
        return ops.nhwc_to_nchw(g.contiguous(), ctx.c), None


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c):
        ctx.cs = x.shape[-1]
        return ops.nhwc_to_nchw(x, c)

    @staticmethod
    def backward(ctx, g):
        return ops.nchw_to_nhwc(g.contiguous(), ctx.cs), None


def _pack_conv(m):
    return (ops.weight_pack(m.weight, ops.PACK_FWD), ops.weight_pack(m.weight, ops.PACK_DGRAD),
            _padded_bias(m))


# Stride-1 data gradients whose output-gradient channel count suits the split-bf16 forward kernel
# run as forward convs over rotated weights (ops.conv2d_dgrad_s1): the fprop kernel (pre-split
# weight planes) sustains ~1.8x the transposed-conv kernel on the ResnetBlock shape.
DGRAD_AS_FPROP = True
# The generator's last conv (4 padded output channels) runs as a tap GEMM on the matrix cores
# (ops.tap_conv_fwd / tap_conv_wgrad) instead of the VALU skinny kernel.
TAP_LAST = True
# ... its forward as the 7x1 conv with (column tap, channel) outputs + a column tap sum (ops.tap_conv_fwd_h:
# a 28-wide intermediate instead of the 196-wide one); False keeps the 1x1 conv + full tap sum.
TAP_H = True
# the image-input first layer's data gradient the same way (ops.tap_conv_dgrad_h); False: tap gather.
TAP_HD = True
# ... and the last layer's weight gradient as the swapped GEMM (ops.tap_conv_wgrad_swap, ops.TAP_SWAP) or the
# 7x1 conv's (ops.tap_conv_wgrad_h); False: tap fold.
TAP_HW = True
# The up-sampling ConvTranspose2d (k3 s2 p1 op1) forward as four sub-pixel phase convs on the
# split-bf16 forward kernel (ops.convT3s2_fwd).
CONVT_PHASES = True


def _ikf(m):
    return ops.weight_pack(m.weight, ops.PACK_IKF) if DGRAD_AS_FPROP else None


def _padded_bias(m):
    if m.bias is None:
        return None
    cp = cpad(m.bias.numel())
    if cp == m.bias.numel():
        return m.bias.detach()
    b = torch.zeros(cp, device=m.bias.device)
    pb = ops.PackBatch._active
    if pb is not None:
        pb.copy_into(b, m.bias.detach())  # refreshed with the packs
    else:
        b[:m.bias.numel()] = m.bias.detach()
    return b


###############################################################################
# ResnetGenerator (networks.py:315-433)
###############################################################################
class ResnetBlock(nn.Module):
    """networks.py:376-433 (reflect padding, instance norm): x + [pad,conv,IN,ReLU,pad,conv,IN](x)."""

    def __init__(self, dim, padding_type, norm_layer, use_dropout, use_bias):
        super().__init__()
        if padding_type != 'reflect':
            raise NotImplementedError('padding [%s] is not on the HIP path' % padding_type)
        if use_dropout:
            raise NotImplementedError('dropout is not on the HIP path (CycleGAN default no_dropout)')
        self.conv_block = nn.Sequential(
            _Marker('ReflectionPad2d(1)'), Conv2d(dim, dim, 3, bias=use_bias), _Marker('InstanceNorm2d'),
            _Marker('ReLU'), _Marker('ReflectionPad2d(1)'), Conv2d(dim, dim, 3, bias=use_bias),
            _Marker('InstanceNorm2d'))


class ResnetGenerator(FlatNet):
    """networks.py:315-373: c7s1-ngf, d(2ngf), d(4ngf), n_blocks x R(4ngf), u(2ngf), u(ngf), c7s1-out, tanh."""

    def __init__(self, input_nc, output_nc, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False,
                 n_blocks=6, padding_type='reflect'):
        assert n_blocks >= 0
        super().__init__()
        if not (isinstance(norm_layer, functools.partial) and norm_layer.func == nn.InstanceNorm2d):
            raise NotImplementedError('only norm=instance is implemented on the HIP path')
        use_bias = True
        self.input_nc, self.output_nc, self.ngf, self.n_blocks = input_nc, output_nc, ngf, n_blocks
        L = [_Marker('ReflectionPad2d(3)'), Conv2d(input_nc, ngf, 7, bias=use_bias),
             _Marker('InstanceNorm2d'), _Marker('ReLU')]
        for i in range(2):
            m = 2 ** i
            L += [Conv2d(ngf * m, ngf * m * 2, 3, stride=2, padding=1, bias=use_bias),
                  _Marker('InstanceNorm2d'), _Marker('ReLU')]
        for _ in range(n_blocks):
            L += [ResnetBlock(ngf * 4, padding_type, norm_layer, use_dropout, use_bias)]
        for i in range(2):
            m = 2 ** (2 - i)
            L += [ConvTranspose2d(ngf * m, ngf * m // 2, 3, stride=2, padding=1, output_padding=1,
                                  bias=use_bias),
                  _Marker('InstanceNorm2d'), _Marker('ReLU')]
        L += [_Marker('ReflectionPad2d(3)'), Conv2d(ngf, output_nc, 7, bias=True), _Marker('Tanh')]
        self.model = nn.Sequential(*L)
        self._flatten()

    # layer handles in execution order
    def _layers(self):
        mdl = self.model
        c0 = mdl[1]
        d = [mdl[4], mdl[7]]
        blocks = [mdl[10 + i] for i in range(self.n_blocks)]
        u = [mdl[10 + self.n_blocks], mdl[13 + self.n_blocks]]
        f = mdl[17 + self.n_blocks]
        return c0, d, blocks, u, f

    def _make_packs(self):
        c0, d, blocks, u, f = self._layers()
        P = {"c0": _pack_conv(c0), "d0": _pack_conv(d[0]), "d1": _pack_conv(d[1]), "f": _pack_conv(f)}
        if CONVT_PHASES:
            # the data gradient of Conv2d(k3, s2, p1) IS ConvTranspose2d(k3, s2, p1, op1) with the
            # conv weight [Co][Ci] read as the transposed weight [in][out]: four phase convs
            for i in (0, 1):
                if d[i].weight.shape[0] % 8 == 0:
                    P[f"d{i}ph"] = ops.convT3s2_phase_packs(d[i].weight)
        if C8_EDGES and not C4_FWD and c0.weight.shape[1] <= 4:
            # the 8-channel forward pack is read only when the image conv runs on 8-channel copies
            P["c08"] = ops.weight_pack(c0.weight, ops.PACK_FWD, Ip=8)
        if TAP_LAST:
            P["ftap"] = ops.weight_pack(f.weight, ops.PACK_CK)
            if TAP_H and f.weight.shape[0] <= 4 and f.weight.shape[2] == f.weight.shape[3]:
                P["ftaph"] = ops.weight_pack(f.weight, ops.PACK_SOK, Op=4)
            if c0.weight.shape[1] <= 4:  # image-input first layer: its data gradient as a tap gather
                P["c0kc"] = ops.weight_pack(c0.weight, ops.PACK_KC)
                if TAP_HD and c0.weight.shape[2] == c0.weight.shape[3]:  # ... or a 7x1 conv + column taps + fold
                    P["c0sokd"] = ops.dgrad_sok_pack(c0.weight)
        P["ikf"] = {}
        # the ResnetBlock data gradients run as forward convs over the IKF packs when the channel
        # count suits the split-bf16 kernel (dgrad_reflect): their IK packs are then never read
        ik_blocks = not (DGRAD_AS_FPROP and cpad(4 * self.ngf) % 8 == 0)
        for i, b in enumerate(blocks):
            for key, m in ((f"b{i}a", b.conv_block[1]), (f"b{i}b", b.conv_block[5])):
                P[key] = _pack_conv(m) if ik_blocks else (ops.weight_pack(m.weight, ops.PACK_FWD), None,
                                                           _padded_bias(m))
            P["ikf"][f"b{i}a"] = _ikf(b.conv_block[1])
            P["ikf"][f"b{i}b"] = _ikf(b.conv_block[5])
        if C4_FWD and DGRAD_AS_FPROP and f.weight.shape[0] <= 4:
            P["ikf"]["f4"] = ops.weight_pack(f.weight, ops.PACK_IKF)
        elif C8_EDGES and DGRAD_AS_FPROP and f.weight.shape[0] <= 4:
            P["ikf"]["f8"] = ops.weight_pack(f.weight, ops.PACK_IKF, Op=8)
        for i, m in enumerate(u):
            # ConvTranspose2d fwd = transposed kernel with rows (r,s,ci) -> CK pack of Wt[Ci][Co];
            # its dgrad = forward conv with KC pack of Wt seen as [O=Ci][I=Co] -> rows (r,s,co), cols ci
            if CONVT_PHASES:
                P[f"u{i}ph"] = ops.convT3s2_phase_packs(m.weight)
            P[f"u{i}"] = (ops.weight_pack(m.weight, ops.PACK_FWD), ops.weight_pack(m.weight, ops.PACK_DGRAD),
                          _padded_bias(m))
        return P

    def forward_nhwc(self, x):
        return _GeneratorFn.apply(x, self._anchor(), self)


# Which operand images the IN passes write for a conv's weight gradient is decided in one place, _wgrad_form,
# from the weight gradient's route; these two switches only say whether the producers write the images of an
# ops.WG_IMAGES route (False: vst_conv2d_wgrad_pre makes its copies itself).
IN_PLANES = True  # the IN backward writes dy's channel-major bf16 planes
IN_XT = True      # the forward IN apply writes x's padded channel-major image
# The IN backward partials of the layer below taken by the ResnetBlock data gradient's own GEMM epilogue and
# border add (ops.conv2d_dgrad_refl_in: no partial pass reading g and the IN input again).
# C2 step A/B, same box: 53.52-53.57 vs 53.79-53.80 ms (profiles/r05h_dgrad_epi_step_ab.jsonl); False
# restores the separate data gradient + IN-backward partial pass.  (Round 6 deleted the two measured-slower
# fusions of that step: the border add in the partial pass, +0.85 ms, and the fold + partials pass.)
DGRAD_EPI = True
# The discriminator head (1 real output channel of 4) runs the one-channel skinny forward
# (ops.conv2d_fwd(co_real=1)); False keeps the 4-channel sums.
D_CO1 = True
# The first PatchGAN layer's data gradient (onto the 4-channel image) as ONE parity-class gather launch
# (ops.conv2d_tfwd -> skinny.hip MODE 1) instead of four 2x2 phase convs + the interleave pass.
D0_TFWD = True
# The ResnetBlock chain's data-gradient inputs as pre-split planes ONLY (the IN backward writes the NHWC bf16
# planes and no fp32 image; the data gradient's 256x128 GEMM stages A from them by LDS-DMA, its weight gradient
# reads the channel-major planes, the border GEMM puts the values back together): C2 step A/B 53.81-53.82 vs
# 53.99-54.05 ms (profiles/r05n_apre_bwd_step_ab.jsonl).  (The forward half — planes written beside the fp32
# activation — measured +0.73 ms in round 5, profiles/r05l_apre_step_ab.jsonl, and was deleted in round 6.)
APRE_BWD = True


def _rb_chain(N, H, W, C):
    """Is the ResnetBlock chain (3x3, reflect pad 1, C -> C at H x W) the planes-only chain (APRE_BWD)?  Only where
    every one of its data gradients takes the epilogue route (ops.conv2d_dgrad_refl_in), which reads the planes;
    the other data-gradient routes read the fp32 image."""
    return APRE_BWD and DGRAD_EPI and C % 8 == 0 and ops.dgrad_refl_epi_ok(N, H, W, C, C)


def _wgrad_form(x_shape, y_shape, R, st, train_w, chain=False):
    """What the producers of a conv's weight-gradient operands write, from its route (ops.wgrad_route) alone:
    (x_t: the forward IN apply writes x's padded channel-major image, planes: the IN backward writes dy's
    channel-major bf16 planes, apre: it writes dy as its NHWC bf16 planes ONLY).  The conv reads x_shape and writes
    y_shape (R x R, stride st, padding (R - 1) // 2); chain: it sits in the planes-only ResnetBlock chain.
        WG_NHWC (False, False, True)    WG_IMAGES (IN_XT, IN_PLANES, chain and IN_PLANES)    others: nothing
    dy is planes-only only when every reader takes planes: the epilogue data gradient (chain) and a weight gradient
    on WG_NHWC, or on WG_IMAGES with the channel-major planes.  Where the weight gradient needs fp32, dy is fp32
    and the next data gradient reads that (Data layout)."""
    if train_w:
        N, H, W, Cx = x_shape
        _, Ho, Wo, Cyp = y_shape
        route = ops.wgrad_route(N, H, W, Cx, Ho, Wo, Cyp, R, R, st, (R - 1) // 2, dy_nhwc_planes=chain)
        if route == ops.WG_NHWC:
            return False, False, True
        if route == ops.WG_IMAGES:
            return IN_XT, IN_PLANES, chain and IN_PLANES
    return False, False, False


def _rb_wgrad_nhwc(N, H, W, C):
    """Do the ResnetBlock convs take their weight gradients on ops.WG_NHWC, dy from the planes-only chain?"""
    return _rb_chain(N, H, W, C) and _wgrad_form((N, H, W, C), (N, H, W, C), 3, 1, True, True) == (False, False, True)


def _in_bwd_for_wgrad(g, y, s, act, slope, db, x_in, R, st, train_w, chain=False):
    """instnorm_act_bwd -> (dy, dy_planes or None), dy in the form the weight gradient of the conv below
    (input x_in, kernel R, stride st) reads (_wgrad_form)."""
    _, planes, apre = _wgrad_form(x_in.shape, y.shape, R, st, train_w, chain)
    r = ops.instnorm_act_bwd(g, y, s, act, slope, db=db, planes=planes, apre=apre)
    return r if planes else (r, None)


class _GeneratorFn(torch.autograd.Function):
    """Whole-generator forward/backward on libvst_hip kernels."""

    @staticmethod
    def forward(ctx, x, anchor, net):
        P = net.packs()
        c0, d, blocks, u, f = net._layers()
        ngf = net.ngf
        sv = {"x": x, "xt": {}}  # xt: id(activation) -> its wgrad A-operand image (or None)
        N, H, W, _ = x.shape
        role = "fwd" if any(ctx.needs_input_grad[:2]) else "infer"

        train_w = role == "fwd" and anchor.requires_grad

        # the ResnetBlock convs' (two stride-2 convs below the input) planes-only chain, decided here for the backward too
        rb = (N, ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1, cpad(4 * ngf))
        sv["chain"] = chain = bool(train_w and blocks and _rb_chain(*rb) and all(
            P["ikf"].get(f"b{i}{c}") is not None for i in range(len(blocks)) for c in "ab"))

        def cp_for(y, cout, st, mode):
            """(pad, mode, stride) of the 3x3 conv consuming act(IN(y)) (cout outputs) when its weight
            gradient will read the padded channel-major image the IN apply can write (_wgrad_form)."""
            N_, H_, W_, _ = y.shape
            out_shape = (N_, (H_ + 2 - 3) // st + 1, (W_ + 2 - 3) // st + 1, cpad(cout))
            # the stride-1 convs are the ResnetBlocks'
            x_t, _, _ = _wgrad_form(y.shape, out_shape, 3, st, train_w, chain=st == 1 and chain)
            return (1, mode, st) if x_t else None

        def in_act(y, s, act, cp, residual=None):
            if cp is None:
                return ops.instnorm_act_fwd(y, s, act, residual=residual), None
            if cp[0] == "planes":
                return ops.instnorm_act_fwd(y, s, act, residual=residual, xpl=cp[1])
            return ops.instnorm_act_fwd(y, s, act, residual=residual, cp=cp)

        def conv_in_relu(inp, key, cout, R, st, pad, mode, nxt=None):
            """conv + IN + ReLU; nxt = (cout, stride, pad mode) of the 3x3 conv consuming the output"""
            kc, _, b = P[key]
            y, s = ops.conv2d_fwd_in(inp, kc, b, cpad(cout), R, R, st, pad, mode, role=role)
            a, at = in_act(y, s, "relu", cp_for(y, *nxt) if nxt else None)
            sv["xt"][id(a)] = at
            return y, s, a

        if C8_EDGES and x.shape[-1] == 4 and (C4_FWD or "c08" in P):
            # the 8-channel copy feeds the forward only without C4_FWD, else just c0's weight gradient
            x8 = _pad_channels(x, 8) if ((train_w and not C4_WGRAD) or not C4_FWD) else None
            _, _, b = P["c0"]
            if C4_FWD:
                y, s = ops.conv2d_fwd_in(x, P["c0"][0], b, cpad(ngf), 7, 7, 1, 3, "reflect", role=role)
            else:
                y, s = ops.conv2d_fwd_in(x8, P["c08"], b, cpad(ngf), 7, 7, 1, 3, "reflect", role=role)
            a, at = in_act(y, s, "relu", cp_for(y, 2 * ngf, 2, "zero"))
            sv["xt"][id(a)] = at
            if x8 is not None:
                sv["x8"] = x8
        else:
            y, s, a = conv_in_relu(x, "c0", ngf, 7, 1, 3, "reflect", nxt=(2 * ngf, 2, "zero"))
        sv["c0"] = (y, s, a)
        y, s, a = conv_in_relu(a, "d0", 2 * ngf, 3, 2, 1, "zero", nxt=(4 * ngf, 2, "zero"))
        sv["d0"] = (y, s, a)
        nb = len(blocks)
        y, s, a = conv_in_relu(a, "d1", 4 * ngf, 3, 2, 1, "zero", nxt=(4 * ngf, 1, "reflect") if nb else None)
        sv["d1"] = (y, s, a)
        h = a
        for i in range(nb):
            kc, _, b = P[f"b{i}b"]
            t, s1, uu = conv_in_relu(h, f"b{i}a", 4 * ngf, 3, 1, 1, "reflect", nxt=(4 * ngf, 1, "reflect"))
            v, s2 = ops.conv2d_fwd_in(uu, kc, b, 4 * ngf, 3, 3, 1, 1, "reflect", role=role)
            hn, hnt = in_act(v, s2, "none", cp_for(v, 4 * ngf, 1, "reflect") if i + 1 < nb else None, residual=h)
            sv["xt"][id(hn)] = hnt
            sv[f"b{i}"] = (h, t, s1, uu, v, s2)
            h = hn
        a = h
        for i in range(2):
            cout = ngf * 2 ** (1 - i)
            _, ck, b = P[f"u{i}"]
            Hi, Wi = a.shape[1], a.shape[2]
            if f"u{i}ph" in P and a.shape[-1] % 8 == 0:
                y = ops.convT3s2_fwd(a, P[f"u{i}ph"], b, cpad(cout), role=role)
            else:
                y = ops.conv2d_tfwd(a, ck, b, 2 * Hi, 2 * Wi, cpad(cout), 3, 3, 2, 1, role=role)
            s = ops.instnorm_stats(y)
            cp = None
            if i == 1 and "ftap" in P:
                # the last layer's weight gradient: the 7x1 conv's (x padded by 4, reflect) or the tap fold's
                # (1x1, pad 0); decided here so the x image below matches the route the backward takes
                sv["ftap_sw"] = ops.tap_conv_wgrad_swap_ok(y, 7, 3, "reflect", co=net.output_nc)
                sv["ftap_h"] = not sv["ftap_sw"] and TAP_HW and ops.tap_conv_wgrad_h_ok(y, 7, 3, "reflect")
            if i == 1 and "ftap" in P and train_w and IN_XT:
                # each tap weight gradient is a GEMM of its own reshaped problem: x's image in that geometry
                if sv["ftap_sw"]:
                    cp = ("planes", (3, "reflect", ops.tap_swap_geom(y.shape[2], 7)[0]))
                elif sv["ftap_h"]:
                    cp = (4, "reflect", 1)
                elif ops.tap_conv_wgrad_bf_ok(y, 7):
                    cp = (0, "zero", 1)
            an, at = in_act(y, s, "relu", cp)
            sv["xt"][id(an)] = at
            sv[f"u{i}"] = (a, y, s, an)
            a = an
        kc, _, b = P["f"]
        if "ftap" in P:
            out = (ops.tap_conv_fwd_h(a, P["ftaph"], b, 7, 3, "reflect", act="tanh", role=role) if "ftaph" in P else
                   ops.tap_conv_fwd(a, P["ftap"], b, 7, 3, "reflect", act="tanh", role=role))
        else:
            out = ops.conv2d_fwd(a, kc, b, cpad(net.output_nc), 7, 7, 1, 3, "reflect", act="tanh", role=role)
        sv["f"] = (a, out)
        ctx.sv, ctx.net, ctx.P = sv, net, P
        ctx.train_w = anchor.requires_grad
        net._note_forward(ctx.train_w)
        return out

    @staticmethod
    def backward(ctx, gout):
        sv, net, P = ctx.sv, ctx.net, ctx.P
        c0, d, blocks, u, f = net._layers()
        ngf = net.ngf
        train_w = ctx.train_w
        gout = gout.contiguous()
        final = train_w and net._bwd_begin()

        def done(mod):  # mod's gradients (and all later layers') are final for this phase
            if final:
                net._grad_done(mod)

        xts = sv["xt"]

        def wgrad(mod, inp, dy, R, st, pad, mode, db=False, dy_planes=None):
            if not train_w:
                return
            w = mod.weight
            co, ci = w.shape[0], w.shape[1]
            ops.conv2d_wgrad(inp, dy, w.grad, mod.bias.grad if (db and mod.bias is not None) else None,
                             R, R, st, pad, mode, co, ci, ci * R * R, R * R, accumulate=True, dy_planes=dy_planes,
                             x_t=xts.get(id(inp)))

        def in_bwd(g, y, s, act, mod, x_in=None, R=3, st=1, chain=False):
            # IN(+act) backward; the bias gradient of the conv feeding the IN comes out of the
            # same reduction (sum of dy per channel).  x_in given: dy in the form that conv's weight
            # gradient reads (_wgrad_form) -> (dy, planes or None)
            db = mod.bias.grad if (train_w and mod.bias is not None) else None
            if x_in is None:
                return ops.instnorm_act_bwd(g, y, s, act, db=db)
            return _in_bwd_for_wgrad(g, y, s, act, 0.0, db, x_in, R, st, train_w, chain=chain)

        def dgrad_reflect(dy, key, cin_p, R, p, H, W, addend=None):
            ikf = P["ikf"].get(key)
            if ikf is not None and dy.shape[-1] % 8 == 0:
                return ops.conv2d_dgrad_s1(dy, ikf, H, W, cin_p, R, p, "reflect", addend=addend)
            _, ck, _ = P[key]
            return ops.conv2d_tfwd(dy, ck, None, H, W, cin_p, R, R, 1, p, pad_mode="reflect",
                                   addend=addend)

        def dgrad_s2(dy, key, cin_p, H, W):
            ph = P.get(key + "ph")
            if ph is not None and H == 2 * dy.shape[1] and W == 2 * dy.shape[2]:
                return ops.convT3s2_fwd(dy, ph, None, cin_p, role="bwd")
            _, ck, _ = P[key]
            return ops.conv2d_tfwd(dy, ck, None, H, W, cin_p, 3, 3, 2, 1)

        # final conv + tanh (no IN after it: bias grad is a channel sum)
        a, out = sv["f"]
        g = ops.act_bwd(gout, out, "tanh")
        if "ftap" in P:
            if train_w:
                db = f.bias.grad if f.bias is not None else None
                if sv.get("ftap_sw"):  # the bias gradient taken by the GEMM's dy staging pass
                    ops.tap_conv_wgrad_swap(a, g, f.weight.grad, 7, 3, "reflect", accumulate=True,
                                            x_pl=xts.get(id(a)), db=db)
                    db = None
                elif sv.get("ftap_h"):
                    ops.tap_conv_wgrad_h(a, g, f.weight.grad, 7, 3, "reflect", accumulate=True, x_t=xts.get(id(a)))
                else:
                    ops.tap_conv_wgrad(a, g, f.weight.grad, 7, 3, "reflect", accumulate=True, x_t=xts.get(id(a)))
                if db is not None:
                    ops.channel_sum(g, db, f.weight.shape[0], accumulate=True)
        else:
            wgrad(f, a, g, 7, 1, 3, "reflect", db=True)
        done(f)
        if "f4" in P["ikf"] and g.shape[-1] == 4 and ops.c4_dgrad_reflect_ok(g, a.shape[-1], 7, 3):
            ga = ops.c4_dgrad_reflect(g, P["ikf"]["f4"], a.shape[1], a.shape[2], a.shape[-1], 7, 3)
        elif "f4" in P["ikf"] and g.shape[-1] == 4:
            ga = ops.conv2d_dgrad_s1(g, P["ikf"]["f4"], a.shape[1], a.shape[2], a.shape[-1], 7, 3, "reflect")
        elif "f8" in P["ikf"] and g.shape[-1] == 4:
            g8 = _pad_channels(g, 8)
            g8.vst_real_c = 3  # (tools/convflops: the MACs of the 3 real channels)
            ga = ops.conv2d_dgrad_s1(g8, P["ikf"]["f8"], a.shape[1], a.shape[2], a.shape[-1], 7, 3, "reflect")
        else:
            ga = dgrad_reflect(g, "f", a.shape[-1], 7, 3, a.shape[1], a.shape[2])
        # up-sampling convT layers
        for i in (1, 0):
            a_in, y, s, an = sv[f"u{i}"]
            m = u[i]
            dy = in_bwd(ga, y, s, "relu", m)
            if train_w:
                # Wt[ci][co] grad = wgrad of the equivalent conv x_T = conv(dy_T, .) (see header)
                ci_t, co_t = m.weight.shape[0], m.weight.shape[1]
                ops.conv2d_wgrad(dy, a_in, m.weight.grad, None, 3, 3, 2, 1, "zero", ci_t, co_t,
                                 co_t * 9, 9, accumulate=True)
            done(m)
            kc, _, _ = P[f"u{i}"]
            ga = ops.conv2d_fwd(dy, kc, None, a_in.shape[-1], 3, 3, 2, 1, "zero", role="bwd")
        def dgrad_reflect_in(dy, key, H, W, y_in, s_in, act, mod, x_w, R_w, st_w, addend=None, chain=False):
            """dgrad_reflect (3x3, pad 1) + the IN(+act) backward of the layer below it (y_in, s_in;
            mod = the conv feeding that IN; x_w / R_w / st_w = that conv's weight-gradient input
            and geometry; chain: that conv sits in the planes-only chain) -> (g, dy_in, dy_in planes or
            None).  The IN-backward partials come from the data gradient's epilogue and border add
            (ops.conv2d_dgrad_refl_in) where it takes the shape; otherwise the two steps run separately."""
            ikf = P["ikf"].get(key)
            cin_p = y_in.shape[-1]
            if DGRAD_EPI and ikf is not None and dy.shape[-1] % 8 == 0:
                db = mod.bias.grad if (train_w and mod.bias is not None) else None
                _, planes, apre = _wgrad_form(x_w.shape, y_in.shape, R_w, st_w, train_w, chain)
                r = ops.conv2d_dgrad_refl_in(dy, ikf, H, W, cin_p, y_in, s_in, act, 0.0, addend=addend, db=db,
                                             planes=planes, apre=apre)
                if r is not None:
                    return r if planes else (r[0], r[1], None)
            if getattr(dy, "vst_planes_only", False):
                raise RuntimeError("dgrad_reflect_in: a planes-only gradient reached a route that reads fp32")
            g = dgrad_reflect(dy, key, cin_p, 3, 1, H, W, addend=addend)
            dyi, pl = in_bwd(g, y_in, s_in, act, mod, x_w, R_w, st_w, chain=chain)
            return g, dyi, pl

        # residual blocks: block i's data gradients each carry the IN backward of the layer below
        # (IN 1 of block i; IN 2 of block i - 1, or the IN of d1 after block 0)
        gh = ga
        nb = len(blocks)
        pre_d1 = None
        # the planes-only chain (the forward's decision): every ResnetBlock conv's dy; not d1's, read as fp32
        chain = sv["chain"]
        if nb:
            dv, dvp = in_bwd(gh, sv[f"b{nb - 1}"][4], sv[f"b{nb - 1}"][5], "none", blocks[-1].conv_block[5],
                             sv[f"b{nb - 1}"][3], chain=chain)
        for i in reversed(range(nb)):
            h, t, s1, uu, v, s2 = sv[f"b{i}"]
            blk = blocks[i].conv_block
            wgrad(blk[5], uu, dv, 3, 1, 1, "reflect", dy_planes=dvp)
            done(blk[5])
            _, dt, dtp = dgrad_reflect_in(dv, f"b{i}b", uu.shape[1], uu.shape[2], t, s1, "relu", blk[1], h, 3, 1,
                                          chain=chain)
            wgrad(blk[1], h, dt, 3, 1, 1, "reflect", dy_planes=dtp)
            done(blk[1])
            if i > 0:
                _, _, _, uup, vp, s2p = sv[f"b{i - 1}"]
                gh, dv, dvp = dgrad_reflect_in(dt, f"b{i}a", h.shape[1], h.shape[2], vp, s2p, "none",
                                               blocks[i - 1].conv_block[5], uup, 3, 1, addend=gh, chain=chain)
            else:
                y1, s1d, _ = sv["d1"]
                gh, dy1, dyp1 = dgrad_reflect_in(dt, f"b{i}a", h.shape[1], h.shape[2], y1, s1d, "relu", d[1],
                                                 sv["d0"][2], 3, 2, addend=gh)
                pre_d1 = (dy1, dyp1)
        ga = gh
        # down-sampling convs
        for key, mod, prev in (("d1", d[1], "d0"), ("d0", d[0], "c0")):
            y, s, _ = sv[key]
            a_in = sv[prev][2]
            if key == "d1" and pre_d1 is not None:
                dy, dyp = pre_d1
            else:
                dy, dyp = in_bwd(ga, y, s, "relu", mod, a_in, 3, 2)
            wgrad(mod, a_in, dy, 3, 2, 1, "zero", dy_planes=dyp)
            done(mod)
            ga = dgrad_s2(dy, key, a_in.shape[-1], a_in.shape[1], a_in.shape[2])
        # first conv
        x = sv["x"]
        y, s, _ = sv["c0"]
        dy, dyp = in_bwd(ga, y, s, "relu", c0, sv.get("x8", x), 7, 1)
        wgrad(c0, sv.get("x8", x), dy, 7, 1, 3, "reflect", dy_planes=dyp)
        done(c0)
        gx = None
        if ctx.needs_input_grad[0]:
            if "c0kc" in P and x.shape[-1] == 4:
                gx = (ops.tap_conv_dgrad_h(dy, P["c0sokd"], 7, 3, "reflect") if "c0sokd" in P else
                      ops.tap_conv_dgrad(dy, P["c0kc"], 7, 3, "reflect"))
            else:
                gx = dgrad_reflect(dy, "c0", x.shape[-1], 7, 3, x.shape[1], x.shape[2])
        ctx.sv = None
        return gx, None, None


###############################################################################
# NLayerDiscriminator (networks.py:538-583)
###############################################################################
class NLayerDiscriminator(FlatNet):
    """PatchGAN: C64(s2)+LReLU, [C(s2)+IN+LReLU] x (n-1), C(s1)+IN+LReLU, C1(s1)."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d):
        super().__init__()
        if not (isinstance(norm_layer, functools.partial) and norm_layer.func == nn.InstanceNorm2d):
            raise NotImplementedError('only norm=instance is implemented on the HIP path')
        self.input_nc, self.output_nc = input_nc, 1
        kw, padw = 4, 1
        seq = [Conv2d(input_nc, ndf, kw, stride=2, padding=padw), _Marker('LeakyReLU(0.2)')]
        self.spec = [(ndf, 2, False)]  # (cout, stride, has_in)
        nf_mult = 1
        for n in range(1, n_layers):
            prev, nf_mult = nf_mult, min(2 ** n, 8)
            seq += [Conv2d(ndf * prev, ndf * nf_mult, kw, stride=2, padding=padw, bias=True),
                    _Marker('InstanceNorm2d'), _Marker('LeakyReLU(0.2)')]
            self.spec.append((ndf * nf_mult, 2, True))
        prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        seq += [Conv2d(ndf * prev, ndf * nf_mult, kw, stride=1, padding=padw, bias=True),
                _Marker('InstanceNorm2d'), _Marker('LeakyReLU(0.2)')]
        self.spec.append((ndf * nf_mult, 1, True))
        seq += [Conv2d(ndf * nf_mult, 1, kw, stride=1, padding=padw)]
        self.spec.append((1, 1, False))
        self.model = nn.Sequential(*seq)
        self._flatten()

    def _convs(self):
        return [m for m in self.model if isinstance(m, Conv2d)]

    def _make_packs(self):
        packs = [_pack_conv(m) for m in self._convs()]
        # stride-1 layers with >= 8 output channels: data gradient as a forward conv (IKF pack)
        self._ikf = [(_ikf(m) if (st == 1 and cout % 8 == 0) else None)
                     for m, (cout, st, _) in zip(self._convs(), self.spec)]
        # stride-2 layers: the data gradient as four 2x2 phase convs (ops.conv4s2_dgrad)
        self._ph = [(ops.conv4s2_dgrad_phase_packs(m.weight) if (CONVT_PHASES and st == 2 and cout % 8 == 0)
                     else None) for m, (cout, st, _) in zip(self._convs(), self.spec)]
        return packs

    def forward_nhwc(self, x):
        return _DiscriminatorFn.apply(x, self._anchor(), self)


SLOPE = 0.2


class _DiscriminatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, net):
        P = net.packs()
        convs = net._convs()
        saved = []
        a = x
        L = len(convs)
        role = "fwd" if any(ctx.needs_input_grad[:2]) else "infer"
        for i, (m, (cout, st, has_in)) in enumerate(zip(convs, net.spec)):
            kc, _, b = P[i]
            last = i == L - 1
            if has_in:
                y, s = ops.conv2d_fwd_in(a, kc, b, cpad(cout), 4, 4, st, 1, "zero", role=role)
                an = ops.instnorm_act_fwd(y, s, "lrelu", SLOPE)
                saved.append((a, y, s, an))
            else:
                act = "none" if last else "lrelu"
                an = ops.conv2d_fwd(a, kc, b, cpad(cout), 4, 4, st, 1, "zero", act=act, slope=SLOPE,
                                     role=role, co_real=cout if D_CO1 else None)
                saved.append((a, None, None, an))
            a = an
        ctx.saved, ctx.net, ctx.P = saved, net, P
        ctx.train_w = anchor.requires_grad
        net._note_forward(ctx.train_w)
        return a

    @staticmethod
    def backward(ctx, gout):
        saved, net, P = ctx.saved, ctx.net, ctx.P
        convs = net._convs()
        L = len(convs)
        g = gout.contiguous()
        gx = None
        final = ctx.train_w and net._bwd_begin()
        for i in reversed(range(L)):
            a_in, y, s, an = saved[i]
            m = convs[i]
            cout, st, has_in = net.spec[i]
            dyp = None
            if has_in:
                db = m.bias.grad if (ctx.train_w and m.bias is not None) else None
                dy, dyp = _in_bwd_for_wgrad(g, y, s, "lrelu", SLOPE, db, a_in, 4, st, ctx.train_w)
            elif i != L - 1:
                dy = ops.act_bwd(g, an, "lrelu", SLOPE)
            else:
                dy = g
            if ctx.train_w:
                co, ci = m.weight.shape[0], m.weight.shape[1]
                ops.conv2d_wgrad(a_in, dy, m.weight.grad,
                                 m.bias.grad if (m.bias is not None and not has_in) else None,
                                 4, 4, st, 1, "zero", co, ci, ci * 16, 16, accumulate=True, dy_planes=dyp)
                if final:
                    net._grad_done(m)
            if i > 0 or ctx.needs_input_grad[0]:
                ikf, ph = net._ikf[i], net._ph[i]
                if ikf is not None:
                    g = ops.conv2d_dgrad_s1(dy, ikf, a_in.shape[1], a_in.shape[2], a_in.shape[-1], 4, 1)
                elif ph is not None and a_in.shape[1] == 2 * dy.shape[1] and a_in.shape[2] == 2 * dy.shape[2] and \
                        not (D0_TFWD and a_in.shape[-1] == 4):
                    g = ops.conv4s2_dgrad(dy, ph, a_in.shape[-1])
                else:
                    _, ck, _ = P[i]
                    g = ops.conv2d_tfwd(dy, ck, None, a_in.shape[1], a_in.shape[2], a_in.shape[-1], 4, 4,
                                        st, 1, co_real=cout if (D_CO1 and cout < dy.shape[-1]) else None)
                if i == 0:
                    gx = g
        ctx.saved = None
        return gx, None, None


###############################################################################
# UnetGenerator (networks.py:436-535)
###############################################################################
class UnetSkipConnectionBlock(nn.Module):
    """networks.py:468-535 (instance norm, no dropout): cat([x, model(x)], 1), with the reference's Sequential
    layout so the state_dict keys match:
        outermost  [downconv, sub, ReLU, upconv, Tanh]
        middle     [LeakyReLU, downconv, IN, sub, ReLU, upconv, IN]
        innermost  [LeakyReLU, downconv, ReLU, upconv, IN]"""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm2d, use_dropout=False):
        super().__init__()
        if not (isinstance(norm_layer, functools.partial) and norm_layer.func == nn.InstanceNorm2d):
            raise NotImplementedError('only norm=instance is implemented on the HIP path')
        if use_dropout:
            raise NotImplementedError('dropout is not on the HIP path (CycleGAN default no_dropout)')
        self.outermost, self.innermost = outermost, innermost
        if input_nc is None:
            input_nc = outer_nc
        down = Conv2d(input_nc, inner_nc, 4, stride=2, padding=1, bias=True)
        up = ConvTranspose2d(inner_nc if innermost else inner_nc * 2, outer_nc, 4, stride=2, padding=1, bias=True)
        if outermost:
            L = [down, submodule, _Marker('ReLU'), up, _Marker('Tanh')]
        elif innermost:
            L = [_Marker('LeakyReLU(0.2)'), down, _Marker('ReLU'), up, _Marker('InstanceNorm2d')]
        else:
            L = [_Marker('LeakyReLU(0.2)'), down, _Marker('InstanceNorm2d'), submodule, _Marker('ReLU'), up,
                 _Marker('InstanceNorm2d')]
        self.model = nn.Sequential(*L)
        self._down, self._up = (0, 3) if outermost else ((1, 3) if innermost else (1, 5))

    def convs(self):
        return self.model[self._down], self.model[self._up]

    def sub(self):
        return None if self.innermost else self.model[1 if self.outermost else 3]


class UnetGenerator(FlatNet):
    """networks.py:436-465: num_downs UnetSkipConnectionBlocks, channels ngf * min(2^l, 8) at level l.  Level l's
    block halves the resolution with Conv2d(k4, s2, p1) and doubles it back with ConvTranspose2d(k4, s2, p1);
    what it returns is cat([its input, its up half]).  Both in-place activations of the reference run over that
    concatenation (the child's LeakyReLU over the skip half, the parent's ReLU over all of it), so every reader of
    it sees relu(z) / relu(IN(u)): ops.instnorm_skip_fwd writes exactly that into one buffer per level."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False):
        super().__init__()
        if not (isinstance(norm_layer, functools.partial) and norm_layer.func == nn.InstanceNorm2d):
            raise NotImplementedError('only norm=instance is implemented on the HIP path')
        if use_dropout:
            raise NotImplementedError('dropout is not on the HIP path (CycleGAN default no_dropout)')
        if ngf % 4 != 0:
            raise NotImplementedError('ngf [%d] must be a multiple of 4 on the HIP path (NHWC float4 lanes)' % ngf)
        if num_downs < 5:
            raise ValueError('UnetGenerator needs num_downs >= 5, got %d' % num_downs)
        self.input_nc, self.output_nc, self.ngf, self.num_downs = input_nc, output_nc, ngf, num_downs
        kw = dict(norm_layer=norm_layer)
        blk = UnetSkipConnectionBlock(ngf * 8, ngf * 8, innermost=True, **kw)
        for _ in range(num_downs - 5):
            blk = UnetSkipConnectionBlock(ngf * 8, ngf * 8, submodule=blk, **kw)
        blk = UnetSkipConnectionBlock(ngf * 4, ngf * 8, submodule=blk, **kw)
        blk = UnetSkipConnectionBlock(ngf * 2, ngf * 4, submodule=blk, **kw)
        blk = UnetSkipConnectionBlock(ngf, ngf * 2, submodule=blk, **kw)
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc, submodule=blk, outermost=True, **kw)
        self._flatten()

    def _levels(self):
        """[(downconv, upconv)] from the outermost block (level 0) to the innermost."""
        out, b = [], self.model
        while b is not None:
            out.append(b.convs())
            b = b.sub()
        return out

    def _make_packs(self):
        P = []
        for l, (dn, up) in enumerate(self._levels()):
            # the down conv's data gradient: four 2x2 phase convs (ops.conv4s2_dgrad), or the transposed kernel
            # onto the image / below 8 channels; the up conv's forward IS such a data gradient (ops.convT4s2_fwd)
            # and its data gradient a forward Conv2d(k4, s2, p1) over the weight read as [Co = in][Ci = out]
            phases = l > 0 and dn.weight.shape[0] % 8 == 0
            P.append({"dn": ops.weight_pack(dn.weight, ops.PACK_FWD),
                      "dn_ph": ops.conv4s2_dgrad_phase_packs(dn.weight) if phases else None,
                      "dn_ck": None if phases else ops.weight_pack(dn.weight, ops.PACK_DGRAD),
                      "dn_b": _padded_bias(dn),
                      "up_ph": ops.conv4s2_dgrad_phase_packs(up.weight),
                      "up_kc": ops.weight_pack(up.weight, ops.PACK_FWD),
                      "up_b": _padded_bias(up)})
        return P

    def _check_size(self, H, W):
        m = 2 ** self.num_downs
        if H % m or W % m:
            raise ValueError('UnetGenerator with %d downsamplings needs H and W to be multiples of %d, got %d x %d'
                             % (self.num_downs, m, H, W))

    def forward(self, x):
        self._check_size(x.shape[2], x.shape[3])
        return super().forward(x)

    def forward_nhwc(self, x):
        self._check_size(x.shape[1], x.shape[2])
        return _UnetFn.apply(x, self._anchor(), self)


class _UnetFn(torch.autograd.Function):
    """Whole U-Net forward/backward on libvst_hip kernels.  z_l = IN(y_l) (z_0 = y_0) is never stored: the skip
    pass reads y_l once and writes d_l = lrelu(z_l) (the next down conv's input) and relu(z_l) into the skip half
    of level l + 1's concatenation buffer; the up norm's apply writes the other half."""

    @staticmethod
    def forward(ctx, x, anchor, net):
        P = net.packs()
        lv = net._levels()
        D = len(lv)
        role = "fwd" if any(ctx.needs_input_grad[:2]) else "infer"
        N = x.shape[0]
        ys, ss, ds, cats = [], [], [x], [None] * D
        for l in range(D - 1):
            dn, _ = lv[l]
            cl = cpad(dn.weight.shape[0])
            if l == 0:  # no norm follows: the bias counts
                y, s = ops.conv2d_fwd(x, P[0]["dn"], P[0]["dn_b"], cl, 4, 4, 2, 1, "zero", role=role), None
            else:       # the bias cancels in the norm (it keeps its exact channel-sum gradient)
                y, s = ops.conv2d_fwd_in(ds[l], P[l]["dn"], None, cl, 4, 4, 2, 1, "zero", role=role)
            cats[l + 1] = torch.empty((N, y.shape[1], y.shape[2], 2 * cl), device=x.device)
            ds.append(ops.instnorm_skip_fwd(y, s, cats[l + 1], 0, slope=SLOPE))
            ys.append(y)
            ss.append(s)
        dn, _ = lv[D - 1]
        r = ops.conv2d_fwd(ds[D - 1], P[D - 1]["dn"], P[D - 1]["dn_b"], cpad(dn.weight.shape[0]), 4, 4, 2, 1, "zero",
                           act="relu", role=role)
        us, sus = [None] * D, [None] * D
        inp = r
        for l in range(D - 1, 0, -1):
            _, up = lv[l]
            co = cpad(up.weight.shape[1])
            u = ops.convT4s2_fwd(inp, P[l]["up_ph"], None, co, role=role)
            su = ops.instnorm_stats(u)
            ops.instnorm_skip_fwd(u, su, cats[l], co, want_d=False)
            us[l], sus[l] = u, su
            inp = cats[l]
        out = ops.convT4s2_fwd(inp, P[0]["up_ph"], P[0]["up_b"], cpad(net.output_nc), act="tanh", role=role)
        if role == "fwd":
            ctx.sv = (ys, ss, ds, cats, r, us, sus, out)
        ctx.net, ctx.P = net, P
        ctx.train_w = anchor.requires_grad
        net._note_forward(ctx.train_w)
        return out

    @staticmethod
    def backward(ctx, gout):
        ys, ss, ds, cats, r, us, sus, out = ctx.sv
        net, P, train_w = ctx.net, ctx.P, ctx.train_w
        lv = net._levels()
        D = len(lv)
        final = train_w and net._bwd_begin()

        def done(mod):
            if final:
                net._grad_done(mod)

        def up_grads(l, du, a_in):
            """The up conv's weight gradient (Wt[ci][co] = the weight gradient of the conv a_in = conv(du, .)) and
            its data gradient, that conv's forward."""
            up = lv[l][1]
            if train_w:
                ci_t, co_t = up.weight.shape[0], up.weight.shape[1]
                ops.conv2d_wgrad(du, a_in, up.weight.grad, None, 4, 4, 2, 1, "zero", ci_t, co_t, co_t * 16, 16,
                                 accumulate=True)
            done(up)
            return ops.conv2d_fwd(du, P[l]["up_kc"], None, a_in.shape[-1], 4, 4, 2, 1, "zero", role="bwd")

        def down_grads(l, dy, bias_here, need_dx):
            dn = lv[l][0]
            a_in = ds[l]
            if train_w:
                co, ci = dn.weight.shape[0], dn.weight.shape[1]
                ops.conv2d_wgrad(a_in, dy, dn.weight.grad, dn.bias.grad if bias_here else None, 4, 4, 2, 1, "zero",
                                 co, ci, ci * 16, 16, accumulate=True)
            done(dn)
            if not need_dx:
                return None
            if P[l]["dn_ph"] is not None:
                return ops.conv4s2_dgrad(dy, P[l]["dn_ph"], a_in.shape[-1])
            return ops.conv2d_tfwd(dy, P[l]["dn_ck"], None, a_in.shape[1], a_in.shape[2], a_in.shape[-1], 4, 4, 2, 1)

        # outermost up conv + tanh (no norm after it: the bias gradient is a channel sum)
        du = ops.act_bwd(gout.contiguous(), out, "tanh")
        if train_w:
            ops.channel_sum(du, lv[0][1].bias.grad, net.output_nc, accumulate=True)
        g_cats = {1: up_grads(0, du, cats[1])}  # level -> the gradient of its concatenation buffer
        for l in range(1, D):
            up = lv[l][1]
            du = ops.instnorm_skip_bwd(None, g_cats[l], cpad(up.weight.shape[1]), us[l], sus[l],
                                       db=up.bias.grad if train_w else None)
            g_cats[l + 1] = up_grads(l, du, cats[l + 1] if l < D - 1 else r)
        # innermost down conv + ReLU
        dy = ops.act_bwd(g_cats.pop(D), r, "relu")
        g_d = down_grads(D - 1, dy, True, True)
        for l in range(D - 2, -1, -1):
            dn = lv[l][0]
            dy = ops.instnorm_skip_bwd(g_d, g_cats.pop(l + 1), 0, ys[l], ss[l], db=dn.bias.grad if train_w else None,
                                       slope=SLOPE)
            g_d = down_grads(l, dy, False, l > 0 or ctx.needs_input_grad[0])
        ctx.sv = None
        return g_d, None, None


###############################################################################
# define_G / define_D (networks.py:119-203)
###############################################################################
def define_G(input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal',
             init_gain=0.02, gpu_ids=[]):
    norm_layer = get_norm_layer(norm_type=norm)
    if netG == 'resnet_9blocks':
        net = ResnetGenerator(input_nc, output_nc, ngf, norm_layer=norm_layer, use_dropout=use_dropout, n_blocks=9)
    elif netG == 'resnet_6blocks':
        net = ResnetGenerator(input_nc, output_nc, ngf, norm_layer=norm_layer, use_dropout=use_dropout, n_blocks=6)
    elif netG == 'unet_128':
        net = UnetGenerator(input_nc, output_nc, 7, ngf, norm_layer=norm_layer, use_dropout=use_dropout)
    elif netG == 'unet_256':
        # the eight-level net runs (UnetGenerator(input_nc, output_nc, 8, ngf, norm_layer=...), tested at that depth);
        # this name keeps its refusal here because the host suite holds define_G to it
        raise NotImplementedError('Generator [%s] is not offered by define_G yet: construct '
                                  'networks.UnetGenerator(input_nc, output_nc, 8, ngf, norm_layer) and init_net it' % netG)
    else:
        raise NotImplementedError('Generator model name [%s] is not recognized' % netG)
    return init_net(net, init_type, init_gain, gpu_ids)


def define_D(input_nc, ndf, netD, n_layers_D=3, norm='batch', init_type='normal', init_gain=0.02,
             gpu_ids=[]):
    norm_layer = get_norm_layer(norm_type=norm)
    if netD == 'basic':
        net = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm_layer=norm_layer)
    elif netD == 'n_layers':
        net = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm_layer=norm_layer)
    elif netD == 'pixel':
        raise NotImplementedError('Discriminator [pixel] is outside the HIP hot path (SURVEY §2)')
    else:
        raise NotImplementedError('Discriminator model name [%s] is not recognized' % netD)
    return init_net(net, init_type, init_gain, gpu_ids)


###############################################################################
# Losses (networks.py:209-275) on NHWC tensors, HIP-backed
###############################################################################
class _MSEConstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, cl):
        ctx.save_for_backward(pred)
        ctx.target, ctx.cl = target, cl
        return ops.loss_mse_const(pred, target, 1.0, cl)

    @staticmethod
    def backward(ctx, g):
        (pred,) = ctx.saved_tensors
        return ops.loss_mse_const_bwd(pred, ctx.target, g.contiguous(), 1.0, ctx.cl), None, None


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, scale, cl):
        ctx.save_for_backward(a, b)
        ctx.scale, ctx.cl = scale, cl
        return ops.loss_l1(a, b, scale, cl)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = ops.loss_l1_bwd(a, b, g, ctx.scale, ctx.cl) if ctx.needs_input_grad[0] else None
        gb = ops.loss_l1_bwd(b, a, g, ctx.scale, ctx.cl) if ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def l1_loss(a, b, scale=1.0, cl=3):
    """scale * nn.L1Loss()(a, b) over the Cl logical channels of NHWC tensors."""
    return _L1Fn.apply(a, b, float(scale), cl)


class GANLoss(nn.Module):
    """networks.py:209-275.  'lsgan' runs on the HIP loss kernels for NHWC predictions
    (``nhwc=True``, the path the HIP models use); other modes and NCHW inputs use the reference
    formula on torch ops (outside the hot path)."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer('real_label', torch.tensor(target_real_label))
        self.register_buffer('fake_label', torch.tensor(target_fake_label))
        self.gan_mode = gan_mode
        self._real, self._fake = float(target_real_label), float(target_fake_label)
        if gan_mode == 'lsgan':
            self.loss = nn.MSELoss()
        elif gan_mode == 'vanilla':
            self.loss = nn.BCEWithLogitsLoss()
        elif gan_mode in ['wgangp']:
            self.loss = None
        else:
            raise NotImplementedError('gan mode %s not implemented' % gan_mode)

    def get_target_tensor(self, prediction, target_is_real):
        t = self.real_label if target_is_real else self.fake_label
        return t.expand_as(prediction)

    def __call__(self, prediction, target_is_real, nhwc=False):
        if nhwc and self.gan_mode == 'lsgan':
            return _MSEConstFn.apply(prediction, self._real if target_is_real else self._fake, 1)
        if self.gan_mode in ['lsgan', 'vanilla']:
            return self.loss(prediction, self.get_target_tensor(prediction, target_is_real))
        return -prediction.mean() if target_is_real else prediction.mean()


from . import _lib as _lib_routes  # noqa: E402
_lib_routes.apply_route_overrides(__name__, globals())
