"""Drop-in for methods/learning-based/fs_lib.py (warp, 5-39), HIP-backed.

``warp(x, flo)`` = grid_sample(x, grid) * (grid_sample(ones, grid) >= 0.9999) with the grid
normalised by max(W-1, 1) / max(H-1, 1) and the container-default align_corners=False — the
sample and its validity come out of one kernel pass (vst_warp_masked_fwd); the backward scatters
only through kept samples (no gradient flows into the flow or the mask, as in the reference).
"""
import torch

from . import ops
from .flowtools import _nchw_to_nhwc, _nhwc_to_nchw


class _WarpMaskedNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow, align_corners):
        ctx.save_for_backward(flow)
        ctx.align = align_corners
        return ops.warp_masked_nhwc(x, flow, align_corners)

    @staticmethod
    def backward(ctx, g):
        (flow,) = ctx.saved_tensors
        return ops.warp_masked_bwd_nhwc(g.contiguous(), flow, ctx.align), None, None


def warp_nhwc(x, flow, align_corners=False):
    """x: [B,H,W,Cs] (Cs % 4 == 0), flow: [B,2,H,W] -> masked warp [B,H,W,Cs]."""
    return _WarpMaskedNHWC.apply(x.contiguous(), flow.contiguous().float(), bool(align_corners))


def warp(x, flo):
    """fs_lib.py:5-39 on NCHW x [B,C,H,W] and flow [B,2,H,W] (pixels, channel 0 = x)."""
    C = x.shape[1]
    return _nhwc_to_nchw(warp_nhwc(_nchw_to_nhwc(x), flo), C)


class _TemporalLossNHWC(torch.autograd.Function):
    """The users of ``warp`` in the reference (fs_huang.py:55-56, fs_reconet.py:61-69) as one fused
    node: warp, validity, mask, optional input term, squared mean (ops.temporal_sqdiff).  ``pair``:
    a and b are the two halves of one batch tensor ``ab`` ([2B,...]: frames 1 then frames 2, the way the
    video trainers run the net), so the backward fills one gradient tensor and no slice node copies."""

    @staticmethod
    def forward(ctx, a, b, flow, mask, scale, ab_scale, cl, i1, i2, pair):
        ctx.save_for_backward(a, b, flow, mask, i1, i2)
        ctx.conf = (scale, ab_scale, cl, pair)
        if pair:
            a, b = a[:a.shape[0] // 2], a[a.shape[0] // 2:]
        return ops.temporal_sqdiff(a, b, flow, mask, scale, cl, ab_scale, None if i1 is None else (i1, i2))

    @staticmethod
    def backward(ctx, g):
        a, b, flow, mask, i1, i2 = ctx.saved_tensors
        scale, ab_scale, cl, pair = ctx.conf
        need_a, need_b = (True, True) if pair else ctx.needs_input_grad[:2]
        if pair:
            B = a.shape[0] // 2
            gab = torch.empty_like(a)
            a, b = a[:B], a[B:]
            ga, gb = gab[:B].zero_(), gab[B:]
        else:
            ga = torch.zeros_like(a) if need_a else None
            gb = torch.empty_like(b) if need_b else None
        if need_a or need_b:
            ops.temporal_sqdiff_bwd(a, b, flow, mask, g.contiguous(), ga, gb, scale, cl, ab_scale,
                                    None if i1 is None else (i1, i2))
        return ((gab, None) if pair else (ga, gb)) + (None,) * 8


def _temporal_args(flow, mask, inputs):
    i1, i2 = (None, None) if inputs is None else (inputs[0].detach().contiguous(), inputs[1].detach().contiguous())
    return flow.detach().contiguous().float(), mask.detach().contiguous().float(), i1, i2


def temporal_loss_nhwc(a, b, flow, mask, scale, inputs=None, ab_scale=1.0, cl=None):
    """scale * mean((mask * (s*b - warp(s*a, flow) - r))^2) as a device scalar, differentiable in a and b.
    a, b: [B,H,W,Cs] (cl logical channels, default Cs); flow [B,2,H,W]; mask [B,1,H,W]; s = ab_scale.
    inputs = (i1, i2), NHWC4 input frames: r = the luminance-weighted input term of fs_reconet.py:66-67
    (a, b then are NHWC4 images, cl = 3); no gradient flows into flow, mask or the inputs."""
    flow, mask, i1, i2 = _temporal_args(flow, mask, inputs)
    return _TemporalLossNHWC.apply(a.contiguous(), b.contiguous(), flow, mask, float(scale), float(ab_scale), cl,
                                   i1, i2, False)


def temporal_loss_pair_nhwc(ab, flow, mask, scale, inputs=None, ab_scale=1.0, cl=None):
    """temporal_loss_nhwc(ab[:B], ab[B:], ...) for the frame pairs stacked as one [2B,H,W,Cs] batch."""
    if ab.shape[0] % 2:
        raise ValueError("temporal_loss_pair_nhwc: the batch holds frame pairs (even size), got %d" % ab.shape[0])
    flow, mask, i1, i2 = _temporal_args(flow, mask, inputs)
    return _TemporalLossNHWC.apply(ab.contiguous(), None, flow, mask, float(scale), float(ab_scale), cl, i1, i2,
                                   True)


class _RuderStackNHWC(torch.autograd.Function):
    """The recurrent input of fs_ruder.py:52 as one node with two outputs: x, the net's 8-channel-padded input,
    and w, the warped previous frame the temporal loss reads.  Differentiable in y_prev only; the backward takes
    both output gradients (the net's input gradient and the temporal loss's) in ONE scatter, so autograd never
    adds two image tensors."""

    @staticmethod
    def forward(ctx, y_prev, img, flow, mask, scale):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(flow)
        ctx.scale = scale
        return ops.ruder_stack(y_prev, img, flow, mask, scale)

    @staticmethod
    def backward(ctx, gx, gw):
        if not ctx.needs_input_grad[0] or (gx is None and gw is None):
            return None, None, None, None, None
        (flow,) = ctx.saved_tensors
        gx = None if gx is None else gx.contiguous()
        gw = None if gw is None else gw.contiguous()
        N, _, H, W = flow.shape
        gy = torch.zeros((N, H, W, 4), device=flow.device, dtype=torch.float32)
        ops.ruder_stack_bwd(gx, gw, flow, gy, ctx.scale)
        return gy, None, None, None, None


def ruder_stack_nhwc(y_prev, img, flow, mask, scale=1.0 / 255.0):
    """(x, w): x [B,H,W,8] = (img rgb, mask, warp(scale * y_prev, flow) rgb, 0), the Ruder net's input for the next
    frame (fs_ruder.py:52), and w [B,H,W,4] = the same warped frame.  y_prev: previous styled frame, NHWC4 0..255;
    img NHWC4 [0,1]; flow [B,2,H,W]; mask [B,1,H,W].  Differentiable in y_prev only."""
    return _RuderStackNHWC.apply(y_prev.contiguous(), img.detach().contiguous(), flow.detach().contiguous().float(),
                                 mask.detach().contiguous().float(), float(scale))


def ruder_blank_nhwc(img):
    """The input of the branch without a previous frame (fs_ruder.py:78): (img rgb, 0, 0, 0, 0, 0), [B,H,W,8]."""
    return ops.ruder_stack(None, img.detach().contiguous(), None, None, want_w=False)[0]


class _RuderTemporalNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, y, mask, scale, ab_scale):
        ctx.save_for_backward(w, y, mask)
        ctx.conf = (scale, ab_scale)
        return ops.ruder_temporal(w, y, mask, scale, ab_scale)

    @staticmethod
    def backward(ctx, g):
        w, y, mask = ctx.saved_tensors
        gw, gy = ops.ruder_temporal_bwd(w, y, mask, g.contiguous(), *ctx.conf, need_w=ctx.needs_input_grad[0],
                                        need_y=ctx.needs_input_grad[1])
        return gw, gy, None, None, None


def ruder_temporal_nhwc(w, y, mask, scale, ab_scale=1.0 / 255.0):
    """scale * mean((mask * (w - ab_scale * y))^2) over the image channels (fs_ruder.py:97) as a device scalar,
    differentiable in w (the warped previous frame of ruder_stack_nhwc) and y (the styled frame, NHWC4 0..255)."""
    return _RuderTemporalNHWC.apply(w.contiguous(), y.contiguous(), mask.detach().contiguous().float(),
                                    float(scale), float(ab_scale))
