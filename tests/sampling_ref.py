"""CPU references (numpy / torch fp64), input generators and comparison functions for the kernels that
gather or scatter at data-dependent positions: the flow warp and its input gradient, the fused temporal
loss, the forward/backward consistency mask (csrc/flow.hip, csrc/flow_det.hip), the correlation pyramid
and lookup (csrc/style.hip) and RAFT's convex upsampling (csrc/raft.hip).  tests/test_gpu_sampling.py
feeds the comparison functions with the device's results, tests/test_sampling_ref_host.py with stock
torch fp32 results (they must pass: the bounds hold for the references alone) and with deliberately
wrong results (`mutate=`, they must be rejected: the cases discriminate).

Two tiers, because bilinear sampling is continuous in the sample position but its floor and validity
decisions are not:

  tight        the sample geometry (x0, y0 and the four weights) comes from the fp32 restatement
               oracle.flow_ref.corner_weights, which tests/test_oracle_golden.py pins to the reference's
               own outputs; the gather, the products and the sums are fp64.  What remains between this
               and a kernel are the roundings of the kernel's own products and sums, which are counted.
  independent  F.grid_sample in fp64 on a grid built in fp64 (autograd for the gradients): shares nothing
               with the restatement.  Its bound is a priori and looser: it has to cover the fp32
               rounding of the sample position.

u = 2^-24 is fp32's unit roundoff throughout.  Every bound below is derived where it is computed; none is
fitted to a device's output.

Flow families leave out NaN, +-inf and any flow whose sample index leaves int32: the reference's own
float -> int conversion is undefined there, so there is nothing to compare against.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref, flow_ref, raft_ref, style_ref

import temporal_style_ref as TS

U = 2.0 ** -24
F64 = torch.float64
f32 = np.float32
f64 = np.float64

MUTATIONS = ("swap_ne_sw", "ignore_align", "chunk0", "image_stride_hw", "swap_hw_norm", "cs_for_cl",
             "gb_pad_unwritten", "lvl_divisor", "transpose_window")

# worst err / bound seen per label in this process (the GPU tests print it at the end of the module)
WORST = {}


def le(err, tol, what, label=None):
    """assert err <= tol everywhere (a NaN fails) after printing the worst ratio; returns that ratio."""
    err, tol = torch.as_tensor(err, dtype=F64), torch.as_tensor(tol, dtype=F64)
    tol = tol.expand_as(err)
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(F64))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not bool(torch.isfinite(err).all()):
        worst = float("inf")
    print(f"{what}: worst err/bound = {worst:.3g} (max err {err.max().item() if err.numel() else 0.0:.3e})")
    if label is not None:
        WORST[label] = max(WORST.get(label, 0.0), worst)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst err/bound {worst:.3g}"
    return worst


def rand(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ============================================================================== flow families
FAMILIES = ("iid", "quarter", "sweep", "oob100", "far", "converge", "ident")
# Seed of every (family, N, H, W): 5 unless 5 puts a sample's validity sum into the band that
# temporal_style_ref.assert_off_threshold refuses; then the next seed that does not (the band never moves).
# tests/test_sampling_ref_host.py asserts the rule for every masked case.
SEED_OVERRIDES = {}


def flow_seed(kind, N, H, W):
    return SEED_OVERRIDES.get((kind, N, H, W), 5)


def make_flow(kind, N, H, W, seed=None):
    """[N, 2, H, W] fp32 flow (channel 0 = x) of a family."""
    seed = flow_seed(kind, N, H, W) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    if kind == "iid":
        return torch.randn(N, 2, H, W, generator=g) * 3.0
    if kind == "quarter":     # multiples of 1/4: with align_corners many samples sit exactly on a pixel centre
        return torch.round(torch.randn(N, 2, H, W, generator=g) * 12.0) / 4.0
    if kind == "oob100":
        return (torch.rand(N, 2, H, W, generator=g) * 2 - 1) * 100.0
    if kind == "far":         # +-1e4 px: every corner of every sample is outside the frame
        return torch.where(torch.rand(N, 2, H, W, generator=g) < 0.5, -1.0, 1.0) * 1e4
    if kind == "converge":    # tests/test_gpu_det.py: everything pulled toward one patch
        f = torch.stack([W / 2 - xs, H / 2 - ys])[None].repeat(N, 1, 1, 1)
        return f + torch.rand(N, 2, H, W, generator=g) * 6 - 3
    if kind == "ident":       # undoes the reference's W / (W - 1) shift: the sample lands on its own pixel
        x64, y64 = torch.arange(W, dtype=F64), torch.arange(H, dtype=F64)
        return torch.stack([((x64 + 0.5) * (W - 1) / W - x64).view(1, W).expand(H, W),
                            ((y64 + 0.5) * (H - 1) / H - y64).view(H, 1).expand(H, W)])[None].repeat(N, 1, 1, 1).float()
    if kind == "sweep":
        # every sample within 2.5 px of one of the four borders of the pixel grid (x = 0, x = W - 1, y = 0,
        # y = H - 1), on either side of it, anywhere along it; the first four pixels of an image aim at the
        # four corners exactly
        d = torch.rand(N, H, W, generator=g) * 5.0 - 2.5
        tx = torch.rand(N, H, W, generator=g) * (W + 1.0) - 1.0
        ty = torch.rand(N, H, W, generator=g) * (H + 1.0) - 1.0
        side = (torch.arange(H * W).view(1, H, W) + torch.arange(N).view(N, 1, 1)) % 4
        tx = torch.where(side == 0, d, torch.where(side == 1, (W - 1.0) + d, tx))
        ty = torch.where(side == 2, d, torch.where(side == 3, (H - 1.0) + d, ty))
        tx, ty = tx.reshape(N, -1), ty.reshape(N, -1)
        for i, (cx, cy) in enumerate(((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0))):
            if i < H * W:
                tx[:, i], ty[:, i] = cx, cy
        return torch.stack([tx.view(N, H, W) - xs, ty.view(N, H, W) - ys], 1).contiguous()
    raise ValueError(kind)


def validity_sums(flow, align=False):
    """temporal_style_ref.validity_sums for either align mode: the fp64 validity sum of every sample."""
    if not align:
        return TS.validity_sums(flow)
    g = _grid64(flow)
    n, _, h, w = flow.shape
    return F.grid_sample(torch.ones(n, 1, h, w, dtype=F64), g, align_corners=True)


def assert_off_threshold(flow, align=False):
    """The rule of temporal_style_ref.assert_off_threshold (the same band) for either align mode."""
    if not align:
        return TS.assert_off_threshold(flow)
    m = validity_sums(flow, True)
    n = int(((m >= 0.9997) & (m <= 0.99995)).sum())
    assert n == 0, "%d samples with a validity sum in [0.9997, 0.99995]: pick another seed" % n
    return float((m < 0.9999).double().mean())


# ============================================================================== warp geometry
def _corner_weights_swapped(flow, H, W, align):
    """MUTATION swap_hw_norm: flow_ref.corner_weights with H and W exchanged in the grid normalisation."""
    N = flow.shape[0]
    w = np.broadcast_to(np.arange(W, dtype=f32)[None, None, :], (N, H, W))
    h = np.broadcast_to(np.arange(H, dtype=f32)[None, :, None], (N, H, W))
    vx, vy = w + flow[:, 0], h + flow[:, 1]
    gx = f32(2.0) * vx / f32(max(H - 1, 1)) - f32(1.0)
    gy = f32(2.0) * vy / f32(max(W - 1, 1)) - f32(1.0)
    ix, iy = flow_ref._src_index(gx.astype(f32), W, align), flow_ref._src_index(gy.astype(f32), H, align)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    we, wn = (ix - fx0).astype(f32), (iy - fy0).astype(f32)
    e, s = (f32(1) - we).astype(f32), (f32(1) - wn).astype(f32)
    wts = [(s * e).astype(f32), (s * we).astype(f32), (wn * e).astype(f32), (wn * we).astype(f32)]
    return fx0.astype(np.int64), fy0.astype(np.int64), wts


def geometry(flow, align=False, mutate=None):
    """(cx[4], cy[4], w[4], inb[4], valid): corner coordinates, fp32 weights and in-frame flags in nw, ne, sw,
    se order, and the fs_lib validity of every sample by the restatement's rule (in-frame weights summed in
    that order in fp32, kept iff the sum >= 0.9999)."""
    fl = np.ascontiguousarray(flow.numpy(), dtype=f32)
    N, _, H, W = fl.shape
    if mutate == "ignore_align":
        align = False
    cw = _corner_weights_swapped if mutate == "swap_hw_norm" else flow_ref.corner_weights
    x0, y0, w = cw(fl, H, W, bool(align))
    if mutate == "swap_ne_sw":
        w = [w[0], w[2], w[1], w[3]]
    cy, cx = [y0, y0, y0 + 1, y0 + 1], [x0, x0 + 1, x0, x0 + 1]
    inb = [(cy[k] >= 0) & (cy[k] < H) & (cx[k] >= 0) & (cx[k] < W) for k in range(4)]
    m = np.zeros((N, H, W), f32)
    for k in range(4):
        m = (m + np.where(inb[k], w[k], f32(0))).astype(f32)
    valid = ~(m < f32(0.9999)) & (m > 0)
    return cx, cy, w, inb, valid


def _grid64(flow):
    """The reference's sampling grid in fp64: 2 (p + f) / max(size - 1, 1) - 1, [N, H, W, 2]."""
    flow = flow.double()
    n, _, h, w = flow.shape
    xx = torch.arange(w, dtype=F64).view(1, 1, w).expand(n, h, w)
    yy = torch.arange(h, dtype=F64).view(1, h, 1).expand(n, h, w)
    return torch.stack([2.0 * (xx + flow[:, 0]) / max(w - 1, 1) - 1.0, 2.0 * (yy + flow[:, 1]) / max(h - 1, 1) - 1.0], -1)


def position_error(flow):
    """A priori bound (dx, dy) [N, H, W] on the error of an fp32 sample position in pixels.

    The position is fma(g + 1, size / 2, -0.5) (or (g + 1) * ((size - 1) / 2)) of g = 2 (p + f) / d - 1,
    d = max(size - 1, 1): four roundings (p + f, the division, - 1, the fma; 2 * . and g + 1 near 0 are exact or
    absorbed), each of a quantity that in pixel units is at most (|p + f| size / d + size) <= 2 (|p + f| + size).
    So delta <= 4 u * 2 (|p + f| + size) = 8 u (|p + f| + size) per axis."""
    flow = flow.double()
    n, _, h, w = flow.shape
    xx = torch.arange(w, dtype=F64).view(1, 1, w)
    yy = torch.arange(h, dtype=F64).view(1, h, 1)
    return 8 * U * ((xx + flow[:, 0]).abs() + w), 8 * U * ((yy + flow[:, 1]).abs() + h)


# ============================================================================== warp forward
def warp_fwd_tight(x, flow, align=False, masked=False, mutate=None):
    """x [N, H, W, C] fp32 NHWC, flow [N, 2, H, W] fp32 -> (ref, bound) fp64 NHWC and valid [N, H, W] bool.

    ref = sum_k w_k v_k in fp64 with the restatement's fp32 weights.  A kernel evaluates it as one multiply
    and three fmas (bilin.h bilerp), four roundings of partial sums none larger than S = sum_k |w_k v_k|, so
    |got - ref| <= 4 u S; where every corner is outside the frame (and, masked, where the sample is invalid)
    S = 0 and the result is exactly 0."""
    cx, cy, w, inb, valid = geometry(flow, align, mutate)
    xs = x.numpy().astype(f64)
    N, H, W, C = xs.shape
    flat = xs.reshape(-1)
    # MUTATION image_stride_hw: image n starts H*W floats after image n - 1 instead of H*W*C
    img = np.arange(N)[:, None, None] * (H * W if mutate == "image_stride_hw" else H * W * C)
    # MUTATION chunk0: every corner reads the first float4 of its pixel (the dropped "+ c4")
    ch = np.arange(C) % 4 if mutate == "chunk0" else np.arange(C)
    ref, S = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for k in range(4):
        yy, xx = np.clip(cy[k], 0, H - 1), np.clip(cx[k], 0, W - 1)
        v = flat[(img + (yy * W + xx) * C)[..., None] + ch]
        t = np.where(inb[k][..., None], w[k].astype(f64)[..., None] * v, 0.0)
        ref += t
        S += np.abs(t)
    if masked:
        ref, S = ref * valid[..., None], S * valid[..., None]
    return torch.from_numpy(ref), torch.from_numpy(4 * U * S), torch.from_numpy(valid)


def warp_fwd_indep(x, flow, align=False, masked=False):
    """(ref, bound) fp64 NHWC from F.grid_sample in fp64 (masked: times the fp64 validity sum >= 0.9999), and
    the keep mask [N, H, W].

    The zero-padded bilinear interpolant of channel c of image n moves by at most 2 max|x_nc| per pixel of
    sample displacement along an axis (neighbouring samples differ by at most that), so the fp32 position error
    (position_error) costs 2 (dx + dy) max|x_nc|; the weights' own roundings (two subtractions and a product
    each) and the four roundings of the sum are covered by 8 u max|x_nc|."""
    x64 = x.double().permute(0, 3, 1, 2)
    grid = _grid64(flow)
    out = F.grid_sample(x64, grid, mode="bilinear", padding_mode="zeros", align_corners=bool(align))
    keep = torch.ones(x.shape[:3], dtype=torch.bool)
    if masked:
        keep = (validity_sums(flow, align) >= 0.9999)[:, 0]
        out = out * keep[:, None]
    dx, dy = position_error(flow)
    mx = x64.abs().amax(dim=(2, 3))                                   # [N, C]
    bound = (2 * (dx + dy) + 8 * U)[..., None] * mx[:, None, None, :]
    return out.permute(0, 2, 3, 1).contiguous(), bound, keep


@functools.lru_cache(maxsize=4)
def warp_source(N, H, W, C):
    """The warped image: randn plus 10 * channel, so that a wrong channel chunk cannot cancel."""
    return (rand(100 + C, (N, H, W, C)) + 10.0 * torch.arange(C, dtype=torch.float32)).contiguous()


@functools.lru_cache(maxsize=8)
def warp_case(shape, family, align, masked):
    N, H, W, C = shape
    x, flow = warp_source(N, H, W, C), make_flow(family, N, H, W)
    if masked:
        assert_off_threshold(flow, align)
    return dict(x=x, flow=flow, shape=shape, family=family, align=align, masked=masked,
                tight=warp_fwd_tight(x, flow, align, masked), indep=warp_fwd_indep(x, flow, align, masked))


def check_warp_fwd(got, case, label="warp_fwd"):
    """The forward comparison: both tiers, exact zeros where the reference is exactly 0."""
    got = got.detach().cpu().to(F64)
    tag = "%s %s %s align=%d masked=%d" % (label, case["shape"], case["family"], case["align"], case["masked"])
    ref, bound, valid = case["tight"]
    assert got.shape == ref.shape
    le((got - ref).abs(), bound, tag + " tight", label + "/tight")
    zero = bound == 0
    assert bool((got[zero] == 0).all()), tag + ": nonzero where every corner is outside"
    if case["family"] == "far":
        assert bool(zero.all()) and bool((got == 0).all()), tag + ": far flow must give all zeros"
    if case["masked"]:
        assert bool((got[~valid] == 0).all()), tag + ": an invalid sample is not exactly 0"
    iref, ibound, keep = case["indep"]
    assert bool((keep == valid).all()) or not case["masked"], tag + ": the tiers disagree on validity"
    le((got - iref).abs(), ibound, tag + " independent", label + "/independent")


# ============================================================================== warp backward
def _scatter16(flow, align, e, cl):
    """sum of e [N, H, W, cl] over every sample whose 4x4 neighbourhood (x0 - 1 .. x0 + 2) holds the target."""
    cx, cy, _, _, _ = geometry(flow, align)
    N, _, H, W = flow.shape
    out = torch.zeros(N * H * W, cl, dtype=F64)
    img = np.broadcast_to(np.arange(N)[:, None, None] * (H * W), (N, H, W))
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            yy, xx = cy[0] + oy, cx[0] + ox
            sel = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            out.index_add_(0, torch.from_numpy((img + yy * W + xx)[sel]), torch.from_numpy(np.ascontiguousarray(e[sel])))
    out = out.numpy()
    return out.reshape(N, H, W, cl)


def warp_bwd_tight(gout, flow, align=False, masked=False, mutate=None, cl=None, negate=False, preset=None):
    """gout [N, H, W, Cs] -> (ref, bound, sum|c|) fp64 [N, H, W, Cs]: the fp64 scatter of w_k * gout (first cl
    channels) with the restatement's fp32 weights, added to preset if given.

    Per target element the atomic path rounds each of its n_t products once and each of its n_t adds once, an
    add being the rounding of a partial sum no larger than |preset| + sum_i |c_i|:
    |got - ref| <= (n_t + 1) u (sum_i |c_i| + |preset|)."""
    cx, cy, w, inb, valid = geometry(flow, align, mutate)
    g = gout.numpy().astype(f64)
    N, H, W, Cs = g.shape
    cl = Cs if cl is None else cl
    P = N * H * W
    sums, abss, cnt = torch.zeros(P, cl, dtype=F64), torch.zeros(P, cl, dtype=F64), torch.zeros(P, dtype=F64)
    img = np.broadcast_to(np.arange(N)[:, None, None] * (H * W), (N, H, W))
    for k in range(4):
        sel = inb[k] & valid if masked else inb[k]
        tgt = torch.from_numpy((img + cy[k] * W + cx[k])[sel])
        c = torch.from_numpy(w[k][sel].astype(f64)[:, None] * g[sel][:, :cl])
        sums.index_add_(0, tgt, -c if negate else c)
        abss.index_add_(0, tgt, c.abs())
        cnt.index_add_(0, tgt, torch.ones(len(tgt), dtype=F64))
    sums, abss, cnt = sums.numpy(), abss.numpy(), cnt.numpy()
    ref, ab, bound = np.zeros((P, Cs)), np.zeros((P, Cs)), np.zeros((P, Cs))
    ref[:, :cl], ab[:, :cl] = sums, abss
    pre = np.zeros((P, Cs)) if preset is None else preset.numpy().astype(f64).reshape(P, Cs)
    bound[:, :cl] = (cnt + 1)[:, None] * U * (abss + np.abs(pre[:, :cl]))
    ref = ref + pre
    sh = (N, H, W, Cs)
    return torch.from_numpy(ref.reshape(sh)), torch.from_numpy(bound.reshape(sh)), torch.from_numpy(ab.reshape(sh))


def warp_bwd_indep(gout, flow, align=False, masked=False):
    """(ref, extra) fp64 NHWC: autograd of the fp64 grid_sample, and what the fp32 sample position adds to the
    tight bound.  A target's weight in a sample is a tent function of the sample position, 1-Lipschitz per axis,
    so a position error (dx, dy) moves a contribution by at most (dx + dy) |gout|; which targets a sample touches
    may differ between the two evaluations, so the term is spread over the 4x4 neighbourhood of its floor."""
    N, H, W, C = gout.shape
    x = torch.zeros(N, C, H, W, dtype=F64, requires_grad=True)
    out = F.grid_sample(x, _grid64(flow), mode="bilinear", padding_mode="zeros", align_corners=bool(align))
    if masked:
        out = out * (validity_sums(flow, align) >= 0.9999)
    out.backward(gout.double().permute(0, 3, 1, 2))
    dx, dy = position_error(flow)
    e = ((dx + dy)[..., None] * gout.double().abs()).numpy()
    return x.grad.permute(0, 2, 3, 1).contiguous(), torch.from_numpy(_scatter16(flow, align, e, C))


@functools.lru_cache(maxsize=4)
def warp_gout(N, H, W, C):
    return (torch.rand(N, H, W, C, generator=torch.Generator().manual_seed(11 + C)) * 2 - 1).contiguous()


@functools.lru_cache(maxsize=8)
def warp_bwd_case(shape, family, align, masked):
    N, H, W, C = shape
    gout, flow = warp_gout(N, H, W, C), make_flow(family, N, H, W)
    if masked:
        assert_off_threshold(flow, align)
    return dict(gout=gout, flow=flow, shape=shape, family=family, align=align, masked=masked,
                tight=warp_bwd_tight(gout, flow, align, masked), indep=warp_bwd_indep(gout, flow, align, masked))


def check_warp_bwd(got, case, label="warp_bwd"):
    """The atomic backward against both tiers; far flows give exact zeros."""
    got = got.detach().cpu().to(F64)
    tag = "%s %s %s align=%d masked=%d" % (label, case["shape"], case["family"], case["align"], case["masked"])
    ref, bound, _ = case["tight"]
    le((got - ref).abs(), bound, tag + " tight", label + "/tight")
    if case["family"] == "far":
        assert bool((ref == 0).all()) and bool((got == 0).all()), tag + ": far flow must give all zeros"
    iref, extra = case["indep"]
    le((got - iref).abs(), bound + extra, tag + " independent", label + "/independent")


# ============================================================================== temporal loss
def temporal_inputs(shape, cs, cl, family="iid", seed=0):
    """a, b NHWC with junk in the pad channels and some exactly equal entries, a fractional mask with exact
    zeros [N, 1, H, W], the family's flow."""
    N, H, W = shape
    a, b = rand(seed + 1, (N, H, W, cs)), rand(seed + 2, (N, H, W, cs))
    a[..., cl:], b[..., cl:] = 777.0, -555.0
    u = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(seed + 3))
    mask = torch.where(u > 0.3, 0.25 + 0.75 * u, torch.zeros_like(u))
    return a.contiguous(), b.contiguous(), make_flow(family, N, H, W), mask.contiguous()


def temporal_tight(a, b, flow, mask, lam, cl, gout, preset=None, mutate=None):
    """The composed form lam * mean((m (b - warp(a)))^2) over N H W cl values and its gradients, from the tight
    warp in fp64.  Returns a dict of fp64 tensors: loss, loss_bound, gb, gb_bound, ga, ga_bound.

    loss: the summands e^2 are non-negative; a thread adds cl of them in fp32, the wave reduce is 6 levels, the
    block adds 4, the rest is fp64 and one rounding to fp32: as _check_loss of test_gpu_reductions.py,
    (cl + 16) 2 u |ref|, which also covers the three roundings of e^2 itself (b - w, * m, the square: 5 u e^2).
    Each warped value carries the tight tier's 4 u S, which reaches e^2 through 2 |e| m.
    gb = k m e, k = fp32(2 lam / (count cl)) * gout: six roundings (k twice, b - w, * m, k * m, * e), 8 u |gb|,
    plus |k| m^2 * 4 u S.
    ga = preset - scatter(w gb): warp_bwd_tight's bound for the scatter itself, plus the scatter of gb's bound."""
    N, H, W, Cs = a.shape
    lam, gout = float(f32(lam)), float(f32(gout))
    wv, wb, _ = warp_fwd_tight(a, flow, False, False, mutate if mutate in ("swap_ne_sw", "swap_hw_norm",
                                                                        "image_stride_hw") else None)
    wv, S = wv[..., :cl], wb[..., :cl] / (4 * U)
    m = mask.double().permute(0, 2, 3, 1)                       # [N, H, W, 1]
    e = m * (b.double()[..., :cl] - wv)
    count = N * H * W * (Cs if mutate == "cs_for_cl" else cl)   # MUTATION cs_for_cl: Cs in the scale
    loss = lam * (e ** 2).sum() / count
    loss_bound = (cl + 16) * 2 * U * loss.abs() + lam / count * (2 * e.abs() * m * 4 * U * S).sum()
    k = 2.0 * lam * gout / count
    gb, gb_bound = torch.zeros(N, H, W, Cs, dtype=F64), torch.zeros(N, H, W, Cs, dtype=F64)
    gb[..., :cl] = k * m * e
    gb_bound[..., :cl] = 8 * U * gb[..., :cl].abs() + abs(k) * m * m * 4 * U * S
    if mutate == "gb_pad_unwritten":    # MUTATION: the pad channels keep what the buffer held
        gb[..., cl:] = float("nan")
    gmut = mutate if mutate in ("swap_ne_sw", "swap_hw_norm") else None
    ga, ga_bound, _ = warp_bwd_tight(torch.nan_to_num(gb), flow, False, False, gmut, cl, True, preset)
    # the scatter of gb's own bound (the weights are non-negative)
    prop, _, _ = warp_bwd_tight(gb_bound, flow, False, False, None, cl, False, None)
    return dict(loss=loss, loss_bound=loss_bound, gb=gb, gb_bound=gb_bound, ga=ga, ga_bound=ga_bound + prop,
                e=e, cl=cl)


def temporal_indep(a, b, flow, mask, lam, cl, gout):
    """The same three results from oracle.cpu_ref.temporal_loss (the reference's composed form) in fp64 with
    autograd, and what the fp32 sample position adds to each tight bound: vb, warp_fwd_indep's value bound,
    reaches the loss through 2 |e| m, gb through |k| m^2, and ga through the scatter of that plus the (dx + dy)
    |gb| term of warp_bwd_indep."""
    N, H, W, Cs = a.shape
    lam, gout = float(f32(lam)), float(f32(gout))
    a64 = a.double()[..., :cl].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    b64 = b.double()[..., :cl].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    m64 = mask.double()
    loss = cpu_ref.temporal_loss(a64, b64, flow.double(), m64, lam)
    (loss * gout).backward()
    ga, gb = torch.zeros(N, H, W, Cs, dtype=F64), torch.zeros(N, H, W, Cs, dtype=F64)
    ga[..., :cl], gb[..., :cl] = a64.grad.permute(0, 2, 3, 1), b64.grad.permute(0, 2, 3, 1)
    _, vb, _ = warp_fwd_indep(a[..., :cl].contiguous(), flow, False, False)
    m = m64.permute(0, 2, 3, 1)
    with torch.no_grad():
        e = m * (b64 - cpu_ref.warp(a64, flow.double())).permute(0, 2, 3, 1)
    count = N * H * W * cl
    k = abs(2.0 * lam * gout / count)
    gb_extra = torch.zeros_like(gb)
    gb_extra[..., :cl] = k * m * m * vb
    dx, dy = position_error(flow)
    pos = torch.zeros_like(gb)
    pos[..., :cl] = torch.from_numpy(_scatter16(flow, False, ((dx + dy)[..., None] * gb[..., :cl].abs()).numpy(), cl))
    prop, _, _ = warp_bwd_tight(gb_extra, flow, False, False, None, cl, False, None)
    return dict(loss=loss.detach(), loss_extra=lam / count * (2 * e.abs() * m * vb).sum(), ga=ga, gb=gb,
                gb_extra=gb_extra, ga_extra=pos + prop)


def check_temporal(loss, ga, gb, ref, preset=None, indep=None, label="temporal"):
    """loss / ga / gb (any may be None) against temporal_tight's dict (and temporal_indep's if given).  The pad
    channels of gb are exactly 0, those of ga keep the preset (0 without one)."""
    cl = ref["cl"]
    if loss is not None:
        le(abs(float(loss) - float(ref["loss"])), ref["loss_bound"], label + " loss", label + "/loss")
        if indep is not None:
            le(abs(float(loss) - float(indep["loss"])), ref["loss_bound"] + indep["loss_extra"],
               label + " loss independent", label + "/loss-independent")
    if gb is not None:
        gb = gb.detach().cpu()
        assert bool((gb[..., cl:] == 0).all()), label + ": gb pad channels are not exactly 0"
        g64 = gb.to(F64)
        le((g64 - ref["gb"])[..., :cl].abs(), ref["gb_bound"][..., :cl], label + " gb", label + "/gb")
        zero = (ref["gb"][..., :cl] == 0) & (ref["gb_bound"][..., :cl] == 0)
        assert bool((g64[..., :cl][zero] == 0).all())
        if indep is not None:
            le((g64 - indep["gb"]).abs(), ref["gb_bound"] + indep["gb_extra"], label + " gb independent",
               label + "/gb-independent")
    if ga is not None:
        ga = ga.detach().cpu()
        want_pad = torch.zeros_like(ga[..., cl:]) if preset is None else preset[..., cl:]
        assert torch.equal(ga[..., cl:], want_pad), label + ": ga pad channels were touched"
        g64 = ga.to(F64)
        le((g64 - ref["ga"])[..., :cl].abs(), ref["ga_bound"][..., :cl], label + " ga", label + "/ga")
        if indep is not None and preset is None:
            le((g64 - indep["ga"]).abs(), ref["ga_bound"] + indep["ga_extra"], label + " ga independent",
               label + "/ga-independent")


# ============================================================================== fbcheck
FBC_SHAPES = [(3, 1, 7), (1, 6, 1), (3, 17, 19), (2, 5, 300)]
FBC_PAIRS = ("consistent", "inconsistent", "quarter")


def fbc_flows(pair, shape, seed=5):
    """(ff, bf) [N, 2, H, W]: near-consistent (ff = -bf plus noise, a smooth bf), unrelated, multiples of 1/4."""
    N, H, W = shape
    if pair == "consistent":
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        bf = torch.stack([1.5 * torch.sin(0.015 * ys + 0.01 * xs) + 1.0, 1.2 * torch.cos(0.012 * xs - 0.02 * ys)])[None]
        bf = bf.repeat(N, 1, 1, 1) * torch.linspace(0.5, 1.5, N).view(N, 1, 1, 1) + rand(seed, (N, 2, H, W), 0.005)
        return (-bf + rand(seed + 1, (N, 2, H, W), 0.3)).contiguous(), bf.contiguous()
    if pair == "inconsistent":
        return rand(seed + 2, (N, 2, H, W), 2.0), rand(seed + 3, (N, 2, H, W), 0.5)
    # the near-consistent pair rounded to multiples of 1/4: plateaus with zero gradient, steps of 1/4 between them
    # (central differences of exactly 1/8), sums of squares that are exact in fp32, so the comparisons tie or nearly do
    ff, bf = fbc_flows("consistent", shape, seed)
    return torch.round(ff * 4) / 4, torch.round(bf * 4) / 4


def fbc_ref(ff, bf):
    """oracle.cpu_ref.fbc_check: the reference's own fp32 sequence of tensor ops, compared bit for bit."""
    return cpu_ref.fbc_check(ff, bf)


# ============================================================================== correlation pyramid / lookup
def pyr_geom(P, H2, W2, ld0, levels):
    """(offsets, (h, w) per level, plane stride per level) of the pyramid buffer: floor-mode halving, level 0
    padded to ld0 floats per plane, the others dense."""
    off, hw, ld, o, h, w = [], [], [], 0, H2, W2
    for lv in range(levels):
        if lv > 0:
            h, w = h // 2, w // 2
        off.append(o)
        hw.append((h, w))
        ld.append(ld0 if lv == 0 else h * w)
        o += P * ld[-1]
    return off + [o], hw, ld


def pyramid_buffer(P, H2, W2, ld0, levels, seed=0, fill=True):
    """A [total] fp32 buffer: level 0 seeded random with junk (1e6) in the padding of every plane; the other
    levels junk (fill=False) or their fp32 avg_pool2d (fill=True, for the lookup tests)."""
    off, hw, ld = pyr_geom(P, H2, W2, ld0, levels)
    buf = torch.full((off[-1],), 1e6)
    lv0 = buf[:P * ld0].view(P, ld0)
    lv0[:, :H2 * W2] = rand(seed + 7, (P, H2 * W2))
    if fill:
        cur = lv0[:, :H2 * W2].reshape(P, 1, H2, W2)
        for lv in range(1, levels):
            cur = F.avg_pool2d(cur, 2, stride=2)
            buf[off[lv]:off[lv + 1]] = cur.reshape(-1)
    return buf


def pyramid_levels(buf, P, H2, W2, ld0, levels):
    """The levels of a buffer as [P, h, w] views."""
    off, hw, ld = pyr_geom(P, H2, W2, ld0, levels)
    return [buf[off[lv]:off[lv + 1]].view(P, ld[lv])[:, :h * w].reshape(P, h, w) for lv, (h, w) in enumerate(hw)]


def pyramid_ref(buf, P, H2, W2, ld0, levels):
    """[(ref, bound)] per level >= 1 from F.avg_pool2d in fp64.  One output is ((x00 + x01) + x10) + x11 over 4:
    three roundings of partial sums (the division by 4 is exact), within the issue's 4 u sum|.| / 4 per level; a
    level inherits the pooled error of the level it is computed from."""
    cur = pyramid_levels(buf, P, H2, W2, ld0, 1)[0].double()[:, None]
    bound = torch.zeros_like(cur)
    out = []
    for _ in range(1, levels):
        nb = F.avg_pool2d(bound, 2, stride=2)
        bound = nb + 4 * U * (F.avg_pool2d(cur.abs(), 2, stride=2) + nb)
        cur = F.avg_pool2d(cur, 2, stride=2)
        out.append((cur[:, 0], bound[:, 0]))
    return out


def lookup_tight(buf, coords, B, H1, W1, H2, W2, ld0, levels, r, cs, mutate=None):
    """(ref, bound) fp64 [B, H1, W1, cs].  The sample geometry restates corr_lookup_k's fp32 sequence (the
    reference's: coords / 2^lvl + delta, bilinear_sampler's 2 p / (size - 1) - 1, grid_sample's align_corners=True
    ((g + 1) / 2) (size - 1), floor, the four weight products; every step a single correctly rounded fp32 operation,
    none contractible); gather, products and sum are fp64.  The kernel's sum has per term one rounding of the
    weight product and one of the value product, and three adds: 6 u sum_k |w_k v_k| covers it.  Window order:
    channel lvl K^2 + a K + c samples x + (a - r), y + (c - r) (meshgrid(d, d) stacked onto (x, y))."""
    P, K = B * H1 * W1, 2 * r + 1
    lv = pyramid_levels(buf, P, H2, W2, ld0, levels)
    co = coords.numpy().astype(f32)
    cxp, cyp = co[:, 0].reshape(P), co[:, 1].reshape(P)
    ref, S = np.zeros((P, cs)), np.zeros((P, cs))
    pidx = np.arange(P)
    for l in range(levels):
        pl = lv[l].numpy().astype(f64)
        Hl, Wl = pl.shape[1:]
        div = f32(1 << l)
        if mutate == "lvl_divisor" and l > 0:     # MUTATION: divide by lvl instead of 2^lvl
            div = f32(l)
        for a in range(K):
            for c in range(K):
                oa, oc = (c, a) if mutate == "transpose_window" else (a, c)   # MUTATION: a -> y, c -> x
                px = (cxp / div + f32(oa - r)).astype(f32)
                py = (cyp / div + f32(oc - r)).astype(f32)
                gx = (f32(2) * px / f32(Wl - 1) - f32(1)).astype(f32)
                gy = (f32(2) * py / f32(Hl - 1) - f32(1)).astype(f32)
                ix = (((gx + f32(1)) / f32(2)) * f32(Wl - 1)).astype(f32)
                iy = (((gy + f32(1)) / f32(2)) * f32(Hl - 1)).astype(f32)
                fx0, fy0 = np.floor(ix), np.floor(iy)
                we, wn = (ix - fx0).astype(f32), (iy - fy0).astype(f32)
                e, s = (f32(1) - we).astype(f32), (f32(1) - wn).astype(f32)
                x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
                ch = l * K * K + a * K + c
                for yy, xx, wt in ((y0, x0, s * e), (y0, x0 + 1, s * we), (y0 + 1, x0, wn * e), (y0 + 1, x0 + 1, wn * we)):
                    ok = (yy >= 0) & (yy < Hl) & (xx >= 0) & (xx < Wl)
                    v = pl[pidx, np.clip(yy, 0, Hl - 1), np.clip(xx, 0, Wl - 1)]
                    t = np.where(ok, wt.astype(f32).astype(f64) * v, 0.0)
                    ref[:, ch] += t
                    S[:, ch] += np.abs(t)
    sh = (B, H1, W1, cs)
    return torch.from_numpy(ref.reshape(sh)), torch.from_numpy((6 * U * S).reshape(sh))


def lookup_indep(buf, coords, B, H1, W1, H2, W2, ld0, levels, r, cs):
    """(ref, bound) fp64 from oracle.style_ref.bilinear_sampler (F.grid_sample, align_corners=True, zeros) in fp64,
    with the reference's delta = stack(meshgrid(d, d)).  Position error per axis as position_error: the sequence
    has at most six roundings of quantities no larger than (|p| + size) pixels, 8 u (|p| + size); the value moves
    by 2 max|plane| per pixel, and its own roundings are within 8 u max|plane|."""
    P, K = B * H1 * W1, 2 * r + 1
    lv = pyramid_levels(buf, P, H2, W2, ld0, levels)
    c64 = coords.double().permute(0, 2, 3, 1).reshape(P, 1, 1, 2)
    d = torch.linspace(-r, r, K, dtype=F64)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, K, K, 2)
    ref, bound = torch.zeros(P, cs, dtype=F64), torch.zeros(P, cs, dtype=F64)
    for l in range(levels):
        pl = lv[l].double()[:, None]
        Hl, Wl = pl.shape[-2:]
        c = c64 / 2 ** l + delta
        ref[:, l * K * K:(l + 1) * K * K] = style_ref.bilinear_sampler(pl, c).reshape(P, K * K)
        dpos = 8 * U * ((c[..., 0].abs() + Wl) + (c[..., 1].abs() + Hl)).reshape(P, K * K)
        bound[:, l * K * K:(l + 1) * K * K] = (2 * dpos + 8 * U) * pl.abs().amax(dim=(1, 2, 3)).view(P, 1)
    return ref.view(B, H1, W1, cs), bound.view(B, H1, W1, cs)


LOOKUP_COORDS = ("grid", "near", "border", "outside")


def lookup_coords(kind, B, H1, W1, H2, W2, r, seed=0):
    """[B, 2, H1, W1] fp32 (channel 0 = x): exactly on the level-0 grid; within +-4 px of the own pixel; at each
    border of the frame +- the radius; wholly outside every level's window."""
    g = torch.Generator().manual_seed(seed + 31)
    P = H1 * W1
    if kind == "grid":
        x = torch.randint(0, W2, (B, P), generator=g).float()
        y = torch.randint(0, H2, (B, P), generator=g).float()
    elif kind == "near":
        base = raft_ref.coords_grid(B, H1, W1).reshape(B, 2, P)
        off = torch.rand(B, 2, P, generator=g) * 8 - 4
        x, y = base[:, 0] * (W2 / W1) + off[:, 0], base[:, 1] * (H2 / H1) + off[:, 1]
    elif kind == "border":
        i = torch.arange(P).view(1, P) + torch.arange(B).view(B, 1)
        d = (torch.rand(B, P, generator=g) * 2 - 1) * (r + 1.0)
        x = torch.rand(B, P, generator=g) * (W2 + 1.0) - 1.0
        y = torch.rand(B, P, generator=g) * (H2 + 1.0) - 1.0
        side = i % 4
        x = torch.where(side == 0, d, torch.where(side == 1, (W2 - 1.0) + d, x))
        y = torch.where(side == 2, d, torch.where(side == 3, (H2 - 1.0) + d, y))
    else:
        s = torch.where(torch.rand(B, 2, P, generator=g) < 0.5, -1.0, 1.0)
        x, y = s[:, 0] * 1000.0 + 500.0, s[:, 1] * 1000.0 + 500.0
    return torch.stack([x, y], 1).view(B, 2, H1, W1).contiguous()


def check_lookup(got, tight, indep, levels, r, label="corr_lookup", outside=False):
    got = got.detach().cpu()
    n = levels * (2 * r + 1) ** 2
    assert bool((got[..., n:] == 0).all()), label + ": pad channels are not exactly 0"
    g64 = got.to(F64)
    le((g64 - tight[0]).abs(), tight[1], label + " tight", label + "/tight")
    assert bool((g64[tight[1] == 0] == 0).all())
    if outside:
        assert bool((got == 0).all()), label + ": coordinates outside every level must give zeros"
    le((g64 - indep[0]).abs(), indep[1], label + " independent", label + "/independent")


# ============================================================================== RAFT convex upsampling
def upsample_inputs(B, h, w, mcs=576, spike=False, seed=0):
    """coords1 [B, 2, h, w] and the NHWC mask [B, h, w, mcs] (junk beyond channel 576); spike: one tap of every
    pixel's 9 gets +60 and another -60."""
    coords1 = raft_ref.coords_grid(B, h, w) + rand(seed + 41, (B, 2, h, w), 2.0)
    m = rand(seed + 42, (B, h, w, 576))
    if spike:
        mv = m.view(B, h, w, 9, 64)
        mv[..., 2, :] += 60.0
        mv[..., 7, :] -= 60.0
    mask = torch.full((B, h, w, mcs), 1e30)
    mask[..., :576] = m
    return coords1.contiguous(), mask.contiguous()


def upsample_ref(coords1, mask):
    """(ref, bound) fp64 [B, 2, 8h, 8w] from oracle.raft_ref.upsample_flow in fp64.

    With d_k = logit_k - max <= 0, e_k = exp(d_k), w_k = e_k / sum e: the kernel's e_k carries (3 + |d_k|) u
    =: r_k u relative (the subtraction's u |d_k| in the argument, expf's 1 ulp = 2 u), the denominator
    (R + 8) u with R = sum w_k r_k (its terms' errors and 8 adds), the division u, so |dw_k| <= w_k (r_k + R + 9) u.
    The flow value 8 (coords - x) carries u; the 9 products and 9 adds 10 u sum w_k |f_k|.  Together
    |got - ref| <= u sum_k w_k |f_k| (r_k + R + 20).  A weight below fp32's smallest normal may flush to 0
    entirely: + 2^-126 max|f|."""
    B, _, h, w = coords1.shape
    flow = coords1.double() - raft_ref.coords_grid(B, h, w, F64)
    m = mask[..., :576].double().permute(0, 3, 1, 2).contiguous()
    ref = raft_ref.upsample_flow(flow, m)
    mv = m.view(B, 1, 9, 8, 8, h, w)
    d = (mv - mv.amax(dim=2, keepdim=True)).abs()
    wk = torch.softmax(mv, dim=2)
    rk = 3 + d
    R = (wk * rk).sum(dim=2, keepdim=True)
    f = F.unfold(8 * flow, [3, 3], padding=1).view(B, 2, 9, 1, 1, h, w).abs()
    bound = U * (wk * f * (rk + R + 20)).sum(dim=2) + 2.0 ** -126 * f.amax()
    bound = bound.permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 8 * h, 8 * w)
    return ref, bound


# ============================================================================== the cases of the GPU tests
WARP_SHAPES = [(2, 37, 53, 4),      # CT = 1
               (2, 37, 53, 64),     # CT = 16; a row is 848 threads: 4 x-blocks with an 80-thread tail
               (2, 9, 11, 128),     # CT = 32; a row is 352 threads: 2 x-blocks with a 96-thread tail
               (3, 5, 7, 8), (3, 5, 7, 20),   # runtime arm, C4 = 2 and 5, N = 3
               (3, 1, 7, 4), (1, 6, 1, 12),   # max(size - 1, 1)
               (1, 3, 300, 4)]      # CT = 1 across two blocks
FWD_CASES = [(s, f) for s in WARP_SHAPES for f in FAMILIES]
BWD_CASES = [(hw + (c,), f) for hw in ((2, 37, 53), (3, 5, 7)) for c in (4, 8, 20, 64, 128)
             for f in ("iid", "sweep", "converge", "far")]
DET_CASES = [(s, f) for s, f in BWD_CASES if s[3] in (4, 8, 20)]
TEMPORAL_SHAPES = [(1, 1, 1), (3, 5, 17), (1, 1, 257), (2, 37, 53), (3, 1, 7), (1, 6, 1)]   # 1, 255, 257, 3922 pixels
TEMPORAL_CSCL = [(4, 3), (4, 1), (4, 4), (8, 5), (64, 64)]
TEMPORAL_CASES = [(s, c) for s in TEMPORAL_SHAPES for c in TEMPORAL_CSCL]
PYRAMID_CASES = [(6, 7, 9, 70, 2), (5, 13, 10, 133, 3), (3, 16, 24, 401, 4)]       # (P, H2, W2, ld0, levels)
LOOKUP_CASES = [(h2, w2, lv, r, kind, 8 if kind in ("border", "outside") else 0)
                for h2, w2, lv in ((7, 9, 2), (13, 10, 3), (16, 24, 4)) for r in (0, 1, 4) for kind in LOOKUP_COORDS]
UPSAMPLE_CASES = [(2, 1, 1, 576, False), (1, 3, 5, 580, True), (2, 5, 6, 576, True), (2, 5, 6, 600, False)]
LAMBDA, GOUT = 10.0, -0.37


@functools.lru_cache(maxsize=4)
def temporal_case(shape, cscl, family="iid"):
    cs, cl = cscl
    a, b, flow, mask = temporal_inputs(shape, cs, cl, family)
    ref = temporal_tight(a, b, flow, mask, LAMBDA, cl, GOUT)
    return dict(a=a, b=b, flow=flow, mask=mask, lam=LAMBDA, gout=GOUT, cs=cs, cl=cl, ref=ref,
                indep=functools.lru_cache(maxsize=1)(lambda: temporal_indep(a, b, flow, mask, LAMBDA, cl, GOUT)))


@functools.lru_cache(maxsize=4)
def lookup_case(H2, W2, levels, r, kind, cs_extra):
    B, H1, W1 = 2, 3, 4
    P, ld0 = B * H1 * W1, H2 * W2 + 5
    cs = (levels * (2 * r + 1) ** 2 + 3) // 4 * 4 + cs_extra
    buf = pyramid_buffer(P, H2, W2, ld0, levels, seed=H2, fill=True)
    coords = lookup_coords(kind, B, H1, W1, H2, W2, r)
    geo = (B, H1, W1, H2, W2, ld0, levels, r, cs)
    return dict(geo=geo, buf=buf, coords=coords, kind=kind, tight=lookup_tight(buf, coords, *geo),
                indep=lookup_indep(buf, coords, *geo))
