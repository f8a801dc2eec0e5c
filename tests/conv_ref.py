"""CPU references (torch fp64), the split-bf16 emulation, exact probe inputs, comparison functions and the
route table for the convolution kernels (csrc/conv.hip, conv_bf.hip, conv_rk.hip, conv_c4.hip, skinny.hip).
tests/test_gpu_conv_arith.py feeds the comparison functions with the device's results,
tests/test_conv_ref_host.py with the emulation itself (it must pass) and with one named slip applied to the
reference side (`mutate=`: it must be rejected, so the cases discriminate).

Arithmetic under test.  An fp32 operand v travels as three bf16 planes, hi = bf16(v), mid = bf16(v - hi),
lo = bf16(v - hi - mid) (round to nearest even; the differences are exact in fp32).  bf16x6 accumulates the six
plane products E6 into fp32, bf16x3 the three products E3 of the hi and mid planes; fp32 is an fma chain.

Tier A (check_exact) uses inputs whose every output is ONE product (one-hot weights or one-hot dy: a conv
with a one-hot weight is a shifted copy) or a short sum whose every partial sum is representable, so the
expected value has no rounding at all and the comparison is on bit patterns.  The output is only right if
every plane of the full-significand operand reached the MFMA, the cross terms were issued, the addressing
(tap, channel, stride, padding, mirror) hit the right element and no K stage was skipped or read twice.

Tier B (check_bound) is a per-output bound on dense data, |y - y64| <= c u B(o) + u |y64| with
B(o) = sum_k |a_k||b_k| of that output and u = 2^-24; c counts roundings and is derived in `c_bound`.

Every tensor here is NCHW / [Co][Ci][R][S] on the CPU; the adaptors move data to the device layouts.
"""
from typing import NamedTuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64 = torch.float64
HI, MID, LO = 0, 1, 2
# (plane of operand a, plane of operand b); both sets are symmetric, so which operand a kernel calls A is moot
E6 = ((LO, HI), (HI, LO), (MID, MID), (MID, HI), (HI, MID), (HI, HI))
E3 = ((MID, HI), (HI, MID), (HI, HI))
TERMS = {"bf16x6": E6, "bf16x3": E3}
DROPS = {"drop_lo_hi": (LO, HI), "drop_hi_lo": (HI, LO), "drop_mid_mid": (MID, MID), "drop_mid_hi": (MID, HI),
         "drop_hi_mid": (HI, MID)}
MUTATIONS = tuple(DROPS) + ("e3", "transpose_taps", "dgrad_unrotated", "symmetric", "skip_last_k_stage",
                            "chan_group", "chunk_first", "chunk_last", "stride_phase")
KSTAGE = 32  # K elements per LDS stage of the split-bf16 tiles (BK = 32; the BK 16 / 64 kinds halve / double it)

# worst err / bound per label in this process and the bit-exact probe counts (the GPU tests print both)
WORST = {}
EXACT = {}


class Conv(NamedTuple):
    """y[N][Co][Ho][Wo] = conv(pad(x[N][Ci][H][W]), w[Co][Ci][R][S]).  ConvTranspose2d(k3, s2, p1, op1) is the
    data gradient ("dgrad") of the stride-2 conv over the 2H x 2W image, its weight read as [Co][Ci]."""
    N: int
    Ci: int
    H: int
    W: int
    Co: int
    R: int
    S: int
    stride: int
    ph: int
    pw: int
    mode: str = "zero"

    @property
    def Ho(self):
        return (self.H + 2 * self.ph - self.R) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pw - self.S) // self.stride + 1

    @property
    def P(self):
        return self.N * self.Ho * self.Wo


def cpad(c):
    return (c + 3) // 4 * 4


# ================================================================================== references
def pad_index(n, p, mode):
    """Source index of the padded positions -p .. n + p - 1 (-1: a zero)."""
    i = torch.arange(-p, n + p)
    if mode == "zero":
        return torch.where((i < 0) | (i >= n), torch.full_like(i, -1), i)
    if mode == "reflect":
        i = i.abs()
        return torch.where(i >= n, 2 * (n - 1) - i, i)
    if mode == "symmetric":  # the edge pixel repeated: the slip a reflect gather makes when it is off by one
        i = torch.where(i < 0, -1 - i, i)
        return torch.where(i >= n, 2 * n - 1 - i, i)
    raise ValueError(mode)


def pad2(x, ph, pw, mode):
    ih, iw = pad_index(x.shape[2], ph, mode), pad_index(x.shape[3], pw, mode)
    xp = x[:, :, ih.clamp_min(0)][:, :, :, iw.clamp_min(0)]
    return xp * ((ih >= 0).to(x.dtype)[:, None] * (iw >= 0).to(x.dtype)[None, :])


def fold2(gp, H, W, ph, pw, mode):
    """The adjoint of pad2: gradient of the padded frame summed back onto the image."""
    ih, iw = pad_index(H, ph, mode), pad_index(W, pw, mode)
    g = torch.zeros(gp.shape[:2] + (H, gp.shape[3]), dtype=gp.dtype)
    g.index_add_(2, ih[ih >= 0], gp[:, :, ih >= 0])
    out = torch.zeros(gp.shape[:2] + (H, W), dtype=gp.dtype)
    out.index_add_(3, iw[iw >= 0], g[:, :, :, iw >= 0])
    return out


def fwd64(c, x, w, mode=None):
    return F.conv2d(pad2(x, c.ph, c.pw, mode or c.mode), w, stride=c.stride)


def dgrad64(c, dy, w, mode=None):
    full = F.conv_transpose2d(dy, w, stride=c.stride)  # the rows / columns the windows reach
    Hp, Wp = c.H + 2 * c.ph, c.W + 2 * c.pw
    full = F.pad(full, (0, Wp - full.shape[3], 0, Hp - full.shape[2]))
    return fold2(full, c.H, c.W, c.ph, c.pw, mode or c.mode)


def wgrad64(c, x, dy, mode=None):
    xp = pad2(x, c.ph, c.pw, mode or c.mode)
    g = F.conv2d(xp.transpose(0, 1), dy.transpose(0, 1), dilation=c.stride)
    return g[:, :, :c.R, :c.S].transpose(0, 1).contiguous()


REF = {"fwd": fwd64, "dgrad": dgrad64, "wgrad": wgrad64}


def ref(kind, c, a, b, mode=None):
    return REF[kind](c, a.to(F64), b.to(F64), mode)


def magnitude(kind, c, a, b):
    """B(o) = sum_k |a_k||b_k| of every output."""
    return REF[kind](c, a.to(F64).abs(), b.to(F64).abs(), None)


def operand_shapes(kind, c):
    x, w, y = (c.N, c.Ci, c.H, c.W), (c.Co, c.Ci, c.R, c.S), (c.N, c.Co, c.Ho, c.Wo)
    return {"fwd": (x, w), "dgrad": (y, w), "wgrad": (x, y)}[kind]


# ============================================================================ split emulation
def bf16_rne(v):
    return v.to(torch.bfloat16).to(torch.float32)


def split3(v):
    """The three RNE planes of an fp32 tensor, as fp32 tensors."""
    v = v.to(torch.float32)
    hi = bf16_rne(v)
    r = v - hi
    mid = bf16_rne(r)
    return hi, mid, bf16_rne(r - mid)


def emulate(kind, c, a, b, terms, mode=None):
    """The listed plane products of the bilinear op, each exact, summed in fp64."""
    pa, pb = split3(a), split3(b)
    return sum(ref(kind, c, pa[i], pb[j], mode) for i, j in terms)


# ================================================================================ probe values
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def masked_full(shape, seed, emax=12):
    """Full-significand fp32 values, exponents uniform in +-emax, with significand bits 15 and 7 cleared: bit 15 is
    bf16's rounding bit, so hi is a truncation and v - hi >= 0; the host test proves what that buys (hi + mid + lo == v
    and all six addition orders of the three planes exact)."""
    g = _gen(seed)
    n = int(torch.tensor(shape).prod())
    mant = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64) & ~((1 << 15) | (1 << 7))
    e = torch.randint(-emax, emax + 1, (n,), generator=g, dtype=torch.int64) + 127
    s = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    bits = (s << 31) | (e << 23) | mant
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(shape).clone()


def pow2(shape, seed, emax):
    g = _gen(seed)
    e = torch.randint(-emax, emax + 1, shape, generator=g).to(torch.float32)
    s = torch.randint(0, 2, shape, generator=g).to(torch.float32) * 2 - 1
    return s * torch.exp2(e)


def midmid(shape, seed, emax):
    """+-2^e (1 + 2^-a), a in {9, 10, 11}: hi = 2^e and mid = 2^(e-a) are one bit each, lo = 0."""
    a = torch.randint(9, 12, shape, generator=_gen(seed + 7)).to(torch.float32)
    return pow2(shape, seed, emax) * (1 + torch.exp2(-a))


def fewhot_x(shape, seed):
    g = _gen(seed)
    m = torch.randint(1, 3, shape, generator=g).to(torch.float32)
    s = torch.randint(0, 2, shape, generator=g).to(torch.float32) * 2 - 1
    return s * m * (1 + 2.0 ** -9 + 2.0 ** -18)


def fewhot_w(shape, seed):
    g = _gen(seed)
    return (torch.randint(0, 2, shape, generator=g).to(torch.float32) * 2 - 1) * \
        torch.randint(1, 3, shape, generator=g).to(torch.float32)


# a: the op's first operand (x, or dy for dgrad), b: its second (w, or dy for wgrad); (values of a, values of b
# before the one-hot mask, exponent ranges as the issue sets them: +-12 activations, +-6 weights)
FAMILIES = ("a_full", "b_full", "midmid", "fewhot")


def family_values(family, kind, c, seed):
    sa, sb = operand_shapes(kind, c)
    ea, eb = (12, 12) if kind == "wgrad" else (12, 6)
    if family == "a_full":
        return masked_full(sa, seed, ea), pow2(sb, seed + 1, eb)
    if family == "b_full":
        return pow2(sa, seed, ea), masked_full(sb, seed + 1, eb)
    if family == "midmid":
        return midmid(sa, seed, ea), midmid(sb, seed + 1, eb)
    if family == "fewhot":
        return fewhot_x(sa, seed), fewhot_w(sb, seed + 1)
    raise ValueError(family)


# ============================================================================== one-hot masks
def k_axes(kind, c):
    """(outputs, K) of the GEMM behind a forward / data-gradient conv: K = (r, s, channel), channel fastest."""
    return (c.Co, c.R * c.S * c.Ci) if kind == "fwd" else (c.Ci, c.R * c.S * c.Co)


def n_sets(kind, c, hot=1):
    if kind == "wgrad":
        return -(-c.P // c.Co)
    o, K = k_axes(kind, c)
    return -(-K // o)


def hot_taps(kind, c, j, hot=1):
    """taps[o][i]: the K index of the i-th non-zero weight of output channel o in set j.  One-hot: (o + j O) mod K,
    so the sets visit every (r, s, channel) at the route's own channel counts; few-hot adds K // 4 strides, which puts
    the four in different K stages wherever K has four stages."""
    o, K = k_axes(kind, c)
    base = (torch.arange(o) + j * o) % K
    return torch.stack([(base + i * (K // 4)) % K for i in range(hot)], 1)


def onehot_w(kind, c, j, vals, hot=1):
    """vals [Co][Ci][R][S] masked to set j's taps."""
    o, K = k_axes(kind, c)
    nch = c.Ci if kind == "fwd" else c.Co
    taps = hot_taps(kind, c, j, hot)
    mask = torch.zeros(o, c.R * c.S, nch)
    mask.view(o, K).scatter_(1, taps, 1.0)
    mask = mask.view(o, c.R, c.S, nch).permute(0, 3, 1, 2)  # [o][channel][R][S]
    if kind == "dgrad":
        mask = mask.transpose(0, 1)                             # [Co][Ci][R][S]
    return vals * mask


def hot_pixels(c, j, hot=1):
    """pix[co][i]: flat (n, ho, wo) index of dy's i-th non-zero of channel co in set j."""
    base = (torch.arange(c.Co) + j * c.Co) % c.P
    return torch.stack([(base + i * (c.P // 4)) % c.P for i in range(hot)], 1)


def onehot_dy(c, j, vals, hot=1, pixels=None):
    pix = hot_pixels(c, j, hot) if pixels is None else pixels
    mask = torch.zeros(c.Co, c.P)
    mask.scatter_(1, pix, 1.0)
    return vals * mask.view(c.Co, c.N, c.Ho, c.Wo).transpose(0, 1)


def chunk_edge_pixels(c, chunk):
    """(first, last) dy pixel of every split-K chunk.  chunk: (pixels per chunk, row width) as the planner counts
    them (vst_conv_plan_wgrad_chunk): chunks run over output rows of row_w >= Wo columns (the Wo-padded plan pads
    rows with zero dy); an edge that falls on a pad column moves to the nearest real pixel inside the chunk.  A
    bare int is a chunk over unpadded rows."""
    chunk, row_w = chunk if isinstance(chunk, tuple) else (chunk, c.Wo)
    Pw = c.N * c.Ho * row_w
    q0 = torch.arange(0, Pw, chunk)
    q1 = torch.clamp(q0 + chunk, max=Pw) - 1
    r0, c0 = q0 // row_w, q0 % row_w
    r0, c0 = torch.where(c0 >= c.Wo, r0 + 1, r0), torch.where(c0 >= c.Wo, torch.zeros_like(c0), c0)
    r1, c1 = q1 // row_w, torch.clamp(q1 % row_w, max=c.Wo - 1)
    first, last = r0 * c.Wo + c0, r1 * c.Wo + c1
    return first[first < c.P], last


def dy_pixel_sets(c, chunk, seed=3, max_launches=32, all_pixels=False):
    """The pixel sets of the one-hot dy probes: every output pixel when that takes at most max_launches sets of Co
    pixels (or all_pixels says so); otherwise every pixel on an image border, the first and last pixel of every
    split-K chunk and a seeded sample, at least a quarter of the pixels.  Returns (list of [Co][1] index tensors,
    pixels covered, P)."""
    P = c.P
    if all_pixels or -(-P // c.Co) <= max_launches:
        want = torch.arange(P)
    else:
        p = torch.arange(P)
        ho, wo = (p // c.Wo) % c.Ho, p % c.Wo
        border = (ho == 0) | (ho == c.Ho - 1) | (wo == 0) | (wo == c.Wo - 1)
        edge = torch.zeros(P, dtype=torch.bool)
        if chunk:
            first, last = chunk_edge_pixels(c, chunk)
            edge[first] = True
            edge[last] = True
        keep = border | edge
        extra = torch.randperm(P, generator=_gen(seed))
        extra = extra[~keep[extra]][:max(0, -(-P // 4) - int(keep.sum()))]
        keep[extra] = True
        want = p[keep]
    n = -(-want.numel() // c.Co)
    want_p = torch.cat([want, want[:n * c.Co - want.numel()]]) if n * c.Co > want.numel() else want
    if want_p.numel() < n * c.Co:  # fewer pixels than channels: repeat
        want_p = want.repeat(-(-n * c.Co // want.numel()))[:n * c.Co]
    return [want_p[i * c.Co:(i + 1) * c.Co].view(c.Co, 1) for i in range(n)], int(want.numel()), P


# ================================================================================== the slips
def mutation_applies(mutate, kind, c, family=None):
    nch_a = c.Co if kind == "dgrad" else c.Ci
    if mutate in DROPS or mutate == "e3":
        return True
    return {"transpose_taps": c.R == c.S and c.R > 1,
            "dgrad_unrotated": kind == "dgrad" and c.R * c.S > 1,
            "symmetric": c.mode == "reflect",
            "skip_last_k_stage": kind != "wgrad",
            "chan_group": nch_a >= 16,
            "chunk_first": kind == "wgrad", "chunk_last": kind == "wgrad",
            "stride_phase": c.stride == 2}[mutate]


def _shift(t, d):
    out = torch.zeros_like(t)
    if d > 0:
        out[..., :-d] = t[..., d:]
    else:
        out[..., -d:] = t[..., :d]
    return out


def reference(kind, c, a, b, terms=None, mutate=None, chunk=None):
    """The fp64 reference side of a comparison: the exact op (terms None) or the listed plane products, with one
    named slip applied.  chunk: pixels per split-K chunk of a weight gradient (chunk_first / chunk_last)."""
    a, b = a.to(torch.float32), b.to(torch.float32)
    mode, post = None, (lambda y: y)
    if mutate in DROPS:
        terms = tuple(t for t in (terms or E6) if t != DROPS[mutate])
    elif mutate == "e3":
        terms = E3
    elif mutate == "transpose_taps":
        if kind == "wgrad":
            post = lambda y: y.transpose(2, 3)  # noqa: E731
        else:
            b = b.transpose(2, 3)
    elif mutate == "dgrad_unrotated":
        b = b.flip(2, 3)
    elif mutate == "symmetric":
        mode = "symmetric"
    elif mutate == "skip_last_k_stage":
        o, K = k_axes(kind, c)
        last = (K - 1) // KSTAGE * KSTAGE
        keep = (torch.arange(K) < last).to(torch.float32)
        nch = c.Ci if kind == "fwd" else c.Co
        keep = keep.view(1, c.R, c.S, nch).permute(0, 3, 1, 2)
        b = b * (keep if kind == "fwd" else keep.transpose(0, 1))
    elif mutate == "chan_group":  # channels 0-7 read in place of 8-15 and back
        idx = torch.arange(a.shape[1])
        idx[:8], idx[8:16] = torch.arange(8, 16), torch.arange(0, 8)
        a = a[:, idx]
    elif mutate in ("chunk_first", "chunk_last"):
        keep = torch.ones(c.P)
        first, last = chunk_edge_pixels(c, chunk)
        keep[first if mutate == "chunk_first" else last] = 0
        b = b * keep.view(c.N, 1, c.Ho, c.Wo)
    elif mutate == "stride_phase":
        if kind == "dgrad":
            post = lambda y: _shift(y, 1)  # noqa: E731
        else:
            a = _shift(a, 1)
    elif mutate is not None:
        raise ValueError(mutate)
    y = ref(kind, c, a, b, mode) if terms is None else emulate(kind, c, a, b, terms, mode)
    return post(y)


# ================================================================================ comparisons
def _canon(t):
    return (t.to(torch.float32) + 0.0).contiguous().view(torch.int32)  # -0 -> +0, then bit patterns


def epilogue(y32, bias=None, act="none", slope=0.0, addend=None, prefill=None):
    """The exact epilogue of an exact fp32 product: one correctly rounded add of the bias, a select (ReLU) or one
    rounded multiply (LeakyReLU), one rounded add of the addend; prefill: what a weight gradient accumulates onto."""
    if prefill is not None:
        return y32 + prefill.to(torch.float32)
    if bias is not None:
        y32 = y32 + bias.to(torch.float32).view(1, -1, 1, 1)
    if act == "relu":
        y32 = torch.where(y32 > 0, y32, torch.zeros_like(y32))
    elif act == "lrelu":
        y32 = torch.where(y32 > 0, y32, y32 * torch.tensor(slope, dtype=torch.float32))
    elif act != "none":
        raise ValueError(act)
    return y32 if addend is None else y32 + addend.to(torch.float32)


def expected_exact(kind, c, a, b, arith, mutate=None, chunk=None, **epi):
    """fl32 of the exact value under fp32 and bf16x6 (and on the VALU routes), of the E3 emulation under bf16x3."""
    terms = E3 if arith == "bf16x3" else (None if mutate is None or arith == "fp32" else E6)
    y = reference(kind, c, a, b, terms, mutate, chunk).to(torch.float32)
    return epilogue(y, **epi) if epi else y


def check_exact(got, kind, c, a, b, arith, mutate=None, chunk=None, what="", taps=None, label=None, sums=False,
                **epi):
    """Bit equality of `got` with the expected value.  taps: per output channel, the K index (forward / data
    gradient) or pixel index (weight gradient) of its non-zero operand, named in the failure message.
    sums=False: outputs that are the sum of two or more non-zero products are left out — the data gradient of a
    reflect-padded conv folds up to four mirrored positions onto a border pixel, and a sum of full-significand
    products rounds; the few-hot probes (sums=True: every partial sum representable) cover those outputs."""
    want = expected_exact(kind, c, a, b, arith, mutate, chunk, **epi)
    got = got.detach().cpu().to(torch.float32)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = _canon(got) != _canon(want)
    if not sums and kind == "dgrad" and c.mode == "reflect":
        single = ref(kind, c, (a != 0).to(F64), (b != 0).to(F64)) <= 1
        assert single.double().mean().item() >= 0.5, (what, "most outputs must be single products")
        bad &= single
    if label is not None:
        k = EXACT.setdefault(label, [0, 0])
        k[0] += int(not bad.any())
        k[1] += 1
    if bad.any():
        idx = tuple(int(v) for v in bad.nonzero()[0])
        ch = idx[0] if kind == "wgrad" else idx[1]
        where = ""
        if taps is not None:
            t = [int(v) for v in taps[ch]]
            nch = k_axes(kind, c)[1] // (c.R * c.S)
            where = (f" dy pixels {t}" if kind == "wgrad" else
                     f" taps (r, s, channel) {[(v // (c.S * nch), v // nch % c.S, v % nch) for v in t]}, "
                     f"K stage {[v // KSTAGE for v in t]}")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ; first at {idx}: got "
                             f"{got[idx].item()!r} ({got[idx].item().hex()}), want {want[idx].item()!r} "
                             f"({want[idx].item().hex()});{where}")


def c_bound(arith, K, slabs=1, mfma_k=16, f32_always=False):
    """Rounding count c of |y - y64| <= c u B + u |y64| for one output of a K-deep GEMM, u = 2^-24.

    Split residual and dropped terms.  With bf16's unit roundoff 2^-8, |mid| <= 2^-8 |v|, |lo| <= 2^-16 |v| and
    v = hi + mid + lo + rho with |rho| <= 2^-24 |v|.  bf16x6 drops mid*lo + lo*mid (2 * 2^-24), lo*lo (2^-32) and
    the rho terms (2 * 2^-24): 4 u |a||b| per product, rounded up to 4.1.  bf16x3 carries v = hi + mid + rho2 with
    |rho2| <= 2^-16 |v| and drops mid*mid (2^-16) and the rho2 terms (2 * 2^-16): 3 * 2^8 u, taken as 769.
    fp32 (and the VALU routes) multiply exactly inside an fma: 0.
    Accumulation.  Every MFMA adds its mfma_k exact products to the fp32 accumulator with one rounding (what the
    tier-A few-hot probes pin for representable sums), so an output takes np * ceil(K / mfma_k) roundings, np = 6
    or 3 plane products; the partial sums are bounded by the sum of the plane products' magnitudes,
    <= (1 + 2^-7) B.  An fma chain rounds once per element: K.  Split-K slabs and the accumulate add: one rounding
    per slab.  The last u |y64| is the final rounding of y64 itself to fp32."""
    if f32_always or arith == "fp32":
        return float(K + slabs)
    steps = -(-K // mfma_k)
    if arith == "bf16x6":
        return 4.1 + (6 * steps + slabs) * (1 + 2.0 ** -7)
    return 769.0 + (3 * steps + slabs) * (1 + 2.0 ** -7)


def check_bound(got, kind, c, a, b, cc, terms=None, mutate=None, chunk=None, what="", label=None, extra=None):
    """|got - ref| <= cc u B + u |ref| for every output, printing the worst ratio first.  The reference is the exact
    fp64 op; with a slip (`mutate`) it is the slipped emulation of `terms`.  extra: exact fp64 tensor added to the
    reference (an accumulate pre-fill or addend)."""
    y = reference(kind, c, a, b, terms if mutate is not None else None, mutate, chunk)
    if extra is not None:
        y = y + extra.to(F64)
    B = magnitude(kind, c, a, b)
    err = (got.detach().cpu().to(F64) - y).abs()
    tol = cc * U * B + U * y.abs()
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), (err > 0).to(F64) * float("inf"))
    worst = ratio.max().item() if bool(torch.isfinite(err).all()) else float("inf")
    print(f"{what}: worst err/bound = {worst:.3g} (c = {cc:.1f})")
    if label is not None:
        WORST[label] = max(WORST.get(label, 0.0), worst)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst err/bound {worst:.3g}"
    return worst


def dense(kind, c, seed):
    """Tier B data: randn times a per-channel power of two spanning 2^+-12 (channels of both operands), so no
    channel group hides behind another."""
    sa, sb = operand_shapes(kind, c)
    g = _gen(seed)

    def scaled(shape, chan_dims):
        t = torch.randn(shape, generator=g)
        for d in chan_dims:
            v = [1] * len(shape)
            v[d] = shape[d]
            t = t * torch.exp2(torch.randint(-12, 13, (shape[d],), generator=g).to(torch.float32)).view(v)
        return t
    if kind == "wgrad":
        return scaled(sa, (1,)), scaled(sb, (1,))
    return scaled(sa, (1,)), scaled(sb, (0, 1)) * 2.0 ** -6


# ==================================================================================== adaptors
def _dev(t):
    return t.to("cuda").contiguous()


def _bias(ops, bias, n):
    if bias is None:
        return None
    bp = torch.zeros(cpad(n), device="cuda")
    bp[:n] = bias.to("cuda")
    return bp


def run_fwd(ops, c, x, w, bias=None, act="none", slope=0.0):
    wp = ops.weight_pack(_dev(w), ops.PACK_FWD)
    xn = ops.nchw_to_nhwc(_dev(x))
    bp = _bias(ops, bias, c.Co)
    if c.ph != c.pw or c.R != c.S:
        assert c.mode == "zero" and slope == 0.0
        y = ops.conv2d_fwd_hw(xn, wp, bp, cpad(c.Co), c.R, c.S, c.stride, c.ph, c.pw, act)
    else:
        y = ops.conv2d_fwd(xn, wp, bp, cpad(c.Co), c.R, c.S, c.stride, c.ph, c.mode, act, slope)
    return ops.nhwc_to_nchw(y, c.Co).cpu()


def run_tfwd(ops, c, dy, w, bias=None, act="none", slope=0.0, addend=None):
    ck = ops.weight_pack(_dev(w), ops.PACK_DGRAD)
    ad = None if addend is None else ops.nchw_to_nhwc(_dev(addend))
    dx = ops.conv2d_tfwd(ops.nchw_to_nhwc(_dev(dy)), ck, _bias(ops, bias, c.Ci), c.H, c.W, cpad(c.Ci), c.R, c.S,
                         c.stride, c.ph, act, slope, pad_mode=c.mode, addend=ad)
    return ops.nhwc_to_nchw(dx, c.Ci).cpu()


def run_dgrad_s1(ops, c, dy, w, addend=None):
    ikf = ops.weight_pack(_dev(w), ops.PACK_IKF)
    ad = None if addend is None else ops.nchw_to_nhwc(_dev(addend))
    dx = ops.conv2d_dgrad_s1(ops.nchw_to_nhwc(_dev(dy)), ikf, c.H, c.W, cpad(c.Ci), c.R, c.ph, c.mode, addend=ad)
    return ops.nhwc_to_nchw(dx, c.Ci).cpu()


def run_wgrad_images(ops, c, x, dy, prefill=None):
    """The operand images as a layer's producers hand them over: x's padded channel-major image written by the IN
    apply (identity statistics, so a == x bit for bit) and dy's channel-major bf16 planes [3][Cyp][ld]."""
    xn, dyn = ops.nchw_to_nhwc(_dev(x)), ops.nchw_to_nhwc(_dev(dy))
    st = torch.zeros((c.N, xn.shape[-1], 2), device="cuda")
    st[..., 1] = 1.0
    a, x_t = ops.instnorm_act_fwd(xn, st, "none", cp=(c.ph, c.mode, c.stride))
    assert torch.equal(a, xn)
    cyp, ld = dyn.shape[-1], ops.lib().vst_cp_ld(c.P)
    pl = torch.zeros((3, cyp, ld), dtype=torch.bfloat16)
    for i, p in enumerate(split3(dyn.cpu().view(c.P, cyp).t())):
        pl[i, :, :c.P] = p.to(torch.bfloat16)
    dw = torch.full((c.Co, c.Ci, c.R, c.S), float("nan"), device="cuda")
    if prefill is not None:
        dw.copy_(prefill)
    ops.conv2d_wgrad(xn, dyn, dw, None, c.R, c.S, c.stride, c.ph, c.mode, c.Co, c.Ci, c.Ci * c.R * c.S, c.R * c.S,
                     accumulate=prefill is not None, dy_planes=pl.to("cuda"), x_t=x_t)
    return dw.cpu()


def run_wgrad_planes(ops, c, x, dy, prefill=None):
    """dy handed over only as its NHWC bf16 planes (what the IN backward writes for the planes-only chain)."""
    return run_wgrad(ops, c, x, dy, prefill, planes=True)


def run_wgrad(ops, c, x, dy, prefill=None, planes=False):
    dw = torch.empty((c.Co, c.Ci, c.R, c.S), device="cuda")
    if prefill is not None:
        dw.copy_(prefill)
    else:
        dw.fill_(float("nan"))
    dyn = ops.nchw_to_nhwc(_dev(dy))
    if planes:
        dyn.vst_apl = torch.stack([p.to(torch.bfloat16).reshape(-1) for p in split3(dyn.cpu())]).to("cuda").contiguous()
        dyn.vst_planes_only = True
        dyn.fill_(float("nan"))  # the fp32 image of a planes-only dy is never written: no route may read it
    ops.conv2d_wgrad(ops.nchw_to_nhwc(_dev(x)), dyn, dw, None, c.R, c.S, c.stride, c.ph, c.mode,
                     c.Co, c.Ci, c.Ci * c.R * c.S, c.R * c.S, accumulate=prefill is not None)
    return dw.cpu()


def run_fwd_head(ops, c, x, w, bias=None, act="none", slope=0.0):
    """One real output channel padded to 4 (the PatchGAN head: vst_conv2d_fwd_ex with co_real = 1 and its workspace)."""
    wp = ops.weight_pack(_dev(w), ops.PACK_FWD)
    y = ops.conv2d_fwd(ops.nchw_to_nhwc(_dev(x)), wp, _bias(ops, bias, 1), 4, c.R, c.S, c.stride, c.ph, c.mode, act, slope,
                       co_real=1)
    return ops.nhwc_to_nchw(y, 1).cpu()


def run_tfwd_head(ops, c, dy, w, addend=None):
    ck = ops.weight_pack(_dev(w), ops.PACK_DGRAD)
    ad = None if addend is None else ops.nchw_to_nhwc(_dev(addend))
    dx = ops.conv2d_tfwd(ops.nchw_to_nhwc(_dev(dy)), ck, None, c.H, c.W, cpad(c.Ci), c.R, c.S, c.stride, c.ph,
                         pad_mode=c.mode, addend=ad, co_real=1)
    return ops.nhwc_to_nchw(dx, c.Ci).cpu()


def run_fwd_in(ops, c, x, w, bias=None, act="none", slope=0.0, want_stats=False):
    """The conv that feeds an InstanceNorm: the statistics partials come out of the GEMM's epilogue."""
    wp = ops.weight_pack(_dev(w), ops.PACK_FWD)
    y, st = ops.conv2d_fwd_in(ops.nchw_to_nhwc(_dev(x)), wp, _bias(ops, bias, c.Co), cpad(c.Co), c.R, c.S, c.stride, c.ph,
                              c.mode)
    y = ops.nhwc_to_nchw(y, c.Co).cpu()
    return (y, st[:, :c.Co].cpu()) if want_stats else y


def run_tap_fwd(ops, c, x, w, bias=None, act="none", slope=0.0):
    ck = ops.weight_pack(_dev(w), ops.PACK_CK)
    y = ops.tap_conv_fwd(ops.nchw_to_nhwc(_dev(x)), ck, _bias(ops, bias, c.Co), c.R, c.ph, c.mode, act, slope)
    return ops.nhwc_to_nchw(y, c.Co).cpu()


def run_tap_fwd_h(ops, c, x, w, bias=None, act="none", slope=0.0):
    sok = ops.weight_pack(_dev(w), ops.PACK_SOK, Op=4)
    y = ops.tap_conv_fwd_h(ops.nchw_to_nhwc(_dev(x)), sok, _bias(ops, bias, c.Co), c.R, c.ph, c.mode, act, slope)
    return ops.nhwc_to_nchw(y, c.Co).cpu()


def run_tap_dgrad(ops, c, dy, w):
    kc = ops.weight_pack(_dev(w), ops.PACK_KC)
    return ops.nhwc_to_nchw(ops.tap_conv_dgrad(ops.nchw_to_nhwc(_dev(dy)), kc, c.R, c.ph, c.mode), c.Ci).cpu()


def run_tap_dgrad_h(ops, c, dy, w):
    sokd = ops.dgrad_sok_pack(_dev(w))
    return ops.nhwc_to_nchw(ops.tap_conv_dgrad_h(ops.nchw_to_nhwc(_dev(dy)), sokd, c.R, c.ph, c.mode), c.Ci).cpu()


def _tap_wgrad(fn_name):
    def run(ops, c, x, dy, prefill=None):
        dw = torch.full((c.Co, c.Ci, c.R, c.S), float("nan"), device="cuda")
        if prefill is not None:
            dw.copy_(prefill)
        getattr(ops, fn_name)(ops.nchw_to_nhwc(_dev(x)), ops.nchw_to_nhwc(_dev(dy)), dw, c.R, c.ph, c.mode,
                              accumulate=prefill is not None)
        return dw.cpu()
    return run


run_tap_wgrad, run_tap_wgrad_h, run_tap_wgrad_swap = (_tap_wgrad(n) for n in
                                                      ("tap_conv_wgrad", "tap_conv_wgrad_h", "tap_conv_wgrad_swap"))


def run_convT3(ops, c, x, wt, bias=None, act="none", slope=0.0):
    """ConvTranspose2d(k3, s2, p1, op1) through its four phase convs: wt [Ci_T][Co_T][3][3] is this table's w."""
    packs = ops.convT3s2_phase_packs(_dev(wt))
    y = ops.convT3s2_fwd(ops.nchw_to_nhwc(_dev(x)), packs, _bias(ops, bias, c.Ci), cpad(c.Ci), act)
    return ops.nhwc_to_nchw(y, c.Ci).cpu()


def run_conv4s2_dgrad(ops, c, dy, w, bias=None, act="none", slope=0.0):
    """Conv2d(k4, s2, p1) data gradient / ConvTranspose2d(k4, s2, p1) forward through four 2x2 phase convs."""
    packs = ops.conv4s2_dgrad_phase_packs(_dev(w))
    y = ops.convT4s2_fwd(ops.nchw_to_nhwc(_dev(dy)), packs, _bias(ops, bias, c.Ci), cpad(c.Ci), act)
    return ops.nhwc_to_nchw(y, c.Ci).cpu()


def run_c4_dgrad_reflect(ops, c, dy, w):
    ikf = ops.weight_pack(_dev(w), ops.PACK_IKF)
    dx = ops.c4_dgrad_reflect(ops.nchw_to_nhwc(_dev(dy)), ikf, c.H, c.W, cpad(c.Ci), c.R, c.ph)
    return ops.nhwc_to_nchw(dx, c.Ci).cpu()


def _run_dgrad_refl_in(apre):
    def run(ops, c, dy, w, addend=None):
        """The reflect-pad-1 data gradient with the IN backward of the layer below in its epilogue: only the data
        gradient g is compared here; apre: dy arrives as the NHWC bf16 planes a producer wrote."""
        ikf = ops.weight_pack(_dev(w), ops.PACK_IKF)
        dyn = ops.nchw_to_nhwc(_dev(dy))
        if apre:
            dyn.vst_apl = torch.stack([p.to(torch.bfloat16).reshape(-1) for p in split3(dyn.cpu())]).to("cuda").contiguous()
        y_in = torch.randn((c.N, c.H, c.W, cpad(c.Ci)), generator=_gen(5)).to("cuda")
        ad = None if addend is None else ops.nchw_to_nhwc(_dev(addend))
        r = ops.conv2d_dgrad_refl_in(dyn, ikf, c.H, c.W, cpad(c.Ci), y_in, ops.instnorm_stats(y_in), "relu", addend=ad)
        assert r is not None, "conv2d_dgrad_refl_in declined the shape"
        return ops.nhwc_to_nchw(r[0], c.Ci).cpu()
    return run


# ================================================================================= route table
class Route(NamedTuple):
    name: str
    kind: str            # fwd | dgrad | wgrad
    run: object          # adaptor
    case: Conv           # tier A shape: the smallest the planner sends this way
    reaches: object      # reaches(ops, case, math) -> bool, host code only
    maths: tuple = ("fp32", "bf16x3", "bf16x6")
    tiles: tuple = (-1, -1, -1)
    flags: dict = {}     # ops module flags flipped for the call
    f32_always: bool = False   # fp32 fmas whatever the policy says: the VALU kernels and the fp32-MFMA conv_wgrad_k
    tier_b: Conv = None  # dense-data shape (K about 27-72) or None: tier A only
    mfma_k: int = 16     # K depth of one accumulation (c_bound): 16 is the 32x32x16 loop's; the 16x16x32 loop and
    #                      the fp32 kernels' split forms round less often, so 16 bounds them all
    slabs: object = None  # slabs(ops, case, math) -> split-K slab count added into an output
    epi: tuple = None    # names of the exact epilogue probes the entry point has (None: all of its kind)
    all_pixels: bool = False  # weight gradients whose GEMM is not the nominal conv's (tap forms, the head kernel):
    #                           its chunks are not this conv's plan, so the one-hot dy visits EVERY pixel
    a_stride: int = 1    # > 1: this row takes every a_stride-th one-hot set (a second arithmetic of a row that has all)
    x3_sums: bool = True  # False: under bf16x3 a folded sum mixes E3 products with fp32 ones (no single expected value)


def _fwd_geom(c):
    return (c.N, c.H, c.W, cpad(c.Ci), cpad(c.Co), c.R, c.S, c.stride)


def _plan_fwd(ops, c, m):
    return ops.conv_plan_fwd(*_fwd_geom(c), c.ph, c.pw, m, with_tail=True)


def _tail(ops, c, m):
    return ops.conv_plan_fwd_tail(*_fwd_geom(c), c.ph, m) if ops.FWD_SPLITK else 0


def _bf_kind(kind):
    def reaches(ops, c, m):
        return m != "fp32" and _plan_fwd(ops, c, m) == (kind, 0, -1) and _tail(ops, c, m) == 0
    return reaches


def _fwd_plan_is(plan_name, tail=False):
    def reaches(ops, c, m):
        k = _plan_fwd(ops, c, m)[0]
        want = getattr(ops, plan_name) if isinstance(plan_name, str) else plan_name
        return k == want and (_tail(ops, c, m) > 0) == tail
    return reaches


def _fwd_auto(ops, c, m):  # the planner's own small-grid tile under the split arithmetics, the [row][k] kernel under fp32
    k = _plan_fwd(ops, c, m)[0]
    return (k == ops.PLAN_RK) if m == "fp32" else (0 <= k <= 9 and _tail(ops, c, m) == 0)


def _fwd_splitk(ops, c, m):
    return _tail(ops, c, m) > 0 and _plan_fwd(ops, c, m)[1] == 0


def _fwd_c4_implicit(ops, c, m):
    return cpad(c.Ci) == 4 and 0 <= _plan_fwd(ops, c, m)[0] <= 9


def _skinny_split(ops, c, m):  # the VALU forward's own split-K test (vst_skinny_split_ok)
    return _plan_fwd(ops, c, m)[0] == ops.PLAN_SKINNY and \
        bool(ops.lib().vst_skinny_split_ok(c.N, c.Ho, c.Wo, cpad(c.Ci), c.R, c.S))


def _skinny_plain(ops, c, m):
    return _plan_fwd(ops, c, m)[0] == ops.PLAN_SKINNY and \
        not ops.lib().vst_skinny_split_ok(c.N, c.Ho, c.Wo, cpad(c.Ci), c.R, c.S)


def _wg_geom(c):
    return (c.N, c.H, c.W, cpad(c.Ci), c.Ho, c.Wo, cpad(c.Co), c.R, c.S, c.stride)


def wgrad_plan(ops, c, m):
    """(route, plan path, tile kind, nsplit) of conv2d_wgrad for an fp32 dy."""
    return (ops.wgrad_route(*_wg_geom(c), c.ph, False, m),) + tuple(ops.conv_plan_wgrad(*_wg_geom(c), m))


def wgrad_chunk(ops, c, m):
    """(pixels per split-K chunk, row width) of the plan, read from the planner (vst_conv_plan_wgrad_chunk): the
    chunk is P / nsplit rounded up to the kernel's K step, over rows padded to row_w columns on the Wo-padded plan."""
    import ctypes
    chunk, row_w = ctypes.c_int(0), ctypes.c_int(0)
    rc = ops.lib().vst_conv_plan_wgrad_chunk(*_wg_geom(c), ops._math(m), ctypes.addressof(chunk), ctypes.addressof(row_w))
    assert rc == 0
    return chunk.value, row_w.value


def _wg(route, path=None):
    def reaches(ops, c, m):
        r, p, _, _ = wgrad_plan(ops, c, m)
        return r == getattr(ops, route) and (path is None or p == ops._C[path])
    return reaches


def _wg_nhwc(planes, im2col=False):
    def reaches(ops, c, m):
        g = _wg_geom(c) + (c.ph,)
        nhwc_ok = bool(ops.lib().vst_conv2d_wgrad_nhwc_ok(*g, ops._math(m)))
        r = ops.wgrad_route(*g, planes, m)
        if planes:
            return r == ops.WG_NHWC and nhwc_ok
        return r == ops.WG_NHWC_F32 and nhwc_ok != im2col and \
            int(ops.lib().vst_conv2d_wgrad_nhwc_f32_ws_bytes(*g, ops._math(m))) > 0
    return reaches


def _wg_tile(pred, kind):
    return lambda ops, c, m: pred(ops, c, m) and wgrad_plan(ops, c, m)[2] == kind


def _wg_slabs(ops, c, m):
    return wgrad_plan(ops, c, m)[3] + 1


def _dgrad_refl_border(ops, c, m):
    return ops.DGRAD_BORDER and c.R == 3 and c.ph == 1 and m != "fp32" and \
        int(ops.lib().vst_conv2d_dgrad_refl_ws_bytes(c.N, c.H, c.W, cpad(c.Co), cpad(c.Ci), ops._math(m))) > 0


def _dgrad_as_fprop(ops, c, m):  # the forward kernel over dy with Cop = cpad(Ci), pad R - 1 (- pad under zero padding)
    p = c.R - 1 - (0 if c.mode == "reflect" else c.ph)
    k = ops.conv_plan_fwd(c.N, c.Ho, c.Wo, cpad(c.Co), cpad(c.Ci), c.R, c.S, 1, p, p, m)[0]
    return (k == ops.PLAN_RK) if m == "fp32" else 0 <= k <= 9


def _plan_tfwd(ops, c):
    import ctypes
    plan = ctypes.c_int(0)
    assert ops.lib().vst_conv_plan_tfwd(cpad(c.Ci), ctypes.addressof(plan)) == 0
    return plan.value


def _tfwd_rk(ops, c, m):  # vst_conv2d_tfwd's own dispatch (vst_conv_plan_tfwd): the [row][k] kernel or the VALU one
    return _plan_tfwd(ops, c) == ops.PLAN_RK


def _tfwd_skinny(ops, c, m):
    return _plan_tfwd(ops, c) == ops.PLAN_SKINNY


SPLIT = ("bf16x3", "bf16x6")
# the two shapes every forced tile kind runs: Ci a multiple of every BK with reflect padding (the staged-A loop with
# the mirror gather), and Ci % 16 != 0, stride 2, zero padding (the per-element gather); M and Co are no multiple of
# any tile, Co spans two 32-wide wave tiles
_FAST = Conv(2, 64, 9, 10, 40, 3, 3, 1, 1, 1, "reflect")
_SLOW = Conv(2, 24, 11, 13, 40, 3, 3, 2, 1, 1, "zero")
_SMALLK = Conv(2, 8, 9, 10, 40, 3, 3, 1, 1, 1, "reflect")   # K = 72

ROUTES = []
for _k in range(10):
    ROUTES.append(Route(f"fwd_bf_kind{_k}_staged", "fwd", run_fwd, _FAST, _bf_kind(_k), SPLIT, (_k, -1, -1),
                        tier_b=_SMALLK))
    ROUTES.append(Route(f"fwd_bf_kind{_k}_gather", "fwd", run_fwd, _SLOW, _bf_kind(_k), SPLIT, (_k, -1, -1)))
ROUTES += [
    Route("fwd_auto", "fwd", run_fwd, _FAST, _fwd_auto, ("fp32", "bf16x3"), tier_b=_SMALLK),
    Route("fwd_auto_s2", "fwd", run_fwd, _SLOW, _fwd_auto, tier_b=Conv(2, 8, 11, 13, 40, 3, 3, 2, 1, 1, "zero")),
    Route("fwd_splitk_full", "fwd", run_fwd, Conv(1, 64, 16, 16, 64, 3, 3, 1, 1, 1, "reflect"), _fwd_splitk,
          ("bf16x6",), slabs=lambda ops, c, m: _tail(ops, c, m)),
    Route("fwd_splitk_full_odd", "fwd", run_fwd, _FAST, _fwd_splitk, ("bf16x6",),
          slabs=lambda ops, c, m: _tail(ops, c, m)),
    Route("fwd_no_splitk", "fwd", run_fwd, Conv(1, 64, 16, 16, 64, 3, 3, 1, 1, 1, "reflect"), _fwd_auto, ("bf16x6",),
          flags={"FWD_SPLITK": False}),
    Route("fwd_rk_c12", "fwd", run_fwd, Conv(2, 12, 9, 10, 40, 3, 3, 1, 1, 1, "reflect"),
          _fwd_plan_is("PLAN_RK"), tier_b=Conv(2, 12, 9, 10, 40, 2, 2, 1, 1, 1, "reflect")),
    Route("fwd_rk_c12_s2", "fwd", run_fwd, Conv(2, 12, 11, 13, 24, 4, 4, 2, 1, 1, "zero"), _fwd_plan_is("PLAN_RK")),
    Route("fwd_c4_direct", "fwd", run_fwd, Conv(1, 3, 16, 32, 64, 7, 7, 1, 3, 3, "reflect"),
          _fwd_plan_is("PLAN_C4_DIRECT"), SPLIT),
    Route("fwd_c4_implicit", "fwd", run_fwd, Conv(2, 3, 12, 14, 16, 4, 4, 2, 1, 1, "zero"), _fwd_c4_implicit, SPLIT,
          tier_b=Conv(2, 3, 12, 14, 16, 4, 4, 2, 1, 1, "zero")),
    Route("fwd_skinny_out", "fwd", run_fwd, Conv(2, 16, 9, 10, 3, 7, 7, 1, 3, 3, "reflect"),
          _skinny_plain, f32_always=True, tier_b=Conv(2, 8, 9, 10, 3, 3, 3, 1, 1, 1, "reflect")),
    Route("fwd_hw_1x5", "fwd", run_fwd, Conv(1, 32, 6, 11, 40, 1, 5, 1, 0, 2, "zero"), _fwd_auto,
          tier_b=Conv(1, 8, 6, 11, 40, 1, 5, 1, 0, 2, "zero")),
    Route("fwd_hw_5x1", "fwd", run_fwd, Conv(1, 32, 11, 6, 40, 5, 1, 1, 2, 0, "zero"), _fwd_auto),
    # ---- data gradients
    Route("tfwd_s1_zero", "dgrad", run_tfwd, Conv(2, 24, 9, 10, 40, 3, 3, 1, 1, 1, "zero"), _tfwd_rk,
          tier_b=Conv(2, 24, 9, 10, 8, 3, 3, 1, 1, 1, "zero")),
    Route("tfwd_s2_zero", "dgrad", run_tfwd, Conv(2, 24, 11, 13, 40, 3, 3, 2, 1, 1, "zero"), _tfwd_rk,
          tier_b=Conv(2, 24, 11, 13, 8, 3, 3, 2, 1, 1, "zero")),
    Route("tfwd_s2_k4", "dgrad", run_tfwd, Conv(2, 16, 12, 14, 24, 4, 4, 2, 1, 1, "zero"), _tfwd_rk),
    Route("tfwd_convT_k3s2", "dgrad", run_tfwd, Conv(2, 16, 12, 14, 24, 3, 3, 2, 1, 1, "zero"), _tfwd_rk,
          tier_b=Conv(2, 16, 12, 14, 8, 3, 3, 2, 1, 1, "zero")),
    Route("tfwd_s1_reflect", "dgrad", run_tfwd, Conv(2, 24, 9, 10, 40, 3, 3, 1, 1, 1, "reflect"), _tfwd_rk,
          tier_b=Conv(2, 24, 9, 10, 8, 3, 3, 1, 1, 1, "reflect")),
    Route("tfwd_c7_reflect", "dgrad", run_tfwd, Conv(1, 8, 9, 10, 16, 7, 7, 1, 3, 3, "reflect"), _tfwd_rk),
    Route("tfwd_skinny_c3", "dgrad", run_tfwd, Conv(2, 3, 9, 10, 16, 7, 7, 1, 3, 3, "reflect"), _tfwd_skinny, f32_always=True),
    Route("tfwd_skinny_c3_s2", "dgrad", run_tfwd, Conv(2, 3, 12, 14, 16, 4, 4, 2, 1, 1, "zero"), _tfwd_skinny, f32_always=True),
    Route("tfwd_rk_kind0", "dgrad", run_tfwd, Conv(2, 24, 9, 10, 40, 3, 3, 1, 1, 1, "reflect"), _tfwd_rk,
          tiles=(-1, 0, -1)),
    Route("tfwd_rk_kind5_s2", "dgrad", run_tfwd, Conv(2, 24, 11, 13, 40, 3, 3, 2, 1, 1, "zero"), _tfwd_rk,
          tiles=(-1, 5, -1)),
    Route("dgrad_s1_zero", "dgrad", run_dgrad_s1, Conv(2, 24, 9, 10, 40, 3, 3, 1, 1, 1, "zero"), _dgrad_as_fprop,
          tier_b=Conv(2, 24, 9, 10, 8, 3, 3, 1, 1, 1, "zero")),
    Route("dgrad_s1_k4_zero", "dgrad", run_dgrad_s1, Conv(2, 24, 9, 11, 32, 4, 4, 1, 1, 1, "zero"), _dgrad_as_fprop),
    Route("dgrad_s1_refl_border", "dgrad", run_dgrad_s1, Conv(2, 24, 9, 10, 32, 3, 3, 1, 1, 1, "reflect"),
          _dgrad_refl_border, SPLIT),
    Route("dgrad_s1_refl_fold", "dgrad", run_dgrad_s1, Conv(2, 24, 9, 10, 32, 3, 3, 1, 1, 1, "reflect"),
          _dgrad_as_fprop, flags={"DGRAD_BORDER": False}, tier_b=Conv(2, 24, 9, 10, 8, 3, 3, 1, 1, 1, "reflect")),
    Route("dgrad_s1_c7_fold", "dgrad", run_dgrad_s1, Conv(1, 8, 9, 10, 16, 7, 7, 1, 3, 3, "reflect"),
          _dgrad_as_fprop),
]
# ---- weight gradients: the shapes are found by tests/test_conv_ref_host.py's predicate, not assumed
ROUTES += [
    Route("wgrad_plain_generic", "wgrad", run_wgrad, Conv(2, 16, 9, 7, 24, 3, 3, 1, 1, 1, "reflect"),
          _wg("WG_PLAIN", "VST_WPLAN_GENERIC"), slabs=_wg_slabs, f32_always=True,
          tier_b=Conv(1, 16, 7, 5, 24, 3, 3, 1, 1, 1, "reflect")),
    Route("wgrad_plain_generic_s2", "wgrad", run_wgrad, Conv(2, 16, 11, 13, 24, 3, 3, 2, 1, 1, "zero"),
          _wg("WG_PLAIN", "VST_WPLAN_GENERIC"), slabs=_wg_slabs, f32_always=True),
    Route("wgrad_plain_rk", "wgrad", run_wgrad, Conv(2, 16, 9, 12, 24, 3, 3, 1, 1, 1, "reflect"),
          _wg("WG_PLAIN", "VST_WPLAN_RK"), ("fp32", "bf16x3"), slabs=_wg_slabs,
          flags={"WGRAD_NHWC_F32": False}, tier_b=Conv(1, 16, 6, 4, 24, 3, 3, 1, 1, 1, "reflect")),
    Route("wgrad_plain_skinny", "wgrad", run_wgrad, Conv(2, 16, 9, 10, 3, 7, 7, 1, 3, 3, "reflect"),
          _wg("WG_PLAIN", "VST_WPLAN_SKINNY"), slabs=_wg_slabs, f32_always=True),
    Route("wgrad_images_bf", "wgrad", run_wgrad, Conv(2, 16, 9, 16, 24, 3, 3, 1, 1, 1, "reflect"),
          _wg("WG_IMAGES", "VST_WPLAN_BF"), ("bf16x6",), slabs=_wg_slabs, flags={"WGRAD_NHWC_F32": False},
          tier_b=Conv(1, 16, 5, 8, 24, 3, 3, 1, 1, 1, "reflect")),
    Route("wgrad_images_bf_s2", "wgrad", run_wgrad, Conv(2, 16, 10, 16, 24, 4, 4, 2, 1, 1, "zero"),
          _wg("WG_IMAGES", "VST_WPLAN_BF"), ("bf16x6",), slabs=_wg_slabs, flags={"WGRAD_NHWC_F32": False}),
    Route("wgrad_images_producer", "wgrad", run_wgrad_images, Conv(2, 16, 9, 16, 24, 3, 3, 1, 1, 1, "reflect"),
          lambda ops, c, m: wgrad_plan(ops, c, m)[1] == ops.WPLAN_BF, ("bf16x6",), slabs=_wg_slabs),
    Route("wgrad_images_producer_s2", "wgrad", run_wgrad_images, Conv(2, 16, 10, 16, 24, 4, 4, 2, 1, 1, "zero"),
          lambda ops, c, m: wgrad_plan(ops, c, m)[1] == ops.WPLAN_BF, ("bf16x6",), slabs=_wg_slabs),
    Route("wgrad_bf_padw", "wgrad", run_wgrad, Conv(2, 16, 9, 11, 24, 3, 3, 1, 1, 1, "zero"),
          _wg("WG_PLAIN", "VST_WPLAN_BF_PADW"), ("bf16x6",), slabs=_wg_slabs, flags={"WGRAD_NHWC_F32": False}),
]


def _fwd_tail(ops, c, m):  # whole rounds of 256x128 tiles, then the last partial round as split-K slabs
    return _plan_fwd(ops, c, m)[0] == 7 and _plan_fwd(ops, c, m)[1] > 0 and _tail(ops, c, m) > 0


def _head_fwd(ops, c, m):
    return c.Co == 1 and int(ops.lib().vst_conv2d_fwd_ex_ws_bytes(c.N, c.H, c.W, cpad(c.Ci), 4, c.R, c.S, c.stride, c.ph,
                                                                  c.ph, ops.PAD[c.mode], ops._math(m), 1)) > 0


def _head_ok(ops, c, m):  # the head kernels' own condition (vst_head_ok) on the width of dy
    return c.Co == 1 and cpad(c.Co) == 4 and bool(ops.lib().vst_head_ok(cpad(c.Ci), c.R, c.S, c.stride, ops.PAD[c.mode],
                                                                        c.Wo))


def _img_wgrad(ops, c, m):  # vst_conv2d_wgrad's own test for the image-input kernel
    return bool(ops.lib().vst_img_wgrad_ok(cpad(c.Ci), cpad(c.Co), c.R, c.S, c.stride, ops.PAD[c.mode], c.Ci, c.Wo))


def _tap64_ok(ops, c, m):
    nch = cpad(c.Co if c.Ci <= 4 else c.Ci)
    W = c.W if c.Ci > 4 else c.Wo
    return bool(ops.lib().vst_tap64_ok(nch, c.R, W, ops._math(m)))


def _tap_h(ops, c, m):
    """vst_tapconv_h_fwd off the direct kernel (vst_tap64_ok false): the R x 1 conv onto 4R channels (its plan a
    split-bf16 tile or the [row][k] kernel) + the column-tap sum.  The data gradient runs it over dy, zero pad R-1."""
    fwd = c.Ci > 4
    nch, pad = cpad(c.Ci if fwd else c.Co), (c.ph if fwd else c.R - 1)
    k = ops.conv_plan_fwd(c.N, c.H, c.W, nch, 4 * c.R, c.R, 1, 1, pad, 0, m)[0]
    return not _tap64_ok(ops, c, m) and ((k == ops.PLAN_RK) if (m == "fp32" or nch % 8) else 0 <= k <= 9)


def _tap_1x1(ops, c, m):  # the tap forms run a 1x1 conv onto R R 4 channels: its plan is a split-bf16 tile / the fp32 kernel
    nch = cpad(c.Co if c.Ci <= 4 else c.Ci)
    k = ops.conv_plan_fwd(c.N, c.H, c.W, nch, c.R * c.R * 4, 1, 1, 1, 0, 0, m)[0]
    return (k == ops.PLAN_RK) if (m == "fp32" or nch % 8) else 0 <= k <= 9


def _shape_x(c):
    return torch.empty((c.N, c.H, c.W, cpad(c.Ci)), device="meta")


def _tap_wgrad_ok(which):
    def reaches(ops, c, m):
        fn = {"bf": lambda: ops.TAP_PLANES and ops.tap_conv_wgrad_bf_ok(_shape_x(c), c.R, m),
              # the fold + the 1x1 weight gradient onto R R 4 channels on conv2d_wgrad's own plan; under bf16x3 that
              # must be the [row][k] plan (split arithmetic): the generic plan would compute in fp32
              "plain": lambda: (not ops.tap_conv_wgrad_bf_ok(_shape_x(c), c.R, m) or not ops.TAP_PLANES) and
              (m != "bf16x3" or ops.conv_plan_wgrad(c.N, c.H, c.W, cpad(c.Ci), c.H, c.W, c.R * c.R * 4, 1, 1, 1, m)[0]
               == ops._C["VST_WPLAN_RK"]),
              "h": lambda: ops.tap_conv_wgrad_h_ok(_shape_x(c), c.R, c.ph, c.mode, m),
              "swap": lambda: ops.tap_conv_wgrad_swap_ok(_shape_x(c), c.R, c.ph, c.mode, m, co=c.Co)}[which]
        return bool(fn())
    return reaches


def _convT3(route):  # ops.convT3s2_route: the function convT3s2_fwd itself branches on
    return lambda ops, c, m: ops.convT3s2_route(cpad(c.Co), cpad(c.Ci), m) == route


def _c4s2(grouped):  # ops.conv4s2_dgrad_grouped: likewise
    return lambda ops, c, m: ops.conv4s2_dgrad_grouped(c.N, c.Ho, c.Wo, cpad(c.Co), cpad(c.Ci), m) == grouped


def _c4_dgrad(ops, c, m):
    return ops.c4_dgrad_reflect_ok(torch.empty((c.N, c.H, c.W, 4), device="meta"), cpad(c.Ci), c.R, c.ph, m)


def _refl_in(ops, c, m):
    return ops.dgrad_refl_epi_ok(c.N, c.H, c.W, cpad(c.Co), cpad(c.Ci), m)


def _fwd_in_stats(ops, c, m):  # the epilogue emits the IN partials: a split-bf16 tile and whole 32-pixel groups
    return m != "fp32" and 0 <= _plan_fwd(ops, c, m)[0] <= 9 and (c.Ho * c.Wo) % 32 == 0


def _tap64(ops, c, m):
    return _tap64_ok(ops, c, m)


_FWD_EPI = ("bias", "relu", "bias+relu", "lrelu", "bias+lrelu")
_HEAD = Conv(2, 32, 9, 10, 1, 4, 4, 1, 1, 1, "zero")
_TAP = Conv(2, 32, 9, 12, 3, 3, 3, 1, 1, 1, "reflect")
_TAP7 = Conv(1, 16, 9, 12, 3, 7, 7, 1, 3, 3, "reflect")
_TAPD = Conv(2, 3, 9, 12, 32, 3, 3, 1, 1, 1, "reflect")     # <= 4 input channels: the tap data gradients
_TAPW = Conv(3, 32, 9, 60, 3, 3, 3, 1, 1, 1, "reflect")     # the k x 1 and swapped weight-gradient forms
_CT = Conv(2, 24, 12, 14, 32, 3, 3, 2, 1, 1, "zero")         # ConvTranspose 32 -> 24 onto 12 x 14
_C4S2 = Conv(1, 64, 126, 126, 32, 4, 4, 2, 1, 1, "zero")     # 4096 rows per phase: the grouped launch's minimum
ROUTES += [
    Route("fwd_tail_splitk", "fwd", run_fwd, Conv(1, 64, 257, 256, 72, 1, 1, 1, 0, 0, "zero"), _fwd_tail, ("bf16x6",),
          slabs=lambda ops, c, m: _tail(ops, c, m), epi=("bias+relu",)),
    Route("fwd_in_stats", "fwd", run_fwd_in, Conv(2, 32, 8, 12, 40, 3, 3, 1, 1, 1, "reflect"), _fwd_in_stats, SPLIT,
          epi=("bias",), tier_b=Conv(2, 8, 8, 12, 40, 3, 3, 1, 1, 1, "reflect")),
    Route("fwd_skinny_split", "fwd", run_fwd, Conv(1, 256, 4, 4, 3, 4, 4, 1, 1, 1, "zero"), _skinny_split, ("bf16x6",),
          f32_always=True, epi=("bias+lrelu",)),
    Route("fwd_tap64_direct", "fwd", run_tap_fwd_h, Conv(1, 64, 4, 256, 3, 7, 7, 1, 3, 3, "reflect"), _tap64, ("bf16x6",),
          epi=("bias",)),
    # the direct kernel's three-product branch: every 16th one-hot set (the bf16x6 row above has them all)
    Route("fwd_tap64_direct_x3", "fwd", run_tap_fwd_h, Conv(1, 64, 4, 256, 3, 7, 7, 1, 3, 3, "reflect"), _tap64,
          ("bf16x3",), epi=("bias",), a_stride=16),
    Route("fwd_head_tap", "fwd", run_fwd_head, _HEAD, _head_fwd, f32_always=True, tier_b=_HEAD),
    Route("fwd_tap", "fwd", run_tap_fwd, _TAP, _tap_1x1, epi=("bias", "relu", "bias+lrelu")),
    Route("fwd_tap_c7", "fwd", run_tap_fwd, _TAP7, _tap_1x1, epi=("bias",)),
    Route("fwd_tap_h", "fwd", run_tap_fwd_h, _TAP, _tap_h,
          epi=("bias", "relu", "bias+lrelu")),
    Route("fwd_tap_h_c7", "fwd", run_tap_fwd_h, _TAP7, _tap_h, epi=("bias",)),
    Route("convT3s2_grouped", "dgrad", run_convT3, _CT, _convT3("grouped"), SPLIT, epi=("bias", "relu", "bias+relu")),
    Route("convT3s2_phase", "dgrad", run_convT3, _CT, _convT3("phase"), SPLIT, flags={"CONVT_GROUPED": False},
          epi=("bias", "relu", "bias+relu")),
    Route("convT3s2_phase_c24", "dgrad", run_convT3, Conv(2, 24, 12, 14, 24, 3, 3, 2, 1, 1, "zero"), _convT3("phase"), SPLIT,
          epi=("bias",), tier_b=Conv(2, 24, 12, 14, 8, 3, 3, 2, 1, 1, "zero")),
    Route("convT3s2_images", "dgrad", run_convT3, _CT, _convT3("images"), flags={"CONVT_DIRECT": False}, epi=("bias",)),
    Route("conv4s2_dgrad_grouped", "dgrad", run_conv4s2_dgrad, _C4S2, _c4s2(True), SPLIT, epi=()),
    Route("conv4s2_dgrad_phases", "dgrad", run_conv4s2_dgrad, Conv(2, 24, 12, 14, 32, 4, 4, 2, 1, 1, "zero"), _c4s2(False),
          epi=("bias", "bias+relu")),
    Route("tfwd_head", "dgrad", run_tfwd_head, _HEAD, _head_ok, f32_always=True, tier_b=_HEAD),
    Route("dgrad_tap", "dgrad", run_tap_dgrad, _TAPD, _tap_1x1, epi=()),
    Route("dgrad_tap_h", "dgrad", run_tap_dgrad_h, _TAPD, _tap_h, epi=()),
    Route("dgrad_c4_reflect", "dgrad", run_c4_dgrad_reflect, Conv(1, 64, 16, 32, 3, 7, 7, 1, 3, 3, "reflect"), _c4_dgrad,
          SPLIT, epi=(), x3_sums=False),  # vst_c4_dgrad_frame adds the mirrored border terms as fp32 VALU products
    Route("dgrad_refl_in", "dgrad", _run_dgrad_refl_in(False), Conv(1, 32, 8, 8, 64, 3, 3, 1, 1, 1, "reflect"), _refl_in,
          ("bf16x6",)),
    Route("dgrad_refl_in_apre", "dgrad", _run_dgrad_refl_in(True), Conv(1, 32, 8, 8, 64, 3, 3, 1, 1, 1, "reflect"), _refl_in,
          ("bf16x6",)),
    Route("wgrad_plain_head", "wgrad", run_wgrad, _HEAD, lambda ops, c, m: _head_ok(ops, c, m) and
          _wg("WG_PLAIN")(ops, c, m), f32_always=True, all_pixels=True, tier_b=_HEAD),
    Route("wgrad_plain_image", "wgrad", run_wgrad, Conv(2, 3, 12, 14, 16, 4, 4, 2, 1, 1, "zero"),
          lambda ops, c, m: _img_wgrad(ops, c, m) and _wg("WG_PLAIN")(ops, c, m), f32_always=True),
    # the tap forms run their own GEMMs (a 1x1, a k x 1 frame, a swapped one): all_pixels
    Route("wgrad_tap", "wgrad", run_tap_wgrad, _TAP, _tap_wgrad_ok("plain"), all_pixels=True),
    Route("wgrad_tap_planes", "wgrad", run_tap_wgrad, Conv(2, 32, 9, 16, 3, 3, 3, 1, 1, 1, "reflect"),
          _tap_wgrad_ok("bf"), ("bf16x6",), all_pixels=True),
    Route("wgrad_tap_h", "wgrad", run_tap_wgrad_h, _TAPW, _tap_wgrad_ok("h"), ("bf16x6",), all_pixels=True),
    Route("wgrad_tap_swap", "wgrad", run_tap_wgrad_swap, _TAPW, _tap_wgrad_ok("swap"), ("bf16x6",), all_pixels=True),
]
_N128 = Conv(1, 64, 16, 32, 72, 3, 3, 1, 1, 1, "reflect")   # Mw = 576: the 128x128 plan, two chunks
_N256 = Conv(1, 32, 32, 64, 72, 4, 4, 2, 1, 1, "zero")      # Mw = 512: the 256x128 plan, two chunks
X6 = ("bf16x6",)
ROUTES += [
    Route("wgrad_nhwc_planes_128x128", "wgrad", run_wgrad_planes, _N128, _wg_tile(_wg_nhwc(True), 0), X6, slabs=_wg_slabs),
    Route("wgrad_nhwc_planes_256x128", "wgrad", run_wgrad_planes, _N256, _wg_tile(_wg_nhwc(True), 7), X6, slabs=_wg_slabs),
    Route("wgrad_nhwc_f32_128x128", "wgrad", run_wgrad, _N128, _wg_tile(_wg_nhwc(False), 0), X6, slabs=_wg_slabs),
    Route("wgrad_nhwc_f32_256x128", "wgrad", run_wgrad, _N256, _wg_tile(_wg_nhwc(False), 7), X6, slabs=_wg_slabs),
    Route("wgrad_nhwc_f32_im2col", "wgrad", run_wgrad, Conv(2, 64, 8, 8, 72, 3, 3, 1, 1, 1, "reflect"),
          _wg_nhwc(False, im2col=True), X6, slabs=_wg_slabs),
    Route("wgrad_nhwc_f32_im2col_s2", "wgrad", run_wgrad, Conv(2, 32, 16, 16, 72, 4, 4, 2, 1, 1, "zero"),
          _wg_nhwc(False, im2col=True), X6, slabs=_wg_slabs),
    Route("wgrad_images_no_im2col", "wgrad", run_wgrad, Conv(2, 64, 8, 8, 72, 3, 3, 1, 1, 1, "reflect"),
          _wg("WG_IMAGES", "VST_WPLAN_BF"), X6, slabs=_wg_slabs, flags={"WGRAD_IM2COL": False}),
]
ROUTE_BY_NAME = {r.name: r for r in ROUTES}


class route_setup:
    """Context: the row's tile override and module flags set for the calling thread, restored on exit."""

    def __init__(self, ops, route):
        self.ops, self.route = ops, route

    def __enter__(self):
        self.prev = {k: getattr(self.ops, k) for k in self.route.flags}
        for k, v in self.route.flags.items():
            setattr(self.ops, k, v)
        self.ops.debug_set_tiles(*self.route.tiles)
        return self

    def __exit__(self, *exc):
        self.ops.debug_set_tiles(-1, -1, -1)
        for k, v in self.prev.items():
            setattr(self.ops, k, v)
        return False


def route_c(ops, route, case, m):
    """c of the tier-B bound for this row (c_bound with the row's K, accumulation depth and slab count)."""
    # the K the kernel walks: channels padded to the layout's multiple of 4 (the pad lanes add exact zeros)
    K = case.P if route.kind == "wgrad" else case.R * case.S * cpad(case.Ci if route.kind == "fwd" else case.Co)
    slabs = route.slabs(ops, case, m) if route.slabs else 1
    return c_bound(m, K, slabs, route.mfma_k, route.f32_always)


# ================================================================================ tier A probes
def _epi_vals(c, kind, seed):
    n = c.Co if kind == "fwd" else c.Ci
    return masked_full((n,), seed + 11, 6)


def probes(route, chunk=None, case=None):
    """Every tier-A launch of a row: dicts with the operands (a, b), the non-zero positions per output channel
    (taps), a label and, for the epilogue probes, the epilogue's arguments (adaptor keywords)."""
    kind, c = route.kind, case or route.case
    for f, family in enumerate(FAMILIES):
        hot = 4 if family == "fewhot" else 1
        va, vb = family_values(family, kind, c, 100 + 10 * f)
        if kind == "wgrad":
            sets, covered, P = dy_pixel_sets(c, chunk, all_pixels=route.all_pixels)
            if family == "a_full":
                sets = sets[::route.a_stride]
            if family != "a_full" and len(sets) > 32:  # every pixel set carries the full-significand x; the
                sets = sets[::-(-len(sets) // 32)]      # other families take at most 32 of them, evenly spread
            if hot > 1:
                sets = [torch.cat([(s + i * (P // 4)) % P for i in range(4)], 1) for s in sets[:-(-len(sets) // 4)]]
            for j, pix in enumerate(sets):
                yield dict(what=f"{family}[{j}]", a=va, b=onehot_dy(c, j, vb, hot, pix), taps=pix, epi={}, sums=hot > 1)
        else:
            n = n_sets(kind, c)
            js = list(range(-(-n // 4) if hot > 1 else n))
            if family == "a_full":
                js = js[::route.a_stride]
            if family != "a_full" and len(js) > 32:     # as above: no tap is left out by the first family
                js = js[::-(-len(js) // 32)]
            for j in js:
                jj = j if hot == 1 else 4 * j
                yield dict(what=f"{family}[{j}]", a=va, b=onehot_w(kind, c, jj, vb, hot), taps=hot_taps(kind, c, jj, hot),
                           epi={}, sums=hot > 1)
    # epilogues, exact by construction, on the first one-hot set of the full-significand family
    va, vb = family_values("a_full", kind, c, 100)
    names = route.epi
    if names is None:
        names = {"fwd": _FWD_EPI if c.R == c.S and c.ph == c.pw else _FWD_EPI[:3], "dgrad": ("addend",), "wgrad": ()}[kind]
    if kind != "wgrad":
        b = onehot_w(kind, c, 0, vb)
        bias = _epi_vals(c, kind, 1)
        sx, _ = operand_shapes("fwd", c)
        for name in names:
            epi = {}
            if "bias" in name:
                epi["bias"] = bias
            if "lrelu" in name:
                epi.update(act="lrelu", slope=0.2)
            elif "relu" in name:
                epi["act"] = "relu"
            if name == "addend":
                epi["addend"] = masked_full(sx, 77, 12)
            yield dict(what="epilogue " + name, a=va, b=b, taps=hot_taps(kind, c, 0), epi=epi)
    else:
        yield dict(what="accumulate onto 0", a=va, b=onehot_dy(c, 0, vb), taps=hot_pixels(c, 0),
                   epi=dict(prefill=torch.zeros(c.Co, c.Ci, c.R, c.S)))
        # accumulate told from overwrite, still exact: few-hot values (multiples of 2^-18, |sum| < 2^5) onto +-2^k,
        # |k| <= 3, so the pre-fill may join the sum at any point (the accumulator, a slab, the final add)
        fa, fb = family_values("fewhot", kind, c, 130)
        yield dict(what="accumulate onto powers of two", a=fa, b=onehot_dy(c, 0, fb, 4), taps=hot_pixels(c, 0, 4),
                   epi=dict(prefill=pow2((c.Co, c.Ci, c.R, c.S), 55, 3)), sums=True)
