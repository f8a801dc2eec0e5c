"""Every reduction geometry of the InstanceNorm kernels (csrc/norm.hip) and of the scalar losses
(csrc/loss.hip, csrc/style.hip) against the fp64 references of tests/reduction_ref.py.

What is checked at op level here and nowhere else: every slice of a split reduction is visited, every
chain of the unrolled folds is added, and the tail of a slice is neither skipped nor read twice.  The
InstanceNorm shapes come from reduction_ref.IN_CASES; tests/test_reduction_ref_host.py proves on the
host that each of them reaches the branch it is listed for.  Comparisons are per (n, c) plane or per
channel, never against one global maximum: a wrong channel group must not hide behind a larger one.

Tolerances are derived from the number formats (u = 2^-24 is fp32's unit roundoff; the kernels
accumulate in fp64) or are the ones the older op tests already use, applied per plane; each is
stated where it is used.  Every check prints its worst error / bound ratio before it asserts.
"""
import functools
import itertools

import pytest
import torch

import reduction_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
U = 2.0 ** -24
EPS = R.f32(1e-5)      # what the C ABI receives for the Python numbers the wrappers pass
SLOPE = R.f32(0.2)
ACTS = ["none", "relu", "lrelu"]
VARIANT_CASES = ["tail_cpb4", "part_unrolled_6", "lp18"]


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    return o


def _randn(seed, shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _le(err, tol, what):
    """assert err <= tol everywhere (a NaN fails), after printing the worst ratio."""
    err, tol = torch.as_tensor(err, dtype=F64), torch.as_tensor(tol, dtype=F64)
    tol = tol.expand_as(err)
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(F64))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{what}: worst err/bound = {worst:.3g} (max err {err.max().item():.3e})")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst err/bound {worst:.3g}"


def _pmax(t):
    """max |t| per (n, c) plane of an NCHW tensor."""
    return t.abs().amax(dim=(2, 3))


# ======================================================================== plain InstanceNorm
@functools.lru_cache(maxsize=2)
def _in_data(case, variant):
    """fp32 NHWC inputs of a case (x, upstream gradient, residual) and their fp64 reference stats."""
    N, H, W, C = R.IN_CASE[case][1]
    seed = 1000 + 10 * [c[0] for c in R.IN_CASES].index(case)
    x = _randn(seed, (N, H, W, C))
    if variant == "offset":      # per-channel means spread over +-100 at std 0.1: |mean| / std = 1e3
        x = torch.linspace(-100, 100, C) + 0.1 * x
    elif variant == "scales":    # per-channel std from 1e-3 to 1e3
        x = torch.logspace(-3, 3, C) * x
    else:
        x = 2.0 * x + 0.5
        if variant == "const":   # one channel of every image is constant
            x[..., C // 2] = 0.75
    g, res = _randn(seed + 1, (N, H, W, C)), _randn(seed + 2, (N, H, W, C))
    x64 = R.nchw64(x)
    mean, rstd = R.in_stats(x64, EPS)
    return x, g, res, mean, rstd


def _check_plain_in(ops, case, variant, act, db_accumulate=True):
    x, g, res, mean, rstd = _in_data(case, variant)
    N, H, W, C = x.shape
    x64, g64 = R.nchw64(x), R.nchw64(g)
    res64 = R.nchw64(res) if act == "none" else None
    xd, gd = x.to(DEV), g.to(DEV)
    tag = f"{case}/{variant}/{act}"

    # ---- stats: one fp32 rounding of an fp64 result (fp64 cancellation <= 1e-10 at |mean|/std <= 1e3)
    st = ops.instnorm_stats(xd)
    st_c = st.cpu()
    m32, r32 = st_c[..., 0], st_c[..., 1]
    mref, rref = mean[:, :, 0, 0], rstd[:, :, 0, 0]
    _le((m32.to(F64) - mref).abs(), 2 * U * mref.abs() + 1e-12 * x64.abs().mean(dim=(2, 3)), tag + " mean")
    _le((r32.to(F64) - rref).abs(), 4 * U * rref, tag + " rstd")
    if variant == "const":
        c = C // 2
        assert (m32[:, c] == 0.75).all() and (r32[:, c] == (1.0 / torch.tensor(EPS, dtype=F64).sqrt()).float()).all()

    # ---- the sign decisions of relu / lrelu, bit-identical to the device's: fp32 subtract then multiply
    # (a subtract feeding a multiply cannot be contracted) on the device's own stats.  An fp64 reference
    # may decide differently where x_hat is within rounding of 0, and one flip moves a whole small plane.
    mask = None
    if act != "none":
        xn = x.permute(0, 3, 1, 2)
        mask = (xn - m32[:, :, None, None]) * r32[:, :, None, None] > 0

    # ---- forward: the stored fp32 mean and rstd, one subtract, one multiply (, one multiply by the
    # slope), one add: |y - ref| <= 2^-22 (|mean| rstd + |x_hat| + |res| + |ref|)
    y = ops.instnorm_act_fwd(xd, st, act, 0.2, residual=res.to(DEV) if act == "none" else None)
    ref = R.in_fwd(x64, mean, rstd, act, SLOPE, res64, mask)
    xh = (x64 - mean) * rstd
    bound = 4 * U * (mean.abs() * rstd + xh.abs() + (res64.abs() if res64 is not None else 0) + ref.abs())
    _le((R.nchw64(y) - ref).abs(), bound, tag + " fwd")
    if variant == "const":
        got = R.nchw64(y)[:, C // 2]
        assert (got == (res64[:, C // 2] if res64 is not None else 0)).all()   # x_hat == 0 exactly

    # ---- backward: 1e-5 of the plane's max |ref| (test_instnorm_act's tolerance, per plane)
    init = 0.5 if db_accumulate else float("nan")
    db = torch.full((C,), init, device=DEV)
    dx = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, db=db, accumulate_db=db_accumulate)
    dref, dbref = R.in_bwd(g64, x64, mean, rstd, act, SLOPE, mask)
    tol = 1e-5 * _pmax(dref)
    if variant == "offset":
        # the stored mean is off by up to u |mean|, so x_hat by u |mean| rstd, and that error is multiplied
        # by rstd * mean(g x_hat) in dx: unavoidable with fp32 stats, 4 u |mean| rstd^2 |mean(g x_hat)|
        gz = g64 * R.act_grad(xh, act, SLOPE, mask)
        tol = tol + 4 * U * (mean.abs() * rstd ** 2 * (gz * xh).mean(dim=(2, 3), keepdim=True).abs())[:, :, 0, 0]
    dgot = R.nchw64(dx)
    assert torch.isfinite(dgot).all()
    _le(_pmax(dgot - dref), tol, tag + " dx")
    # conv-bias gradient = per-channel sum of dx (0 in exact arithmetic), test_instnorm_act's form
    dbc = db.cpu().to(F64)
    assert torch.isfinite(dbc).all()
    _le((dbc - (0.5 if db_accumulate else 0.0) - dbref).abs(), 1e-5 * dref.abs().sum(dim=(0, 2, 3)), tag + " db")


IN_BASE = [(c[0], a) for c in R.IN_CASES for a in ACTS]


@pytest.mark.parametrize("case,act", IN_BASE, ids=["-".join(p) for p in IN_BASE])
def test_instnorm_geometry(ops, case, act):
    _check_plain_in(ops, case, "base", act)


IN_VARIANTS = [(c, v, a) for c in VARIANT_CASES for v in ("offset", "scales", "const") for a in ACTS]


@pytest.mark.parametrize("case,variant,act", IN_VARIANTS, ids=["-".join(p) for p in IN_VARIANTS])
def test_instnorm_data_variants(ops, case, variant, act):
    _check_plain_in(ops, case, variant, act)


@pytest.mark.parametrize("case", VARIANT_CASES)
def test_instnorm_db_overwrite(ops, case):
    """accumulate_db=False writes db: a NaN-filled buffer comes back finite and right."""
    _check_plain_in(ops, case, "base", "lrelu", db_accumulate=False)


@pytest.mark.parametrize("C", [1028, 6])
def test_instnorm_unsupported_width_raises(ops, C):
    with pytest.raises(RuntimeError):
        ops.instnorm_stats(torch.zeros((1, 2, 2, C), device=DEV))


def test_instnorm_bwd_fewer_elements_than_channels(ops):
    """N = 1, HW = 2, C = 64: the apply pass has too few threads to also reduce db, which is refused;
    without db the backward runs and matches."""
    x, g = 2.0 * _randn(7, (1, 1, 2, 64)) + 0.5, _randn(8, (1, 1, 2, 64))
    xd, gd = x.to(DEV), g.to(DEV)
    st = ops.instnorm_stats(xd)
    with pytest.raises(RuntimeError, match="fewer elements than channels"):
        ops.instnorm_act_bwd(gd, xd, st, "none", 0.0, db=torch.zeros(64, device=DEV))
    dx = ops.instnorm_act_bwd(gd, xd, st, "none", 0.0)
    x64 = R.nchw64(x)
    mean, rstd = R.in_stats(x64, EPS)
    g64 = R.nchw64(g)
    dref, _ = R.in_bwd(g64, x64, mean, rstd, "none", 0.0)
    # With two pixels x_hat = +-a, a^2 = var / (var + eps), and dx = +-rstd (g - mean g)(1 - a^2): the three
    # terms of rstd (g - mean g - x_hat mean(g x_hat)) cancel to ~eps / var of their size, so the bound is
    # on the terms, not on the result: each carries a few fp32 roundings (8 u covers them), x_hat also the
    # stored mean's u |mean| rstd.
    xh = (x64 - mean) * rstd
    mg, mgx = g64.mean(dim=(2, 3), keepdim=True), (g64 * xh).mean(dim=(2, 3), keepdim=True)
    bound = 8 * U * rstd * (g64.abs() + mg.abs() + (xh.abs() + mean.abs() * rstd) * mgx.abs())
    _le((R.nchw64(dx) - dref).abs(), bound, "HW=2 dx")


# ======================================================================= affine InstanceNorm
# seeds for which the reference's pre-activation z keeps clear of 0 (asserted below)
AFFINE_SEEDS = {"tail_cpb4": 6830, "fold4_unrolled": 63160, "c1024_pg1": 17140, "lp3": 100, "lp18": 100,
                "lp34_cpb4": 3660, "tiny_hw": 100}
# The geometries whose rows reach the 4x unrolled loop of the partial walk (with a remainder and a ragged last
# slice) run without an activation: at 2.8 M elements no seed keeps |z| clear of 0, and the walk does not depend
# on the activation.  The gated option takes the four-sum partial (sum gy*a) through the unrolled rows.
AFFINE_UNROLLED = ("part_unrolled_6", "c1024_unrolled")
AFFINE_SEEDS.update({c: 100 for c in AFFINE_UNROLLED})
# act, gate, residual, accumulate
AFFINE_OPTS = [("none", None, False, True), ("relu", 0.7, True, False), ("lrelu", -0.4, True, True),
               ("lrelu", None, False, False), ("none", 0.7, True, False)]
GATE_MULT = 0.9


@functools.lru_cache(maxsize=2)
def _affine_data(case, seed):
    N, H, W, C = R.IN_CASE[case][1]
    x = 2.0 * _randn(seed, (N, H, W, C)) + 0.5
    gamma, beta = 1.0 + _randn(seed + 1, (C,), 0.2), _randn(seed + 2, (C,), 0.2)
    g, res = _randn(seed + 3, (N, H, W, C)), _randn(seed + 4, (N, H, W, C))
    mean, rstd = R.in_stats(R.nchw64(x), EPS)
    return x, gamma, beta, g, res, mean, rstd


def _affine_z_margin(case, seed):
    """min |z| / max |z| of the reference's pre-activation over the whole tensor."""
    x, gamma, beta, _, _, mean, rstd = _affine_data(case, seed)
    z = (R.nchw64(x) - mean) * rstd * gamma.to(F64).view(1, -1, 1, 1) + beta.to(F64).view(1, -1, 1, 1)
    return (z.abs().min() / z.abs().max()).item()


AFFINE = [(c, i) for c in AFFINE_SEEDS for i in ((0, 4) if c in AFFINE_UNROLLED else range(4))]


@pytest.mark.parametrize("case,opt", AFFINE, ids=[f"{c}-{'-'.join(map(str, AFFINE_OPTS[i]))}" for c, i in AFFINE])
def test_instnorm_affine_geometry(ops, case, opt):
    act, gate, with_res, accumulate = AFFINE_OPTS[opt]
    x, gamma, beta, g, res, mean, rstd = _affine_data(case, AFFINE_SEEDS[case])
    N, H, W, C = x.shape
    tag = f"{case}/{act}/gate={gate}"
    if act != "none":
        # z = x * alpha + beta' may be contracted to an fma on the device, so its sign decisions cannot be
        # replicated; instead the inputs keep |z| clear of 0 (the device's z is within ~1e-7 max|z|)
        assert _affine_z_margin(case, AFFINE_SEEDS[case]) >= 1e-6
    x64, g64, gam64, bet64 = R.nchw64(x), R.nchw64(g), gamma.to(F64), beta.to(F64)
    res64 = R.nchw64(res) if with_res else None
    xd, gd, gamd, betd = x.to(DEV), g.to(DEV), gamma.to(DEV), beta.to(DEV)
    kw = {}
    gate32 = None
    if gate is not None:
        gate32 = R.f32(gate)
        kw = dict(gate=torch.tensor([gate], device=DEV), gate_mult=GATE_MULT)
    st = ops.instnorm_stats(xd)

    # forward: 1e-5 of max |ref| (test_instnorm_affine_fwd_bwd's), per plane
    y = ops.instnorm_affine_fwd(xd, st, gamd, betd, act, residual=res.to(DEV) if with_res else None, slope=0.2, **kw)
    ref = R.in_affine_fwd(x64, mean, rstd, gam64, bet64, act, SLOPE, gate32, R.f32(GATE_MULT), res64)
    _le(_pmax(R.nchw64(y) - ref), 1e-5 * _pmax(ref), tag + " fwd")

    init = 0.25 if accumulate else float("nan")
    bufs = {k: torch.full((1 if k == "dgate" else C,), init, device=DEV) for k in ("dgamma", "dbeta", "dgate", "dbias")}
    if gate is None:
        del bufs["dgate"]
    dx = ops.instnorm_affine_bwd(gd, xd, st, gamd, betd, act, accumulate=accumulate, slope=0.2, **bufs, **kw)
    r = R.in_affine_bwd(g64, x64, mean, rstd, gam64, bet64, act, SLOPE, gate32, R.f32(GATE_MULT))
    # dx: 1e-4 of max |ref| (the older test's), per plane
    dgot = R.nchw64(dx)
    assert torch.isfinite(dgot).all()
    _le(_pmax(dgot - r["dx"]), 1e-4 * _pmax(r["dx"]), tag + " dx")
    base = 0.25 if accumulate else 0.0
    for k in bufs:
        got = bufs[k].cpu().to(F64) - base
        assert torch.isfinite(got).all(), k
        want = r[k].reshape(got.shape)
        if k == "dbias":   # 0 in exact arithmetic; against the reference's fp64 sum, test_instnorm_act's form
            tol = 1e-5 * r["dx"].abs().sum(dim=(0, 2, 3))
        else:
            # 1e-4 relative, per channel.  A signed sum can cancel far below its terms, and no fp32 evaluation
            # of the terms (<= 8 roundings each, summed in fp64) can do better than 8 u sum|term|, so that
            # floor is added; accumulating onto the preset value rounds once more.
            tol = 1e-4 * want.abs() + 8 * U * r[k + "_abs"].reshape(got.shape) + 2 * U * (base + want.abs())
        _le((got - want).abs(), tol, f"{tag} {k}")


# ======================================================================== running statistics
@pytest.mark.parametrize("C,N,hw", itertools.product([12, 300], [1, 3], [(1, 2), (7, 9)]))
def test_instnorm_running_stats(ops, C, N, hw):
    H, W = hw
    HW, mom = H * W, R.f32(0.1)
    x = _randn(C + N + HW, (N, H, W, C)) + 5.0       # means well away from 0: no cancellation in running_mean
    rm0 = 1.0 + torch.rand(C, generator=torch.Generator().manual_seed(3))
    rv0 = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(4))
    st = ops.instnorm_stats(x.to(DEV))
    rm, rv = rm0.to(DEV, copy=True), rv0.to(DEV, copy=True)
    ops.instnorm_running_update(st, rm, rv, HW, momentum=0.1)
    mean, rstd = R.in_stats(R.nchw64(x), EPS)
    var = (1.0 / rstd ** 2 - EPS)[:, :, 0, 0]
    rm_ref, rv_ref = R.running_update(mean[:, :, 0, 0], var, rm0.to(F64), rv0.to(F64), HW, mom)
    # the stored fp32 mean, then one rounding of the result
    _le((rm.cpu().to(F64) - rm_ref).abs(), 4 * U * rm_ref.abs(), "running_mean")
    # var is recovered from an fp32 rstd: 1/rstd^2 carries 2 u (var + eps), doubled for the device's own
    # stats rounding; then one rounding of the result
    unb = HW / (HW - 1.0)
    _le((rv.cpu().to(F64) - rv_ref).abs(), 4 * U * (var + EPS).mean(dim=0) * mom * unb + 2 * U * rv_ref.abs(),
        "running_var")
    # eval mode: every n gets {running_mean, 1 / sqrt(running_var + eps)}
    st2 = ops.instnorm_stats_from_running(rm, rv, N).cpu()
    assert st2.shape == (N, C, 2) and (st2 == st2[0:1]).all()
    assert (st2[0, :, 0] == rm.cpu()).all()
    rref = 1.0 / torch.sqrt(rv.cpu().to(F64) + EPS)
    _le((st2[0, :, 1].to(F64) - rref).abs(), 4 * U * rref, "stats_from_running rstd")


# ============================================================================= scalar losses
GOUT = R.f32(-0.37)
SCALE = 2.5
NPIX = [1, 255, 257, 65537, 3 * 65536 + 5]     # the last two: 257 and 769 partials for the finish kernels
CSCL = [(4, 3), (4, 1), (4, 4), (8, 5)]


def _loss_inputs(npix, cs, cl, seed=0):
    """a, b [1, 1, npix, cs] with junk in the padding channels and some exactly equal entries; a mask
    [1, 1, 1, npix] with exact zeros."""
    a, b = _randn(seed + 1, (1, 1, npix, cs)), _randn(seed + 2, (1, 1, npix, cs))
    a[..., cl:], b[..., cl:] = 777.0, -555.0
    b[0, 0, ::7, 0] = a[0, 0, ::7, 0]
    u = torch.rand(1, 1, 1, npix, generator=torch.Generator().manual_seed(seed + 3))
    mask = torch.where(u > 0.3, 0.25 + 0.75 * u, torch.zeros_like(u))
    return a, b, mask


def _check_loss(tag, cl, loss, grad, ref_pair, zero_at=None):
    ref, gref = ref_pair
    # non-negative summands: cl fp32 adds per thread, 6 wave-reduce levels, 4 block adds, then fp64
    _le(abs(loss.item() - ref.item()), (cl + 16) * 2 * U * abs(ref.item()), tag + " value")
    # elementwise, <= 4 roundings
    got = R.nchw64(grad)
    _le((got - gref).abs(), 8 * U * gref.abs(), tag + " grad")
    assert (got[:, cl:] == 0).all()
    if zero_at is not None:
        assert zero_at.any() and (got[:, :cl][zero_at.expand_as(got[:, :cl])] == 0).all()


LOSS = list(itertools.product(NPIX, CSCL))


@pytest.mark.parametrize("npix,cscl", LOSS, ids=[f"{n}px-cs{c[0]}cl{c[1]}" for n, c in LOSS])
def test_scalar_losses(ops, npix, cscl):
    cs, cl = cscl
    a, b, mask = _loss_inputs(npix, cs, cl)
    ad, bd, md = a.to(DEV), b.to(DEV), mask.to(DEV)
    gout = torch.tensor(GOUT, device=DEV)
    a64, b64, m64 = R.nchw64(a), R.nchw64(b), mask.to(F64)
    eq = (a64[:, :cl] == b64[:, :cl])
    tag = f"{npix}px cs{cs} cl{cl} "
    _check_loss(tag + "l1", cl, ops.loss_l1(ad, bd, SCALE, cl), ops.loss_l1_bwd(ad, bd, gout, SCALE, cl),
                R.l1(a64, b64, cl, SCALE, GOUT), zero_at=eq)
    t = 0.9
    _check_loss(tag + "mse_const", cl, ops.loss_mse_const(ad, t, SCALE, cl),
                ops.loss_mse_const_bwd(ad, t, gout, SCALE, cl), R.mse_const(a64, R.f32(t), cl, SCALE, GOUT))
    _check_loss(tag + "masked_l1(None)", cl, ops.loss_masked_l1(ad, bd, None, SCALE, cl),
                ops.loss_masked_l1_bwd(ad, bd, None, gout, SCALE, cl), R.masked_l1(a64, b64, None, cl, SCALE, GOUT),
                zero_at=eq)
    _check_loss(tag + "masked_l1", cl, ops.loss_masked_l1(ad, bd, md, SCALE, cl),
                ops.loss_masked_l1_bwd(ad, bd, md, gout, SCALE, cl), R.masked_l1(a64, b64, m64, cl, SCALE, GOUT),
                zero_at=(m64 == 0) if (m64 == 0).any() else None)
    _check_loss(tag + "mse", cl, ops.loss_mse(ad, bd, SCALE, cl), ops.loss_mse_bwd(ad, bd, gout, SCALE, cl),
                R.mse(a64, b64, cl, SCALE, GOUT), zero_at=eq)


def test_loss_mse_wide_and_accumulating(ops):
    """(Cs, Cl) = (64, 64) through cl=None, out= with accumulate=True, and loss_mse_bwd(grad=...)."""
    npix, cs = 65537, 64
    a, b = _randn(21, (1, 1, npix, cs)), _randn(22, (1, 1, npix, cs))
    b[0, 0, ::7, 0] = a[0, 0, ::7, 0]
    ad, bd = a.to(DEV), b.to(DEV)
    gout = torch.tensor(GOUT, device=DEV)
    a64, b64 = R.nchw64(a), R.nchw64(b)
    ref, gref = R.mse(a64, b64, cs, SCALE, GOUT)
    _check_loss("mse 64/64", cs, ops.loss_mse(ad, bd, SCALE), ops.loss_mse_bwd(ad, bd, gout, SCALE), (ref, gref),
                zero_at=(a64 == b64))
    # onto a preset value: the loss's own bound plus one rounding of the sum
    out = torch.tensor(3.25, device=DEV)
    assert ops.loss_mse(ad, bd, SCALE, out=out, accumulate=True) is out
    _le(abs(out.item() - 3.25 - ref.item()), (cs + 16) * 2 * U * abs(ref.item()) + U * (3.25 + abs(ref.item())),
        "mse out= accumulate")
    # accumulate=False overwrites whatever out held
    out = torch.tensor(float("nan"), device=DEV)
    ops.loss_mse(ad, bd, SCALE, out=out)
    _le(abs(out.item() - ref.item()), (cs + 16) * 2 * U * abs(ref.item()), "mse out= overwrite")
    # onto a preset gradient: the gradient's own bound plus one rounding of the sum
    g0 = _randn(23, (1, 1, npix, cs))
    gd = g0.to(DEV, copy=True)
    assert ops.loss_mse_bwd(ad, bd, gout, SCALE, grad=gd) is gd
    want = R.nchw64(g0) + gref
    _le((R.nchw64(gd) - want).abs(), 8 * U * gref.abs() + U * want.abs(), "mse_bwd grad= accumulate")


def _tv_image(shape, flat, seed):
    """30 * randn rounded to multiples of 1/8: every difference is exact in fp32, so a flat patch gives
    r == 0 exactly on both sides; the padding channel holds junk."""
    N, H, W = shape
    img = torch.round(_randn(seed, (N, H, W, 4), 30.0) * 8) / 8
    if flat:
        img[0, 5:11, 4:10, :] = 2.5
    img[..., 3] = 123.0
    return img


TV = [((1, 2, 2), False), ((2, 17, 19), True), ((1, 258, 257), False)]   # the last: 65 792 terms, 257 partials


@pytest.mark.parametrize("cl", [3, 1])
@pytest.mark.parametrize("shape,flat", TV, ids=["2x2", "17x19-flat-patch", "258x257"])
def test_loss_tv(ops, shape, flat, cl):
    img = _tv_image(shape, flat, seed=31)
    if cl == 1:
        img[..., 1] = 55.0    # now junk too
    imd = img.to(DEV)
    i64 = R.nchw64(img)
    scale = 0.5
    ref = scale * R.tv(i64, cl)
    # 1e-5 relative (test_mse_tv_gram's)
    _le(abs(ops.loss_tv(imd, scale, cl).item() - ref.item()), 1e-5 * abs(ref.item()), "tv value")
    gref = scale * GOUT * R.tv_grad(i64, cl)
    got = R.nchw64(ops.loss_tv_bwd(imd, torch.tensor(GOUT, device=DEV), scale, cl))
    assert torch.isfinite(got).all() and (got[:, cl:] == 0).all()
    # 1e-5 of max |ref| (test_mse_tv_gram's)
    _le((got - gref).abs(), 1e-5 * gref.abs().max(), "tv grad")
    if flat:   # inside the patch every term a pixel takes part in has r == 0: exactly 0, not NaN
        assert (gref[0, :cl, 6:10, 5:9] == 0).all() and (got[0, :cl, 6:10, 5:9] == 0).all()


# ==================================================================================== axpby
@pytest.mark.parametrize("ab", [(1.0 / 480, 0.0), (0.5, -2.0)], ids=["scale-only", "general"])
@pytest.mark.parametrize("n", [1, 255, 1025])
def test_axpby(ops, n, ab):
    a, b = ab
    a32, b32 = R.f32(a), R.f32(b)
    x, y = _randn(41, (n,)), _randn(42, (n,))
    for alias in (False, True):   # ops.gram scales its result in place: x is y
        yd = y.to(DEV, copy=True)
        xd = yd if alias else x.to(DEV)
        xs = y if alias else x
        ops.axpby(xd, yd, a, b)
        got = yd.cpu()
        if b == 0:   # overwrites: exactly the fp32 product a * x
            assert (got == (xs.to(F64) * a32).float()).all()
        else:        # two products and a sum, fused or not: 2 u (|a x| + |b y|)
            want = a32 * xs.to(F64) + b32 * y.to(F64)
            _le((got.to(F64) - want).abs(), 2 * U * ((a32 * xs.to(F64)).abs() + (b32 * y.to(F64)).abs()), "axpby")
