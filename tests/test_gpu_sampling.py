"""Every sampling geometry of the kernels that gather or scatter at data-dependent positions, against the fp64
references of tests/sampling_ref.py: the flow warp (csrc/flow.hip warp_fwd_k: the CT = 1 / 16 / 32 and runtime
channel arms, several x-blocks and their tails, N = 3, H = 1, W = 1), its input gradient (atomic warp_bwd_k and the
deterministic csrc/flow_det.hip), the fused temporal loss (temporal_k), the forward/backward consistency mask
(fbcheck_k), the correlation pyramid and lookup (csrc/style.hip) and RAFT's convex upsampling (csrc/raft.hip).

The cases, the references and the comparison functions live in sampling_ref.py; tests/test_sampling_ref_host.py
proves on the host that stock fp32 torch passes each comparison used here and that each of a list of one-line
slips fails one.  Every bound is exact (bit-equal, exactly 0) or derived from a count of roundings in
sampling_ref.py; every check prints its worst error / bound ratio before it asserts, and the module prints the
worst ratio per kernel when it is done.
"""
import numpy as np
import pytest
import torch

import sampling_ref as S
from oracle import flow_ref
from sampling_ref import (BWD_CASES, DET_CASES, FWD_CASES, LOOKUP_CASES, PYRAMID_CASES, TEMPORAL_CASES, UPSAMPLE_CASES,
                          lookup_case, temporal_case)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


def _sid(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    prev = o.set_deterministic(False)
    yield o
    o.set_deterministic(prev)
    for k in sorted(S.WORST):
        print(f"WORST {k}: {S.WORST[k]:.3g} of the bound")


@pytest.fixture
def det(ops):
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(False)


# =================================================================================== warp forward
@pytest.mark.parametrize("shape,family", FWD_CASES, ids=[f"{_sid(s)}-{f}" for s, f in FWD_CASES])
def test_warp_fwd(ops, shape, family):
    x, flow = S.warp_source(*shape).to(DEV), S.make_flow(family, *shape[:3]).to(DEV)
    for align in (False, True):
        S.check_warp_fwd(ops.warp_nhwc(x, flow, align), S.warp_case(shape, family, align, False), "warp_fwd")
        S.check_warp_fwd(ops.warp_masked_nhwc(x, flow, align), S.warp_case(shape, family, align, True),
                         "warp_masked_fwd")


# =================================================================================== warp backward
@pytest.mark.parametrize("shape,family", BWD_CASES, ids=[f"{_sid(s)}-{f}" for s, f in BWD_CASES])
def test_warp_bwd(ops, shape, family):
    """The fp32-atomic scatter against fp64, per target element."""
    gout, flow = S.warp_gout(*shape).to(DEV), S.make_flow(family, *shape[:3]).to(DEV)
    for align, masked in ((False, False), (True, False), (False, True), (True, True)):
        bwd = ops.warp_masked_bwd_nhwc if masked else ops.warp_bwd_nhwc
        S.check_warp_bwd(bwd(gout, flow, align), S.warp_bwd_case(shape, family, align, masked),
                         "warp_masked_bwd" if masked else "warp_bwd")


@pytest.mark.parametrize("shape,family", DET_CASES, ids=[f"{_sid(s)}-{f}" for s, f in DET_CASES])
def test_warp_bwd_det(det, shape, family):
    """The deterministic path: bit-exact against the ordered oracle (C = 4, 8, 20: one partial channel group, one
    whole, two whole and a tail of 4), bit-identical run to run."""
    g, flow = S.warp_gout(*shape), S.make_flow(family, *shape[:3])
    gd, fd = g.to(DEV), flow.to(DEV)
    for align, masked in ((False, False), (True, False), (False, True)):
        bwd = det.warp_masked_bwd_nhwc if masked else det.warp_bwd_nhwc
        a, b = bwd(gd, fd, align), bwd(gd, fd, align)
        assert torch.equal(a, b)
        ref = flow_ref.warp_bwd_ordered(g.numpy(), flow.numpy(), align=align, masked=masked)
        np.testing.assert_array_equal(a.cpu().numpy(), ref)
        if family == "far":
            assert float(a.abs().max()) == 0.0


# =================================================================================== temporal loss
def _dev(c):
    return tuple(c[k].to(DEV) for k in ("a", "b", "flow", "mask")) + (torch.tensor([c["gout"]], device=DEV),)


@pytest.mark.parametrize("shape,cscl", TEMPORAL_CASES, ids=[f"{_sid(s)}-cs{c[0]}cl{c[1]}" for s, c in TEMPORAL_CASES])
def test_temporal(ops, shape, cscl):
    c = temporal_case(shape, cscl, "iid")
    a, b, flow, mask, gout = _dev(c)
    lam, cl, ref = c["lam"], c["cl"], c["ref"]
    indep = c["indep"]() if shape == (3, 5, 17) else None
    tag = f"temporal {_sid(shape)} cs{c['cs']} cl{cl}"
    loss = ops.loss_temporal(a, b, flow, mask, lam, cl)
    # both gradients into a zeroed ga and a NaN-filled gb
    ga, gb = torch.zeros_like(a), torch.full_like(b, float("nan"))
    ops.loss_temporal_bwd(a, b, flow, mask, gout, ga, gb, lam, cl)
    S.check_temporal(loss, ga, gb, ref, None, indep, "temporal")
    # each gradient alone
    gb1 = torch.full_like(b, float("nan"))
    ops.loss_temporal_bwd(a, b, flow, mask, gout, None, gb1, lam, cl)
    assert torch.equal(gb1, gb), tag + ": gb differs without ga"
    ga1 = torch.zeros_like(a)
    ops.loss_temporal_bwd(a, b, flow, mask, gout, ga1, None, lam, cl)
    S.check_temporal(None, ga1, None, ref, None, None, "temporal")
    # the kernel adds into ga: preset + gradient, pad channels of the preset untouched
    preset = S.rand(77, a.shape, 0.01)
    preset[..., cl:] = 321.0
    ga2 = preset.to(DEV)
    ops.loss_temporal_bwd(a, b, flow, mask, gout, ga2, None, lam, cl)
    pref = S.temporal_tight(c["a"], c["b"], c["flow"], c["mask"], lam, cl, c["gout"], preset)
    S.check_temporal(None, ga2, None, pref, preset, None, "temporal_preset")
    # the deterministic switch: gb unchanged, ga bit-exact against the ordered scatter of -gb
    ops.set_deterministic(True)
    try:
        ga3, gb3 = torch.zeros_like(a), torch.full_like(b, float("nan"))
        ops.loss_temporal_bwd(a, b, flow, mask, gout, ga3, gb3, lam, cl)
        ga4 = torch.zeros_like(a)
        ops.loss_temporal_bwd(a, b, flow, mask, gout, ga4, None, lam, cl)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(gb3, gb), tag + ": gb depends on the deterministic switch"
    want = flow_ref.warp_bwd_ordered(gb.cpu().numpy(), c["flow"].numpy(), cl=cl, negate=True)
    np.testing.assert_array_equal(ga3.cpu().numpy(), want)
    assert torch.equal(ga4, ga3)


def test_temporal_ident_flow(ops):
    """The flow that undoes the reference's W / (W - 1) shift: every sample lands on its own pixel (up to the
    rounding of the position, which the tight tier's weights carry), so on interior pixels ga == -gb within the
    gradient bounds plus what that rounding moves between neighbours."""
    shape, cscl = (2, 37, 53), (8, 5)
    c = temporal_case(shape, cscl, "ident")
    a, b, flow, mask, gout = _dev(c)
    cl, ref = c["cl"], c["ref"]
    ga, gb = torch.zeros_like(a), torch.full_like(b, float("nan"))
    ops.loss_temporal_bwd(a, b, flow, mask, gout, ga, gb, c["lam"], cl)
    S.check_temporal(ops.loss_temporal(a, b, flow, mask, c["lam"], cl), ga, gb, ref, None, None, "temporal_ident")
    # The position's rounding leaves the weights within 8 u (|p + f| + size) per axis of 0 or 1
    # (sampling_ref.position_error), which moves at most that share of a pixel's own gb and of each of its four
    # neighbours' into or out of its ga: 5 (dx + dy) max over the 3x3 neighbourhood of the reference's |gb|, taken
    # as 6 because a neighbour's position bound is its own, 8 u larger at most.
    dx, dy = S.position_error(c["flow"])
    nb = torch.nn.functional.max_pool2d(ref["gb"].abs().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    bound = ref["ga_bound"] + ref["gb_bound"] + 6 * (dx + dy)[..., None] * nb
    inner = (slice(None), slice(1, -1), slice(1, -1), slice(0, cl))
    g64 = gb.cpu().to(F64)
    S.le((ga.cpu().to(F64) + g64).abs()[inner], bound[inner], "temporal ident ga == -gb", "temporal/ident")


def test_temporal_far_flow(ops):
    """Every corner outside: loss = lambda mean((m b)^2), ga identically 0."""
    shape, cscl = (2, 37, 53), (4, 3)
    c = temporal_case(shape, cscl, "far")
    a, b, flow, mask, gout = _dev(c)
    cl, ref = c["cl"], c["ref"]
    ga, gb = torch.zeros_like(a), torch.full_like(b, float("nan"))
    ops.loss_temporal_bwd(a, b, flow, mask, gout, ga, gb, c["lam"], cl)
    loss = ops.loss_temporal(a, b, flow, mask, c["lam"], cl)
    S.check_temporal(loss, ga, gb, ref, None, None, "temporal_far")
    assert float(ga.abs().max()) == 0.0
    m = c["mask"].double().permute(0, 2, 3, 1)
    want = float(np.float32(c["lam"])) * ((m * c["b"].double()[..., :cl]) ** 2).mean()
    S.le(abs(float(loss) - float(want)), (cl + 16) * 2 * S.U * abs(float(want)), "temporal far loss", "temporal/far-loss")


def test_zero_sized_calls_raise(ops):
    z = torch.zeros(0, 4, 4, 4, device=DEV)
    f, m = torch.zeros(0, 2, 4, 4, device=DEV), torch.zeros(0, 1, 4, 4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.warp_bwd_nhwc(z, f)
    with pytest.raises(RuntimeError):
        ops.warp_masked_bwd_nhwc(z, f)
    with pytest.raises(RuntimeError):
        ops.loss_temporal(z, z, f, m, 1.0, 3)
    a = torch.zeros(1, 4, 4, 4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.loss_temporal(a, a, torch.zeros(1, 2, 4, 4, device=DEV), torch.zeros(1, 1, 4, 4, device=DEV), 1.0, 0)


# =================================================================================== fbcheck
@pytest.mark.parametrize("pair", S.FBC_PAIRS)
@pytest.mark.parametrize("shape", S.FBC_SHAPES, ids=_sid)
def test_fbcheck(ops, shape, pair):
    ff, bf = S.fbc_flows(pair, shape)
    got = ops.fbcheck(ff.to(DEV), bf.to(DEV)).cpu()
    assert torch.equal(got, S.fbc_ref(ff, bf))


# =================================================================================== correlation pyramid / lookup
@pytest.mark.parametrize("geo", PYRAMID_CASES, ids=_sid)
def test_corr_pyramid(ops, geo):
    P, H2, W2, ld0, levels = geo
    assert ops.corr_pyramid_floats(P, H2, W2, ld0, levels) == S.pyr_geom(P, H2, W2, ld0, levels)[0][-1]
    buf = S.pyramid_buffer(P, H2, W2, ld0, levels, fill=False)
    dbuf = buf.to(DEV)
    ops.corr_pyramid(dbuf, P, H2, W2, ld0, levels)
    got = dbuf.cpu()
    assert torch.equal(got[:P * ld0], buf[:P * ld0])          # level 0 and the junk in its padding: untouched
    lv = S.pyramid_levels(got, P, H2, W2, ld0, levels)
    for l, (ref, bound) in enumerate(S.pyramid_ref(buf, P, H2, W2, ld0, levels), 1):
        S.le((lv[l].double() - ref).abs(), bound, f"corr_pyramid {_sid(geo)} level {l}", "corr_pyramid")


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=["-".join(map(str, c)) for c in LOOKUP_CASES])
def test_corr_lookup(ops, case):
    c = lookup_case(*case)
    B, H1, W1, H2, W2, ld0, levels, r, cs = c["geo"]
    default = cs == ops.cpad(levels * (2 * r + 1) ** 2)
    got = ops.corr_lookup(c["buf"].to(DEV), c["coords"].to(DEV), B, H1, W1, H2, W2, ld0, levels, r, None if default else cs)
    assert got.shape == (B, H1, W1, cs)
    S.check_lookup(got, c["tight"], c["indep"], levels, r, "corr_lookup", c["kind"] == "outside")


def test_corr_lookup_small_level_raises(ops):
    """3 levels of a 7x9 map end at 1x2: refused, as ops.corr_lookup documents."""
    P, H2, W2, ld0, levels = 24, 7, 9, 64, 3
    buf = S.pyramid_buffer(P, H2, W2, ld0, levels).to(DEV)
    with pytest.raises(RuntimeError, match="smaller than 2x2"):
        ops.corr_lookup(buf, torch.zeros(2, 2, 3, 4, device=DEV), 2, 3, 4, H2, W2, ld0, levels, 1)


# =================================================================================== RAFT convex upsampling
@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=["-".join(map(str, c)) for c in UPSAMPLE_CASES])
def test_raft_upsample(ops, case):
    B, h, w, mcs, spike = case
    coords1, mask = S.upsample_inputs(B, h, w, mcs, spike)
    ref, bound = S.upsample_ref(coords1, mask)
    got = ops.raft_upsample(coords1.to(DEV), mask.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    S.le((got.double() - ref).abs(), bound, f"raft_upsample {case}", "raft_upsample")
