"""The conv arithmetic pinned on the device, route by route (tests/conv_ref.py holds the references, the probes,
the comparisons and the route table; tests/test_conv_ref_host.py proves on the CPU that the probes are exact, that
every named slip is rejected and that every row reaches its route).

Tier A: one-hot, mid*mid and few-hot probes, compared on BIT PATTERNS under fp32, bf16x3 and bf16x6.  Every output
is one product of a full-significand value with a power of two (or a short sum whose partial sums are all fp32
numbers), so a kernel that loses a plane, drops one of its six MFMAs, reads a stale lo plane, skips or repeats a K
stage or addresses the wrong tap, channel, phase or mirrored pixel returns different bits.  Under bf16x3 the
expected value is the three-product emulation, exact as well.
Tier B: dense data with per-channel scales over 2^+-12, |y - y64| <= c u B(o) + u |y64| per output with the
rounding count c of conv_ref.c_bound (derived there from the split and the K loop, not fitted).

Both print what they measured (worst err / bound per row, bit-exact probe counts) at the end of the module."""
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    yield o
    for label, (k, n) in sorted(R.EXACT.items()):
        print(f"tier A {label}: bit-exact on {k} of {n} probes")
    for label, w in sorted(R.WORST.items()):
        print(f"tier B {label}: worst err/bound {w:.3g}")


def _ids(params):
    return [f"{r.name}-{m}" for r, m in params]


TIER_A = [(r, m) for r in R.ROUTES for m in r.maths]
TIER_B = [(r, m) for r in R.ROUTES if r.tier_b is not None for m in r.maths]


@pytest.mark.parametrize("route,math", TIER_A, ids=_ids(TIER_A))
def test_tier_a_bit_exact(ops, route, math):
    """Every probe of the row (conv_ref.probes: the one-hot sets that visit every tap or pixel with a
    full-significand x, with a full-significand w / dy, the mid*mid pairs, the few-hot sums and the exact epilogues)
    returns the expected bits.  All probes run before the assertion, so the message names each failing family."""
    kind, c = route.kind, route.case
    arith = "fp32" if route.f32_always else math
    prev = ops.set_conv_math(math)
    try:
        with R.route_setup(ops, route):
            assert route.reaches(ops, c, math), (route.name, "the planner no longer sends this shape here")
            chunk = R.wgrad_chunk(ops, c, math) if kind == "wgrad" else None
            if kind == "wgrad":
                sets, covered, P = R.dy_pixel_sets(c, chunk, all_pixels=route.all_pixels)
                print(f"{route.name}: one-hot dy covers {covered} of {P} output pixels in {len(sets)} launches")
            fails, n = [], 0
            for p in R.probes(route, chunk):
                if math == "bf16x3" and p.get("sums") and not route.x3_sums:
                    continue
                got = route.run(ops, c, p["a"], p["b"], **p["epi"])
                n += 1
                try:
                    R.check_exact(got, kind, c, p["a"], p["b"], arith, what=f"{route.name} {math} {p['what']}",
                                  taps=p["taps"], label=f"{route.name} {math}", sums=p.get("sums", False),
                                  **p["epi"])
                except AssertionError as e:
                    fails.append(str(e))
            print(f"{route.name} {math}: bit-exact on {n - len(fails)} of {n} probes")
            assert not fails, f"{len(fails)} of {n} probes differ:\n" + "\n".join(fails[:6])
    finally:
        ops.set_conv_math(prev)


@pytest.mark.parametrize("route,math", TIER_B, ids=_ids(TIER_B))
def test_tier_b_per_output_bound(ops, route, math):
    """|y - y64| <= c u B(o) + u |y64| on dense data; c = conv_ref.route_c: 4.1 (bf16x6: the dropped mid*lo, lo*mid,
    lo*lo and split-residual terms) or 769 (bf16x3) plus one rounding per MFMA accumulation (6 or 3 per 16-deep K
    step) and per split-K slab, or K + slabs for an fma chain (fp32, the VALU routes).  Weight gradients run again
    accumulating onto a dense pre-fill (one more add, counted among the slabs)."""
    kind, c = route.kind, route.tier_b
    prev = ops.set_conv_math(math)
    try:
        with R.route_setup(ops, route):
            assert route.reaches(ops, c, math), (route.name, "the planner no longer sends this shape here")
            cc = R.route_c(ops, route, c, math)
            a, b = R.dense(kind, c, 7)
            label = f"{route.name} {math}"
            got = route.run(ops, c, a, b, want_stats=True) if route.run is R.run_fwd_in else route.run(ops, c, a, b)
            if route.run is R.run_fwd_in:
                # the statistics the GEMM epilogue emitted, against fp64 statistics of the device's own y, with the
                # bounds tests/test_gpu_reductions.py states for instnorm_stats: 2 u |mean| (+ 1e-12 mean|y|), 4 u rstd
                got, st = got
                y64 = got.double()
                mean, var = y64.mean(dim=(2, 3)), y64.var(dim=(2, 3), unbiased=False)
                rstd = 1.0 / torch.sqrt(var + ops.IN_EPS)
                em, er = (st[..., 0].double() - mean).abs(), (st[..., 1].double() - rstd).abs()
                tm, tr = 2 * R.U * mean.abs() + 1e-12 * y64.abs().mean(dim=(2, 3)), 4 * R.U * rstd
                print(f"{label} epilogue stats: worst err/bound mean {(em / tm).max().item():.3g}, rstd "
                      f"{(er / tr).max().item():.3g}")
                assert bool((em <= tm).all()) and bool((er <= tr).all()), label + " epilogue statistics"
            R.check_bound(got, kind, c, a, b, cc, what=label, label=label)
            if kind == "wgrad":
                y = R.ref(kind, c, a, b)
                pre = (torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).double() * y.abs()).float()
                got = route.run(ops, c, a, b, prefill=pre)
                # the pre-fill enters the bound's magnitude as one more term of the sum
                err = (got.double() - (y + pre.double())).abs()
                tol = cc * R.U * (R.magnitude(kind, c, a, b) + pre.double().abs()) + R.U * (y + pre.double()).abs()
                worst = (err / tol.clamp_min(1e-300)).max().item()
                print(f"{label} accumulate: worst err/bound = {worst:.3g} (c = {cc:.1f})")
                R.WORST[label + " accumulate"] = worst
                assert bool((err <= tol).all()), f"{label} accumulate: worst err/bound {worst:.3g}"
    finally:
        ops.set_conv_math(prev)


PACKS = ["PACK_KC", "PACK_CK", "PACK_OK", "PACK_IK", "PACK_IKF", "PACK_SOK"]


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("mode", PACKS)
def test_pack_planes_are_the_rne_split(ops, mode, batch):
    """The bf16 planes every split-arithmetic conv reads (weight_pack's and PackBatch's ``vst_split``, and
    ops.split_planes): hi == bf16_rne(w) bit for bit and hi + mid + lo == w exactly, for every pack mode, on raw
    fp32 weights (mid and lo of either sign) and on the masked full-significand values."""
    O, I_, Rr, S = 10, 6, 3, 2
    w = torch.cat([torch.randn(O // 2, I_, Rr, S, generator=torch.Generator().manual_seed(1)) * 0.1,
                   R.masked_full((O - O // 2, I_, Rr, S), 2, 6)]).to(DEV)
    kw = dict(Op=4) if mode == "PACK_SOK" else {}
    if mode == "PACK_SOK":
        w = w[:3].contiguous()
    if batch:
        with ops.PackBatch():
            wp = ops.weight_pack(w, getattr(ops, mode), **kw)
    else:
        wp = ops.weight_pack(w, getattr(ops, mode), **kw)
    for what, planes in (("pack", wp.vst_split), ("split_planes", ops.split_planes(wp.clone()).vst_split)):
        hi, mid, lo = (p.float().cpu() for p in planes)
        v = wp.cpu()
        assert int((v != 0).sum()) == int((w != 0).sum())   # the pack holds the weights themselves, pad lanes zero
        assert torch.equal(hi.view(torch.int32), R.bf16_rne(v).view(torch.int32)), (mode, what, "hi != bf16_rne(w)")
        assert torch.equal(hi.double() + mid.double() + lo.double(), v.double()), (mode, what, "hi + mid + lo != w")
        want = R.split3(v)
        assert torch.equal(mid, want[1]) and torch.equal(lo, want[2]), (mode, what)
        assert int((lo != 0).sum()) > 0.8 * w.numel()


@pytest.mark.parametrize("act", ["relu", "none"])
def test_producer_planes_are_the_rne_split(ops, act):
    """The operand planes a layer's IN backward writes for the weight and data gradients that consume them (the rows
    above feed those consumers planes built on the CPU): the channel-major planes [3][C][ld] (conv2d_wgrad's
    dy_planes) and the NHWC planes ``vst_apl`` (WG_NHWC, conv2d_dgrad_refl_in) are, bit for bit, the RNE split of the
    fp32 dy the same pass writes."""
    N, H, W, C = 2, 8, 16, 64
    g = torch.Generator().manual_seed(21)
    scale = torch.exp2(torch.randint(-12, 13, (C,), generator=g).float())
    y = (torch.randn(N, H, W, C, generator=g) * scale).to(DEV)
    ga = (torch.randn(N, H, W, C, generator=g) * scale.flip(0)).to(DEV)
    st = ops.instnorm_stats(y)
    dy, pl = ops.instnorm_act_bwd(ga, y, st, act, planes=True)
    dyn = ops.instnorm_act_bwd(ga, y, st, act, apre=True)
    want = R.split3(dy.cpu())
    assert int((want[2] != 0).sum()) > 0.8 * dy.numel()
    P = N * H * W
    apl, cm = dyn.vst_apl.float().cpu().view(3, N, H, W, C), pl.float().cpu()
    for i, name in enumerate(("hi", "mid", "lo")):
        assert torch.equal(apl[i], want[i]), f"NHWC {name} plane"
        assert torch.equal(cm[i, :, :P], want[i].view(P, C).t()), f"channel-major {name} plane"
