"""CPU-only: (a) the fp64 conv references of tests/conv_ref.py against float64 autograd of the stock ops, (b) the
tier-A probes are exact — every addition order of their plane products gives the same fp32 value — so a bit
comparison is a fair demand, (c) the masked full-significand values really carry all three planes, (d) every
named slip is rejected by the comparison it is meant for on the GPU suite's own cases, and the clean emulation
passes them all, (e) every row of the route table reaches its route, read off the built library's host planners
(no device needed), so a later planner change cannot silently un-cover a route, (f) the one-hot sets cover every
tap / pixel."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from conv_ref import Conv

RTOL = 1e-10


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    return o


@pytest.fixture(scope="module")
def flags0(ops):
    """The module route switches before any row flipped one."""
    return ops.route_flags()


def _g(seed, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _same(got, ref, what):
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    assert got.shape == ref.shape and err <= RTOL * scale, f"{what}: {err:.3e} of {scale:.3e}"


# ------------------------------------------------------------------- a. reference self-check
REF_CASES = [Conv(2, 3, 9, 8, 5, 3, 3, 1, 1, 1, "reflect"), Conv(2, 3, 9, 8, 5, 3, 3, 1, 1, 1, "zero"),
             Conv(1, 4, 11, 13, 3, 3, 3, 2, 1, 1, "zero"), Conv(2, 2, 10, 9, 3, 4, 4, 2, 1, 1, "zero"),
             Conv(1, 2, 10, 12, 3, 3, 3, 2, 1, 1, "reflect"), Conv(1, 2, 9, 8, 3, 7, 7, 1, 3, 3, "reflect"),
             Conv(1, 3, 6, 11, 4, 1, 5, 1, 0, 2, "zero"), Conv(1, 3, 9, 8, 4, 4, 4, 1, 1, 1, "zero")]


@pytest.mark.parametrize("c", REF_CASES, ids=str)
def test_refs_vs_autograd(c):
    x = _g(1, (c.N, c.Ci, c.H, c.W)).requires_grad_(True)
    w = _g(2, (c.Co, c.Ci, c.R, c.S)).requires_grad_(True)
    xp = F.pad(x, (c.pw, c.pw, c.ph, c.ph), mode="reflect") if c.mode == "reflect" else F.pad(x, (c.pw, c.pw, c.ph, c.ph))
    y = F.conv2d(xp, w, stride=c.stride)
    assert y.shape == (c.N, c.Co, c.Ho, c.Wo)
    gy = _g(3, tuple(y.shape))
    y.backward(gy)
    _same(R.ref("fwd", c, x.detach(), w.detach()), y.detach(), "fwd")
    _same(R.ref("dgrad", c, gy, w.detach()), x.grad, "dgrad")
    _same(R.ref("wgrad", c, x.detach(), gy), w.grad, "wgrad")
    # the magnitudes are the same ops on |.|
    _same(R.magnitude("fwd", c, x.detach(), w.detach()), F.conv2d(xp.detach().abs(), w.detach().abs(), stride=c.stride), "B")


def test_conv_transpose_is_the_stride2_data_gradient():
    """ConvTranspose2d(k3, s2, p1, op1): x [N][Ci][h][w] -> [N][Co][2h][2w] is dgrad of Conv(Ci=Co_T, Co=Ci_T)."""
    x, wt = _g(4, (2, 5, 6, 7)), _g(5, (5, 3, 3, 3))
    c = Conv(2, 3, 12, 14, 5, 3, 3, 2, 1, 1, "zero")
    _same(R.ref("dgrad", c, x, wt), F.conv_transpose2d(x, wt, stride=2, padding=1, output_padding=1), "convT")


# --------------------------------------------------------------------- b. exactness, proved
def _orders_agree(terms, want, what):
    for p in itertools.permutations(range(len(terms))):
        s = terms[p[0]].clone()
        for i in p[1:]:
            s = s + terms[i]  # fp32 adds
        assert torch.equal(s, want), (what, p)


def test_masked_values_split_exactly():
    """c. hi + mid + lo == v, both bf16 roundings of the split leave planes whose every partial sum is an fp32
    number, and lo != 0 on >= 90 %, mid != 0 on >= 99 % of the values (a condition on the inputs)."""
    v = R.masked_full((200000,), 1, 12)
    hi, mid, lo = R.split3(v)
    assert torch.equal(hi.double() + mid.double() + lo.double(), v.double())
    assert torch.equal(hi, R.bf16_rne(v))
    assert (lo != 0).double().mean().item() >= 0.90 and (mid != 0).double().mean().item() >= 0.99
    w = R.pow2((200000,), 2, 6)
    _orders_agree([hi * w, mid * w, lo * w], v * w, "one-hot, full-significand operand times a power of two")
    assert torch.equal((v * w).double(), v.double() * w.double())
    # bf16x3 carries hi and mid: their two products add exactly too
    _orders_agree([hi * w, mid * w], ((hi.double() + mid.double()) * w.double()).float(), "bf16x3")
    assert torch.equal((hi * w + mid * w).double(), (hi.double() + mid.double()) * w.double())


def test_midmid_probe_is_exact_in_every_order():
    a, b = R.midmid((20000,), 3, 12), R.midmid((20000,), 5, 6)
    pa, pb = R.split3(a), R.split3(b)
    for p in (pa, pb):
        assert bool((p[R.LO] == 0).all()) and bool((p[R.MID] != 0).all())
        assert torch.equal(p[R.HI].abs().log2().frac(), torch.zeros_like(p[R.HI]))  # hi is one bit
    want = (a.double() * b.double()).float()
    assert torch.equal(want.double(), a.double() * b.double())       # the four-term product is an fp32 number
    terms = [pa[i] * pb[j] for i, j in R.E6]
    for t, (i, j) in zip(terms, R.E6):
        assert torch.equal(t.double(), pa[i].double() * pb[j].double())
    _orders_agree(terms, want, "mid*mid pairs, 6! orders")
    # without mid*mid the value differs on every element: the probe pins that term
    assert bool((sum(t.double() for t, ij in zip(terms, R.E6) if ij != (R.MID, R.MID)) != want.double()).all())


@pytest.mark.parametrize("kind,c", [("fwd", Conv(2, 64, 9, 10, 40, 3, 3, 1, 1, 1, "reflect")),
                                    ("dgrad", Conv(2, 24, 9, 10, 40, 3, 3, 1, 1, 1, "reflect")),
                                    ("wgrad", Conv(1, 64, 16, 32, 72, 3, 3, 1, 1, 1, "reflect"))], ids=lambda v: str(v))
def test_fewhot_sufficient_condition(kind, c):
    """Few-hot sums: every plane product is a multiple of one quantum q and the sum of magnitudes stays below
    2^24 q, so every partial sum in every order (MFMA stages, split-K slabs) is an fp32 number."""
    a, b = R.family_values("fewhot", kind, c, 130)
    b = R.onehot_dy(c, 0, b, 4) if kind == "wgrad" else R.onehot_w(kind, c, 0, b, 4)
    q = 2.0 ** -18
    pa, pb = R.split3(a), R.split3(b)
    tot = 0
    for i, j in R.E6:
        t = R.ref(kind, c, pa[i].abs(), pb[j].abs())
        tot = tot + t
        for pl in (pa[i], pb[j]):
            assert torch.equal((pl.double() / 2.0 ** -18).frac(), torch.zeros_like(pl, dtype=torch.float64))
    assert tot.max().item() < 2 ** 24 * q and tot.max().item() > 0
    assert torch.equal(R.emulate(kind, c, a, b, R.E6), R.ref(kind, c, a, b))  # hi + mid + lo == x for these values


# ------------------------------------------------------------ d. the slips, on the GPU cases
def _distinct(key):
    seen, out = set(), []
    for r in R.ROUTES:
        k = key(r)
        if k is not None and k not in seen:
            seen.add(k)
            out.append(r)
    return out


TIER_A = _distinct(lambda r: (r.kind, r.case))
FAMILY_OF = {"drop_lo_hi": "a_full", "drop_mid_hi": "a_full", "drop_hi_lo": "b_full", "drop_hi_mid": "b_full",
             "drop_mid_mid": "midmid", "e3": "a_full"}


def _clean(kind, c, p, arith):
    """What a correct kernel returns, computed the way the arithmetic does: the plane products' fp64 sum rounded once
    (exact for these probes, as proved above), or stock fp32."""
    if arith == "fp32":
        y = R.REF[kind](c, p["a"].float(), p["b"].float(), None)
    else:
        y = R.emulate(kind, c, p["a"], p["b"], R.TERMS[arith]).float()
    return R.epilogue(y, **p["epi"]) if p["epi"] else y


def _rejected(kind, c, p, arith, got, mutate, chunk):
    try:
        R.check_exact(got, kind, c, p["a"], p["b"], arith, mutate=mutate, chunk=chunk, sums=p.get("sums", False),
                      **p["epi"])
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("route", TIER_A, ids=lambda r: f"{r.kind}-{'x'.join(map(str, r.case))}")
def test_tier_a_clean_passes_and_slips_are_rejected(ops, route):
    kind, c = route.kind, route.case
    chunk = max(1, c.P // 3)
    allp = list(R.probes(route, chunk))
    fam = lambda f: [p for p in allp if p["what"].startswith(f + "[")]  # noqa: E731
    # the clean emulation passes the first and last probe of every family and every epilogue probe, under each math
    for p in [q for f in R.FAMILIES for q in (fam(f)[0], fam(f)[-1])] + [p for p in allp if "[" not in p["what"]]:
        for arith in ("fp32", "bf16x6") + (("bf16x3",) if p is allp[0] or "[" not in p["what"] else ()):
            R.check_exact(_clean(kind, c, p, arith), kind, c, p["a"], p["b"], arith, what=p["what"], taps=p["taps"],
                          sums=p.get("sums", False),
                          **p["epi"])
    # product slips: EVERY probe of the named family rejects them (first, middle and last set checked)
    for mutate, f in FAMILY_OF.items():
        ps = fam(f)
        for p in {id(q): q for q in (ps[0], ps[len(ps) // 2], ps[-1])}.values():
            assert _rejected(kind, c, p, "bf16x6", _clean(kind, c, p, "bf16x6"), mutate, chunk), (mutate, p["what"])
    for mutate in ("drop_mid_hi", "drop_hi_mid"):  # the two cross terms bf16x3 has
        p = fam(FAMILY_OF[mutate])[0]
        assert _rejected(kind, c, p, "bf16x3", _clean(kind, c, p, "bf16x3"), mutate, chunk), (mutate, "bf16x3")
    # addressing slips: some probe of the one-hot family rejects each
    for mutate in R.MUTATIONS:
        if mutate in FAMILY_OF or not R.mutation_applies(mutate, kind, c):
            continue
        ps = fam("a_full")  # the last set first: it holds the last K stage / chunk, where the tail slips show
        assert any(_rejected(kind, c, p, "bf16x6", _clean(kind, c, p, "bf16x6"), mutate, chunk)
                   for p in [ps[-1], ps[0]] + ps[1:-1]), (mutate, route.name)


TIER_B = _distinct(lambda r: (r.kind, r.tier_b, r.f32_always) if r.tier_b else None)


@pytest.mark.parametrize("route", TIER_B, ids=lambda r: f"{r.kind}-{'x'.join(map(str, r.tier_b))}")
def test_tier_b_bound_passes_clean_and_rejects_product_slips(ops, route):
    """Under the derived c (conv_ref.c_bound) the emulated six / three products rounded to fp32 pass on the dense
    data, and each dropped product, and E3 in place of E6, is rejected on the same data."""
    kind, c = route.kind, route.tier_b
    a, b = R.dense(kind, c, 7)
    for m in route.maths:
        with R.route_setup(ops, route):
            cc = R.route_c(ops, route, c, m)
        if m == "fp32" or route.f32_always:
            R.check_bound(R.REF[kind](c, a, b, None), kind, c, a, b, cc, what=f"{route.name} {m} stock fp32")
            continue
        terms = R.TERMS[m]
        got = R.emulate(kind, c, a, b, terms).float()
        R.check_bound(got, kind, c, a, b, cc, what=f"{route.name} {m} clean")
        slips = [k for k, t in R.DROPS.items() if t in terms] + (["e3"] if m == "bf16x6" else [])
        for mutate in slips:
            with pytest.raises(AssertionError):
                R.check_bound(got, kind, c, a, b, cc, terms=terms, mutate=mutate, what=f"{route.name} {m} {mutate}")


# --------------------------------------------------------- e. every row reaches its route
@pytest.mark.parametrize("route", R.ROUTES, ids=lambda r: r.name)
def test_route_table_reaches_its_route(ops, route, flags0):
    for case in (route.case,) + ((route.tier_b,) if route.tier_b else ()):
        for m in route.maths:
            with R.route_setup(ops, route):
                assert route.reaches(ops, case, m), (route.name, case, m)
    assert ops.route_flags() == flags0
    assert len({r.name for r in R.ROUTES}) == len(R.ROUTES)


def test_forced_tile_kinds_cover_the_table(ops):
    """Every split-bf16 tile kind debug_set_tiles can force is a row (kinds 2, 5, 6 and 9 included), on the
    staged and on the gathering A loader; the planner returns the forced kind and no tail."""
    kinds = sorted(k for k in ops.TILE_NAMES if k >= 0)
    assert kinds == list(range(10))
    for k in kinds:
        for suffix in ("staged", "gather"):
            r = R.ROUTE_BY_NAME[f"fwd_bf_kind{k}_{suffix}"]
            assert r.tiles == (k, -1, -1)
            # staged: Ci a multiple of the kind's BK (64 covers all); gather: not a multiple of 16
            assert (r.case.Ci % 64 == 0) == (suffix == "staged") and (suffix == "staged" or r.case.Ci % 16)


# ------------------------------------------------------------------------- f. coverage
@pytest.mark.parametrize("route", TIER_A, ids=lambda r: f"{r.kind}-{'x'.join(map(str, r.case))}")
def test_onehot_sets_cover_every_tap_and_pixel(ops, route):
    kind, c = route.kind, route.case
    if kind == "wgrad":
        for m in route.maths:
            with R.route_setup(ops, route):
                chunk = R.wgrad_chunk(ops, c, m)
            sets, covered, P = R.dy_pixel_sets(c, chunk, all_pixels=route.all_pixels)
            seen = torch.zeros(P, dtype=torch.long)
            for s in sets:
                assert s.shape == (c.Co, 1)
                seen.index_add_(0, s.view(-1), torch.ones(c.Co, dtype=torch.long))
            assert int((seen > 0).sum()) == covered
            # the chunk is the planner's own: a multiple of the kernel's K step (8 pixels at least on the GEMM plans)
            # over rows of row_w >= Wo columns, and nsplit chunks of it hold every (padded) pixel
            ch, row_w = chunk
            path, _, ns = ops.conv_plan_wgrad(*R._wg_geom(c), m)
            assert row_w >= c.Wo and (row_w > c.Wo) == (path == ops._C["VST_WPLAN_BF_PADW"])
            assert (ns - 1) * ch < c.N * c.Ho * row_w <= ns * ch
            if route.all_pixels or -(-P // c.Co) <= 32:
                assert covered == P
            else:
                p = torch.arange(P)
                ho, wo = (p // c.Wo) % c.Ho, p % c.Wo
                must = (ho == 0) | (ho == c.Ho - 1) | (wo == 0) | (wo == c.Wo - 1)
                first, last = R.chunk_edge_pixels(c, chunk)
                assert first.numel() == ns and last.numel() == ns and int(last[-1]) == P - 1 and int(first[0]) == 0
                must[first] = True
                must[last] = True
                assert bool((seen[must] > 0).all()) and covered * 4 >= P
        return
    o, K = R.k_axes(kind, c)
    n = R.n_sets(kind, c)
    seen = torch.zeros(K, dtype=torch.long)
    for j in range(n):
        w = R.onehot_w(kind, c, j, torch.ones(c.Co, c.Ci, c.R, c.S))
        per_out = w.sum(dim=(1, 2, 3)) if kind == "fwd" else w.sum(dim=(0, 2, 3))
        assert torch.equal(per_out, torch.ones(o))                       # one non-zero weight per output channel
        wk = w.permute(0, 2, 3, 1) if kind == "fwd" else w.permute(1, 2, 3, 0)   # [o][r][s][channel] = [o][K]
        assert torch.equal(wk.reshape(o, K).argmax(1), R.hot_taps(kind, c, j)[:, 0])
        seen += wk.reshape(o, K).sum(0).long()
    # every (r, s, channel) exactly once, except the wrap of the last set (n O - K taps twice)
    assert int(seen.min()) >= 1 and int(seen.sum()) == n * o and int(seen.max()) <= (2 if K >= o else -(-o // K))
    if (n * o) % K == 0 and K >= o:
        assert int(seen.max()) == 1
