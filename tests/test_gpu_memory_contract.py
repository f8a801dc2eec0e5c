"""The memory contract of every kernel: each op run plain and inside guarded buffers pre-filled with 0x00, 0xFF (NaN)
and 0x7F (3.4e38) — tests/mem_guard.py is the instrument, tests/test_mem_guard_host.py proves it on the CPU.

Per row (run_row):
  a. no guard byte of any allocation written, no placed input modified (MemGuard.failures), under every fill;
  b. no allocation of the package bypassed the instrument;
  c. exact rows (the default; everything in deterministic mode): every output bit-identical across the plain run and
     the three fills — a stale workspace read, an unwritten output lane or an out-of-bounds operand read that reaches
     the result changes bits.  Lanes the contract leaves unwritten are named in the row (`windows`): there the lanes
     must still hold the fill;
  d. bounded rows: only the fp32-atomic scatters (each row cites its atomicAdd), run with set_deterministic(False):
     under every fill the result meets the bound its own test applies against fp64;
  e. the 0xFF run passes the fp64 reference and bound of the table the row comes from, so four identically wrong
     runs do not pass.

The `-s` output lists per row: exact / bounded, guarded allocations, placed inputs and bytes."""
import contextlib
import ctypes
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import mem_guard as M
import reduction_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
U = 2.0 ** -24
T0 = time.time()
ROWS_SEEN = []


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    yield o
    exact = sum(1 for r in ROWS_SEEN if r[1] == "exact")
    print(f"\nmemory contract: {len(ROWS_SEEN)} rows ({exact} exact, {len(ROWS_SEEN) - exact} bounded), "
          f"{sum(r[2] for r in ROWS_SEEN)} guarded allocations, {sum(r[3] for r in ROWS_SEEN)} bytes, "
          f"{time.time() - T0:.1f} s since import")
    for r in ROWS_SEEN:
        if r[1] != "exact":
            print("  bounded:", r[0])


@contextlib.contextmanager
def _stop_on_device_fault():
    """A HIP error inside a row ends the session: nothing more is started on a device that has faulted."""
    try:
        yield
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault, nothing more is run: {e}", returncode=3)
        raise


def _g(seed, shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _plain(t, inout=False):
    return t.detach().to(DEV).contiguous().clone()


def _le(err, tol, what):
    err, tol = torch.as_tensor(err, dtype=F64), torch.as_tensor(tol, dtype=F64)
    tol = tol.expand_as(err)
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(F64))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"    {what}: worst err/bound = {worst:.3g}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst err/bound {worst:.3g}"


def _rel_le(got, ref, bar, what):
    """max |got - ref| <= bar * max |ref| (the form of the older op tests' bars)."""
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    _le((got - ref).abs().max(), bar * ref.abs().max() + 1e-300, what)


class Row:
    """fn(ops, dev) -> {name: device tensor}; dev(t, inout=False) hands an input over (placed in a guarded window under
    a fill).  check(outs): the fp64 reference and bound of the row's table, on CPU copies of the outputs.
    windows: {output: mask(shape) -> bool tensor} of lanes the contract leaves unwritten.  atomic: names of the outputs
    an fp32-atomic scatter adds into (a bounded row; `cite` names the atomicAdd)."""

    def __init__(self, name, fn, check=None, windows=None, atomic=(), cite=None, context=None, math=None):
        self.name, self.fn, self.check, self.windows = name, fn, check, windows or {}
        self.atomic, self.cite, self.context, self.math = tuple(atomic), cite, context, math
        assert bool(self.atomic) == bool(cite), name

    def __repr__(self):
        return self.name


def last_dim_from(P):
    """Window: the last dimension's lanes from P on (the padding columns of a leading dimension)."""
    def mask(shape):
        m = torch.zeros(shape, dtype=torch.bool)
        m[..., P:] = True
        return m
    return mask


def run_row(ops, row):
    kind = "bounded" if row.atomic else "exact"
    prev_det = ops.set_deterministic(not row.atomic)
    prev_math = ops.set_conv_math(row.math) if row.math else None
    res, note = {}, ""
    try:
        with _stop_on_device_fault():
            for fill in (None,) + M.FILLS:
                with (row.context(ops) if row.context else contextlib.nullcontext()):
                    if fill is None:
                        outs = row.fn(ops, _plain)
                        torch.cuda.synchronize()
                        res[None] = {k: v.detach().cpu() for k, v in outs.items()}
                        continue
                    with M.MemGuard(fill) as mg:
                        outs = row.fn(ops, mg.place)
                        fails = mg.failures()
                        skew = mg.misaligned(256)
                        res[fill] = {k: v.detach().cpu() for k, v in outs.items()}
                        kept = {k: mg.unwritten(outs[k]).all(dim=-1).cpu() for k in row.windows}
                        note, n_alloc, n_bytes = mg.summary(), sum(1 for a in mg.allocs if a.kind != "place"), mg.bytes
                        passed = list(mg.passthrough)
                        mg.drop()
                tag = f"{row.name} [fill {M.FILL_NAMES[fill]}]"
                assert not fails, tag + ": " + "; ".join(fails[:6])                                            # a
                assert not skew, tag + ": guarded windows not 256-byte aligned: " + "; ".join(skew[:6])
                assert not passed, tag + ": allocations that bypassed the instrument: " + "; ".join(passed[:6])  # b
                assert n_alloc > 0, tag + ": the row made no guarded allocation"
                for k, mask in row.windows.items():
                    m = mask(tuple(outs[k].shape))
                    assert bool(m.any()), (tag, k, "empty window")
                    assert bool(kept[k][m].all()), f"{tag}: {k}: {int((~kept[k][m]).sum())} lanes of the unwritten window " \
                                                   f"were written"
            print(f"  {row.name}: {kind}; {note}" + (f"; atomic: {row.cite}" if row.atomic else ""))
            ROWS_SEEN.append((row.name, kind, n_alloc, n_bytes))
            base = res[None]
            for fill in M.FILLS:                                                                               # c
                assert res[fill].keys() == base.keys()
                for k, v in res[fill].items():
                    if k in row.atomic:
                        continue
                    a, b = _bits(v), _bits(base[k])
                    assert a.shape == b.shape, (row.name, k)
                    if k in row.windows:
                        keep = ~row.windows[k](tuple(v.shape))
                        a, b = a[keep], b[keep]
                    if not torch.equal(a, b):
                        d = (a != b)
                        raise AssertionError(f"{row.name}: output {k} differs from the plain run under fill "
                                             f"{M.FILL_NAMES[fill]}: {int(d.sum())} of {d.numel()} lanes, first at "
                                             f"{tuple(int(i) for i in d.nonzero()[0])}")
            if row.check is not None:
                for fill in (M.FILLS if row.atomic else (0xFF,)):                                              # d, e
                    row.check(res[fill])
    finally:
        ops.set_deterministic(prev_det)
        if row.math:
            ops.set_conv_math(prev_math)


# ===================================================================================================== conv routes
@functools.lru_cache(maxsize=4)
def _conv_data(route_name):
    r = CR.ROUTE_BY_NAME[route_name]
    a, b = CR.dense(r.kind, r.case, 7)
    return a, b, CR.ref(r.kind, r.case, a, b), CR.magnitude(r.kind, r.case, a, b)


def _conv_variants(route):
    """(label, adaptor keywords): plain, then every epilogue the entry point has (the names of conv_ref.probes); weight
    gradients overwrite a NaN-filled dw and accumulate onto a dense pre-fill."""
    kind, c = route.kind, route.case
    if kind == "wgrad":
        pre = _g(9, (c.Co, c.Ci, c.R, c.S), 0.5)
        return [("overwrite", {}), ("accumulate", dict(prefill=pre))]
    names = route.epi
    if names is None:
        names = {"fwd": CR._FWD_EPI if c.R == c.S and c.ph == c.pw else CR._FWD_EPI[:3], "dgrad": ("addend",)}[kind]
    n = c.Co if kind == "fwd" else c.Ci
    out = [("plain", {})]
    for name in names:
        epi = {}
        if "bias" in name:
            epi["bias"] = _g(11, (n,), 0.5)
        if "lrelu" in name:
            epi.update(act="lrelu", slope=0.2)
        elif "relu" in name:
            epi["act"] = "relu"
        if name == "addend":
            epi["addend"] = _g(12, CR.operand_shapes("fwd", c)[0])
        out.append((name, epi))
    return out


def _conv_check(ops, route, math, epi, label):
    """|y - y64| <= (c + 3) u (B + E) + u |y64|: c of conv_ref.route_c (the tier-B bound at this shape), B the sum of
    the products' magnitudes, E = |bias| + |addend| + |prefill|; the 3 are the epilogue's roundings (the bias add, the
    slope's fp32 value and product, the addend / accumulate add), each at most u times the terms it joins."""
    kind, c = route.kind, route.case
    a, b, y64, B = _conv_data(route.name)
    cc = CR.route_c(ops, route, c, math) + 3
    y, E = y64, torch.zeros_like(y64)
    if "prefill" in epi:
        y, E = y + epi["prefill"].to(F64), epi["prefill"].to(F64).abs()
    if "bias" in epi:
        bv = epi["bias"].to(F64).view(1, -1, 1, 1)
        y, E = y + bv, E + bv.abs()
    act = epi.get("act", "none")
    if act == "relu":
        y = y.clamp_min(0)
    elif act == "lrelu":
        y = torch.where(y > 0, y, y * float(np.float32(0.2)))
    if "addend" in epi:
        y, E = y + epi["addend"].to(F64), E + epi["addend"].to(F64).abs()

    def check(outs):
        got = outs["y"].to(F64)
        assert got.shape == y.shape, (label, got.shape, y.shape)
        _le((got - y).abs(), cc * U * (B + E) + U * y.abs(), f"{label} vs fp64 (c = {cc:.1f})")
    return check


@contextlib.contextmanager
def _conv_dev(dev):
    prev, CR._dev = CR._dev, dev
    try:
        yield
    finally:
        CR._dev = prev


CONV = [(r, m) for r in CR.ROUTES for m in r.maths]


@pytest.mark.parametrize("route,math", CONV, ids=[f"{r.name}-{m}" for r, m in CONV])
def test_conv_route(ops, route, math):
    """Every row of conv_ref.ROUTES at its tier-A shape on dense data, through its own adaptor with conv_ref._dev
    placing the operands: the split-K slabs, the head kernels' z / part workspaces, img_wgrad's slabs, the skinny split
    and the reflect-border workspaces all live in poisoned memory."""
    kind, c = route.kind, route.case
    a, b = _conv_data(route.name)[:2]
    stats = route.run is CR.run_fwd_in
    for label, epi in _conv_variants(route):
        def fn(ops, dev, epi=epi):
            with _conv_dev(lambda t: dev(t)):
                assert route.reaches(ops, c, math), (route.name, "the planner no longer sends this shape here")
                kw = {k: v for k, v in epi.items() if not (k == "slope" and v == 0.0)}
                if stats:
                    y, st = route.run(ops, c, a, b, want_stats=True, **kw)
                    return {"y": y.to(DEV), "stats": st.to(DEV)}
                return {"y": route.run(ops, c, a, b, **kw).to(DEV)}
        name = f"{route.name} {math} {label}"
        run_row(ops, Row(name, fn, _conv_check(ops, route, math, epi, name), math=math,
                         context=lambda ops: CR.route_setup(ops, route)))


def _wgrad_db_row(ops, name, route, math, accumulate):
    """conv2d_wgrad with the bias gradient db, written or accumulated (the adaptors of conv_ref pass db=None), at the
    tier-A shape of a route of conv_ref.ROUTES and under that route's own bound."""
    c = route.case
    x, dy = CR.dense("wgrad", c, 17)
    pre_w, pre_b = _g(18, (c.Co, c.Ci, c.R, c.S), 0.5), _g(19, (c.Co,), 0.5)

    def fn(ops, dev):
        assert route.reaches(ops, c, math), (route.name, "the planner no longer sends this shape here")
        dw = dev(pre_w if accumulate else torch.full_like(pre_w, float("nan")), inout=True)
        db = dev(pre_b if accumulate else torch.full_like(pre_b, float("nan")), inout=True)
        xn, dyn = ops.nchw_to_nhwc(dev(x)), ops.nchw_to_nhwc(dev(dy))
        ops.conv2d_wgrad(xn, dyn, dw, db, c.R, c.S, c.stride, c.ph, c.mode, c.Co, c.Ci, c.Ci * c.R * c.S, c.R * c.S,
                         accumulate=accumulate)
        return {"dw": dw, "db": db}

    def check(outs):
        y, B = CR.ref("wgrad", c, x, dy), CR.magnitude("wgrad", c, x, dy)
        pw = pre_w.to(F64) if accumulate else torch.zeros_like(y)
        cc = CR.route_c(ops, route, c, math) + 3       # the route's own c, + 3 as in _conv_check
        _le((outs["dw"].to(F64) - y - pw).abs(), cc * U * (B + pw.abs()) + U * (y + pw).abs(), name + " dw vs fp64")
        s = dy.to(F64).sum(dim=(0, 2, 3))
        pb = pre_b.to(F64) if accumulate else torch.zeros_like(s)
        # test_channel_sum_wide's bar (1e-6 of max |ref|) plus the accumulate add's rounding
        _le((outs["db"].to(F64) - s - pb).abs(), 1e-6 * (s + pb).abs().max() + U * (s + pb).abs(), name + " db vs fp64")
    return Row(name, fn, check, math=math, context=lambda ops: CR.route_setup(ops, route))


# (row, the route of conv_ref.ROUTES whose shape, reach predicate and bound it takes, arithmetic)
WGRAD_DB = [("generic", "wgrad_plain_generic", "fp32"), ("image_fused", "wgrad_plain_image", "bf16x6"),
            ("head_fused", "wgrad_plain_head", "bf16x6"), ("nhwc_f32", "wgrad_nhwc_f32_128x128", "bf16x6")]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("case", WGRAD_DB, ids=lambda c: c[0])
def test_conv_wgrad_with_db(ops, case, accumulate):
    tag, route, math = case
    run_row(ops, _wgrad_db_row(ops, f"wgrad+db {tag} {math} {'accumulate' if accumulate else 'overwrite'}",
                               CR.ROUTE_BY_NAME[route], math, accumulate))


@pytest.mark.parametrize("name", ["wgrad_images_producer", "wgrad_images_producer_s2"])
def test_conv_wgrad_fed_producer_images(ops, name):
    """The x6 weight gradient fed both images as their producers leave them in poisoned memory: x_t from
    instnorm_act_fwd(cp=...) and dy's channel-major planes from instnorm_act_bwd(planes=True), whose padding columns
    [P, vst_cp_ld(P)) hold the fill (the route rows build dy's planes on the host with zeroed padding).  dw must come
    back with the bits of the plain run, so the kernel reads neither image's padding columns."""
    route = CR.ROUTE_BY_NAME[name]
    c, math = route.case, "bf16x6"
    x = CR.dense("wgrad", c, 27)[0]
    y, ga = _g(28, (c.N, c.Ho, c.Wo, CR.cpad(c.Co))), _g(29, (c.N, c.Ho, c.Wo, CR.cpad(c.Co)))
    pre = _g(30, (c.Co, c.Ci, c.R, c.S), 0.5)

    def fn(ops, dev):
        assert route.reaches(ops, c, math), name
        xn = ops.nchw_to_nhwc(dev(x))
        ident = torch.zeros((c.N, xn.shape[-1], 2), device=DEV)
        ident[..., 1] = 1.0
        a, x_t = ops.instnorm_act_fwd(xn, ident, "none", cp=(c.ph, c.mode, c.stride))
        assert torch.equal(a, xn)
        yd = dev(y)
        dy, pl = ops.instnorm_act_bwd(dev(ga), yd, ops.instnorm_stats(yd), "relu", planes=True)
        dw = dev(pre, inout=True)
        ops.conv2d_wgrad(xn, dy, dw, None, c.R, c.S, c.stride, c.ph, c.mode, c.Co, c.Ci, c.Ci * c.R * c.S, c.R * c.S,
                         accumulate=True, dy_planes=pl, x_t=x_t)
        return {"dw": dw, "dy": dy, "pl": pl, "x_t": x_t}

    def check(outs):      # against the fp64 weight gradient of the device's own dy, the route's bound
        dy = outs["dy"][..., :c.Co].permute(0, 3, 1, 2).contiguous()
        want = CR.ref("wgrad", c, x, dy) + pre.to(F64)
        B = CR.magnitude("wgrad", c, x, dy) + pre.to(F64).abs()
        cc = CR.route_c(ops, route, c, math) + 3
        assert float(dy.abs().max()) > 0
        _le((outs["dw"].to(F64) - want).abs(), cc * U * B + U * want.abs(), f"{name} fed producer images vs fp64")
    windows = {"pl": last_dim_from(c.P), "x_t": last_dim_from(c.N * (c.H + 2 * c.ph) * (c.W + 2 * c.pw))}
    run_row(ops, Row(f"{name} fed producer images", fn, check, windows=windows, math=math,
                     context=lambda ops: CR.route_setup(ops, route)))


@pytest.mark.parametrize("apre", [False, True], ids=["fp32_dy", "apre"])
@pytest.mark.parametrize("planes", [False, True], ids=["noplanes", "planes"])
def test_conv_dgrad_refl_in_whole(ops, apre, planes):
    """conv2d_dgrad_refl_in's every output (the route rows above compare g alone): g, the IN backward dy_in (fp32, or
    its NHWC planes only with apre), db accumulated, the channel-major planes [3][C][ld] with their padding columns
    ld - N H W named as the unwritten window."""
    c = CR.ROUTE_BY_NAME["dgrad_refl_in"].case
    dy, w = CR.dense("dgrad", c, 7)
    y_in, ad = _g(5, (c.N, c.H, c.W, CR.cpad(c.Ci))), _g(6, (c.N, c.Ci, c.H, c.W))
    P = c.N * c.H * c.W

    def fn(ops, dev):
        ikf = ops.weight_pack(dev(w), ops.PACK_IKF)
        yi = dev(y_in)
        db = dev(torch.full((CR.cpad(c.Ci),), 0.5), inout=True)
        r = ops.conv2d_dgrad_refl_in(ops.nchw_to_nhwc(dev(dy)), ikf, c.H, c.W, CR.cpad(c.Ci), yi, ops.instnorm_stats(yi),
                                     "relu", addend=ops.nchw_to_nhwc(dev(ad)), db=db, planes=planes, apre=apre)
        assert r is not None
        out = {"g": r[0], "db": db}
        if apre:
            out["dyi_apl"] = r[1].vst_apl
        else:
            out["dyi"] = r[1]
        if planes:
            out["pl"] = r[2]
        return out

    def check(outs):
        y = CR.ref("dgrad", c, dy, w) + ad.to(F64)
        B = CR.magnitude("dgrad", c, dy, w) + ad.to(F64).abs()
        cc = CR.route_c(ops, CR.ROUTE_BY_NAME["dgrad_refl_in"], c, "bf16x6") + 3
        g = ops.nhwc_to_nchw(outs["g"].to(DEV), c.Ci).cpu().to(F64)
        _le((g - y).abs(), cc * U * B + U * y.abs(), "dgrad_refl_in g vs fp64")
    # (with apre dy_in's fp32 image is not written, vst_planes_only: it is not among the outputs)
    windows = {"pl": last_dim_from(P)} if planes else {}
    run_row(ops, Row(f"dgrad_refl_in whole apre={apre} planes={planes}", fn, check, windows=windows, math="bf16x6"))


# ====================================================================================================== tap family
def _tap_chunked(ops, per_image):
    @contextlib.contextmanager
    def cm(ops):
        prev, ops.TAP_CHUNK_BYTES = ops.TAP_CHUNK_BYTES, per_image
        try:
            yield
        finally:
            ops.TAP_CHUNK_BYTES = prev
    return cm


TAP_ROUTES = ["fwd_tap", "fwd_tap_h", "dgrad_tap", "dgrad_tap_h", "wgrad_tap", "wgrad_tap_planes", "wgrad_tap_h",
              "wgrad_tap_swap"]


@pytest.mark.parametrize("chunked", [False, True], ids=["one_chunk", "chunked"])
@pytest.mark.parametrize("name", TAP_ROUTES)
def test_tap_family_chunks(ops, name, chunked):
    """The tap forms in one chunk (TAP_CHUNK_BYTES = 0) and one image per chunk, as test_tap_conv_image_chunks sets it:
    the zbuf / dbuf of a chunk is reused by the next on poisoned memory."""
    route = CR.ROUTE_BY_NAME[name]
    c, math = route.case, "bf16x6"
    a, b = _conv_data(name)[:2]
    per_image = c.H * c.W * c.R * c.R * 16 if chunked else 0

    def fn(ops, dev):
        with _conv_dev(lambda t: dev(t)):
            if not chunked:
                assert route.reaches(ops, c, math), name
            return {"y": route.run(ops, c, a, b).to(DEV)}
    label = f"{name} {'chunked' if chunked else 'one chunk'}"
    run_row(ops, Row(label, fn, _conv_check(ops, route, math, {}, label), math=math, context=_tap_chunked(ops, per_image)))


@pytest.mark.parametrize("form", ["wgrad", "wgrad_h", "wgrad_swap", "wgrad_swap_db"])
def test_tap_wgrad_with_producer_images(ops, form):
    """The tap weight gradients fed the images their producer writes: x_t (the IN apply's channel-major image,
    instnorm_act_fwd(cp=...)) and x_pl (its bf16 planes, xpl=...); the images' padding columns are the window."""
    route = CR.ROUTE_BY_NAME[{"wgrad": "wgrad_tap_planes", "wgrad_h": "wgrad_tap_h", "wgrad_swap": "wgrad_tap_swap",
                              "wgrad_swap_db": "wgrad_tap_swap"}[form]]
    c = route.case
    x, dy = _conv_data(route.name)[:2]
    pad = c.ph
    pre = _g(9, (c.Co, c.Ci, c.R, c.S), 0.5)
    wx = 0

    def fn(ops, dev):
        xn, dyn = ops.nchw_to_nhwc(dev(x)), ops.nchw_to_nhwc(dev(dy))
        st = torch.zeros((c.N, xn.shape[-1], 2), device=DEV)
        st[..., 1] = 1.0
        dw = dev(pre, inout=True)
        out = {"dw": dw}
        assert route.reaches(ops, c, "bf16x6")
        if form == "wgrad":
            a, img = ops.instnorm_act_fwd(xn, st, "none", cp=(0, "zero", 1))
            ops.tap_conv_wgrad(xn, dyn, dw, c.R, pad, c.mode, accumulate=True, x_t=img)
        elif form == "wgrad_h":
            a, img = ops.instnorm_act_fwd(xn, st, "none", cp=(pad + 1, "reflect", 1))
            ops.tap_conv_wgrad_h(xn, dyn, dw, c.R, pad, c.mode, accumulate=True, x_t=img)
        else:
            a, img = ops.instnorm_act_fwd(xn, st, "none", xpl=(pad, "reflect", ops.tap_swap_geom(c.W, c.R)[0]))
            db = None
            if form == "wgrad_swap_db":
                db = out["db"] = dev(torch.full((4,), 0.25), inout=True)
            ops.tap_conv_wgrad_swap(xn, dyn, dw, c.R, pad, c.mode, accumulate=True, x_pl=img, db=db)
        assert torch.equal(a, xn)
        out["img"] = img
        return out

    if form == "wgrad":
        P = c.N * c.H * c.W
    elif form == "wgrad_h":
        P = c.N * (c.H + 2 * pad + 2) * (c.W + 2 * pad + 2)
    else:
        wx = (8 - (c.W + c.R - 1) % 8) % 8
        P = c.N * (c.H + 2 * pad) * (c.W + 2 * pad + wx)
    check0 = _conv_check(ops, route, "bf16x6", dict(prefill=pre), f"tap {form} with producer image")

    def check(outs):
        check0({"y": outs["dw"]})
        if "db" in outs:
            s = dy.to(F64).sum(dim=(0, 2, 3))
            _le((outs["db"][:c.Co].to(F64) - 0.25 - s).abs(), 1e-6 * s.abs().max() + U * (0.25 + s.abs()), "tap swap db")
    run_row(ops, Row(f"tap {form} + producer image", fn, check, windows={"img": last_dim_from(P)}, math="bf16x6"))


# ===================================================================================================== norm family
EPS = RR.f32(1e-5)
SLOPE = RR.f32(0.2)
NORM_VARIANT_CASES = list(M.ROW_SHAPES["norm_variant_cases"])


@functools.lru_cache(maxsize=2)
def _in_data(case):
    N, H, W, C = RR.IN_CASE[case][1]
    seed = 1000 + 10 * [c[0] for c in RR.IN_CASES].index(case)
    x = 2.0 * _g(seed, (N, H, W, C)) + 0.5
    g, res = _g(seed + 1, (N, H, W, C)), _g(seed + 2, (N, H, W, C))
    mean, rstd = RR.in_stats(RR.nchw64(x), EPS)
    return x, g, res, mean, rstd


def _pmax(t):
    return t.abs().amax(dim=(2, 3))


def _check_plain_in(case, act, outs, db_base):
    """test_gpu_reductions._check_plain_in's references and bounds on this row's outputs."""
    x, g, res, mean, rstd = _in_data(case)
    x64, g64 = RR.nchw64(x), RR.nchw64(g)
    res64 = RR.nchw64(res) if act == "none" else None
    st = outs["stats"]
    m32, r32 = st[..., 0], st[..., 1]
    mref, rref = mean[:, :, 0, 0], rstd[:, :, 0, 0]
    _le((m32.to(F64) - mref).abs(), 2 * U * mref.abs() + 1e-12 * x64.abs().mean(dim=(2, 3)), case + " mean")
    _le((r32.to(F64) - rref).abs(), 4 * U * rref, case + " rstd")
    mask = None
    if act != "none":
        mask = (x.permute(0, 3, 1, 2) - m32[:, :, None, None]) * r32[:, :, None, None] > 0
    if "y" in outs:
        ref = RR.in_fwd(x64, mean, rstd, act, SLOPE, res64, mask)
        xh = (x64 - mean) * rstd
        bound = 4 * U * (mean.abs() * rstd + xh.abs() + (res64.abs() if res64 is not None else 0) + ref.abs())
        _le((RR.nchw64(outs["y"]) - ref).abs(), bound, f"{case}/{act} fwd")
    if "dx" in outs:
        dref, dbref = RR.in_bwd(g64, x64, mean, rstd, act, SLOPE, mask)
        dgot = RR.nchw64(outs["dx"])
        assert torch.isfinite(dgot).all()
        _le(_pmax(dgot - dref), 1e-5 * _pmax(dref), f"{case}/{act} dx")
        if "db" in outs:
            _le((outs["db"].to(F64) - db_base - dbref).abs(), 1e-5 * dref.abs().sum(dim=(0, 2, 3)), f"{case}/{act} db")


@pytest.mark.parametrize("case", [c[0] for c in RR.IN_CASES])
def test_instnorm_plain(ops, case):
    """instnorm_stats, instnorm_act_fwd and instnorm_act_bwd (db accumulated) at every reduction geometry: the
    partial buffers [N][nsplit][C] of both reductions in poisoned memory."""
    x, g, res, _, _ = _in_data(case)
    C = x.shape[-1]
    act = "relu"

    def fn(ops, dev):
        xd, gd = dev(x), dev(g)
        st = ops.instnorm_stats(xd)
        y = ops.instnorm_act_fwd(xd, st, act, 0.2)
        db = dev(torch.full((C,), 0.5), inout=True)
        dx = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, db=db, accumulate_db=True)
        return {"stats": st, "y": y, "dx": dx, "db": db}
    run_row(ops, Row(f"instnorm plain {case}", fn, lambda o: _check_plain_in(case, act, o, 0.5)))


@pytest.mark.parametrize("variant", ["residual", "cp", "xpl", "bwd_db_overwrite", "bwd_planes", "bwd_apre",
                                     "bwd_apre_planes"])
@pytest.mark.parametrize("case", NORM_VARIANT_CASES)
def test_instnorm_variants(ops, case, variant):
    """The forms of the IN apply and backward that write a second image: the channel-major `at` (cp=), the bf16 plane
    images (xpl=, planes=) and the NHWC planes (apre=).  Their leading dimensions (vst_cp_ld) are padded: the padding
    columns are the unwritten window; with apre the fp32 dy is not written at all (its window is every lane)."""
    x, g, res, _, _ = _in_data(case)
    N, H, W, C = x.shape
    windows, act = {}, "relu"
    if variant == "cp":
        windows["img"] = last_dim_from(N * (H + 2) * (W + 2))
    elif variant == "xpl":
        windows["img"] = last_dim_from(N * (H + 2) * (W + 2 + 3))
    elif variant in ("bwd_planes", "bwd_apre_planes"):
        windows["pl"] = last_dim_from(N * H * W)
    if variant.startswith("bwd_apre"):
        windows["dx_fp32"] = lambda shape: torch.ones(shape, dtype=torch.bool)
    if variant == "residual":
        act = "none"

    def fn(ops, dev):
        xd, gd = dev(x), dev(g)
        st = ops.instnorm_stats(xd)
        out = {"stats": st}
        if variant == "residual":
            out["y"] = ops.instnorm_act_fwd(xd, st, "none", 0.0, residual=dev(res))
        elif variant == "cp":
            out["y"], out["img"] = ops.instnorm_act_fwd(xd, st, act, 0.2, cp=(1, "reflect", 1))
        elif variant == "xpl":
            out["y"], out["img"] = ops.instnorm_act_fwd(xd, st, act, 0.2, xpl=(1, "reflect", 3))
        elif variant == "bwd_db_overwrite":
            db = out["db"] = dev(torch.full((C,), float("nan")), inout=True)
            out["dx"] = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, db=db, accumulate_db=False)
        elif variant == "bwd_planes":
            out["dx"], out["pl"] = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, planes=True)
        elif variant == "bwd_apre":
            dx = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, apre=True)
            out["dx_fp32"], out["apl"] = dx, dx.vst_apl
        else:
            dx, out["pl"] = ops.instnorm_act_bwd(gd, xd, st, act, 0.2, planes=True, apre=True)
            out["dx_fp32"], out["apl"] = dx, dx.vst_apl
        return out

    def check(outs):
        _check_plain_in(case, act, outs, 0.0)
        dref = None
        if "apl" in outs or "pl" in outs:
            mean, rstd = _in_data(case)[3:]
            st = outs["stats"]
            mask = (x.permute(0, 3, 1, 2) - st[..., 0][:, :, None, None]) * st[..., 1][:, :, None, None] > 0
            dref = RR.in_bwd(RR.nchw64(g), RR.nchw64(x), mean, rstd, act, SLOPE, mask)[0]
        if "apl" in outs:       # hi + mid + lo of the NHWC planes is dy to 2^-24 of itself: the dx bound holds for it
            dy = outs["apl"].to(F64).sum(0).view(N, H, W, C).permute(0, 3, 1, 2)
            _le(_pmax(dy - dref), 1e-5 * _pmax(dref) + 2 * U * _pmax(dref), f"{case} apre planes sum vs fp64")
        if "pl" in outs:        # the channel-major planes [3][C][ld]: the same values, transposed
            dy = outs["pl"].to(F64).sum(0)[:, :N * H * W].view(C, N, H, W).permute(1, 0, 2, 3)
            _le(_pmax(dy - dref), 1e-5 * _pmax(dref) + 2 * U * _pmax(dref), f"{case} channel-major planes vs fp64")
        if variant == "cp":      # at[c][n][hp][wp] is a's reflect-padded image, bit for bit
            a = outs["y"].permute(0, 3, 1, 2)
            ap = F.pad(a, (1, 1, 1, 1), mode="reflect")
            want = ap.permute(1, 0, 2, 3).reshape(C, -1)
            assert torch.equal(outs["img"][:, :want.shape[1]], want), f"{case} channel-major image != padded a"
        if variant == "xpl":
            a = outs["y"].permute(0, 3, 1, 2)
            ap = F.pad(F.pad(a, (1, 1, 1, 1), mode="reflect"), (0, 3))
            want = ap.permute(1, 0, 2, 3).reshape(C, -1)
            got = outs["img"].to(F64).sum(0)[:, :want.shape[1]]
            _le((got - want.to(F64)).abs(), 2 * U * want.to(F64).abs(), f"{case} plane image sum vs padded a")
    run_row(ops, Row(f"instnorm {variant} {case}", fn, check, windows=windows))


AFFINE_CASES = list(M.ROW_SHAPES["affine_cases"])


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("case", AFFINE_CASES)
def test_instnorm_affine(ops, case, accumulate):
    """instnorm_affine_fwd / _bwd with gate and residual, the four parameter gradients written or accumulated
    (test_instnorm_affine_geometry's references and bounds, without an activation so no sign decision hangs on
    rounding)."""
    x, g, res, mean, rstd = _in_data(case)
    N, H, W, C = x.shape
    gamma, beta = 1.0 + _g(31, (C,), 0.2), _g(32, (C,), 0.2)
    gate, mult = 0.7, 0.9
    init = 0.25 if accumulate else float("nan")

    def fn(ops, dev):
        xd, gd, gam, bet, gt = dev(x), dev(g), dev(gamma), dev(beta), dev(torch.tensor([gate]))
        st = ops.instnorm_stats(xd)
        y = ops.instnorm_affine_fwd(xd, st, gam, bet, "none", gate=gt, gate_mult=mult, residual=dev(res))
        bufs = {k: dev(torch.full((1 if k == "dgate" else C,), init), inout=True)
                for k in ("dgamma", "dbeta", "dgate", "dbias")}
        dx = ops.instnorm_affine_bwd(gd, xd, st, gam, bet, "none", gate=gt, gate_mult=mult, accumulate=accumulate, **bufs)
        return dict(bufs, y=y, dx=dx)

    def check(outs):
        x64, g64 = RR.nchw64(x), RR.nchw64(g)
        gate32, mult32 = RR.f32(gate), RR.f32(mult)
        ref = RR.in_affine_fwd(x64, mean, rstd, gamma.to(F64), beta.to(F64), "none", SLOPE, gate32, mult32, RR.nchw64(res))
        _le(_pmax(RR.nchw64(outs["y"]) - ref), 1e-5 * _pmax(ref), case + " affine fwd")
        r = RR.in_affine_bwd(g64, x64, mean, rstd, gamma.to(F64), beta.to(F64), "none", SLOPE, gate32, mult32)
        _le(_pmax(RR.nchw64(outs["dx"]) - r["dx"]), 1e-4 * _pmax(r["dx"]), case + " affine dx")
        base = 0.25 if accumulate else 0.0
        for k in ("dgamma", "dbeta", "dgate", "dbias"):
            got = outs[k].to(F64) - base
            want = r[k].reshape(got.shape)
            tol = (1e-5 * r["dx"].abs().sum(dim=(0, 2, 3)) if k == "dbias" else
                   1e-4 * want.abs() + 8 * U * r[k + "_abs"].reshape(got.shape) + 2 * U * (base + want.abs()))
            _le((got - want).abs(), tol, f"{case} affine {k}")
    run_row(ops, Row(f"instnorm_affine {case} {'accumulate' if accumulate else 'overwrite'}", fn, check))


@pytest.mark.parametrize("case", M.ROW_SHAPES["cond_cases"])
def test_cond_instnorm_adain_skip_running(ops, case):
    """The other norm kernels that take the shared partial buffers, once each at a reduction geometry with several
    slices: cond_instnorm_fwd / _bwd, adain_fwd / _bwd, instnorm_skip_fwd / _bwd, instnorm_running_update and
    instnorm_stats_from_running.  References in fp64 composed from reduction_ref's IN, with the bars of their own
    tables (test_gpu_multistyle, test_gpu_stargan2, test_gpu_unet: forward 1e-5, dx 1e-4 of max |ref|)."""
    x, g, res, mean, rstd = _in_data(case)
    N, H, W, C = x.shape
    Sn = 3
    ids = [2, 0][:N] if N <= 2 else [2, 0, 2][:N]
    E = torch.cat([1.0 + _g(41, (Sn, C), 0.2), _g(42, (Sn, C), 0.2)], dim=1).contiguous()
    bw, bb = 1.0 + _g(43, (C,), 0.2), _g(44, (C,), 0.2)
    h = _g(45, (N, 2 * C), 0.3)
    g_s = _g(46, (N, H, W, C))
    rm0, rv0 = 1.0 + torch.rand(C, generator=torch.Generator().manual_seed(3)), \
        0.5 + torch.rand(C, generator=torch.Generator().manual_seed(4))

    def fn(ops, dev):
        xd, gd = dev(x), dev(g)
        st = ops.instnorm_stats(xd)
        out = {"stats": st}
        sid = dev(torch.tensor(ids, dtype=torch.int32))
        Ed, wd, bd = dev(E), dev(bw), dev(bb)
        out["cond_y"] = ops.cond_instnorm_fwd(xd, st, sid, Ed, wd, bd, "none")
        cb = {k: dev(torch.full(s, float("nan")), inout=True) for k, s in
              (("dembed", (Sn, 2 * C)), ("dbn_w", (C,)), ("dbn_b", (C,)), ("dbias", (C,)))}
        out["cond_dx"] = ops.cond_instnorm_bwd(gd, xd, st, sid, Ed, wd, bd, "none", accumulate=False, **cb)
        out.update({"cond_" + k: v for k, v in cb.items()})
        hd = dev(h)
        out["adain_y"] = ops.adain_fwd(xd, st, hd, "none", 0.2)
        dh, dbias = dev(torch.full((N, 2 * C), float("nan")), inout=True), dev(torch.full((C,), float("nan")), inout=True)
        out["adain_dx"] = ops.adain_bwd(gd, xd, st, hd, "none", 0.2, dh=dh, dbias=dbias)
        out["adain_dh"], out["adain_dbias"] = dh, dbias
        cat = dev(torch.full((N, H, W, 2 * C), 7.0), inout=True)
        out["skip_d"] = ops.instnorm_skip_fwd(xd, st, cat, C)
        out["skip_cat"] = cat
        g_cat = torch.full((N, H, W, 2 * C), float("nan"))
        g_cat[..., C:] = g_s
        sdb = dev(torch.full((C,), 0.5), inout=True)
        out["skip_dy"] = ops.instnorm_skip_bwd(gd, dev(g_cat), C, xd, st, db=sdb, accumulate_db=True)
        out["skip_db"] = sdb
        rm, rv = dev(rm0, inout=True), dev(rv0, inout=True)
        ops.instnorm_running_update(st, rm, rv, H * W, momentum=0.1)
        out["rm"], out["rv"] = rm, rv
        out["st_run"] = ops.instnorm_stats_from_running(rm, rv, N)
        return out

    def check(outs):
        x64, g64 = RR.nchw64(x), RR.nchw64(g)
        xh = (x64 - mean) * rstd
        idx = torch.tensor(ids)
        ge, be = E[idx, :C].to(F64), E[idx, C:].to(F64)
        gam, bet = (ge * bw.to(F64))[:, :, None, None], (ge * bb.to(F64) + be)[:, :, None, None]
        _rel_le(RR.nchw64(outs["cond_y"]), gam * xh + bet, 1e-5, "cond_instnorm fwd")
        # the IN backward of dz = g * gamma (no activation): rstd (dz - mean dz - xhat mean(dz xhat))
        def in_bwd(dz):
            return rstd * (dz - dz.mean(dim=(2, 3), keepdim=True) - xh * (dz * xh).mean(dim=(2, 3), keepdim=True))
        _rel_le(RR.nchw64(outs["cond_dx"]), in_bwd(g64 * gam), 1e-4, "cond_instnorm dx")
        sgx, sg = (g64 * xh).sum(dim=(2, 3)), g64.sum(dim=(2, 3))
        dE = torch.zeros(Sn, 2 * C, dtype=F64)
        for n, s in enumerate(ids):
            dE[s, :C] += bw.to(F64) * sgx[n] + bb.to(F64) * sg[n]
            dE[s, C:] += sg[n]
        sabs = (g64 * xh).abs().sum(dim=(2, 3)).sum(0) + g64.abs().sum(dim=(2, 3)).sum(0)
        _le((outs["cond_dembed"].to(F64) - dE).abs(), 1e-4 * dE.abs() + 8 * U * 2 * torch.cat([sabs, sabs]),
            "cond_instnorm dembed")
        _le((outs["cond_dbn_w"].to(F64) - (ge * sgx).sum(0)).abs(), 1e-4 * (ge * sgx).sum(0).abs() + 8 * U * 2 * sabs,
            "cond_instnorm dbn_w")
        _le((outs["cond_dbn_b"].to(F64) - (ge * sg).sum(0)).abs(), 1e-4 * (ge * sg).sum(0).abs() + 8 * U * 2 * sabs,
            "cond_instnorm dbn_b")
        h64 = h.to(F64)
        ga, ba = (1 + h64[:, :C])[:, :, None, None], h64[:, C:][:, :, None, None]
        _rel_le(RR.nchw64(outs["adain_y"]), ga * xh + ba, 1e-5, "adain fwd")
        _rel_le(RR.nchw64(outs["adain_dx"]), in_bwd(g64 * ga), 1e-4, "adain dx")
        dh = torch.cat([sgx, sg], dim=1)
        habs = torch.cat([(g64 * xh).abs().sum(dim=(2, 3)), g64.abs().sum(dim=(2, 3))], dim=1)
        _le((outs["adain_dh"].to(F64) - dh).abs(), 1e-5 * habs, "adain dh")
        # the sign decisions as the device takes them (fp32 subtract, then multiply, on its own stats), as
        # test_gpu_reductions._check_plain_in does: one flipped decision would move a whole small plane of dy
        st32 = outs["stats"]
        pos = (x.permute(0, 3, 1, 2) - st32[..., 0][:, :, None, None]) * st32[..., 1][:, :, None, None] > 0
        z = xh
        _rel_le(RR.nchw64(outs["skip_d"]), torch.where(pos, z, z * SLOPE), 1e-5, "skip d")
        _rel_le(RR.nchw64(outs["skip_cat"][..., C:]), torch.where(pos, z, torch.zeros_like(z)), 1e-5, "skip cat half")
        assert bool((outs["skip_cat"][..., :C] == 7.0).all()), "skip: the other half of cat was written"
        gz = g64 * torch.where(pos, 1.0, float(SLOPE)) + RR.nchw64(g_s) * pos
        _rel_le(RR.nchw64(outs["skip_dy"]), in_bwd(gz), 1e-4, "skip dy")
        var = (1.0 / rstd ** 2 - EPS)[:, :, 0, 0]
        rm_ref, rv_ref = RR.running_update(mean[:, :, 0, 0], var, rm0.to(F64), rv0.to(F64), H * W, RR.f32(0.1))
        _le((outs["rm"].to(F64) - rm_ref).abs(), 4 * U * rm_ref.abs(), "running_mean")
        unb = H * W / (H * W - 1.0)
        _le((outs["rv"].to(F64) - rv_ref).abs(), 4 * U * (var + EPS).mean(dim=0) * RR.f32(0.1) * unb + 2 * U * rv_ref.abs(),
            "running_var")
        rref = 1.0 / torch.sqrt(outs["rv"].to(F64) + EPS)
        assert bool((outs["st_run"][..., 0] == outs["rm"]).all())
        _le((outs["st_run"][0, :, 1].to(F64) - rref).abs(), 4 * U * rref, "stats_from_running rstd")
    # skip_d / the z sign decisions: the device decides on its own fp32 xhat, so the references above take a relative
    # bar of max |ref| (their tables'), under which a decision within rounding of 0 moves ~1e-7
    run_row(ops, Row(f"cond / adain / skip / running {case}", fn, check))


# ============================================================================================ reductions with partials
GOUT = RR.f32(-0.37)
SCALE = 2.5


def _loss_inputs(npix, cs, cl, seed=0):
    a, b = _g(seed + 1, (1, 1, npix, cs)), _g(seed + 2, (1, 1, npix, cs))
    a[..., cl:], b[..., cl:] = 777.0, -555.0
    b[0, 0, ::7, 0] = a[0, 0, ::7, 0]
    u = torch.rand(1, 1, 1, npix, generator=torch.Generator().manual_seed(seed + 3))
    mask = torch.where(u > 0.3, 0.25 + 0.75 * u, torch.zeros_like(u))
    return a, b, mask


@pytest.mark.parametrize("npix,cs,cl", M.ROW_SHAPES["losses"], ids=lambda v: str(v))
def test_scalar_losses(ops, npix, cs, cl):
    """loss_l1, loss_mse_const, loss_masked_l1, loss_mse (also out= / accumulate and grad=) with their backwards: the
    `part` buffers of vst_loss_part_floats(npix) floats (2 and 257 partials) in poisoned memory."""
    a, b, mask = _loss_inputs(npix, cs, cl)
    g0 = _g(23, (1, 1, npix, cs))

    def fn(ops, dev):
        ad, bd, md, gout = dev(a), dev(b), dev(mask), dev(torch.tensor(GOUT))
        out = {"l1": ops.loss_l1(ad, bd, SCALE, cl), "l1_g": ops.loss_l1_bwd(ad, bd, gout, SCALE, cl),
               "msec": ops.loss_mse_const(ad, 0.9, SCALE, cl), "msec_g": ops.loss_mse_const_bwd(ad, 0.9, gout, SCALE, cl),
               "ml1": ops.loss_masked_l1(ad, bd, md, SCALE, cl), "ml1_g": ops.loss_masked_l1_bwd(ad, bd, md, gout, SCALE, cl),
               "mse": ops.loss_mse(ad, bd, SCALE, cl), "mse_g": ops.loss_mse_bwd(ad, bd, gout, SCALE, cl)}
        acc = dev(torch.tensor(3.25), inout=True)
        assert ops.loss_mse(ad, bd, SCALE, cl, out=acc, accumulate=True) is acc
        over = dev(torch.tensor(float("nan")), inout=True)
        ops.loss_mse(ad, bd, SCALE, cl, out=over)
        gd = dev(g0, inout=True)
        ops.loss_mse_bwd(ad, bd, gout, SCALE, cl, grad=gd)
        out.update(mse_acc=acc, mse_over=over, mse_gacc=gd)
        return out

    def check(outs):
        a64, b64, m64 = RR.nchw64(a), RR.nchw64(b), mask.to(F64)
        refs = {"l1": RR.l1(a64, b64, cl, SCALE, GOUT), "msec": RR.mse_const(a64, RR.f32(0.9), cl, SCALE, GOUT),
                "ml1": RR.masked_l1(a64, b64, m64, cl, SCALE, GOUT), "mse": RR.mse(a64, b64, cl, SCALE, GOUT)}
        for k, (ref, gref) in refs.items():     # test_gpu_reductions._check_loss
            _le(abs(outs[k].item() - ref.item()), (cl + 16) * 2 * U * abs(ref.item()), f"{k} value")
            got = RR.nchw64(outs[k + "_g"])
            _le((got - gref).abs(), 8 * U * gref.abs(), f"{k} grad")
            assert (got[:, cl:] == 0).all()
        ref, gref = refs["mse"]
        _le(abs(outs["mse_acc"].item() - 3.25 - ref.item()), (cl + 16) * 2 * U * abs(ref.item()) + U * (3.25 + abs(ref.item())),
            "mse out= accumulate")
        _le(abs(outs["mse_over"].item() - ref.item()), (cl + 16) * 2 * U * abs(ref.item()), "mse out= overwrite")
        want = RR.nchw64(g0) + gref
        _le((RR.nchw64(outs["mse_gacc"]) - want).abs()[:, :cl], (8 * U * gref.abs() + U * want.abs())[:, :cl],
            "mse_bwd grad= accumulate")
    run_row(ops, Row(f"scalar losses {npix}px cs{cs} cl{cl}", fn, check))


@pytest.mark.parametrize("shape", M.ROW_SHAPES["tv"], ids=lambda s: "x".join(map(str, s)))
def test_loss_tv(ops, shape):
    N, H, W = shape
    img = torch.round(_g(31, (N, H, W, 4), 30.0) * 8) / 8
    img[..., 3] = 123.0

    def fn(ops, dev):
        im = dev(img)
        return {"tv": ops.loss_tv(im, 0.5, 3), "tv_g": ops.loss_tv_bwd(im, dev(torch.tensor(GOUT)), 0.5, 3)}

    def check(outs):      # test_gpu_reductions.test_loss_tv's bars
        i64 = RR.nchw64(img)
        ref = 0.5 * RR.tv(i64, 3)
        _le(abs(outs["tv"].item() - ref.item()), 1e-5 * abs(ref.item()), "tv value")
        gref = 0.5 * GOUT * RR.tv_grad(i64, 3)
        got = RR.nchw64(outs["tv_g"])
        assert (got[:, 3:] == 0).all()
        _le((got - gref).abs(), 1e-5 * gref.abs().max(), "tv grad")
    run_row(ops, Row(f"loss_tv {shape}", fn, check))


@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 129, 67)], ids=["3x64x64", "2x129x67"])
def test_r1_and_bce(ops, shape):
    B, H, W = shape
    gen = torch.Generator().manual_seed(41)
    gimg = torch.randn(B, H, W, 4, generator=gen)
    gimg[..., 3] = 1e3
    nd = 3
    z = 3.0 * torch.randn(B, 4, generator=gen)
    y = torch.randint(0, nd, (B,), generator=gen)

    def fn(ops, dev):
        gd, go = dev(gimg), dev(torch.tensor(0.75))
        zd, yd = dev(z), dev(y)
        return {"r1": ops.r1(gd), "r1_g": ops.r1_bwd(gd, go), "bce": ops.bce_logits(zd, yd, nd, 1),
                "bce_g": ops.bce_logits_bwd(zd, yd, nd, 1, go)}

    def check(outs):      # test_gpu_stargan2_d's references, bar 1e-6
        g64 = gimg[..., :3].double()
        want = 0.5 * g64.pow(2).flatten(1).sum(1).mean(0)
        _le(abs(float(outs["r1"]) - float(want)), 1e-6 * float(want), "r1 value")
        _rel_le(outs["r1_g"][..., :3], 0.75 * g64 / B, 1e-6, "r1 grad")
        assert not bool(outs["r1_g"][..., 3].any())
        v = z.double()[torch.arange(B), y]
        want = (v.clamp(min=0) - v + torch.log1p(torch.exp(-v.abs()))).mean()
        _le(abs(float(outs["bce"]) - float(want)), 1e-6 * abs(float(want)), "bce value")
        wg = torch.zeros(B, 4, dtype=F64)
        wg[torch.arange(B), y] = (torch.sigmoid(v) - 1) / B * 0.75
        _rel_le(outs["bce_g"], wg, 1e-6, "bce grad")
    run_row(ops, Row(f"r1 + bce {shape}", fn, check))


def test_gram(ops):
    """gram (the split-K weight gradient of a 1x1 conv, its slabs per image) and gram_bwd; bar 2e-5 of max |ref|
    (test_gpu_abi.test_gram_and_corr_volume's, the fp32-equivalent bf16x6 arithmetic)."""
    B, C, h, w = 2, 64, 12, 16
    f, dG = _g(21, (B, C, h, w)), _g(22, (B, C, C))

    def fn(ops, dev):
        fn_ = ops.nchw_to_nhwc(dev(f))
        return {"G": ops.gram(fn_), "df": ops.gram_bwd(fn_, dev(dG))}

    def check(outs):
        f64 = f.to(F64).view(B, C, h * w)
        _rel_le(outs["G"], torch.bmm(f64, f64.transpose(1, 2)) / (h * w), 2e-5, "gram")
        df = torch.bmm(dG.to(F64) + dG.to(F64).transpose(1, 2), f64) / (h * w)
        _rel_le(RR.nchw64(outs["df"]), df.view(B, C, h, w), 2e-5, "gram_bwd")
    run_row(ops, Row("gram + gram_bwd", fn, check, math="bf16x6"))


@pytest.mark.parametrize("nhw,cs,cl", M.ROW_SHAPES["channel_sum"])      # test_channel_sum_wide's shapes
def test_channel_sum(ops, nhw, cs, cl):
    x = _g(71, (nhw, cs))

    def fn(ops, dev):
        xd = dev(x)
        acc, over = dev(torch.full((cl,), 0.5), inout=True), dev(torch.full((cl,), float("nan")), inout=True)
        ops.channel_sum(xd, acc, cl, accumulate=True)
        ops.channel_sum(xd, over, cl, accumulate=False)
        return {"acc": acc, "over": over}

    def check(outs):      # test_channel_sum_wide's bar
        s = x[:, :cl].double().sum(0)
        _rel_le(outs["acc"], s + 0.5, 1e-6, "channel_sum accumulate")
        _rel_le(outs["over"], s, 1e-6, "channel_sum overwrite")
    run_row(ops, Row(f"channel_sum {nhw}x{cs} cl{cl}", fn, check))


def test_reflect_fold(ops):
    N, H, W, C, p = 2, 9, 10, 8, 3
    dxp, ad = _g(81, (N, C, H + 2 * p, W + 2 * p)), _g(82, (N, C, H, W))

    def fn(ops, dev):
        return {"dx": ops.reflect_fold(ops.nchw_to_nhwc(dev(dxp)), p, ops.nchw_to_nhwc(dev(ad)))}

    def check(outs):      # at most 4 folded terms and the addend: 5 roundings of the terms' magnitudes
        want = CR.fold2(dxp.to(F64), H, W, p, p, "reflect") + ad.to(F64)
        mag = CR.fold2(dxp.to(F64).abs(), H, W, p, p, "reflect") + ad.to(F64).abs()
        _le((RR.nchw64(outs["dx"]) - want).abs(), 5 * U * mag, "reflect_fold")
    run_row(ops, Row("reflect_fold", fn, check))


# =========================================================================================================== sampling
WARP = (M.ROW_SHAPES["warp"], "sweep")      # every sample within 2.5 px of a border of the grid, on either side of it


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_warp_forward_and_det_backward(ops, masked):
    shape, family = WARP
    x, gout, flow = S.warp_source(*shape), S.warp_gout(*shape), S.make_flow(family, *shape[:3])

    def fn(ops, dev):
        xd, gd, fd = dev(x), dev(gout), dev(flow)
        fwd, bwd = (ops.warp_masked_nhwc, ops.warp_masked_bwd_nhwc) if masked else (ops.warp_nhwc, ops.warp_bwd_nhwc)
        return {"y": fwd(xd, fd, False), "gx": bwd(gd, fd, False)}

    def check(outs):
        S.check_warp_fwd(outs["y"], S.warp_case(shape, family, False, masked), "warp_fwd")
        S.check_warp_bwd(outs["gx"], S.warp_bwd_case(shape, family, False, masked), "warp_bwd_det")
    run_row(ops, Row(f"warp {'masked ' if masked else ''}fwd + deterministic bwd", fn, check))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_warp_backward_atomic(ops, masked):
    shape, family = WARP
    gout, flow = S.warp_gout(*shape), S.make_flow(family, *shape[:3])

    def fn(ops, dev):
        bwd = ops.warp_masked_bwd_nhwc if masked else ops.warp_bwd_nhwc
        return {"gx": bwd(dev(gout), dev(flow), False)}

    def check(outs):      # test_gpu_sampling.test_warp_bwd's
        S.check_warp_bwd(outs["gx"], S.warp_bwd_case(shape, family, False, masked), "warp_bwd")
    run_row(ops, Row(f"warp {'masked ' if masked else ''}bwd atomic", fn, check, atomic=("gx",),
                     cite="csrc/flow.hip:91, warp_bwd_k's atomicAdd into gx"))


def _temporal_row(det):
    shape, cscl = M.ROW_SHAPES["temporal"]
    c = S.temporal_case(shape, cscl, "iid")

    def fn(ops, dev):
        a, b, flow, mask = (dev(c[k]) for k in ("a", "b", "flow", "mask"))
        gout = dev(torch.tensor([c["gout"]]))
        loss = ops.loss_temporal(a, b, flow, mask, c["lam"], c["cl"])
        ga, gb = torch.zeros_like(a), torch.full_like(b, float("nan"))
        ga, gb = dev(ga, inout=True), dev(gb, inout=True)
        ops.loss_temporal_bwd(a, b, flow, mask, gout, ga, gb, c["lam"], c["cl"])
        return {"loss": loss, "ga": ga, "gb": gb}

    def check(outs):
        S.check_temporal(outs["loss"], outs["ga"], outs["gb"], c["ref"], None, None, "temporal")
    if det:
        return Row("loss_temporal + deterministic bwd", fn, check)
    return Row("loss_temporal + atomic bwd", fn, check, atomic=("ga",),
               cite="csrc/flow.hip:127, temporal_k's atomicAdd into ga")


@pytest.mark.parametrize("det", [True, False], ids=["det", "atomic"])
def test_loss_temporal(ops, det):
    run_row(ops, _temporal_row(det))


def _sqdiff_row(det):
    N, H, W, Cs, cl = M.ROW_SHAPES["sqdiff"]
    a, b = _g(91, (N, H, W, Cs)), _g(92, (N, H, W, Cs))
    flow = S.make_flow("sweep", N, H, W)      # samples on either side of every border
    S.assert_off_threshold(flow)              # no validity decision hangs on rounding
    mask = (torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(93)) < 0.8).float()

    def fn(ops, dev):
        ad, bd, fd, md = dev(a), dev(b), dev(flow), dev(mask)
        loss = ops.temporal_sqdiff(ad, bd, fd, md, 50.0, cl)
        ga, gb = dev(torch.zeros_like(a), inout=True), dev(torch.full_like(b, float("nan")), inout=True)
        ops.temporal_sqdiff_bwd(ad, bd, fd, md, dev(torch.tensor(2.0)), ga, gb, 50.0, cl)
        return {"loss": loss, "ga": ga, "gb": gb}

    def check(outs):
        # test_gpu_temporal_style's reference and bars (test_feature_form / test_output_form_with_input_term): the
        # composed form temporal_style_ref.temporal_ref in fp64 with autograd -> loss, d/da, d/db; the loss within
        # 1e-5 relative, each gradient within 1e-5 of max |ref| + 1e-6 (its _close), pad channels exactly 0
        import temporal_style_ref as TS
        a64 = a[..., :cl].permute(0, 3, 1, 2).double().requires_grad_(True)
        b64 = b[..., :cl].permute(0, 3, 1, 2).double().requires_grad_(True)
        loss = TS.temporal_ref(a64, b64, flow.double(), mask.double(), 50.0)
        (2.0 * loss).backward()      # gout = 2: gradients of order 0.5, the bar's 1e-6 floor is not what passes them
        want = float(loss.detach())
        _le(abs(float(outs["loss"]) - want), 1e-5 * abs(want), "temporal_sqdiff loss")
        for name, ref in (("ga", a64.grad), ("gb", b64.grad)):
            got = outs[name][..., :cl].permute(0, 3, 1, 2).double()
            assert float(ref.abs().max()) > 0.1, name        # the gradient is not vacuous
            _le((got - ref).abs().max(), 1e-5 * float(ref.abs().max()) + 1e-6, "temporal_sqdiff " + name)
            assert not bool(outs[name][..., cl:].any()), name + ": pad channels written"
    if det:
        return Row("temporal_sqdiff + deterministic bwd", fn, check)
    return Row("temporal_sqdiff + atomic bwd", fn, check, atomic=("ga",),
               cite="csrc/temporal.hip:128-138, temporal_sq_k's atomicAdd into ga")


@pytest.mark.parametrize("det", [True, False], ids=["det", "atomic"])
def test_temporal_sqdiff(ops, det):
    run_row(ops, _sqdiff_row(det))


def _ruder_row(det):
    import ruder_ref as RU
    N, H, W = M.ROW_SHAPES["ruder"]
    y = _g(970, (N, 3, H, W), 60.0) + 127.0
    img = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(971))
    flow = S.make_flow("sweep", N, H, W)      # samples on either side of every border
    S.assert_off_threshold(flow)
    mask = (torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(972)) < 0.8).float()
    gx, gw = _g(973, (N, 7, H, W)), _g(974, (N, 3, H, W))

    def fn(ops, dev):
        yn, im = ops.nchw_to_nhwc(dev(y)), ops.nchw_to_nhwc(dev(img))
        fd, md = dev(flow), dev(mask)
        x, w = ops.ruder_stack(yn, im, fd, md)
        gy = dev(torch.zeros(N, H, W, 4), inout=True)
        ops.ruder_stack_bwd(ops.nchw_to_nhwc(dev(gx), 8), ops.nchw_to_nhwc(dev(gw)), fd, gy)
        loss = ops.ruder_temporal(w, yn, md, 50.0)
        tw, ty = ops.ruder_temporal_bwd(w, yn, md, dev(torch.tensor(1.7)), 50.0)
        return {"x": x, "w": w, "gy": gy, "loss": loss, "tw": tw, "ty": ty}

    def check(outs):      # test_gpu_ruder's composed fp64 reference, bar 1e-5 of max |ref|
        yr = y.double().clone().requires_grad_(True)
        xr, wr = RU.stack_ref(yr, img.double(), flow.double(), mask.double())
        ((xr * gx.double()).sum() + (wr * gw.double()).sum()).backward()
        _rel_le(outs["x"][..., :7].permute(0, 3, 1, 2), xr.detach(), 1e-5, "ruder_stack x")
        _rel_le(outs["w"][..., :3].permute(0, 3, 1, 2), wr.detach(), 1e-5, "ruder_stack w")
        _rel_le(outs["gy"][..., :3].permute(0, 3, 1, 2), yr.grad, 1e-5, "ruder_stack_bwd")
        w64 = outs["w"][..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
        y2 = y.double().clone().requires_grad_(True)
        lr = RU.temporal_ref(w64, y2, mask.double(), 50.0)
        (lr * 1.7).backward()
        _le(abs(float(outs["loss"]) - float(lr.detach())), 1e-5 * abs(float(lr.detach())), "ruder_temporal loss")
        assert float(outs["w"].abs().max()) > 0.1 and float(outs["gy"].abs().max()) > 0      # the warp is not vacuous
        _rel_le(outs["tw"][..., :3].permute(0, 3, 1, 2), w64.grad, 1e-5, "ruder_temporal d/dw")
        _rel_le(outs["ty"][..., :3].permute(0, 3, 1, 2), y2.grad, 1e-5, "ruder_temporal d/dy")
    if det:
        return Row("ruder_stack / _bwd / ruder_temporal, deterministic", fn, check)
    return Row("ruder_stack / _bwd / ruder_temporal, atomic", fn, check, atomic=("gy",),
               cite="csrc/ruder.hip:134-136, ruder_stack_bwd_k's atomicAdd into gy_prev")


@pytest.mark.parametrize("det", [True, False], ids=["det", "atomic"])
def test_ruder(ops, det):
    run_row(ops, _ruder_row(det))


def test_fbcheck(ops):
    shape = (3, 17, 19)
    ff, bf = S.fbc_flows("quarter", shape)

    def check(outs):
        assert torch.equal(outs["mask"], S.fbc_ref(ff, bf)), "fbcheck != reference"
    run_row(ops, Row("fbcheck", lambda ops, dev: {"mask": ops.fbcheck(dev(ff), dev(bf))}, check))


def test_corr_pyramid_and_lookup(ops):
    """corr_pyramid in place on a placed buffer whose level 0 holds the data and whose upper levels hold junk, then
    corr_lookup with coordinates outside the map."""
    P, H2, W2, ld0, levels = M.ROW_SHAPES["corr_pyramid"]
    buf = S.pyramid_buffer(P, H2, W2, ld0, levels, fill=False)
    c = S.lookup_case(*[lc for lc in S.LOOKUP_CASES if lc[4] == "outside"][0])
    B, H1, W1, h2, w2, l0, lv, r, cs = c["geo"]

    def fn(ops, dev):
        d = dev(buf, inout=True)
        ops.corr_pyramid(d, P, H2, W2, ld0, levels)
        out = ops.corr_lookup(dev(c["buf"]), dev(c["coords"]), B, H1, W1, h2, w2, l0, lv, r,
                              None if cs == ops.cpad(lv * (2 * r + 1) ** 2) else cs)
        return {"pyr": d, "look": out}

    def check(outs):
        got = outs["pyr"]
        assert torch.equal(got[:P * ld0], buf[:P * ld0])
        lvl = S.pyramid_levels(got, P, H2, W2, ld0, levels)
        for l, (ref, bound) in enumerate(S.pyramid_ref(buf, P, H2, W2, ld0, levels), 1):
            S.le((lvl[l].double() - ref).abs(), bound, f"corr_pyramid level {l}", "corr_pyramid")
        S.check_lookup(outs["look"], c["tight"], c["indep"], lv, r, "corr_lookup", True)
    run_row(ops, Row("corr_pyramid + corr_lookup (outside)", fn, check))


def test_altcorr(ops):
    """altcorr_pyramid / altcorr_lookup with coordinates outside the map, against the all-pairs form in fp64:
    <f1, bilinear(level l of f2)> / sqrt(D) = bilinear lookup of the all-pairs volume (test_gpu_altcorr compares the
    two device forms; here fp64 decides), bar 1e-5 of max |ref|."""
    B, H, W, D, levels, r = M.ROW_SHAPES["altcorr"]
    f1, f2 = _g(61, (B, D, H, W)), _g(62, (B, D, H, W))
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    coords = torch.stack([gx, gy])[None] + _g(63, (B, 2, H, W), 4.0)      # several samples leave the map

    def fn(ops, dev):
        n1, n2 = ops.nchw_to_nhwc(dev(f1)), ops.nchw_to_nhwc(dev(f2))
        # the pooled levels' buffer, NaN before the call: a float the pyramid kernel leaves out reaches the lookup
        pyr = dev(torch.full((ops.altcorr_pyramid_floats(B, H, W, D, levels),), float("nan")), inout=True)
        ops.altcorr_pyramid(n2, pyr, levels)
        return {"out": ops.altcorr_lookup(n1, n2, pyr, dev(coords), D, levels, r)}

    def check(outs):
        K = 2 * r + 1
        f1d, lvl = f1.to(F64), f2.to(F64)
        want = torch.zeros(B, H, W, levels * K * K, dtype=F64)
        for l in range(levels):
            if l:
                lvl = F.avg_pool2d(lvl, 2)
            h, w = lvl.shape[2:]
            for i in range(K):
                for j in range(K):
                    # channel l K^2 + i K + j samples x + (i - r), y + (j - r) (corr.py's transposed window)
                    px = coords[:, 0].to(F64) / 2 ** l + (i - r)
                    py = coords[:, 1].to(F64) / 2 ** l + (j - r)
                    grid = torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], dim=-1)
                    s = F.grid_sample(lvl, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
                    want[..., l * K * K + i * K + j] = (f1d * s).sum(1) / D ** 0.5
        got = outs["out"][..., :levels * K * K]
        _rel_le(got, want, 1e-5, "altcorr_lookup vs fp64")
        assert not bool(outs["out"][..., levels * K * K:].any())
    run_row(ops, Row("altcorr_pyramid + altcorr_lookup", fn, check))


def test_raft_upsample(ops):
    B, h, w, mcs, spike = 1, 3, 5, 580, True
    coords1, mask = S.upsample_inputs(B, h, w, mcs, spike)

    def check(outs):
        ref, bound = S.upsample_ref(coords1, mask)
        S.le((outs["up"].double() - ref).abs(), bound, "raft_upsample", "raft_upsample")
    run_row(ops, Row("raft_upsample", lambda ops, dev: {"up": ops.raft_upsample(dev(coords1), dev(mask))}, check))


# =============================================================================================================== glue
@pytest.mark.parametrize("mode", ["same", "pool", "up"])
def test_merge_and_avgpool(ops, mode):
    shape = (2, 6, 10, 8)
    import stargan2_ref as S2
    N, H, W, C = shape
    bs = {"same": shape, "pool": (N, 2 * H, 2 * W, C), "up": (N, H // 2, W // 2, C)}[mode]
    a, b, g = _g(37, shape), _g(38, bs), _g(39, shape)
    x = _g(31, (N, 2 * H, 2 * W, C))
    s = 2 ** -0.5

    def fn(ops, dev):
        out = ops.merge(dev(a), dev(b), mode, s)
        ga, gb = ops.merge_bwd(dev(g), mode, s)
        return {"out": out, "ga": ga, "gb": gb, "pool": ops.avgpool2(dev(x)), "pool_g": ops.avgpool2_bwd(dev(g))}

    def check(outs):      # test_gpu_stargan2's references, bar 1e-6
        rs = float(np.float32(s))
        _rel_le(RR.nchw64(outs["out"]), S2.merge_fwd(RR.nchw64(a), RR.nchw64(b), mode, rs), 1e-6, "merge fwd")
        ra, rb = S2.merge_bwd(RR.nchw64(g), mode, rs)
        _rel_le(RR.nchw64(outs["ga"]), ra, 1e-6, "merge ga")
        _rel_le(RR.nchw64(outs["gb"]), rb, 1e-6, "merge gb")
        _rel_le(RR.nchw64(outs["pool"]), F.avg_pool2d(RR.nchw64(x), 2), 1e-6, "avgpool2")
        _rel_le(RR.nchw64(outs["pool_g"]), S2.merge_bwd(RR.nchw64(g), "pool", 1.0)[1], 1e-6, "avgpool2_bwd")
    run_row(ops, Row(f"merge {mode} + avgpool2", fn, check))


def test_fc2_unpack_and_u8_image(ops):
    B, H, W = 2, 5, 7
    from oracle import formats_ref
    raw = torch.rand(B, H, W, 9, generator=torch.Generator().manual_seed(51))
    raw[..., 6:] = _g(53, (B, H, W, 3), 2.0)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(52), dtype=torch.uint8)

    def fn(ops, dev):
        i1, i2, mask, flow = ops.fc2_unpack(dev(raw))
        return {"i1": i1, "i2": i2, "mask": mask, "flow": flow, "img": ops.u8_image_to_nhwc4(dev(u8))}

    def check(outs):
        for n in range(B):      # test_formats.test_fc2_unpack_bit_exact's references, bit for bit
            r1, r2, rm, rf = formats_ref.fc2_sample(raw[n].numpy())
            for got, ref in ((outs["i1"], r1), (outs["i2"], r2)):
                assert torch.equal(got[n][..., :3].permute(2, 0, 1), ref) and not bool(got[n][..., 3].any())
            assert torch.equal(outs["mask"][n], rm) and torch.equal(outs["flow"][n], rf)
            assert torch.equal(outs["img"][n][..., :3].permute(2, 0, 1), formats_ref.u8_image(u8[n].numpy()))
        assert not bool(outs["img"][..., 3].any())
    run_row(ops, Row("fc2_unpack + u8_image_to_nhwc4", fn, check))


# ======================================================================================================== whole steps
def _step_bits(t):
    return _bits(t.detach().cpu())


def _four_steps(ops, build_and_step, label):
    """One train step (or forward) plain and under each fill, in deterministic mode with the same seeds: the returned
    tensors (losses, parameter gradients, updated parameters) bit-identical, every allocation of the step checked."""
    prev = ops.set_deterministic(True)
    res = {}
    try:
        for fill in (None,) + M.FILLS:
            torch.manual_seed(1234)
            if fill is None:
                out = build_and_step(_plain)
                torch.cuda.synchronize()
                res[None] = {k: _step_bits(v) for k, v in out.items()}
                continue
            with M.MemGuard(fill) as mg, _stop_on_device_fault():
                out = build_and_step(mg.place)
                fails = mg.failures() + ["not 256-byte aligned: " + d for d in mg.misaligned(256)]
                res[fill] = {k: _step_bits(v) for k, v in out.items()}
                note, passed = mg.summary(), list(mg.passthrough)
                n_alloc, n_bytes = sum(1 for a in mg.allocs if a.kind != "place"), mg.bytes
                mg.drop()
            assert not fails, f"{label} [fill {M.FILL_NAMES[fill]}]: " + "; ".join(fails[:6])
            assert not passed, f"{label}: allocations that bypassed the instrument: " + "; ".join(passed[:6])
        print(f"  {label}: exact; {note}")
        ROWS_SEEN.append((label, "exact", n_alloc, n_bytes))
        for fill in M.FILLS:
            assert res[fill].keys() == res[None].keys()
            bad = [k for k in res[None] if not torch.equal(res[fill][k], res[None][k])]
            assert not bad, f"{label}: differs from the plain run under fill {M.FILL_NAMES[fill]}: {bad[:8]}"
    finally:
        ops.set_deterministic(prev)
    return res


def test_cyclegan_golden_step(ops, golden):
    """The small CycleGANCon golden step of test_gpu_models (_load_step_model): losses, every parameter gradient and
    every updated parameter bit-identical across the plain run and the three fills; the 0xFF run's losses within
    test_train_step_vs_reference_golden's step-0 tolerance (1e-3 relative) of the reference's."""
    import gbvst
    from test_gpu_models import _load_step_model
    g = golden("step_small")
    names = [str(n) for n in g["loss_names"]]
    losses = {}

    def step(dev):
        m, data = _load_step_model(gbvst, g)
        m.set_input_fc2(data)
        m.optimize_parameters()
        torch.cuda.synchronize()
        cur = m.get_current_losses()
        out = {"loss_" + n: torch.tensor(cur[n], dtype=torch.float64) for n in names}
        losses[len(losses)] = [cur[n] for n in names]
        for net in ("G_A", "G_B", "D_A", "D_B"):
            for k, p in getattr(m, "net" + net).named_parameters():
                out[f"{net}.{k}"] = p
                if p.grad is not None:
                    out[f"{net}.{k}.grad"] = p.grad
        return out
    _four_steps(ops, step, "CycleGANCon golden step")
    got = np.array(losses[2])       # plain, 0x00, 0xFF, 0x7F
    rel = np.abs(got - g["losses"][0]) / np.abs(g["losses"][0])
    assert rel.max() <= 1e-3, rel


def _params_and_grads(out, net, tag):
    for k, p in net.named_parameters():
        out[f"{tag}.{k}"] = p
        if p.grad is not None:
            out[f"{tag}.{k}.grad"] = p.grad


def test_johnson_step(ops, golden):
    """The Johnson fast-style step of test_gpu_style (style_small golden): losses, gradients and the Adam update
    bit-identical across the four runs; the 0xFF run's losses within the golden's 1e-3."""
    import gbvst
    from gbvst import faststyle
    from test_gpu_style import _fsn, _vgg
    g = golden("style_small")
    emph = tuple(float(v) for v in g["js_emph"])
    losses = []

    def step(dev):
        model, vgg = _fsn(gbvst, 540), _vgg(gbvst, "vgg16", 550)
        J = faststyle.Johnson([torch.from_numpy(g["js_style"])], emphasis=emph, lr=1e-3, batch_sz=2, device=DEV, vgg=vgg,
                              model=model)
        x = ops.nchw_to_nhwc(dev(torch.from_numpy(g["js_img"])))
        J.adam.zero_grad()
        loss, cl, sl, tv, _ = J.losses_nhwc(x)
        loss.backward()
        out = {"loss": loss, "content": cl, "style": sl, "tv": tv}
        losses.append([float(v) for v in (loss, cl, sl, tv)])
        _params_and_grads(out, model, "fsn")
        out = {k: v.detach().clone() for k, v in out.items()}
        J.adam.step()
        torch.cuda.synchronize()
        out.update({"after." + k: p.detach() for k, p in model.named_parameters()})
        return out
    _four_steps(ops, step, "Johnson fast-style step")
    rel = np.abs(np.array(losses[2]) - g["js_losses"][0]) / np.abs(g["js_losses"][0])
    assert rel.max() < 1e-3, rel


def test_ruder_step(ops):
    """The Ruder recurrent step of test_gpu_ruder (3 frames, roll); the 0xFF run's losses within 1e-3 of the
    reference run's."""
    import ruder_ref as RU
    from test_gpu_ruder import _dev_inputs, _trainer
    losses = []

    def step(dev):
        T = _trainer(RU.EMPH)
        T.adam.zero_grad()
        out_ = T.losses_nhwc(*_dev_inputs(3), True)
        out_[0].backward()
        out = {f"loss{i}": v for i, v in enumerate(out_[:-1])}
        out["styled"] = out_[-1]
        losses.append([float(v.detach()) for v in out_[:-1]])
        _params_and_grads(out, T.model, "fsn")
        out = {k: v.detach().clone() for k, v in out.items()}
        T.adam.step()
        torch.cuda.synchronize()
        out.update({"after." + k: p.detach() for k, p in T.model.named_parameters()})
        return out
    _four_steps(ops, step, "Ruder recurrent step, 3 frames")
    ref = np.array(RU.reference_run(3, RU.EMPH, True)[0][0])
    rel = np.abs(np.array(losses[2]) - ref) / np.abs(ref)
    assert rel.max() < 1e-3, rel


def test_stargan2_discriminator_step(ops, golden):
    """The StarGAN v2 discriminator step of test_gpu_stargan2_d (R1 through the twice-differentiable D, then Adam);
    the 0xFF run's real and reg terms within the fixture's 1e-4 (test_compute_d_loss_end_to_end's)."""
    import copy
    import types
    from gbvst import stargan2 as SG
    from test_gpu_stargan2_d import DR, _case
    g = golden("stargan2_dstep")
    _, (x_real, z_trg, _), nets0 = _case()
    parts = []

    def step(dev):
        nets = types.SimpleNamespace(**{k: copy.deepcopy(v) for k, v in vars(nets0).items()})
        args = types.SimpleNamespace(lambda_reg=DR.LAMBDA_REG, lr=1e-4, beta1=0.0, beta2=0.99, weight_decay=1e-4)
        trainer = SG.DiscriminatorTrainer(nets, args)
        y_org, y_trg = torch.tensor(DR.Y_ORG, device=DEV), torch.tensor(DR.Y_TRG, device=DEV)
        ls = trainer.d_step(dev(torch.from_numpy(x_real)), y_org, y_trg, z_trg=dev(torch.from_numpy(z_trg)))
        torch.cuda.synchronize()
        parts.append(ls)
        out = {k: torch.tensor(float(ls[k]), dtype=torch.float64) for k in ("real", "fake", "reg")}
        _params_and_grads(out, nets.discriminator, "D")
        return out
    _four_steps(ops, step, "StarGAN v2 discriminator step")
    for n in ("real", "reg"):
        want = float(g["latent_" + n])
        assert abs(float(parts[2][n]) - want) <= 1e-4 * abs(want), (n, float(parts[2][n]), want)


def test_raft_forward(ops, golden):
    """One RAFT forward at the smallest golden size (the buffers raft.py and raft_corr.py allocate): the low-resolution
    and upsampled flows bit-identical across the four runs, the 0xFF run within the golden's tolerance."""
    from test_gpu_raft import _model
    g = golden("raft_small")
    pads = tuple(int(v) for v in g["pads"])

    def fwd(dev):
        m, _ = _model()
        with torch.no_grad():
            low, up = m(dev(torch.from_numpy(g["img1"])), dev(torch.from_numpy(g["img2"])), iters=6, test_mode=True,
                        pads=pads)
        return {"low": low, "up": up}
    res = _four_steps(ops, fwd, "RAFT forward (raft_small golden)")
    up = res[0xFF]["up"].view(torch.float32).double()
    ref = torch.from_numpy(g["up6"]).double()
    assert float((up - ref).abs().max() / ref.abs().max()) < 1e-3      # test_raft_vs_reference_golden's


# ========================================================================================= the ws_bytes argument
def _guarded_bytes(n, fill=0x7F):
    """A device window of exactly n bytes with GUARD bytes of `fill` on either side: (window pointer, whole buffer)."""
    buf = torch.full((n + 2 * M.GUARD,), fill, dtype=torch.uint8, device=DEV)
    return buf.data_ptr() + M.GUARD, buf


def _guards_ok(buf, n, fill=0x7F):
    return bool((buf[:M.GUARD] == fill).all()) and bool((buf[M.GUARD + n:] == fill).all())


def _ws_cases(ops):
    """(entry, queried bytes, call(ws_ptr, ws_bytes) -> rc, outputs [(buffer, bytes)]) for every entry point with a
    ws_bytes parameter, at mem_guard.WS_SHAPES; every output is a guarded 0x7F-filled window.  Each call's arguments
    are tuples built HERE (entry() below), never names read when the call is made: the sections reuse N, H, W, ..."""
    import gbvst
    _lib = gbvst._lib
    lib = _lib.load()
    C, MATH, SH = _lib.CONSTANTS, _lib.MATH_MODES, M.WS_SHAPES
    x6, f32m = MATH["bf16x6"], MATH["fp32"]
    zero, refl = C["VST_PAD_ZERO"], C["VST_PAD_REFLECT"]
    s = torch.cuda.current_stream().cuda_stream
    keep, cases = [], []

    def entry(name, nb, fn, pre, post, outs):
        pre, post, outs = tuple(pre), tuple(post), list(outs)
        assert all(isinstance(v, (int, float, type(None))) or hasattr(v, "_obj") for v in pre + post), name
        cases.append((name, int(nb), lambda w_, n_: fn(*pre, w_, n_, *post), outs))

    def out(nfloats):
        p, buf = _guarded_bytes(4 * nfloats)
        return p, (buf, 4 * nfloats)

    def dev(t):
        keep.append(t.to(DEV).contiguous())
        return keep[-1]

    def ptr(t):
        keep.append(t)
        return t.data_ptr()

    # ---- vst_conv2d_fwd_ex: the split-K slabs; the _desc forward and weight gradient at the same shape
    N, H, W, Cx, Cop, R, S_, st, ph, pw = SH["fwd_splitk"]
    x, wt = dev(_g(1, (N, H, W, Cx))), dev(_g(2, (Cop, Cx, R, S_), 0.1))
    wp = ops.weight_pack(wt, ops.PACK_OK)
    yp, yo = out(N * H * W * Cop)
    entry("vst_conv2d_fwd_ex split-K", lib.vst_conv2d_fwd_ex_ws_bytes(N, H, W, Cx, Cop, R, S_, st, ph, pw, refl, x6, Cop),
          lib.vst_conv2d_fwd_ex, (ptr(x), ptr(wp), ptr(wp.vst_split), None, yp, N, H, W, Cx, Cop, R, S_, st, ph, pw, refl,
                                  0, 0.0, x6, Cop, None, None), (s,), [yo])
    d = M.conv_desc(_lib, x6, refl, **SH["desc"])
    keep.append(d)
    ydp, ydo = out(N * H * W * Cop)
    entry("vst_conv2d_fwd_desc", lib.vst_workspace_size(ctypes.byref(d), 0), lib.vst_conv2d_fwd_desc,
          (ctypes.byref(d), ptr(x), ptr(wp), ptr(wp.vst_split), None, ydp, None, None), (s,), [ydo])
    dyd = dev(_g(3, (N, H, W, Cop)))
    dwp, dwo = out(Cop * Cx * R * S_)
    entry("vst_conv2d_wgrad_desc", lib.vst_workspace_size(ctypes.byref(d), 2), lib.vst_conv2d_wgrad_desc,
          (ctypes.byref(d), ptr(x), ptr(dyd), dwp, Cop, Cx, 0), (s,), [dwo])

    # ---- the _desc data gradient of a transposed conv (a forward conv over its output gradient)
    t = SH["desc_T"]
    dT = M.conv_desc(_lib, x6, zero, **t)
    keep.append(dT)
    gyT = dev(_g(4, (t["N"], 2 * t["H"], 2 * t["W"], t["K"])))
    wT = ops.weight_pack(dev(_g(5, (t["C"], t["K"], 3, 3), 0.1)), ops.PACK_OK)
    dxp, dxo = out(t["N"] * t["H"] * t["W"] * t["C"])
    entry("vst_conv2d_dgrad_desc", lib.vst_workspace_size(ctypes.byref(dT), 1), lib.vst_conv2d_dgrad_desc,
          (ctypes.byref(dT), ptr(gyT), ptr(wT), ptr(wT.vst_split), dxp), (s,), [dxo])

    # ---- vst_conv2d_fwd_ex: the PatchGAN head's tap GEMM
    N, H, W, Cx, Cop, R, S_, st, ph, pw = SH["fwd_head"]
    hx = dev(_g(6, (N, H, W, Cx)))
    hwp = ops.weight_pack(dev(_g(7, (1, Cx, R, S_), 0.1)), ops.PACK_OK)
    Ho, Wo = H + 2 * ph - R + 1, W + 2 * pw - S_ + 1
    hyp, hyo = out(N * Ho * Wo * 4)
    entry("vst_conv2d_fwd_ex head", lib.vst_conv2d_fwd_ex_ws_bytes(N, H, W, Cx, 4, R, S_, 1, ph, pw, zero, f32m, 1),
          lib.vst_conv2d_fwd_ex, (ptr(hx), ptr(hwp), None, None, hyp, N, H, W, Cx, 4, R, S_, 1, ph, pw, zero, 0, 0.0, f32m,
                                  1, None, None), (s,), [hyo])

    # ---- vst_conv2d_wgrad / _pre / _bias
    N, H, W, Cx, Ho, Wo, Cyp, R, S_, st = SH["wgrad"]
    wx_, wdy = dev(_g(8, (N, H, W, Cx))), dev(_g(9, (N, Ho, Wo, Cyp)))
    nbg = lib.vst_conv2d_wgrad_ws_bytes(*SH["wgrad"])
    tail = (N, H, W, Cx, Ho, Wo, Cyp, R, S_, st, 1, refl, Cyp, Cx, Cx * R * S_, R * S_, 0, f32m, s)
    p_, o_ = out(Cyp * Cx * R * S_)
    entry("vst_conv2d_wgrad", nbg, lib.vst_conv2d_wgrad, (ptr(wx_), ptr(wdy), p_), tail, [o_])
    p_, o_ = out(Cyp * Cx * R * S_)
    entry("vst_conv2d_wgrad_pre", nbg, lib.vst_conv2d_wgrad_pre, (ptr(wx_), None, ptr(wdy), None, p_), tail, [o_])
    N, H, W, Cx, Ho, Wo, Cyp, R, S_, st = SH["wgrad_image"]
    ix, idy = dev(_g(10, (N, H, W, Cx))), dev(_g(11, (N, Ho, Wo, Cyp)))
    ip, io = out(Cyp * 3 * R * S_)
    ibp, ibo = out(Cyp)
    entry("vst_conv2d_wgrad_bias", lib.vst_conv2d_wgrad_ws_bytes(*SH["wgrad_image"]), lib.vst_conv2d_wgrad_bias,
          (ptr(ix), ptr(idy), ip, ibp), (N, H, W, Cx, Ho, Wo, Cyp, R, S_, st, 1, zero, Cyp, 3, 3 * R * S_, R * S_, 0, f32m, s),
          [io, ibo])

    # ---- vst_conv2d_wgrad_nhwc (dy as its NHWC planes) / _nhwc_f32
    geom = SH["wgrad_nhwc"]
    N, H, W, Cx, Ho, Wo, Cyp, R, S_, st, pad = geom
    nx, ndy = dev(_g(12, (N, H, W, Cx))), dev(_g(13, (N, Ho, Wo, Cyp)))
    apl = dev(torch.stack([p.to(torch.bfloat16).reshape(-1) for p in CR.split3(ndy.cpu())]))
    for name, dyp in (("vst_conv2d_wgrad_nhwc", apl), ("vst_conv2d_wgrad_nhwc_f32", ndy)):
        p_, o_ = out(Cyp * Cx * R * S_)
        entry(name, getattr(lib, name + "_ws_bytes")(*geom, x6), getattr(lib, name), (ptr(nx), ptr(dyp), p_),
              geom + (refl, Cyp, Cx, Cx * R * S_, R * S_, 0, x6, s), [o_])

    # ---- the reflect-border data gradients
    N, H, W, Cy, Cx = SH["dgrad_refl"]
    rdy = dev(_g(14, (N, H, W, Cy)))
    rw = ops.weight_pack(dev(_g(15, (Cy, Cx, 3, 3), 0.1)), ops.PACK_IKF)
    rp, ro = out(N * H * W * Cx)
    entry("vst_conv2d_dgrad_refl", lib.vst_conv2d_dgrad_refl_ws_bytes(N, H, W, Cy, Cx, x6), lib.vst_conv2d_dgrad_refl,
          (ptr(rdy), ptr(rw.vst_split), None, rp), (N, H, W, Cy, Cx, x6, s), [ro])
    N, H, W, Cy, Cx = SH["dgrad_refl_in"]
    edy, eyin = dev(_g(16, (N, H, W, Cy))), dev(_g(17, (N, H, W, Cx)))
    ew = ops.weight_pack(dev(_g(18, (Cy, Cx, 3, 3), 0.1)), ops.PACK_IKF)
    est = ops.instnorm_stats(eyin)
    nbe = lib.vst_conv2d_dgrad_refl_in_epi_ws_bytes(N, H, W, Cy, Cx, x6)
    relu = ops.ACT["relu"]
    gp, go = out(N * H * W * Cx)
    entry("vst_conv2d_dgrad_refl_epi_part", nbe, lib.vst_conv2d_dgrad_refl_epi_part,
          (ptr(edy), None, ptr(ew.vst_split), None, gp, ptr(eyin), ptr(est)), (N, H, W, Cy, Cx, relu, 0.0, x6, s), [go])
    gp2, go2 = out(N * H * W * Cx)
    dp2, do2 = out(N * H * W * Cx)
    entry("vst_conv2d_dgrad_refl_in_epi", nbe, lib.vst_conv2d_dgrad_refl_in_epi,
          (ptr(edy), ptr(ew.vst_split), None, gp2, ptr(eyin), ptr(est), dp2, None),
          (N, H, W, Cy, Cx, relu, 0.0, 1, None, 0, x6, s), [go2, do2])

    # ---- vst_warp_bwd_input_det (gx is accumulated into: a zeroed buffer, its guards checked as zeros)
    N, H, W = SH["warp_det"]
    wg, wf = dev(_g(19, (N, H, W, 4))), dev(_g(20, (N, 2, H, W), 2.0))
    wgx = torch.zeros(N * H * W * 4 + 2 * M.GUARD // 4, device=DEV)
    entry("vst_warp_bwd_input_det", lib.vst_warp_bwd_det_ws_bytes(N, H, W), lib.vst_warp_bwd_input_det,
          (ptr(wg), ptr(wf), ptr(wgx) + M.GUARD), (N, H, W, 4, 4, 0, 0, 0, s), [(wgx, None)])

    # ---- vst_tap_wgrad_swap / _db
    N, H, W, Ci, R = SH["tap_swap"]
    tdy, tx = dev(_g(21, (N, H, W, 4))), dev(_g(22, (N, H, W, Ci)))
    tst = torch.zeros((N, Ci, 2), device=DEV)
    tst[..., 1] = 1.0
    _, xpl = ops.instnorm_act_fwd(tx, tst, "none", xpl=((R - 1) // 2, "reflect", ops.tap_swap_geom(W, R)[0]))
    assert tuple(xpl.shape) == (3, Ci, int(lib.vst_tap_wgrad_swap_ld(N, H, W, R)))
    nbt = lib.vst_tap_wgrad_swap_ws_bytes(N, H, W, Ci, R)
    p_, o_ = out(3 * Ci * R * R)
    entry("vst_tap_wgrad_swap", nbt, lib.vst_tap_wgrad_swap, (ptr(tdy), ptr(xpl), p_), (N, H, W, Ci, R, 3, 0, x6, s), [o_])
    p_, o_ = out(3 * Ci * R * R)
    bp, bo = out(4)
    entry("vst_tap_wgrad_swap_db", nbt, lib.vst_tap_wgrad_swap_db, (ptr(tdy), ptr(xpl), p_, bp),
          (N, H, W, Ci, R, 3, 0, x6, s), [o_, bo])

    # ---- vst_gram, vst_corr_volume
    HW, Cg = SH["gram"]
    gf = dev(_g(23, (2, HW, Cg)))
    Gp, Go = out(2 * Cg * Cg)
    entry("vst_gram", lib.vst_gram_ws_bytes(HW, Cg), lib.vst_gram, (ptr(gf), Gp, 2, HW, Cg), (x6, s), [Go])
    B, H, W, Dp = SH["corr_volume"]
    c1, c2 = dev(_g(24, (B, H, W, Dp))), dev(_g(25, (B, H, W, Dp)))
    sq = dev(torch.full((Dp,), float(Dp) ** 0.5))
    levels, ld0 = 2, (H * W + 3) // 4 * 4
    pp, po = out(int(lib.vst_corr_pyramid_floats(B * H * W, H, W, ld0, levels)))
    entry("vst_corr_volume", lib.vst_corr_volume_ws_bytes(B, H, W, Dp), lib.vst_corr_volume,
          (ptr(c1), ptr(c2), pp, B, H, W, Dp, Dp, ptr(sq), levels), (x6, s), [po])
    return cases, keep


def test_ws_bytes_is_honoured(ops):
    """Every entry point with a ws_bytes parameter, through ctypes as test_gpu_abi.py calls them: with ws_bytes one
    below the query the call returns VST_EINVAL and launches nothing (the outputs still hold their fill) — the pointer
    it received was a guarded buffer of the FULL queried size, so nothing could be written outside owned memory
    whatever the entry did; with exactly the queried size it succeeds and stays inside the buffer byte-exact (the guard
    begins at byte `queried`, not at the next multiple of 4)."""
    import gbvst
    einval = gbvst._lib.CONSTANTS["VST_EINVAL"]
    cases, keep = _ws_cases(ops)
    seen, refused = set(), []
    for entry, nb, call, outs in cases:
        assert nb > 1, (entry, nb)
        seen.add(entry.split()[0])
        wsp, wsbuf = _guarded_bytes(nb)
        with _stop_on_device_fault():
            rc = call(wsp, nb - 1)
            torch.cuda.synchronize()
        if rc != einval:        # every entry is tried before the assertion names them all
            refused.append(f"{entry}: ws_bytes = query - 1 returned {rc}, not VST_EINVAL ({einval})")
            assert _guards_ok(wsbuf, nb), f"{entry}: wrote outside the workspace"
            continue
        assert bool((wsbuf == 0x7F).all()), f"{entry}: the workspace was written although the call was refused"
        for buf, n in outs:
            if n is not None:
                assert bool((buf == 0x7F).all()), f"{entry}: an output was written although the call was refused"
            else:
                assert not bool(buf.any()), f"{entry}: an output was written although the call was refused"
        with _stop_on_device_fault():
            rc = call(wsp, nb)
            torch.cuda.synchronize()
        assert rc == 0, f"{entry}: the exact queried size was refused (rc {rc})"
        assert _guards_ok(wsbuf, nb), f"{entry}: wrote outside a workspace of exactly the queried {nb} bytes"
        for buf, n in outs:
            if n is not None:
                assert _guards_ok(buf, n), f"{entry}: wrote outside an output"
                assert not bool((buf[M.GUARD:M.GUARD + n].view(torch.int32) == 0x7F7F7F7F).all()), \
                    f"{entry}: the output was not written by the successful call"
            else:
                g4 = M.GUARD // 4
                assert not bool(buf[:g4].any()) and not bool(buf[-g4:].any()), f"{entry}: wrote outside an output"
        print(f"  {entry}: {nb} bytes; query - 1 -> VST_EINVAL, exact size ok and byte-exact")
    assert not refused, "\n".join(refused)
    assert seen == set(M.WS_BYTES_ENTRIES), seen ^ set(M.WS_BYTES_ENTRIES)
