"""GPU parity of the StarGAN v2 networks (gbvst.stargan2) and of the kernels under them.

Op level, against the fp64 references of tests/stargan2_ref.py: vst_adain_fwd / _bwd over the InstanceNorm geometries
of reduction_ref.IN_CASE that change a code path plus the generator's widest norm (2, 16, 16, 512), with act none and
lrelu, with and without dbias, each run twice for bit-equality; vst_avgpool2_* and vst_merge_* in all three modes
with sentinel-guarded buffers.  Bars, relative to max|ref| of the tensor (those of test_gpu_reductions /
test_gpu_unet): forward 1e-5, dx 1e-4, each dh / dbias entry within 1e-5 of the sum of the absolute values of the
terms it sums; pooling and merge forward 1e-6 (one or two fp32 roundings per element).  Every figure is printed before
it is asserted.

Net level: the four networks against the fixture the reference's own modules produced
(tests/golden/stargan2_small.npz) and against the fp64 reference: output 1e-4 of max|ref|; the input gradients
(norm-wise) and the parameter gradients (max-relative) within 1e-3 or within the reference's own movement under a
1e-6 relative perturbation of its weights (gradients are a discontinuous function of the forward values; the band is
computed only when the tight bound misses).  Inference: StyleGuided through sintel_eval.evaluate_video against the
same TCL computed from the CPU reference's frames, at test_gpu_sintel.py's tolerance.
"""
import functools
import types

import numpy as np
import pytest
import torch

import reduction_ref as R
import stargan2_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SLOPE = R.f32(0.2)
RSQRT2 = R.f32(2 ** -0.5)
GEOMS = {k: R.IN_CASE[k][1] for k in ("tiny_hw", "c4", "c8", "tail_cpb4", "fold4_unrolled", "lp18", "part_unrolled_6")}
GEOMS["gen_widest"] = (2, 16, 16, 512)
SENTINEL = -12345.678
PAD = 64    # sentinel floats on either side of a guarded buffer


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _rel(got, ref):
    got, ref = _np(got), _np(ref)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def _nrel(got, ref):
    got, ref = _np(got), _np(ref)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


# ================================================================================== op level
@functools.lru_cache(maxsize=None)
def _op_data(geom):
    """fp32 NHWC x, g, h [N, 2C] of a geometry and the fp64 references.  The seed is the first whose reference
    pre-activation z keeps min|z| / max|z| >= 1e-6, so no lrelu decision hangs on fp32 rounding.  part_unrolled_6
    has 2.8 M elements, and no seed keeps that many values clear of a crossing that lies inside the data: there the
    values are moved away from their mean by a gap (x = sign(r) (2 |r| + 0.2)) and the shift beta is kept small
    (0.005 N(0, 1), with 1 + gamma >= 0.5), so the crossing xhat = -beta / (1 + gamma) falls inside the gap."""
    N, H, W, C = GEOMS[geom]
    base = 5000 + 50 * sorted(GEOMS).index(geom)
    gapped = geom == "part_unrolled_6"
    for seed in range(base, base + 50):
        gen = torch.Generator().manual_seed(seed)
        r = torch.randn(N, H, W, C, generator=gen)
        x = 2.0 * r + 0.5
        h = torch.randn(N, 2 * C, generator=gen)
        if gapped:
            x = torch.sign(r) * (2.0 * r.abs() + 0.2)
            h[:, :C] = (0.5 * h[:, :C]).clamp(-0.5, 1.5)
            h[:, C:] = 0.005 * h[:, C:]
        z = S.adain_fwd(R.nchw64(x), h.to(F64), "none", SLOPE)[1]
        if float(z.abs().min() / z.abs().max()) >= 1e-6:
            break
    else:
        raise AssertionError("no well-conditioned seed for " + geom)
    g = torch.randn(N, H, W, C, generator=gen)
    x64, g64, h64 = R.nchw64(x), R.nchw64(g), h.to(F64)
    ref = {act: (S.adain_fwd(x64, h64, act, SLOPE)[0], S.adain_bwd(g64, x64, h64, act, SLOPE))
           for act in ("none", "lrelu")}
    return x, g, h, z, ref


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_adain_kernels_vs_fp64(gb, geom):
    from gbvst import ops
    N, H, W, C = GEOMS[geom]
    x, g, h, z, ref = _op_data(geom)
    assert float(z.abs().min() / z.abs().max()) >= 1e-6        # on the reference alone
    xd, gd, hd = x.to(DEV), g.to(DEV), h.to(DEV)
    st = ops.instnorm_stats(xd)
    for act in ("none", "lrelu"):
        y_ref, b = ref[act]
        tag = f"{geom}/{act}"
        y1, y2 = ops.adain_fwd(xd, st, hd, act, 0.2), ops.adain_fwd(xd, st, hd, act, 0.2)
        assert torch.equal(y1, y2), tag
        e_y = _rel(R.nchw64(y1), y_ref)
        print(f"{tag}: fwd {e_y:.3e} (bar 1e-5)")
        assert e_y <= 1e-5, tag
        outs = []
        for with_db in (True, True, False):
            dh = torch.full((N, 2 * C), float("nan"), device=DEV)
            db = torch.full((C,), float("nan"), device=DEV) if with_db else None
            dx = ops.adain_bwd(gd, xd, st, hd, act, 0.2, dh=dh, dbias=db)
            outs.append((dx, dh, db))
        for o in outs[1:]:                                      # twice, and without dbias: bit-equal
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), tag
        assert torch.equal(outs[0][2], outs[1][2]), tag
        assert torch.equal(ops.adain_bwd(gd, xd, st, hd, act, 0.2), outs[0][0]), tag      # dx alone
        dx, dh, db = outs[0]
        assert torch.isfinite(dx).all() and torch.isfinite(dh).all() and torch.isfinite(db).all()
        e_dx = _rel(R.nchw64(dx), b["dx"])
        r_dh = float(((dh.cpu().to(F64) - b["dh"]).abs() / (1e-5 * b["dh_abs"])).max())
        r_db = float(((db.cpu().to(F64) - b["dbias"]).abs() / (1e-5 * b["dbias_abs"])).max())
        print(f"{tag}: dx {e_dx:.3e} (bar 1e-4) dh/bound {r_dh:.3g} dbias/bound {r_db:.3g} (bar 1)")
        assert e_dx <= 1e-4, tag
        assert r_dh <= 1.0 and r_db <= 1.0, tag
        # accumulated: one more fp32 rounding of 0.5 + value
        dh2, db2 = torch.full((N, 2 * C), 0.5, device=DEV), torch.full((C,), 0.5, device=DEV)
        ops.adain_bwd(gd, xd, st, hd, act, 0.2, dh=dh2, dbias=db2, accumulate=True)
        e2 = (dh2.cpu().to(F64) - 0.5 - b["dh"]).abs()
        assert bool((e2 <= 1e-5 * b["dh_abs"] + 2.0 ** -24 * (0.5 + b["dh"].abs())).all()), tag
        e3 = (db2.cpu().to(F64) - 0.5 - b["dbias"]).abs()
        assert bool((e3 <= 1e-5 * b["dbias_abs"] + 2.0 ** -24 * (0.5 + b["dbias"].abs())).all()), tag


def _guarded(shape):
    """(view of `shape`, the whole sentinel-filled buffer it sits in)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
    return buf[PAD:PAD + n].view(shape), buf


def _guards_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


SHAPES = [(1, 2, 2, 4), (2, 6, 10, 8), (1, 32, 64, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool2_vs_fp64(gb, shape):
    """shape: the pooled (output) side; the input is twice as high and wide."""
    import torch.nn.functional as F
    from gbvst import ops
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(N, 2 * H, 2 * W, C, generator=gen)
    gy = torch.randn(N, H, W, C, generator=gen)
    y, ybuf = _guarded(shape)
    gx, gbuf = _guarded((N, 2 * H, 2 * W, C))
    xd, gyd = x.to(DEV), gy.to(DEV)
    ops._call("vst_avgpool2_fwd", ops._p(xd), ops._p(y), N, H, W, C, ops._stream())
    ops._call("vst_avgpool2_bwd", ops._p(gyd), ops._p(gx), N, H, W, C, ops._stream())
    torch.cuda.synchronize()
    assert _guards_intact(ybuf) and _guards_intact(gbuf)
    assert not bool((y == SENTINEL).any()) and not bool((gx == SENTINEL).any())
    e_y = _rel(R.nchw64(y), F.avg_pool2d(R.nchw64(x), 2))
    e_g = _rel(R.nchw64(gx), S.merge_bwd(R.nchw64(gy), "pool", 1.0)[1])
    print(f"avgpool2 {shape}: fwd {e_y:.3e} bwd {e_g:.3e} (bar 1e-6)")
    assert e_y <= 1e-6 and e_g <= 1e-6
    assert torch.equal(ops.avgpool2(xd), y) and torch.equal(ops.avgpool2_bwd(gyd), gx)
    assert torch.equal(gx, (gyd * 0.25).repeat_interleave(2, 1).repeat_interleave(2, 2))   # exact: a power of two


@pytest.mark.parametrize("mode", ["same", "pool", "up"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_vs_fp64(gb, shape, mode):
    """shape: a's (and the output's); b's follows from the mode."""
    from gbvst import ops
    N, H, W, C = shape
    bs = ops._merge_b_shape(shape, mode)
    lo = bs if mode == "up" else shape
    gen = torch.Generator().manual_seed(37)
    a, b, g = (torch.randn(s, generator=gen) for s in (shape, bs, shape))
    ad, bd, gd = a.to(DEV), b.to(DEV), g.to(DEV)
    out, obuf = _guarded(shape)
    ga, gabuf = _guarded(shape)
    gbt, gbbuf = _guarded(bs)
    scale = 2 ** -0.5
    ops._call("vst_merge_fwd", ops._p(ad), ops._p(bd), ops._p(out), lo[0], lo[1], lo[2], lo[3], ops.MERGE[mode],
              scale, ops._stream())
    ops._call("vst_merge_bwd", ops._p(gd), ops._p(ga), ops._p(gbt), lo[0], lo[1], lo[2], lo[3], ops.MERGE[mode],
              scale, ops._stream())
    torch.cuda.synchronize()
    for buf, t in ((obuf, out), (gabuf, ga), (gbbuf, gbt)):
        assert _guards_intact(buf) and not bool((t == SENTINEL).any())
    e_o = _rel(R.nchw64(out), S.merge_fwd(R.nchw64(a), R.nchw64(b), mode, RSQRT2))
    ra, rb = S.merge_bwd(R.nchw64(g), mode, RSQRT2)
    e_a, e_b = _rel(R.nchw64(ga), ra), _rel(R.nchw64(gbt), rb)
    print(f"merge {mode} {shape}: fwd {e_o:.3e} ga {e_a:.3e} gb {e_b:.3e} (bar 1e-6)")
    assert e_o <= 1e-6 and e_a <= 1e-6 and e_b <= 1e-6
    # the wrappers launch the same kernels
    assert torch.equal(ops.merge(ad, bd, mode, scale), out)
    wa, wb = ops.merge_bwd(gd, mode, scale)
    assert torch.equal(wa, ga) and torch.equal(wb, gbt)
    s32 = torch.tensor(scale, dtype=torch.float32, device=DEV)
    if mode != "pool":   # no resampling arithmetic: bit-equal to the fp32 composition (a + f(b)) * s
        fb = bd if mode == "same" else bd.repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert torch.equal(out, (ad + fb) * s32)
        assert torch.equal(ga, gd * s32)


def test_avgpool2_past_2_31_elements(gb):
    """An input of more than 2^31 elements (8.6 GB): the last pooled rows, which only 64-bit element indices reach,
    against the same rows pooled by torch from a slice; forward and backward."""
    from gbvst import ops
    H, W, C = 4104, 4096, 32                       # x [1, 8208, 8192, 32]: 2^31 + 2^22 elements
    x = torch.empty((1, 2 * H, 2 * W, C), device=DEV)
    x.view(-1)[:1 << 20].normal_()
    tail = x[:, -8:]                               # the rows behind the 2^31st element
    tail.normal_()
    assert x.numel() > 2 ** 31 and (x.numel() - tail.numel()) > 2 ** 31
    y = ops.avgpool2(x)
    want = torch.nn.functional.avg_pool2d(tail.permute(0, 3, 1, 2).double(), 2).permute(0, 2, 3, 1)
    e = _rel(y[:, -4:], want)
    print(f"avgpool2 past 2^31: tail rows {e:.3e} (bar 1e-6)")
    assert e <= 1e-6
    del x, tail
    gx = ops.avgpool2_bwd(y)
    assert torch.equal(gx[:, -8:], (y[:, -4:] * 0.25).repeat_interleave(2, 1).repeat_interleave(2, 2))


def test_library_ops_opcheck_and_autograd(gb):
    """vst::adain_act, vst::avg_pool2 and vst::merge pass opcheck's schema, fake-tensor and autograd-registration
    checks, and autograd through them equals the op-level kernels."""
    from gbvst import library, ops  # noqa: F401
    gen = torch.Generator().manual_seed(79)
    x = (2.0 * torch.randn(2, 16, 6, 4, generator=gen) + 0.5).to(DEV)
    h = torch.randn(2, 32, generator=gen).to(DEV)
    g = torch.randn(2, 16, 6, 4, generator=gen).to(DEV)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    xg, hg = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.vst.adain_act.default, (xg, hg, "lrelu", 0.2), test_utils=utils)
    y = torch.ops.vst.adain_act(xg, hg, "lrelu", 0.2)
    (y * g).sum().backward()
    xn = ops.nchw_to_nhwc(x)
    st = ops.instnorm_stats(xn)
    assert torch.equal(y.detach(), ops.nhwc_to_nchw(ops.adain_fwd(xn, st, h, "lrelu", 0.2), 16))
    dh = torch.empty_like(h)
    dx = ops.adain_bwd(ops.nchw_to_nhwc(g), xn, st, h, "lrelu", 0.2, dh=dh)
    assert torch.equal(xg.grad, ops.nhwc_to_nchw(dx, 16)) and torch.equal(hg.grad, dh)
    b = S.adain_bwd(g.double().cpu(), x.double().cpu(), h.double().cpu(), "lrelu", SLOPE)
    assert _rel(xg.grad, b["dx"]) <= 1e-4 and _rel(hg.grad, b["dh"]) <= 1e-4
    xg = x.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.vst.avg_pool2.default, (xg,), test_utils=utils)
    p = torch.ops.vst.avg_pool2(xg)
    (p * g[:, :, :3, :2]).sum().backward()
    assert _rel(p, torch.nn.functional.avg_pool2d(x.double().cpu(), 2)) <= 1e-6
    assert _rel(xg.grad, S.merge_bwd(g[:, :, :3, :2].double().cpu(), "pool", 1.0)[1]) <= 1e-6
    for mode, bshape in (("same", (2, 16, 6, 4)), ("pool", (2, 16, 12, 8)), ("up", (2, 16, 3, 2))):
        a = x.clone().requires_grad_(True)
        bt = torch.randn(bshape, generator=gen).to(DEV).requires_grad_(True)
        torch.library.opcheck(torch.ops.vst.merge.default, (a, bt, mode, 0.5), test_utils=utils)
        o = torch.ops.vst.merge(a, bt, mode, 0.5)
        (o * g).sum().backward()
        assert _rel(o, S.merge_fwd(x.double().cpu(), bt.detach().double().cpu(), mode, 0.5)) <= 1e-6
        ra, rb = S.merge_bwd(g.double().cpu(), mode, 0.5)
        assert _rel(a.grad, ra) <= 1e-6 and _rel(bt.grad, rb) <= 1e-6


# ================================================================================= net level
def _build(kind, cfg, dev=DEV):
    from gbvst import stargan2 as M
    if kind == "generator":
        net = M.Generator(cfg["img_size"], cfg["style_dim"], cfg["max_conv_dim"], w_hpf=0)
    else:
        net = {"mapping_network": M.MappingNetwork, "style_encoder": M.StyleEncoder,
               "discriminator": M.Discriminator}[kind](**cfg)
    return net.to(dev)


def _cond(name):
    c = S.CASES[name]
    if c["kind"] == "generator":
        return S.style_code(c["seed"] + 2, c["x"][0], c["cfg"]["style_dim"])
    return c["y"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(net with the case's weights, sd, x, r, cond, the fp64 reference's (out, dx, ds, grads)), computed once."""
    c = S.CASES[name]
    kind, cfg = c["kind"], c["cfg"]
    sd = S.make_state(c["seed"], S.shapes(kind, **cfg))
    x, r = S.case_inputs(c["seed"] + 1, c["x"], S.out_shape(name))
    cond = _cond(name)
    net = _build(kind, cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net, sd, x, r, cond, S.run_case(kind, cfg, sd, x, cond, r, F64)


def _run_net(name):
    net, sd, x, r, cond, _ = _case(name)
    kind = S.CASES[name]["kind"]
    net.zero_grad(set_to_none=True)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    ct = torch.from_numpy(cond).to(DEV).requires_grad_(True) if kind == "generator" else torch.tensor(cond, device=DEV)
    out = net(xt, ct)
    (out * torch.from_numpy(r).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xt.grad, (ct.grad if kind == "generator" else None), \
        {k: p.grad for k, p in net.named_parameters()}


def _bands(name, ref, eps=1e-6, seeds=(0, 1, 2, 3)):
    """How far the fp64 reference's own gradients move when every weight is scaled by (1 + eps N(0, 1)) (the band
    of test_gpu_unet._bands).  Returns (dx band, ds band, {param: band})."""
    _, sd, x, r, cond, _ = _case(name)
    c = S.CASES[name]
    _, ref_dx, ref_ds, ref_g = ref
    dxb, dsb, pb = 0.0, 0.0, {}
    for s in seeds:
        gen = torch.Generator().manual_seed(s)
        sp = {k: (torch.from_numpy(v).double() * (1 + eps * torch.randn(v.shape, generator=gen, dtype=F64))).numpy()
              for k, v in sd.items()}
        _, dx, ds, gp = S.run_case(c["kind"], c["cfg"], sp, x, cond, r, F64)
        dxb = max(dxb, _nrel(dx, ref_dx))
        if ds is not None:
            dsb = max(dsb, _nrel(ds, ref_ds))
        for k in ref_g:
            if float(ref_g[k].abs().max()) > 0:
                pb[k] = max(pb.get(k, 0.0), _rel(gp[k], ref_g[k]))
    return dxb, dsb, pb


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_nets_vs_fixture_and_fp64(gb, golden, name):
    g = golden("stargan2_small")
    c = S.CASES[name]
    kind, cfg = c["kind"], c["cfg"]
    net, sd, x, r, cond, ref = _case(name)
    assert list(net.state_dict()) == list(g[name + "_keys"])
    out, dx, ds, grads = _run_net(name)
    ref_out, ref_dx, ref_ds, ref_g = ref
    bands = []

    def band():
        if not bands:
            bands.append(_bands(name, ref))
        return bands[0]

    for tag, r_out, r_dx, r_ds in (("fixture", g[name + "_out"], g[name + "_dx"], g[name + "_ds"] if ds is not None
                                    else None), ("fp64", ref_out, ref_dx, ref_ds)):
        e_out = _rel(out, r_out)
        e_dx = _nrel(dx, r_dx)
        e_ds = _nrel(ds, r_ds) if ds is not None else 0.0
        print(f"{name} vs {tag}: out {e_out:.3e} (bar 1e-4) dx {e_dx:.3e} ds {e_ds:.3e} (bar 1e-3)")
        assert e_out <= 1e-4
        if e_dx >= 1e-3:
            assert e_dx < band()[0], (tag, e_dx, band()[0])
        if e_ds >= 1e-3:
            assert e_ds < band()[1], (tag, e_ds, band()[1])
    zero = S.normed_bias_keys(kind, **cfg)
    gmax = max(float(v.abs().max()) for v in ref_g.values())
    worst, n_zero = 0.0, 0
    for k, rg in ref_g.items():
        got = grads[k]
        assert got is not None, k            # dense zeros, never None, for the heads no sample selects
        if k in zero:
            # exact gradient 0: both sides are rounding noise
            assert float(got.abs().max()) < 1e-3 * max(1.0, gmax), k
            continue
        if float(rg.abs().max()) == 0:
            assert not bool(got.any()) and not np.any(g[f"{name}_g_{k}"]), k
            n_zero += 1
            continue
        for tag, rr, gg in (("fixture", g[f"{name}_g_{k}"], S.stored(got)), ("fp64", rg, got)):
            e = _rel(gg, rr)
            worst = max(worst, e)
            if e >= 1e-3:
                print(f"{name} vs {tag}: {k}: {e:.3e}, the reference's own band {band()[2][k]:.3e}")
                assert e < band()[2][k], (tag, k, e, band()[2][k])
    print(f"{name}: worst parameter gradient {worst:.3e} (bar 1e-3); {n_zero} exactly-zero gradients")
    assert n_zero == {"G": 0, "D": 0, "E": 2, "F": 16}[name]
    if name == "D":     # y = [2, 0]: the logit channel of domain 1 is selected by no sample
        head = "main.%d" % (len(S.trunk_plan(cfg["img_size"], cfg["max_conv_dim"])) + 4)
        assert not bool(grads[head + ".weight"][1].any()) and float(grads[head + ".bias"][1]) == 0.0
        assert bool(grads[head + ".weight"][0].any()) and bool(grads[head + ".weight"][2].any())


def test_generator_is_independent_of_batch_composition(gb):
    """InstanceNorm and AdaIN are per sample: a sample's output does not depend on its batch mates beyond the
    forward bar."""
    net, sd, x, r, cond, ref = _case("G")
    xt, st = torch.from_numpy(x).to(DEV), torch.from_numpy(cond).to(DEV)
    with torch.no_grad():
        both = net(xt, st)
        alone = [net(xt[i:i + 1].contiguous(), st[i:i + 1].contiguous()) for i in (0, 1)]
        swapped = net(xt.flip(0).contiguous(), st.flip(0).contiguous())
    for i in (0, 1):
        e1, e2 = _rel(alone[i], both[i:i + 1]), _rel(swapped[1 - i], both[i])
        print(f"sample {i}: alone {e1:.3e} swapped {e2:.3e} (bar 1e-4)")
        assert e1 <= 1e-4 and e2 <= 1e-4
        assert _rel(alone[i], ref[0][i:i + 1]) <= 1e-4


def test_default_size_generator_forward(gb):
    """Generator(256, 64) (33.9 M parameters, C = 64 ... 512) at 1x3x64x64 — the net is fully convolutional —
    against the fp32 CPU reference."""
    cfg = S.DEFAULTS["generator"]
    sd = S.make_state(840, S.shapes("generator", **cfg))
    x, _ = S.case_inputs(841, (1, 3, 64, 64), (1, 3, 64, 64))
    s = S.style_code(842, 1, cfg["style_dim"])
    with torch.no_grad():
        want = S.generator_forward({k: torch.from_numpy(v) for k, v in sd.items()}, torch.from_numpy(x),
                                   torch.from_numpy(s), **cfg)
    net = _build("generator", cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with torch.no_grad():
        got = net(torch.from_numpy(x).to(DEV), torch.from_numpy(s).to(DEV))
    e = _rel(got, want)
    print(f"Generator(256, 64) at 64x64: {e:.3e} (bar 1e-4)")
    assert tuple(got.shape) == (1, 3, 64, 64) and e <= 1e-4


# ================================================================================= inference
def _given_flows(frames):
    """The harness's flow hook over given flows: flow(frame i -> frame j) = (j - i) * a smooth field of about
    (1.5, -0.75) pixels, so forward and backward flows are consistent and fbcheck keeps most pixels."""
    H, W = frames[0].shape[2:]
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    field = torch.stack([1.5 + 0.1 * yy, -0.75 + 0.1 * xx])[None]

    def flow(a, b):
        i, j = (next(k for k, f in enumerate(frames) if torch.equal(f, t.cpu())) for t in (a, b))
        return ((j - i) * field).to(a.device).contiguous()
    return flow


def _frames(n, H, W, seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (3, H, W))
    return [torch.from_numpy(np.clip(np.roll(base, i, axis=2) + rng.normal(0, 0.05, (3, H, W)), -1, 1)
                             .astype(np.float32)).unsqueeze(0) for i in range(n)]


def test_style_guided_inference_through_the_sintel_harness(gb, tmp_path):
    from gbvst import sintel_eval as se, stargan2 as M
    from oracle import cpu_ref
    states = {n: _case(n)[1] for n in "GEF"}
    tens = {n: {k: torch.from_numpy(v) for k, v in states[n].items()} for n in "GEF"}
    cfgs = {n: S.CASES[n]["cfg"] for n in "GEF"}
    nets = types.SimpleNamespace(generator=_build("generator", cfgs["G"]),
                                 mapping_network=_build("mapping_network", cfgs["F"]),
                                 style_encoder=_build("style_encoder", cfgs["E"]))
    # a nets_ema checkpoint written by CheckpointIO from CPU modules holding the reference-layout tensors (what the
    # reference's own CheckpointIO saves), loaded into the GPU nets
    tmpl = str(tmp_path / "{:06d}_nets_ema.ckpt")
    names = {"generator": "G", "mapping_network": "F", "style_encoder": "E"}
    cpu_nets = {k: _build(k, cfgs[n], "cpu") for k, n in names.items()}
    for k, n in names.items():
        cpu_nets[k].load_state_dict(tens[n])
    M.CheckpointIO(tmpl, **cpu_nets).save(50000)
    raw = torch.load(tmpl.format(50000), map_location="cpu", weights_only=True)
    assert list(raw) == list(names) and all(not v.is_cuda for sd_ in raw.values() for v in sd_.values())
    M.CheckpointIO(tmpl, **vars(nets)).load(50000)
    with torch.no_grad():
        x0 = torch.from_numpy(_case("G")[2]).to(DEV)
        assert torch.equal(nets.generator(x0, torch.from_numpy(_case("G")[4]).to(DEV)),
                           _case("G")[0](x0, torch.from_numpy(_case("G")[4]).to(DEV)))
    frames = _frames(3, 32, 64, 11)
    flow = _given_flows(frames)
    z = torch.from_numpy(S.case_inputs(851, (1, 16), (1, 16))[0])
    x_ref = torch.from_numpy(S.case_inputs(852, (1, 3, 64, 64), (1, 16))[0])
    guided = {"latent": (M.StyleGuided.from_latent(nets, z.to(DEV), torch.tensor([1], device=DEV)),
                         S.mapping_forward(tens["F"], z, [1], **cfgs["F"])),
              "reference": (M.StyleGuided.from_reference(nets, x_ref.to(DEV), torch.tensor([2], device=DEV)),
                            S.encoder_forward(tens["E"], x_ref, [2], **cfgs["E"]))}
    for how, (model, s_ref) in guided.items():
        with torch.no_grad():
            s_ref = s_ref.detach()
            e_s = _rel(model.s_trg, s_ref)
            print(f"{how}: style code {e_s:.3e} (bar 1e-4)")
            assert tuple(model.s_trg.shape) == (1, 16) and e_s <= 1e-4
            st, lt, dt = se.evaluate_video(model, frames, flow, "vid_" + how, lt_len=2)
            fake = [S.generator_forward(tens["G"], f, s_ref, **cfgs["G"]) for f in frames]
            sts, lts = [], []
            for i in range(1, 3):
                for j, vals in ((i - 1, sts), (i - 2, lts)):
                    if j >= 0:
                        ff, bf = flow(frames[j], frames[i]), flow(frames[i], frames[j])
                        mask = cpu_ref.fbc_check(ff, bf)
                        assert 0.5 < float(mask.mean()) < 1.0          # the check is not vacuous
                        vals.append(cpu_ref.tcl(fake[i], fake[j], bf, mask).item())
        for got, ref in ((st["TCL-ST_vid_" + how], np.mean(sts)), (lt["TCL-LT_vid_" + how], np.mean(lts))):
            print(f"{how}: TCL {got:.6f} reference {ref:.6f}")
            assert ref > 0.1 and abs(got - ref) <= 1e-3 * abs(ref) + 1e-6, (how, got, ref)
        assert dt["DT_vid_" + how] > 0
