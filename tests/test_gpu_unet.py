"""GPU parity of the U-Net generators (unet_128 / unet_256) and of the skip-connection kernels under them.

Op level: vst_instnorm_skip_fwd / _bwd against the fp64 references of tests/unet_ref.py over the InstanceNorm
geometries of reduction_ref.IN_CASE that change a code path (plus one 1x2-pixel map), at both halves of a
concatenation buffer, with and without statistics, with and without the lrelu output / its gradient.  Bars, relative
to max|ref| of the tensor (those of test_gpu_reductions / test_gpu_multistyle): forward 1e-5, dy 1e-4, the bias
gradient within 1e-5 * sum|dy| of its channel.  Every figure is printed before it is asserted.

Net level: UnetGenerator against the fixture the reference's own module produced (tests/golden/unet_small.npz) and,
at unet_256's depth, against the fp64 reference: output 1e-4 of max|ref|; the input gradient (norm-wise) and the
parameter gradients (max-relative) within 1e-3 or within the reference's own movement under a 1e-6 relative
perturbation of its weights (gradients are a discontinuous function of the forward values; the band is computed
only when the tight bound misses).  Step level: two CycleGAN optimize_parameters() steps with netG=unet_128 against
oracle.cpu_ref's step over the fp64 U-Net.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import reduction_ref as R
import unet_ref as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SLOPE = R.f32(0.2)
INST = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
GEOMS = {k: R.IN_CASE[k][1] for k in ("tiny_hw", "c4", "c8", "tail_cpb4", "fold4_unrolled", "lp18", "part_unrolled_6")}
GEOMS["map_1x2"] = (2, 1, 2, 32)
# Input scale per geometry: y = 2 N(0, 1) + 0.5, except on the 2-pixel map.  There x_hat = +-a with
# a^2 = h^2 / (h^2 + eps) (h: half the difference of the two values), and the InstanceNorm backward is
# dy = rstd (g - mean g) (1 - a^2): at h ~ 2 the two terms cancel to eps / h^2 = 2.5e-6 of their size, so the fp32
# rounding of the stored mean and rstd (2^-24 relative) alone is 2e-2 of the result, in any fp32 implementation.
# At h ~ sqrt(eps) = 3e-3 (y = 3e-3 N(0, 1)) 1 - a^2 ~ 0.5 and the problem is as well conditioned as the others.
# part_unrolled_6 (rows reach the 4x unrolled loop of the partial walk, with a remainder and a ragged last slice)
# has 2.8 M elements, and no seed keeps that many Gaussian values clear of 0; the signs are intrinsic to these
# kernels, so its values are moved away from 0 by a gap instead: y = sign(r) (2 |r| + 0.2), r = N(0, 1).
Y_SCALE = {"map_1x2": (3e-3, 0.0), "part_unrolled_6": (2.0, 0.0, 0.2)}
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


def _rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def _nrel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


# ================================================================================== op level
@functools.lru_cache(maxsize=None)
def _op_data(geom, use_stats):
    """fp32 NHWC y, g_d, g_s of a geometry and the fp64 references of both kernels.  The seed is the first whose
    reference z keeps min|z| / max|z| >= 1e-6, so no relu / lrelu decision hangs on fp32 rounding."""
    N, H, W, C = GEOMS[geom]
    base = 4000 + 50 * sorted(GEOMS).index(geom)
    for seed in range(base, base + 50):
        gen = torch.Generator().manual_seed(seed)
        scale, shift, gap = (Y_SCALE.get(geom, (2.0, 0.5)) + (0.0,))[:3]
        r = torch.randn(N, H, W, C, generator=gen)
        y = scale * r + shift
        if gap:
            y = y + gap * torch.sign(r)
        z = U.skip_fwd(R.nchw64(y), use_stats, SLOPE)[2]
        if float(z.abs().min() / z.abs().max()) >= 1e-6:
            break
    else:
        raise AssertionError("no well-conditioned seed for " + geom)
    g_d, g_s = torch.randn(N, H, W, C, generator=gen), torch.randn(N, H, W, C, generator=gen)
    y64 = R.nchw64(y)
    d, s, z = U.skip_fwd(y64, use_stats, SLOPE)
    bwd = {has_gd: U.skip_bwd(R.nchw64(g_d) if has_gd else None, R.nchw64(g_s), y64, use_stats, SLOPE)
           for has_gd in (True, False)}
    return y, g_d, g_s, d, s, z, bwd


@pytest.mark.parametrize("half", [0, 1], ids=["skip_half", "up_half"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_skip_kernels_vs_fp64(gb, geom, half):
    from gbvst import ops
    N, H, W, C = GEOMS[geom]
    Cs, c0, o0 = 2 * C, half * C, (1 - half) * C        # o0: the half that must stay untouched
    for use_stats in (True, False):
        y, g_d, g_s, d_ref, s_ref, z, bwd = _op_data(geom, use_stats)
        assert float(z.abs().min() / z.abs().max()) >= 1e-6
        yd = y.to(DEV)
        st = ops.instnorm_stats(yd) if use_stats else None
        g_cat = torch.full((N, H, W, Cs), SENTINEL)
        g_cat[..., c0:c0 + C] = g_s
        g_cat = g_cat.to(DEV)
        for want in (True, False):
            tag = f"{geom}/c0={c0}/stats={use_stats}/d={want}"
            # ---- forward, twice: bit-equal, the other half untouched
            runs = []
            for _ in range(2):
                cat = torch.full((N, H, W, Cs), SENTINEL, device=DEV)
                d = ops.instnorm_skip_fwd(yd, st, cat, c0, want_d=want)
                runs.append((d, cat))
            assert (runs[0][0] is None) == (not want)
            assert torch.equal(runs[0][1], runs[1][1]) and (not want or torch.equal(runs[0][0], runs[1][0]))
            d, cat = runs[0]
            assert bool((cat[..., o0:o0 + C] == SENTINEL).all()), tag
            e_s = _rel(R.nchw64(cat[..., c0:c0 + C]), s_ref)
            e_d = _rel(R.nchw64(d), d_ref) if want else 0.0
            print(f"{tag}: fwd skip {e_s:.3e} d {e_d:.3e} (bar 1e-5)")
            assert e_s <= 1e-5 and e_d <= 1e-5, tag
            # ---- backward (want: with g_d), twice: bit-equal; db written and accumulated
            dy_ref, db_ref = bwd[want]
            gd = g_d.to(DEV) if want else None
            outs = []
            for acc in (False, True, True):
                db = torch.full((C,), 0.5 if acc else float("nan"), device=DEV)
                dy = ops.instnorm_skip_bwd(gd, g_cat, c0, yd, st, db=db, accumulate_db=acc)
                outs.append((dy, db))
            assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])
            assert torch.equal(outs[0][0], outs[1][0])
            assert torch.equal(ops.instnorm_skip_bwd(gd, g_cat, c0, yd, st), outs[0][0])      # without db
            dy = R.nchw64(outs[0][0])
            assert torch.isfinite(dy).all()
            e_dy = _rel(dy, dy_ref)
            bound = 1e-5 * dy_ref.abs().sum(dim=(0, 2, 3))
            e_db = (outs[0][1].cpu().to(F64) - db_ref).abs()
            e_dba = (outs[1][1].cpu().to(F64) - 0.5 - db_ref).abs()
            print(f"{tag}: dy {e_dy:.3e} (bar 1e-4) db/bound {float((e_db / bound).max()):.3g} "
                  f"accumulated {float((e_dba / bound).max()):.3g}")
            assert e_dy <= 1e-4, tag
            # the accumulated form adds one fp32 rounding of 0.5 + db
            assert bool((e_db <= bound).all()), tag
            assert bool((e_dba <= bound + 2.0 ** -24 * (0.5 + db_ref.abs())).all()), tag


def test_skip_kernels_refuse_contract_violations(gb):
    """Geometries outside the contract come back as VST_EUNSUPPORTED, null or non-positive arguments as VST_EINVAL,
    through vst_last_error, and nothing is launched: the output buffers keep their sentinel."""
    from gbvst import ops
    lib = ops.lib()
    N, H, W = 1, 4, 4
    y = torch.zeros((N, H, W, 8), device=DEV)
    cat = torch.full((N, H, W, 2056), SENTINEL, device=DEV)
    out = torch.full((N, H, W, 1028), SENTINEL, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    p = ops._p

    def fwd(C=8, Cs=16, c0=8, yy=y, N_=N):
        return lib.vst_instnorm_skip_fwd(p(yy), None, p(out), p(cat), N_, H * W, C, Cs, c0, 0.2, None)

    def bwd(C=8, Cs=16, c0=8, yy=y, N_=N):
        return lib.vst_instnorm_skip_bwd(None, p(cat), Cs, c0, p(yy), None, p(out), None, 0, p(ws), N_, H * W, C, 0.2,
                                         None)

    for call in (fwd, bwd):
        for kw in (dict(C=6, c0=0), dict(c0=2), dict(c0=12), dict(Cs=18), dict(C=1028, Cs=2056, c0=0)):
            assert call(**kw) == 2, (call.__name__, kw)
            assert b"instnorm_skip" in lib.vst_last_error()
        for kw in (dict(yy=None), dict(N_=0), dict(C=0), dict(c0=-4)):
            assert call(**kw) == 1, (call.__name__, kw)
    with pytest.raises(ValueError):
        ops.instnorm_skip_fwd(y, None, torch.zeros((N, H, W, 12), device=DEV), 8)
    with pytest.raises(RuntimeError):       # C % 4 != 0 reaches the library and is refused there
        ops.instnorm_skip_fwd(torch.zeros((N, H, W, 6), device=DEV), None, torch.zeros((N, H, W, 12), device=DEV), 0)
    torch.cuda.synchronize()
    assert bool((cat == SENTINEL).all()) and bool((out == SENTINEL).all())


def test_library_op_opcheck_and_autograd(gb):
    """vst::instance_norm_skip passes opcheck's schema, fake-tensor and autograd-registration checks, and autograd
    through it equals the op-level kernels bit for bit."""
    from gbvst import library, ops  # noqa: F401
    gen = torch.Generator().manual_seed(77)
    y = (2.0 * torch.randn(2, 16, 6, 5, generator=gen) + 0.5).to(DEV)
    g_d, g_s = (torch.randn(2, 16, 6, 5, generator=gen).to(DEV) for _ in range(2))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for normalize in (True, False):
        yg = y.clone().requires_grad_(True)
        torch.library.opcheck(torch.ops.vst.instance_norm_skip.default, (yg, normalize, 0.2), test_utils=utils)
        d, s = torch.ops.vst.instance_norm_skip(yg, normalize, 0.2)
        ((d * g_d).sum() + (s * g_s).sum()).backward()
        yn = ops.nchw_to_nhwc(y)
        st = ops.instnorm_stats(yn) if normalize else None
        cat = torch.empty_like(yn)
        d0 = ops.instnorm_skip_fwd(yn, st, cat, 0)
        dy0 = ops.instnorm_skip_bwd(ops.nchw_to_nhwc(g_d), ops.nchw_to_nhwc(g_s), 0, yn, st)
        assert torch.equal(d.detach(), ops.nhwc_to_nchw(d0, 16)) and torch.equal(s.detach(), ops.nhwc_to_nchw(cat, 16))
        assert torch.equal(yg.grad, ops.nhwc_to_nchw(dy0, 16))
        dref, sref, _ = U.skip_fwd(y.double().cpu(), normalize, SLOPE)
        assert _rel(d, dref) <= 1e-5 and _rel(s, sref) <= 1e-5
        assert _rel(yg.grad, U.skip_bwd(g_d.double().cpu(), g_s.double().cpu(), y.double().cpu(), normalize,
                                        SLOPE)[0]) <= 1e-4


@pytest.mark.parametrize("shape,cout,bias_act", [((2, 5, 3, 16), 8, False), ((1, 1, 2, 32), 32, False),
                                                   ((1, 1, 1, 64), 64, False), ((2, 6, 4, 16), 3, True),
                                                   ((1, 64, 64, 32), 64, False)],
                         ids=["odd", "map_1x2", "map_1x1", "image_bias_tanh", "grouped"])
def test_convT4s2_vs_torch(gb, shape, cout, bias_act):
    """ops.convT4s2_fwd against float64 F.conv_transpose2d(k4, s2, p1) at the conv tolerance of tests/conftest.py
    (bf16x6: 2e-5 of max|ref|): odd maps, the 1x2 and 1x1 bottlenecks, the 4-channel image layer with its bias and
    tanh in the phase epilogues, and a shape the grouped launch takes."""
    from gbvst import ops
    N, H, W, Ci = shape
    gen = torch.Generator().manual_seed(91)
    x = torch.randn(N, Ci, H, W, generator=gen)
    w = torch.randn(Ci, cout, 4, 4, generator=gen) / np.sqrt(4 * Ci)
    b = torch.randn(cout, generator=gen) if bias_act else None
    ref = torch.nn.functional.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2,
                                               padding=1)
    ref = torch.tanh(ref) if bias_act else ref
    wd = w.to(DEV)
    packs = ops.conv4s2_dgrad_phase_packs(wd)
    bp = None
    if b is not None:
        bp = torch.zeros(ops.cpad(cout), device=DEV)
        bp[:cout] = b.to(DEV)
    out = ops.convT4s2_fwd(ops.nchw_to_nhwc(x.to(DEV)), packs, bp, ops.cpad(cout), act="tanh" if bias_act else "none")
    assert tuple(out.shape) == (N, 2 * H, 2 * W, ops.cpad(cout))
    e = _rel(ops.nhwc_to_nchw(out, cout), ref)
    print(f"convT4s2 {shape} -> {cout}: {e:.3e}")
    assert e <= 2e-5


# ================================================================================= net level
def _net(gb, D, ngf, seed):
    from gbvst import networks
    net = networks.UnetGenerator(3, 3, D, ngf, norm_layer=INST).to(DEV)
    sd = U.make_state(seed, U.unet_shapes(3, 3, D, ngf))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net, sd


def _bands(sd, x, r, D, dtype, ref_dx, ref_g, eps=1e-6, seeds=(0, 1, 2, 3)):
    """How far the reference's own gradients move when every weight is scaled by (1 + eps N(0, 1)) — forward
    changes of the size another fp32 summation order makes flip ReLU decisions (test_gpu_style's
    _fsn_perturbed_bands).  Returns (input-gradient band, norm-wise; {param: band, max-relative})."""
    dxb, pb = 0.0, {}
    for s in seeds:
        gen = torch.Generator().manual_seed(s)
        sp = {k: (torch.from_numpy(v).double() * (1 + eps * torch.randn(v.shape, generator=gen, dtype=F64)))
              .numpy().astype(np.float32 if dtype == torch.float32 else np.float64) for k, v in sd.items()}
        _, dx, gp = U.run_case(sp, x, r, D, dtype)
        dxb = max(dxb, _nrel(dx, ref_dx))
        for k in ref_g:
            pb[k] = max(pb.get(k, 0.0), _rel(gp[k], ref_g[k]))
    return dxb, pb


def _check_net(net, sd, x, r, D, ref_out, ref_dx, ref_g, band_dtype, tag):
    net.zero_grad()
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = net(xt)
    (out * torch.from_numpy(r).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    e_out = _rel(out, ref_out)
    print(f"{tag}: out {e_out:.3e} (bar 1e-4)")
    assert e_out <= 1e-4
    bands = []

    def band():
        if not bands:
            bands.append(_bands(sd, x, r, D, band_dtype, ref_dx, ref_g))
        return bands[0]

    e_dx = _nrel(xt.grad, ref_dx)
    print(f"{tag}: dx {e_dx:.3e} (bar 1e-3)")
    if e_dx >= 1e-3:
        assert e_dx < band()[0], (e_dx, band()[0])
    params = dict(net.named_parameters())
    zero = U.normed_bias_keys(D)
    gmax = max(float(np.abs(np.asarray(v)).max()) for v in ref_g.values())
    worst = 0.0
    for k, ref in ref_g.items():
        if k in zero:
            # a bias in front of an InstanceNorm: exact gradient 0, both sides are rounding noise
            assert float(params[k].grad.abs().max()) < 1e-3 * max(1.0, gmax), k
            continue
        e = _rel(params[k].grad, ref)
        worst = max(worst, e)
        if e >= 1e-3:
            assert e < band()[1][k], (k, e, band()[1][k])
    print(f"{tag}: worst parameter gradient {worst:.3e} (bar 1e-3)")
    return out


@pytest.mark.parametrize("case", ["a", "b"])
def test_unet_vs_reference_golden(gb, golden, case):
    g = golden("unet_small")
    D, seed = U.CASES[case]
    net, sd = _net(gb, D, 4, seed)
    # the state_dict round-trips through the reference's key names
    assert list(net.state_dict()) == list(g[case + "_keys"])
    for k, v in net.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), sd[k]), k
    ref_g = {k[len(case) + 3:]: g[k] for k in g.files if k.startswith(case + "_g_")}
    x = g[case + "_x"]
    out = _check_net(net, sd, x, g[case + "_r"], D, g[case + "_out"], g[case + "_dx"], ref_g, torch.float32,
                     "case " + case)
    # the no-grad forward replays a captured graph and equals the eager one bit for bit
    xt = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        y1, y2, y3 = net(xt), net(xt), net._forward_eager(xt)
    assert net._graphs and torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(y1, out.detach())


def test_unet256_depth_vs_fp64(gb):
    """num_downs=8 at 1x3x256x256, ngf=8: the smallest shape that reaches the 1x1 bottleneck through all eight
    levels, against the fp64 reference."""
    D, ngf = 8, 8
    net, sd = _net(gb, D, ngf, 720)
    rs = np.random.RandomState(721)
    x = ((rs.randint(0, 256, (1, 3, 256, 256)).astype(np.float32) / 255.0) - 0.5) / 0.5
    r = rs.randint(-4, 5, (1, 3, 256, 256)).astype(np.float32) / 4.0
    out, dx, gp = U.run_case(sd, x, r, D, F64)
    _check_net(net, sd, x, r, D, out, dx, {k: v.numpy() for k, v in gp.items()}, F64, "unet_256 depth")


def test_grad_ready_offsets_fall_to_zero(gb):
    """With a recording _grad_ready_cb the offsets reported during one backward are non-increasing and end at 0
    (the backward's layer order is the reverse of the parameter order: the data-parallel bucket hooks)."""
    net, _ = _net(gb, 5, 4, 730)
    seen = []
    net._grad_ready_cb = seen.append
    try:
        net._reset_pending()
        x = torch.randn(1, 3, 32, 32, device=DEV)
        net(x).sum().backward()
    finally:
        net._grad_ready_cb = None
    assert len(seen) == 10 and seen == sorted(seen, reverse=True) and seen[-1] == 0 and len(set(seen)) == 10


# ================================================================================ step level
def _step_inputs(B, H, W):
    from oracle import prng
    a, a2, b = (prng.uniform_f32(s, (B, 3, H, W), -1, 1) for s in (741, 742, 743))
    mask = (prng.uniform_f32(744, (B, 1, H, W)) < 0.8).astype(np.float32)
    flow = prng.normal(745, (B, 2, H, W), std=2.0)
    return [torch.from_numpy(v) for v in (a, a2, b, mask, flow)]


def _ref_step(sds, t, perturb=None):
    from oracle import cpu_ref
    ref = U.ref_cyclegan_unet(8, 8, 7)
    for name, net in ref.nets().items():
        sd = sds[name]
        if perturb is not None:
            gen = torch.Generator().manual_seed(perturb)
            sd = {k: (torch.from_numpy(v).double() * (1 + 1e-6 * torch.randn(v.shape, generator=gen, dtype=F64)))
                  .numpy() for k, v in sd.items()}
        if name.startswith("G"):
            net.load_np(sd)
        else:
            cpu_ref.load_np_state(net, {k: np.asarray(v, np.float64) for k, v in sd.items()})
    ref.set_input_fc2(*(v.double() for v in t))
    return ref


def _g_grads(nets):
    return [{k: p.grad.detach().double().cpu().clone() for k, p in
             (n.named().items() if hasattr(n, "named") else n.named_parameters())} for n in nets]


def test_cyclegan_unet128_steps_vs_fp64(gb):
    """Two optimize_parameters() steps, netG=unet_128, ngf=ndf=8, B=2 at 128x128: every loss within 1e-3 relative
    of the fp64 reference step; step-0 generator gradients within 1e-3 or the reference's own 1e-6-perturbation
    band."""
    from gbvst.cycle_gan_model import CycleGANModel
    from gbvst.options import default_opt
    from oracle import cpu_ref, prng
    opt = default_opt(True, ngf=8, ndf=8, pool_size=0, gpu_ids=[0], netG="unet_128", no_dropout=True)
    m = CycleGANModel(opt)
    assert type(m.netG_A).__name__ == "UnetGenerator" and m.netG_A.num_downs == 7
    shapes = U.unet_shapes(3, 3, 7, 8)
    sds = {"G_A": U.make_state(751, shapes), "G_B": U.make_state(752, shapes)}
    dshape = cpu_ref.state_shapes(cpu_ref.RefNLayerDiscriminator(3, 8))
    sds["D_A"], sds["D_B"] = prng.init_state_dict(dshape, base_seed=753), prng.init_state_dict(dshape, base_seed=754)
    for name, sd in sds.items():
        getattr(m, "net" + name).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    t = _step_inputs(2, 128, 128)
    ref = _ref_step(sds, t)
    got_g, ref_g = [], []
    for s in range(2):
        ref.optimize_parameters(grad_hook_G=(lambda nets: ref_g.extend(_g_grads(nets))) if s == 0 else None)
        m.set_input_fc2((t[0], t[1], t[2], None, t[3], t[4]))
        m.optimize_parameters(grad_hook_G=(lambda nets: got_g.extend(_g_grads(nets))) if s == 0 else None)
        torch.cuda.synchronize()
        got, want = m.get_current_losses(), ref.get_current_losses()
        rel = {k: abs(got[k] - want[k]) / abs(want[k]) for k in want}
        print(f"step {s}: worst relative loss error {max(rel.values()):.3e} (bar 1e-3)", rel)
        assert max(rel.values()) <= 1e-3, (s, rel)
    bands = []

    def band():
        if not bands:
            b = [{}, {}]
            for sd in (0, 1, 2, 3):     # the seeds and eps of test_gpu_style._fsn_perturbed_bands
                pr = _ref_step(sds, t, perturb=sd)
                pg = []
                pr.optimize_parameters(grad_hook_G=lambda nets: pg.extend(_g_grads(nets)))
                for i in (0, 1):
                    for k in pg[i]:
                        b[i][k] = max(b[i].get(k, 0.0), _rel(pg[i][k], ref_g[i][k]))
            bands.append(b)
        return bands[0]

    zero = U.normed_bias_keys(7)
    worst = 0.0
    for i in (0, 1):
        gmax = max(float(v.abs().max()) for v in ref_g[i].values())
        for k, rg in ref_g[i].items():
            if k in zero:
                assert float(got_g[i][k].abs().max()) < 1e-3 * max(1.0, gmax), (i, k)
                continue
            e = _rel(got_g[i][k], rg)
            worst = max(worst, e)
            if e >= 1e-3:
                print(f"step 0: G_{'AB'[i]} {k}: {e:.3e}, the reference's own band {band()[i][k]:.3e}")
                assert e < band()[i][k], (i, k, e, band()[i][k])
    print(f"step 0: worst generator gradient {worst:.3e} (bar 1e-3)")
