"""GPU parity of the multi-style fast-style path: the conditional InstanceNorm kernels (csrc/norm.hip cond_*), the
multi-style net and the Dumoulin train step.

Op level — against the fp64 references of tests/reduction_ref.py (in_affine_fwd / in_affine_bwd per sample, with that
sample's effective gamma = ge * w and beta = ge * b + be), per (n, c) plane or per channel, with the bars of
test_gpu_reductions.test_instnorm_affine_geometry:
  forward 1e-5 of max|ref|; dx 1e-4 of max|ref|; parameter gradients 1e-4 relative + 8 u sum|term| (no fp32
  evaluation of the terms, <= 8 roundings each and summed in fp64, can do better; u = 2^-24) + one rounding of the
  accumulate; the conv-bias gradient (0 in exact arithmetic) within 1e-5 sum|dx|.
  For relu the seeds keep the reference's own min|z| / max|z| >= 1e-6 (asserted): the device's z may be an fma.
  Rows of dE for absent styles, and the pad channels of y and dx, are exactly 0; two runs are bit-equal.
Net level — against tests/golden/multistyle_small.npz (produced by the reference's modules): outputs 1e-4 of
  max|ref|; the input gradient (norm-wise) and the parameter gradients (max-relative) within max(1e-3, band), band =
  how far the CPU reference's own gradients move when its weights are scaled by (1 + 1e-6 N(0, 1)), as
  test_gpu_style.test_faststylenet_vs_reference_golden computes it; per-sample ids against RefMultiStyleNet in fp64
  at 1e-4.
Step level — two Dumoulin.train_steps against multistyle_ref.dumoulin_losses + torch.optim.Adam in fp64: losses
  1e-3 relative; step-0 gradients norm-wise within max(1e-3, band) as test_johnson_step_vs_reference_golden;
  infer_method 1e-3 of max|ref|."""
import functools

import numpy as np
import pytest
import torch

import multistyle_ref as MR
import reduction_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
U = 2.0 ** -24
EPS = R.f32(1e-5)


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


def _randn(seed, shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _le(err, tol, what):
    err, tol = torch.as_tensor(err, dtype=F64), torch.as_tensor(tol, dtype=F64)
    tol = tol.expand_as(err)
    ok = err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(F64))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{what}: worst err/bound = {worst:.3g} (max err {err.max().item():.3e})")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst err/bound {worst:.3g}"


def _pmax(t):
    return t.abs().amax(dim=(2, 3))


# ============================================================================= op level
# id: ((N, H, W, C), Cl, S, ids, relu seed).  The first five are reduction_ref.IN_CASE geometries with N >= 2; then a
# repeated id + an unused style, one sample over many slices (nsplit 200), and real channels Cl < C.  The seeds were
# picked on the CPU so that the fp64 reference's pre-activation keeps clear of 0 (asserted in the relu cases).
def _in(case):
    return R.IN_CASE[case][1]


OP_CASES = {
    "tail_cpb4": (_in("tail_cpb4"), 64, 3, [2, 0], 4110),
    "lp3": (_in("lp3"), 12, 3, [1, 1], 4200),
    "lp18": (_in("lp18"), 72, 3, [0, 2], 4300),
    "tiny_hw": (_in("tiny_hw"), 64, 3, [1, 0, 1], 4400),
    "c8": (_in("c8"), 8, 4, [0, 2, 2, 1], 4500),
    "repeat_unused": ((3, 17, 23, 32), 32, 4, [2, 0, 2], 4600),
    "one_sample": ((1, 40, 40, 128), 128, 3, [1], 4703),
    "pad_channels": ((2, 11, 13, 16), 13, 3, [2, 1], 4800),
    # rows reach the 4x unrolled loop of the partial walk, with a remainder and a ragged last slice
    "part_unrolled_6": (_in("part_unrolled_6"), 128, 3, [2, 0], 4900),
    "c1024_unrolled": (_in("c1024_unrolled"), 1024, 3, [1], 5000),
}
# These run without an activation: at 2.8 M elements no seed keeps |z| clear of 0 (the relu condition below), and
# the walk does not depend on the activation.
OP_UNROLLED = ("part_unrolled_6", "c1024_unrolled")
OP_PARAMS = [(c, a) for c in OP_CASES for a in ("none", "relu") if a == "none" or c not in OP_UNROLLED]
assert all(R.IN_CASE[c][1][0] >= 2 for c in ("tail_cpb4", "lp3", "lp18", "tiny_hw", "c8"))


@functools.lru_cache(maxsize=2)
def _op_data(case):
    (N, H, W, C), Cl, S, ids, seed = OP_CASES[case]
    x = 2.0 * _randn(seed, (N, H, W, C)) + 0.5
    g = _randn(seed + 1, (N, H, W, C))
    E = torch.cat([1.0 + _randn(seed + 2, (S, Cl), 0.2), _randn(seed + 3, (S, Cl), 0.2)], dim=1).contiguous()
    w, b = 1.0 + _randn(seed + 4, (Cl,), 0.2), _randn(seed + 5, (Cl,), 0.2)
    x64 = R.nchw64(x, Cl)
    mean, rstd = R.in_stats(x64, EPS)
    ge, be = E[ids, :Cl].to(F64), E[ids, Cl:].to(F64)
    gam, bet = ge * w.to(F64), ge * b.to(F64) + be          # [N, Cl] effective affine per sample
    return x, g, E, w, b, x64, R.nchw64(g, Cl), mean, rstd, gam, bet


def _op_reference(case, act):
    """Per-sample in_affine_fwd / in_affine_bwd, then the chain rule into E, bn.weight, bn.bias."""
    (N, H, W, C), Cl, S, ids, _ = OP_CASES[case]
    x, g, E, w, b, x64, g64, mean, rstd, gam, bet = _op_data(case)
    w64, b64 = w.to(F64), b.to(F64)
    ys, dxs, zs = [], [], []
    dE, dE_abs = torch.zeros(S, 2 * Cl, dtype=F64), torch.zeros(S, 2 * Cl, dtype=F64)
    dw, dw_abs, db, db_abs = (torch.zeros(Cl, dtype=F64) for _ in range(4))
    dbias = torch.zeros(Cl, dtype=F64)
    for n in range(N):
        sl = slice(n, n + 1)
        ys.append(R.in_affine_fwd(x64[sl], mean[sl], rstd[sl], gam[n], bet[n], act, 0.0))
        r = R.in_affine_bwd(g64[sl], x64[sl], mean[sl], rstd[sl], gam[n], bet[n], act, 0.0)
        dxs.append(r["dx"])
        zs.append(r["z"])
        sgx, sg, sgx_a, sg_a = r["dgamma"], r["dbeta"], r["dgamma_abs"], r["dbeta_abs"]
        s, ge = ids[n], E[ids[n], :Cl].to(F64)
        dE[s, :Cl] += w64 * sgx + b64 * sg
        dE[s, Cl:] += sg
        dE_abs[s, :Cl] += w64.abs() * sgx_a + b64.abs() * sg_a
        dE_abs[s, Cl:] += sg_a
        dw += ge * sgx
        db += ge * sg
        dw_abs += ge.abs() * sgx_a
        db_abs += ge.abs() * sg_a
        dbias += r["dbias"]
    dx = torch.cat(dxs)
    return dict(y=torch.cat(ys), dx=dx, z=torch.cat(zs), dembed=dE, dembed_abs=dE_abs, dbn_w=dw, dbn_w_abs=dw_abs,
                dbn_b=db, dbn_b_abs=db_abs, dbias=dbias, dx_abs=dx.abs().sum(dim=(0, 2, 3)))


@pytest.mark.parametrize("case,act", OP_PARAMS, ids=["-".join(p) for p in OP_PARAMS])
def test_cond_instnorm_geometry(gb, case, act):
    from gbvst import ops
    (N, H, W, C), Cl, S, ids, _ = OP_CASES[case]
    x, g, E, w, b = _op_data(case)[:5]
    ref = _op_reference(case, act)
    tag = f"{case}/{act}"
    if act == "relu":
        margin = (ref["z"].abs().min() / ref["z"].abs().max()).item()
        print(tag, "z margin", margin)
        assert margin >= 1e-6
    accumulate = act == "relu"
    xd, gd, Ed, wd, bd = (t.to(DEV) for t in (x, g, E, w, b))
    sid = ops.style_ids(ids, N, S, DEV)
    assert sid.dtype == torch.int32 and sid.is_cuda and sid.tolist() == ids
    st = ops.instnorm_stats(xd)
    base = 0.25 if accumulate else 0.0
    init = 0.25 if accumulate else float("nan")

    def run():
        y = ops.cond_instnorm_fwd(xd, st, sid, Ed, wd, bd, act)
        bufs = dict(dembed=torch.full((S, 2 * Cl), init, device=DEV), dbn_w=torch.full((Cl,), init, device=DEV),
                    dbn_b=torch.full((Cl,), init, device=DEV), dbias=torch.full((Cl,), init, device=DEV))
        dx = ops.cond_instnorm_bwd(gd, xd, st, sid, Ed, wd, bd, act, accumulate=accumulate, **bufs)
        return y, dx, bufs

    y, dx, bufs = run()
    _le(_pmax(R.nchw64(y, Cl) - ref["y"]), 1e-5 * _pmax(ref["y"]), tag + " fwd")
    dgot = R.nchw64(dx, Cl)
    assert torch.isfinite(dgot).all()
    _le(_pmax(dgot - ref["dx"]), 1e-4 * _pmax(ref["dx"]), tag + " dx")
    if Cl < C:      # pad channels: exactly 0 whatever x and gy hold there
        assert float(y[..., Cl:].abs().max()) == 0.0 and float(dx[..., Cl:].abs().max()) == 0.0
    for k, buf in bufs.items():
        got = buf.cpu().to(F64) - base
        assert torch.isfinite(got).all(), k
        want = ref[k]
        if k == "dbias":
            tol = 1e-5 * ref["dx_abs"]
        else:
            tol = 1e-4 * want.abs() + 8 * U * ref[k + "_abs"] + 2 * U * (base + want.abs())
        _le((got - want).abs(), tol, f"{tag} {k}")
    absent = [s for s in range(S) if s not in ids]
    for s in absent:        # written, and exactly zero (or exactly the preset it was added to)
        assert bool((bufs["dembed"][s] == base).all()), (tag, s)
    # bit-equal on a second run (fixed-order fp64 reductions, no atomics)
    y2, dx2, bufs2 = run()
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    for k in bufs:
        assert torch.equal(bufs[k], bufs2[k]), k


def test_every_op_case_has_an_absent_style_somewhere():
    """The absent-row check above runs: most cases leave at least one style of S unused."""
    n = sum(1 for (_, _, S, ids, _) in OP_CASES.values() if set(range(S)) - set(ids))
    assert n >= 6 and set(OP_CASES["repeat_unused"][3]) == {0, 2} and OP_CASES["repeat_unused"][2] == 4


def test_host_ids_out_of_range_raise(gb):
    from gbvst import faststyle, ops
    for bad in (3, -1, [0, 3], torch.tensor(3), torch.tensor(-1.5)):
        with pytest.raises(ValueError):
            ops.style_ids(bad, 2, 3, DEV)
    net = faststyle.MultiStyleNet(3, 3).to(DEV)
    x = torch.rand(2, 3, 8, 8, device=DEV)
    with torch.no_grad():
        for bad in (3, [0, 5], torch.tensor(7)):
            with pytest.raises(ValueError):
                net(x, s_id=bad)
        with pytest.raises(ValueError):
            net(x, s_id=[0, 1, 2])
    # a device tensor is converted on the device: float ids truncate like .long()
    assert ops.style_ids(torch.tensor([1.9, 0.3], device=DEV), 2, 3, DEV).tolist() == [1, 0]
    assert ops.style_ids(torch.tensor(2.5, device=DEV), 3, 3, DEV).tolist() == [2, 2, 2]


def test_library_op_equals_ops_path(gb):
    from gbvst import library, ops  # noqa: F401
    N, C, H, W, S = 2, 32, 12, 20, 3
    x = (2.0 * _randn(1, (N, C, H, W)) + 0.5).to(DEV)
    gy = _randn(2, (N, C, H, W)).to(DEV)
    E = torch.cat([1.0 + _randn(3, (S, C), 0.2), _randn(4, (S, C), 0.2)], dim=1).to(DEV)
    w, b = (1.0 + _randn(5, (C,), 0.2)).to(DEV), _randn(6, (C,), 0.2).to(DEV)
    sid = ops.style_ids([2, 0], N, S, DEV)
    for act in ("relu", "none"):
        xn = ops.nchw_to_nhwc(x)
        st = ops.instnorm_stats(xn)
        y_ops = ops.nhwc_to_nchw(ops.cond_instnorm_fwd(xn, st, sid, E, w, b, act), C)
        de, dw, db = torch.empty_like(E), torch.empty_like(w), torch.empty_like(b)
        dx_ops = ops.nhwc_to_nchw(ops.cond_instnorm_bwd(ops.nchw_to_nhwc(gy), xn, st, sid, E, w, b, act, dembed=de,
                                                        dbn_w=dw, dbn_b=db, accumulate=False), C)
        xr, Er, wr, br = (t.clone().requires_grad_(True) for t in (x, E, w, b))
        y = torch.ops.vst.cond_instance_norm(xr, sid, Er, wr, br, act)
        y.backward(gy)
        assert torch.equal(y.detach(), y_ops), act
        assert torch.equal(xr.grad, dx_ops) and torch.equal(Er.grad, de), act
        assert torch.equal(wr.grad, dw) and torch.equal(br.grad, db), act
        assert float(Er.grad[1].abs().max()) == 0.0 and float(Er.grad[2].abs().max()) > 0.0
    with pytest.raises(ValueError):
        torch.ops.vst.cond_instance_norm(x, sid, E, w, b, "lrelu")


# ============================================================================= net level
BASE, GF, GI, STRENGTH = 560, 562, 563, 0.8     # tools/gen_golden_multistyle.py


def _rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def _nrel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


def _msn(base, n_styles=3):
    from gbvst import faststyle
    from oracle import style_ref
    net = faststyle.MultiStyleNet(3, n_styles).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         style_ref.fsn_weights(MR.RefMultiStyleNet(3, n_styles), base).items()})
    return net


def _perturb(modules, eps, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in modules:
            for p in m.parameters():
                p.mul_(1 + eps * torch.randn(p.shape, generator=gen, dtype=p.dtype))


@functools.lru_cache(maxsize=None)
def _net_bands(sid, eps=1e-6, seeds=(0, 1, 2, 3)):
    """(dx band (norm-wise), {param: band (max-relative)}): the CPU reference's own movement against the fixture
    under (1 + eps N(0, 1)) weight perturbations (test_gpu_style._fsn_perturbed_bands)."""
    from oracle import prng
    g = np.load(MR.__file__.replace("multistyle_ref.py", "golden/multistyle_small.npz"), allow_pickle=False)
    dxb, pb = 0.0, {}
    for sd in seeds:
        m = MR.make(3, 3, BASE)
        _perturb([m], eps, sd)
        x = torch.from_numpy(g["x"]).requires_grad_(True)
        feats, img = m(x, STRENGTH, torch.tensor(sid))
        gf = torch.from_numpy(prng.normal(GF, tuple(feats.shape)))
        gi = torch.from_numpy(prng.normal(GI, tuple(img.shape)))
        ((feats * gf).sum() + (img * gi).sum()).backward()
        dxb = max(dxb, _nrel(x.grad, g[f"s{sid}_dx"]))
        for k, p in m.named_parameters():
            key = f"s{sid}_g_{k}"
            if key in g.files:
                pb[k] = max(pb.get(k, 0.0), _rel(p.grad[:g[key].shape[0]], g[key]))
    return dxb, pb


@pytest.fixture(scope="module")
def msn(gb):
    return _msn(BASE)


@pytest.mark.parametrize("sid", [0, 2])
def test_multistylenet_vs_reference_golden(msn, golden, sid):
    from oracle import prng
    g = golden("multistyle_small")
    msn.zero_grad()
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    feats, img = msn(x, STRENGTH, s_id=sid)
    ef, ei = _rel(feats, g[f"s{sid}_feats"]), _rel(img, g[f"s{sid}_img"])
    print("sid", sid, "feats", ef, "img", ei)
    assert ef < 1e-4 and ei < 1e-4
    gf = torch.from_numpy(prng.normal(GF, tuple(feats.shape))).to(DEV)
    gi = torch.from_numpy(prng.normal(GI, tuple(img.shape))).to(DEV)
    ((feats * gf).sum() + (img * gi).sum()).backward()
    err = _nrel(x.grad, g[f"s{sid}_dx"])
    print("sid", sid, "dx nrel", err)
    if err >= 1e-3:
        assert err < _net_bands(sid)[0], (err, _net_bands(sid)[0])
    params = dict(msn.named_parameters())
    keys = [k[len(f"s{sid}_g_"):] for k in g.files if k.startswith(f"s{sid}_g_")]
    assert set(MR.COND_KEYS) <= set(keys) and len(keys) == 21
    for k in keys:
        ref = g[f"s{sid}_g_{k}"]
        e = _rel(params[k].grad[:ref.shape[0]], ref)
        print("sid", sid, k, "rel", e)
        if e >= 1e-3:
            assert e < _net_bands(sid)[1][k], (k, e, _net_bands(sid)[1][k])
    for layer in MR.WIDTHS:     # dense embedding gradient: rows of the styles not used are exactly zero
        ge = params[layer + ".instance.embed.weight"].grad
        assert all(float(ge[r].abs().max()) == 0.0 for r in range(3) if r != sid) and float(ge[sid].abs().max()) > 0


def test_float_id_truncates_bit_equal(msn, golden):
    g = golden("multistyle_small")
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        a = msn(x, STRENGTH, s_id=torch.tensor(1.7, device=DEV))
        b = msn(x, STRENGTH, s_id=1)
        c = msn(x, STRENGTH, s_id=torch.tensor(1.7))
        d = msn(x, STRENGTH, s_id=torch.tensor(1, device=DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(c[1], b[1]) and torch.equal(d[1], b[1])
    assert _rel(a[1], g["f17_img"]) < 1e-4
    assert _rel(msn(x, STRENGTH, s_id=2)[1].detach(), g["f17_img"]) > 1e-3


def test_per_sample_ids_vs_reference_fp64(msn):
    ids = [2, 0, 2]
    x = torch.rand(3, 3, 24, 32, generator=torch.Generator().manual_seed(77))
    ref = MR.make(3, 3, BASE, F64)
    with torch.no_grad():
        fr, ir = ref(x.double(), STRENGTH, torch.tensor(ids))
        outs = [msn(x.to(DEV), STRENGTH, s_id=s) for s in (ids, torch.tensor(ids, device=DEV), torch.tensor(ids))]
    for f, im in outs:
        assert _rel(f, fr) < 1e-4 and _rel(im, ir) < 1e-4
        assert torch.equal(f, outs[0][0]) and torch.equal(im, outs[0][1])
    # samples 0 and 2 carry the same style but different images
    assert not torch.equal(outs[0][1][0], outs[0][1][2])


# ============================================================================= step level
# beta: the fp64 reference's Gram term is ~60 per unit beta on these inputs, its content term ~5 per unit alpha
STEP_BASE, VGG_BASE, EMPH, STEP_IDS = 570, 550, (1.0, 0.1), (2, 0)
GRAD_KEYS = ("conv1.conv2d.weight", "conv2.conv2d.weight", "res1.conv1.conv2d.weight", "res5.conv2.conv2d.weight",
             "deconv1.conv2d.weight", "deconv3.conv2d.weight")


def _step_inputs():
    gen = torch.Generator().manual_seed(571)
    styles = [torch.rand(1, 3, 32, 32, generator=gen) for _ in range(3)]
    return torch.rand(2, 3, 24, 32, generator=gen), styles


@functools.lru_cache(maxsize=None)
def _step_reference(eps=0.0, seed=0, steps=2):
    """fp64: (losses per step [(total, content, style)], step-0 gradients by name, the model after the steps)."""
    from oracle import style_ref
    img, styles = _step_inputs()
    model = MR.make(3, 3, STEP_BASE, F64)
    vgg = style_ref.RefVGG("vgg16")
    style_ref.load_np(vgg, style_ref.vgg_weights(vgg, VGG_BASE))
    vgg = vgg.double()
    if eps:
        _perturb([model, vgg], eps, seed)
    with torch.no_grad():
        grams = [[style_ref.gram_matrix(f) for f in vgg(style_ref.normalize(s.double()))] for s in styles]
    adam = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses, grads = [], {}
    for s in range(steps):
        adam.zero_grad()
        ls = MR.dumoulin_losses(model, vgg, img.double(), grams, *EMPH, STEP_IDS[s])
        ls[0].backward()
        losses.append([float(v.detach()) for v in ls[:3]])
        if s == 0:
            grads = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
        adam.step()
    return losses, grads, model


def _vgg16(base):
    from gbvst import perceptual
    from oracle import style_ref
    net = perceptual.Vgg16(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         style_ref.vgg_weights(style_ref.RefVGG("vgg16"), base).items()})
    net.bump_version()
    return net


def test_dumoulin_train_steps_vs_reference(gb):
    from gbvst import faststyle
    img, styles = _step_inputs()
    losses_ref, grads_ref, _ = _step_reference()
    D = faststyle.Dumoulin(styles, emphasis=EMPH, lr=1e-3, batch_sz=2, device=DEV, vgg=_vgg16(VGG_BASE),
                           model=_msn(STEP_BASE))
    assert D.n_styles == 3 and isinstance(D.model, faststyle.MultiStyleNet)
    params = dict(D.model.named_parameters())
    emb0 = {l: params[l + ".instance.embed.weight"].detach().clone() for l in MR.WIDTHS}
    for s, sid in enumerate(STEP_IDS):
        ref = np.array(losses_ref[s])
        assert (np.abs(ref[1:]) >= 0.01 * abs(ref[0])).all(), ref          # the total cannot hide a term
        (total, cl, sl), styled = D.train_step(img, style_id=sid)
        got = np.array([float(total), float(cl), float(sl)])
        rel = np.abs(got - ref) / np.abs(ref)
        print("dumoulin step", s, "style", sid, "losses", got, "rel", rel)
        assert rel.max() < 1e-3, (s, rel)
        assert styled.shape == (2, 24, 32, 4)
        if s == 0:
            pert = [_step_reference(1e-6, sd, 1)[1] for sd in (0, 1)]
            for k in MR.COND_KEYS + GRAD_KEYS:
                band = max(_nrel(pg[k], grads_ref[k]) for pg in pert)
                err = _nrel(params[k].grad, grads_ref[k])
                print(f"dumoulin {k}: nrel {err:.3e} band {band:.3e}")
                assert err < max(1e-3, band), (k, err, band)
            for l in MR.WIDTHS:      # only the drawn style's row learns: zero gradient, zero Adam update
                e = params[l + ".instance.embed.weight"].detach()
                assert torch.equal(e[0], emb0[l][0]) and torch.equal(e[1], emb0[l][1]), l
                assert not torch.equal(e[2], emb0[l][2]), l
    assert D.itr == 2
    with pytest.raises(ValueError):
        D.train_step(img, style_id=3)
    assert ((2, 2) in D._gram_cache) and ((2, 0) in D._gram_cache) and len(D._gram_cache) == 2
    # infer_method against the CPU net carrying the trained weights
    ref = MR.RefMultiStyleNet(3, 3)
    ref.load_state_dict({k: v.detach().cpu() for k, v in D.model.state_dict().items()})
    ref = ref.double()
    frame = torch.rand(1, 3, 24, 32, generator=torch.Generator().manual_seed(572))
    for sid in (2, 1):
        with torch.no_grad():
            want = ref(frame.double(), 1.0, torch.tensor(sid))[1] / 255.0
        got = D.infer_method(frame, style_id=sid)
        e = _rel(got, want)
        print("infer style", sid, "rel", e)
        assert got.shape == (1, 3, 24, 32) and e < 1e-3


def test_dumoulin_draws_when_no_id_given(gb):
    """train_step(img) makes the reference's one np.random.randint draw and trains that style's rows only."""
    from gbvst import faststyle
    img, styles = _step_inputs()
    D = faststyle.Dumoulin(styles, emphasis=[(1.0, 0.1), (1.0, 0.2), (0.5, 0.1)], lr=1e-3, batch_sz=2, device=DEV,
                           vgg=_vgg16(VGG_BASE), model=_msn(STEP_BASE))
    np.random.seed(99)
    want = int(np.random.randint(0, 3))
    tail = np.random.random()
    np.random.seed(99)
    e0 = D.model.conv1.instance.embed.weight.detach().clone()
    D.train_step(img)
    assert np.random.random() == tail
    e1 = D.model.conv1.instance.embed.weight.detach()
    assert [not torch.equal(e0[r], e1[r]) for r in range(3)] == [r == want for r in range(3)]
    assert list(D._gram_cache) == [(2, want)]
