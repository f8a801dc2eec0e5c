"""GPU parity of the temporal video style path: the fused masked-warp squared-difference loss
(csrc/temporal.hip: feature form, output form with the luminance input term), the bilinear plane
resize, their vst::* operators, and the Huang / ReCoNet train steps (gbvst.faststyle) against the CPU
reference composed in tests/temporal_style_ref.py from the oracle pieces pinned to the reference
(methods/learning-based/fs_huang.py:28-67, fs_reconet.py:28-78).

Bars.  Op level: loss and both gradients within 1e-5 relative (|err| <= 1e-5 max|ref| + 1e-6, the
bar of test_gpu_ops.test_losses for the CycleGAN temporal loss) of the composed form evaluated in fp64;
deterministic mode bit-equal run to run, atomic mode within 1e-5 max|ga| of it (test_gpu_det);
resize within 2e-6 max|ref| of F.interpolate (the warp golden's bound).  Step level: every loss of two
steps within 1e-3 relative, step-0 parameter gradients (norm-wise) within max(1e-3, the reference's own
movement under 1e-6 weight perturbations), as test_gpu_style.test_johnson_step_vs_reference_golden;
the step-level reference is evaluated in fp64 (temporal_style_ref.reference_run says why: its fp32
evaluation differs from its own fp64 evaluation by 7.9e-3 in the temporal-only gradients, one ReLU decision).
Inputs keep every warp sample's validity sum out of [0.9997, 0.99995] (asserted): the validity test
is a hard threshold at 0.9999 and no test may hinge on its rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import temporal_style_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


@pytest.fixture
def det(gb):
    from gbvst import ops
    prev = ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(prev)


def _close(got, ref, tol=1e-5, what=""):
    """tests/test_gpu_ops.py _close: |err| <= tol * max|ref| + 1e-6."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    print(f"{what}: max|err|={err:.3e} scale={scale:.3e}")
    assert err <= tol * scale + 1e-6, f"{what}: max|err|={err:.3e} scale={scale:.3e}"


def _close_scalar(got, ref, tol=1e-5, what="loss"):
    got, ref = float(got), float(ref)
    print(f"{what}: got {got:.9g} ref {ref:.9g} rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= tol * abs(ref), (what, got, ref)


def _nhwc(x, ops):
    return ops.nchw_to_nhwc(x.to(DEV).float().contiguous())


def _nchw(y, c, ops):
    return ops.nhwc_to_nchw(y.contiguous(), c).cpu()


def _ref64(a, b, flow, mask, scale, ab_scale=1.0, inputs=None):
    """The composed form in fp64 with autograd -> (loss, d/da, d/db)."""
    a, b = a.double().requires_grad_(True), b.double().requires_grad_(True)
    inputs = None if inputs is None else tuple(t.double() for t in inputs)
    loss = R.temporal_ref(a, b, flow.double(), mask.double(), scale, ab_scale, inputs)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def _run(ops, a, b, flow, mask, scale, cl, ab_scale=1.0, inputs=None, gout=1.0):
    """ops.temporal_sqdiff + _bwd on device tensors -> (loss, ga, gb)."""
    loss = ops.temporal_sqdiff(a, b, flow, mask, scale, cl, ab_scale, inputs)
    ga, gbt = torch.zeros_like(a), torch.empty_like(b)
    ops.temporal_sqdiff_bwd(a, b, flow, mask, torch.full((), gout, device=DEV), ga, gbt, scale, cl, ab_scale, inputs)
    return loss, ga, gbt


# ------------------------------------------------------------------------------- op level
# C4 = 1, the runtime path, C4 = 16 and C4 = 32 (the lane-transposed scatter; 20 * 32 is no multiple of 256)
@pytest.mark.parametrize("C", [4, 8, 64, 128])
def test_feature_form(gb, C):
    from gbvst import ops
    N, H, W = 2, 12, 20
    a, b = R.rand(910 + C, (N, C, H, W)), R.rand(911 + C, (N, C, H, W))
    flow = R.rand(901, (N, 2, H, W), 3.0)
    R.assert_off_threshold(flow)
    mask = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(905))   # fractional, as at feature size
    lr, gar, gbr = _ref64(a, b, flow, mask, 7.0)
    loss, ga, gbt = _run(ops, _nhwc(a, ops), _nhwc(b, ops), flow.to(DEV), mask.to(DEV), 7.0, C)
    _close_scalar(loss, lr)
    _close(_nchw(ga, C, ops), gar, 1e-5, "d/da")
    _close(_nchw(gbt, C, ops), gbr, 1e-5, "d/db")


def test_output_form_with_input_term(gb):
    from gbvst import ops
    N, H, W = 2, 17, 23
    a, b = R.rand(920, (N, 3, H, W), 60.0) + 127.0, R.rand(921, (N, 3, H, W), 60.0) + 127.0   # the net's 0..255 scale
    i1, i2 = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(s)) for s in (922, 923))
    flow = R.rand(902, (N, 2, H, W), 3.0)
    R.assert_off_threshold(flow)
    mask = (torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(924)) < 0.8).float()
    s = 1.0 / 255.0
    for inputs in ((i1, i2), None):    # ReCoNet's output loss; Huang's (no input term)
        lr, gar, gbr = _ref64(a, b, flow, mask, 50.0, s, inputs)
        dev_in = None if inputs is None else (_nhwc(i1, ops), _nhwc(i2, ops))
        loss, ga, gbt = _run(ops, _nhwc(a, ops), _nhwc(b, ops), flow.to(DEV), mask.to(DEV), 50.0, 3, s, dev_in)
        _close_scalar(loss, lr)
        _close(_nchw(ga, 3, ops), gar, 1e-5, "d/da")
        _close(_nchw(gbt, 3, ops), gbr, 1e-5, "d/db")
        assert float(gbt[..., 3].abs().max()) == 0.0      # the pad channel of gb is exactly 0
        assert float(ga[..., 3].abs().max()) == 0.0


def test_edge_flows(gb):
    from gbvst import ops
    N, C, H, W = 2, 8, 12, 20
    a, b = R.rand(930, (N, C, H, W)), R.rand(931, (N, C, H, W))
    mask = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(932))
    an, bn, mk = _nhwc(a, ops), _nhwc(b, ops), mask.to(DEV)
    # flow == 0.  The reference normalises the grid by W - 1 and samples with align_corners=False, so its warp by a
    # zero flow is NOT the identity (sample x = w W / (W - 1) - 0.5; column 0 is invalid; tests/golden fsw_zero_*):
    # the composed reference decides, and the unwarped form is checked with the flow that undoes that shift.
    zero = torch.zeros(N, 2, H, W)
    R.assert_off_threshold(zero)
    lr, gar, gbr = _ref64(a, b, zero, mask, 3.0)
    loss, ga, gbt = _run(ops, an, bn, zero.to(DEV), mk, 3.0, C)
    _close_scalar(loss, lr)
    _close(_nchw(ga, C, ops), gar, 1e-5, "zero flow d/da")
    _close(_nchw(gbt, C, ops), gbr, 1e-5, "zero flow d/db")
    xs, ys = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    ident = torch.stack([((xs + 0.5) * (W - 1) / W - xs).view(1, W).expand(H, W),
                         ((ys + 0.5) * (H - 1) / H - ys).view(H, 1).expand(H, W)])[None].repeat(N, 1, 1, 1).float()
    R.assert_off_threshold(ident)
    loss, ga, gbt = _run(ops, an, bn, ident.to(DEV), mk, 3.0, C)
    _close_scalar(loss, 3.0 * ((mask.double() * (b.double() - a.double())) ** 2).mean(), what="unwarped loss")
    _close(ga, -gbt, 1e-5, "ga == -gb without a warp")
    # flow == +1000: every sample invalid -> mean((m * (b - r))^2) * scale and no gradient into a
    far = torch.full((N, 2, H, W), 1000.0)
    loss, ga, gbt = _run(ops, an, bn, far.to(DEV), mk, 3.0, C)
    _close_scalar(loss, 3.0 * ((mask.double() * b.double()) ** 2).mean())
    assert float(ga.abs().max()) == 0.0
    a3, b3 = R.rand(933, (N, 3, H, W)), R.rand(934, (N, 3, H, W))
    i1, i2 = R.rand(935, (N, 3, H, W)), R.rand(936, (N, 3, H, W))
    loss, ga, _ = _run(ops, _nhwc(a3, ops), _nhwc(b3, ops), far.to(DEV), mk, 3.0, 3, 1.0,
                       (_nhwc(i1, ops), _nhwc(i2, ops)))
    r = (0.2126 * i2[:, 0] + 0.7152 * i2[:, 1] + 0.0722 * i2[:, 2]).unsqueeze(1).double()
    _close_scalar(loss, 3.0 * ((mask.double() * (b3.double() - r)) ** 2).mean())
    assert float(ga.abs().max()) == 0.0


@pytest.mark.parametrize("C,cl,with_inputs", [(128, 128, False), (4, 3, True)])
def test_determinism(det, C, cl, with_inputs):
    ops = det
    N, H, W = 2, 17, 23
    g = torch.Generator().manual_seed(940 + C)
    a, b = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    if cl < C:
        a[..., cl:] = 0
        b[..., cl:] = 0
    flow = R.rand(902, (N, 2, H, W), 3.0)
    mask = torch.rand(N, 1, H, W, generator=g)
    A, Bt, Fl, M = (t.to(DEV).contiguous() for t in (a, b, flow, mask))
    inputs = tuple(torch.rand(N, H, W, 4, generator=g).to(DEV) for _ in range(2)) if with_inputs else None
    l1, ga1, gb1 = _run(ops, A, Bt, Fl, M, 5.0, cl, 1.0, inputs, gout=1.7)
    l2, ga2, gb2 = _run(ops, A, Bt, Fl, M, 5.0, cl, 1.0, inputs, gout=1.7)
    assert torch.equal(l1, l2) and torch.equal(ga1, ga2) and torch.equal(gb1, gb2)
    ops.set_deterministic(False)
    l3, ga3, gb3 = _run(ops, A, Bt, Fl, M, 5.0, cl, 1.0, inputs, gout=1.7)
    l4, _, _ = _run(ops, A, Bt, Fl, M, 5.0, cl, 1.0, inputs, gout=1.7)
    ops.set_deterministic(True)
    assert torch.equal(l3, l4) and torch.equal(l3, l1)     # the forward has one (fixed-order) route
    assert torch.equal(gb3, gb1)
    assert (ga3 - ga1).abs().max().item() <= 1e-5 * ga1.abs().max().item()


@pytest.mark.parametrize("shape,size", [((2, 2, 32, 40), (8, 10)), ((1, 1, 17, 23), (5, 7)), ((2, 2, 7, 9), (16, 21))])
def test_resize_bilinear(gb, shape, size):
    from gbvst import library, ops  # noqa: F401  (library registers torch.ops.vst.*)
    x = R.rand(950, shape, 3.0)
    mult = [0.25, -1.5][:shape[1]]
    ref = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    got = ops.resize_bilinear(x.to(DEV), size).cpu()
    assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
    ref_m = ref * torch.tensor(mult).view(1, -1, 1, 1)
    got_m = ops.resize_bilinear(x.to(DEV), size, mult).cpu()
    assert (got_m - ref_m).abs().max().item() <= 2e-6 * ref_m.abs().max().item()
    assert torch.equal(torch.ops.vst.resize_bilinear(x.to(DEV), size[0], size[1], mult).cpu(), got_m)


def test_library_ops_and_autograd(gb):
    """vst::temporal_sqdiff / vst::resize_bilinear pass opcheck's schema, fake-tensor and autograd-registration
    checks; autograd through the operator and through fs_lib.temporal_loss_nhwc equals the op-level backward."""
    from gbvst import fs_lib, library, ops  # noqa: F401
    N, H, W = 2, 12, 20
    flow = R.rand(901, (N, 2, H, W), 3.0).to(DEV)
    mask = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(905)).to(DEV)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for C, inputs in ((8, None), (3, (R.rand(961, (N, 3, H, W)).to(DEV), R.rand(962, (N, 3, H, W)).to(DEV)))):
        a = R.rand(963, (N, C, H, W)).to(DEV).requires_grad_(True)
        b = R.rand(964, (N, C, H, W)).to(DEV).requires_grad_(True)
        i1, i2 = inputs if inputs is not None else (None, None)
        torch.library.opcheck(torch.ops.vst.temporal_sqdiff.default, (a, b, flow, mask, 4.0, 0.5, i1, i2),
                              test_utils=utils)
        loss = torch.ops.vst.temporal_sqdiff(a, b, flow, mask, 4.0, 0.5, i1, i2)
        (loss * 1.3).backward()
        an, bn = _nhwc(a.detach(), ops), _nhwc(b.detach(), ops)
        dev_in = None if inputs is None else (_nhwc(i1, ops), _nhwc(i2, ops))
        l0, ga, gbt = _run(ops, an, bn, flow, mask, 4.0, C, 0.5, dev_in, gout=1.3)
        assert torch.equal(loss.detach(), l0)
        atol = 1e-5 * float(ga.abs().max())        # ga: fp32 atomics, summation order only
        assert (a.grad.cpu() - _nchw(ga, C, ops)).abs().max().item() <= atol
        assert torch.equal(b.grad.cpu(), _nchw(gbt, C, ops))
        # the autograd-level NHWC entry
        x, y = an.clone().requires_grad_(True), bn.clone().requires_grad_(True)
        l1 = fs_lib.temporal_loss_nhwc(x, y, flow, mask, 4.0, inputs=dev_in, ab_scale=0.5, cl=C)
        torch.autograd.backward(l1, torch.full((), 1.3, device=DEV))
        assert torch.equal(l1.detach(), l0) and torch.equal(y.grad, gbt)
        assert (x.grad - ga).abs().max().item() <= atol
        # ... and its stacked-pair form (what the trainers call)
        xy = torch.cat([an, bn]).requires_grad_(True)
        l2 = fs_lib.temporal_loss_pair_nhwc(xy, flow, mask, 4.0, inputs=dev_in, ab_scale=0.5, cl=C)
        torch.autograd.backward(l2, torch.full((), 1.3, device=DEV))
        assert torch.equal(l2.detach(), l0) and torch.equal(xy.grad[N:], gbt)
        assert (xy.grad[:N] - ga).abs().max().item() <= atol
    torch.library.opcheck(torch.ops.vst.resize_bilinear.default, (flow, 3, 5, [0.25, 0.5]), test_utils=utils[:1] + utils[2:])


# ----------------------------------------------------------------------------- step level
def _fsn(base):
    from gbvst import faststyle
    from oracle import style_ref
    net = faststyle.FastStyleNet(3, 1).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         style_ref.fsn_weights(style_ref.RefFastStyleNet(3), base).items()})
    return net


def _vgg(base):
    from gbvst import perceptual
    from oracle import style_ref
    net = perceptual.Vgg16(DEV)
    sd = style_ref.vgg_weights(style_ref.RefVGG("vgg16"), base)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.bump_version()
    return net


def _nrel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


# the parameter tensors test_johnson_step_vs_reference_golden checks: first / last layers, both ends of the
# residual stack, a decoder layer
GRAD_KEYS = ["conv1.conv2d.weight", "conv2.conv2d.weight", "res1.conv1.conv2d.weight", "res5.conv2.conv2d.weight",
             "deconv1.conv2d.weight", "deconv3.conv2d.weight"]
METHODS = {"huang": ("Huang", R.HUANG_EMPH, R.HUANG_TEMPORAL_ONLY),
           "reconet": ("Reconet", R.RECONET_EMPH, R.RECONET_TEMPORAL_ONLY)}


def _trainer(method, emph):
    from gbvst import faststyle
    _, style, _, _ = R.step_inputs()
    return getattr(faststyle, METHODS[method][0])([style], emphasis=emph, lr=1e-3, batch_sz=2, device=DEV,
                                                  vgg=_vgg(R.VGG_SEED), model=_fsn(R.FSN_SEED))


def _check_grads(T, method, emph, grads_ref):
    params = dict(T.model.named_parameters())
    pert = [R.reference_run(method, emph, 1e-6, sd, 1)[1] for sd in (0, 1)]
    for k in GRAD_KEYS:
        band = max(_nrel(pg[k], grads_ref[k]) for pg in pert)
        err = _nrel(params[k].grad, grads_ref[k])
        print(f"{method} {k}: nrel {err:.3e} band {band:.3e}")
        assert err < max(1e-3, band), (k, err, band)


def _check_inputs():
    imgs, _, mask, flow = R.step_inputs()
    R.assert_off_threshold(flow)
    ff, _ = R.feature_flow_mask(flow, mask, R.H // 4, R.W // 4)
    R.assert_off_threshold(ff)
    assert 0.1 < float((mask == 0).float().mean()) < 0.3


@pytest.mark.parametrize("method", ["huang", "reconet"])
def test_train_step_vs_reference(gb, train_math, method):
    """Two train steps with an Adam update between them: every loss within 1e-3 relative of the reference and
    no reference term below 1 % of its total; step-0 parameter gradients within max(1e-3, band)."""
    from gbvst import ops
    _check_inputs()
    emph = METHODS[method][1]
    losses_ref, grads_ref = R.reference_run(method, emph)
    T = _trainer(method, emph)
    imgs, _, mask, flow = R.step_inputs()
    x = ops.nchw_to_nhwc(torch.cat(imgs).to(DEV))
    for s in range(2):
        ref = np.array(losses_ref[s])
        assert (np.abs(ref[1:]) >= 0.01 * abs(ref[0])).all(), ref      # the total cannot hide a term
        T.adam.zero_grad()
        out = T.losses_nhwc(x, flow.to(DEV), mask.to(DEV))
        out[0].backward()
        got = np.array([float(v) for v in out[:-1]])
        rel = np.abs(got - ref) / np.abs(ref)
        print(method, "step", s, "losses", got, "rel", rel)
        assert got.shape == ref.shape and rel.max() < 1e-3, (s, rel)
        if s == 0:
            _check_grads(T, method, emph, grads_ref)
        T.adam.step()


@pytest.mark.parametrize("method", ["huang", "reconet"])
def test_temporal_only_gradients(gb, train_math, method):
    """alpha = beta = delta = 0: the parameter gradients come from the fused temporal kernels alone (ReCoNet: the
    feature-map loss into the net's feature gradient and the output loss), so they cannot hide behind the style term."""
    from gbvst import ops
    _check_inputs()
    emph = METHODS[method][2]
    losses_ref, grads_ref = R.reference_run(method, emph, steps=1)
    T = _trainer(method, emph)
    imgs, _, mask, flow = R.step_inputs()
    T.adam.zero_grad()
    out = T.losses_nhwc(ops.nchw_to_nhwc(torch.cat(imgs).to(DEV)), flow.to(DEV), mask.to(DEV))
    out[0].backward()
    assert abs(float(out[0]) - losses_ref[0][0]) <= 1e-3 * abs(losses_ref[0][0])
    _check_grads(T, method, emph, grads_ref)


def test_train_step_interface(gb):
    """train_step on the reference's layout (imgs list, masks [B,k,H,W], flows [B,2k,H,W]; pair 0 is used): the
    loss graph's values as device scalars in the reference's order, styled frame 2, and one Adam update (every
    parameter moves by at most lr on the first step)."""
    from gbvst import ops
    imgs, _, mask, flow = R.step_inputs()
    masks = torch.cat([mask, torch.zeros_like(mask)], 1)
    flows = torch.cat([flow, torch.full_like(flow, 50.0)], 1)
    for method, n in (("huang", 5), ("reconet", 6)):
        T, U = _trainer(method, METHODS[method][1]), _trainer(method, METHODS[method][1])
        p0 = T.model.flat_param.clone()
        losses, styled2 = T.train_step(imgs, masks, flows)
        out = U.losses_nhwc(ops.nchw_to_nhwc(torch.cat(imgs).to(DEV)), flow.to(DEV), mask.to(DEV))
        assert len(losses) == n and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in losses)
        for v, w in zip(losses, out[:-1]):
            assert abs(float(v) - float(w)) <= 1e-5 * abs(float(w))
        assert styled2.shape == (R.B, R.H, R.W, 4)
        assert (styled2 - out[-1][R.B:]).abs().max().item() <= 1e-4 * 255.0
        step = (T.model.flat_param - p0).abs()
        assert T.itr == 1 and 0.0 < float(step.max()) <= 1e-3 * (1 + 1e-3)
        frame = T.infer_method(imgs[1])
        assert frame.shape == (R.B, 3, R.H, R.W) and -0.1 <= float(frame.min()) and float(frame.max()) <= 1.1
