"""GPU parity of the Ruder recurrent video style path (methods/learning-based/fs_ruder.py:38-121): the
recurrence glue kernels (csrc/ruder.hip: input stacking with the masked warp, its combined scatter backward,
the last-frame temporal loss), their vst::* operators, FastStyleNet(7, 1) -- the 8-channel-padded input through
conv1, its weight gradient and its input data gradient -- and the Ruder train step / inference entries
(gbvst.faststyle.Ruder) against the CPU reference composed in tests/ruder_ref.py from the oracle pieces pinned
to the reference.

Bars.  Op level: within 1e-5 relative (|err| <= 1e-5 max|ref| + 1e-6, the bar of test_gpu_temporal_style) of the
composed form in fp64; deterministic mode bit-equal run to run, atomic mode within 1e-5 max of it.
FastStyleNet(7, 1): outputs at 1e-4 (test_gpu_style.test_faststylenet_vs_reference_golden), gradients norm-wise
within max(1e-3, the reference's own movement under 1e-6 weight perturbations), as
test_gpu_style.test_johnson_step_vs_reference_golden.  Step level: every loss within 1e-3 relative, step-0
parameter gradients within max(1e-3, band), as test_gpu_temporal_style.test_train_step_vs_reference.
Inputs keep every warp sample's validity sum out of [0.9997, 0.99995] (asserted)."""
import functools

import numpy as np
import pytest
import torch

import ruder_ref as RR
import temporal_style_ref as R
from test_gpu_temporal_style import GRAD_KEYS, _close, _close_scalar, _nrel, _vgg

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 1.0 / 255.0
SHAPES = [(2, 12, 20), (2, 17, 23)]
FLOW_SEED = {(2, 12, 20): 901, (2, 17, 23): 902}      # the seeds test_gpu_temporal_style uses at these sizes


@pytest.fixture(scope="module")
def gb():
    import gbvst
    from gbvst import library  # noqa: F401  (registers torch.ops.vst.*)
    gbvst._lib.load()
    return gbvst


@pytest.fixture
def det(gb):
    from gbvst import ops
    prev = ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(prev)


def _nhwc(x, ops):
    return ops.nchw_to_nhwc(x.to(DEV).float().contiguous())


def _nchw(y, c, ops):
    return ops.nhwc_to_nchw(y.contiguous(), c).cpu()


@functools.lru_cache(maxsize=None)
def _op_inputs(shape, flow_kind="rand"):
    """(y_prev 0..255, img [0,1], flow, binary mask, gx [N,7,H,W], gw [N,3,H,W]) on the CPU, fp32."""
    N, H, W = shape
    y = R.rand(970, (N, 3, H, W), 60.0) + 127.0            # the net's 0..255 scale
    img = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(971))
    if flow_kind == "rand":
        flow = R.rand(FLOW_SEED[shape], (N, 2, H, W), 3.0)
    else:
        flow = torch.full((N, 2, H, W), float(flow_kind))
    mask = (torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(972)) < 0.8).float()
    gx, gw = R.rand(973, (N, 7, H, W)), R.rand(974, (N, 3, H, W))
    if flow_kind != 1000.0:
        R.assert_off_threshold(flow)
    return y, img, flow, mask, gx, gw


@functools.lru_cache(maxsize=None)
def _stack_ref64(shape, flow_kind="rand"):
    """The composed form in fp64 -> (x, w, d/dy from gx alone, from gw alone, from both)."""
    y, img, flow, mask, gx, gw = (t.double() for t in _op_inputs(shape, flow_kind))
    grads = []
    for use_x, use_w in ((True, False), (False, True), (True, True)):
        yr = y.clone().requires_grad_(True)
        x, w = RR.stack_ref(yr, img, flow, mask)
        ((x * gx).sum() * float(use_x) + (w * gw).sum() * float(use_w)).backward()
        grads.append(yr.grad)
    return (x.detach(), w.detach()) + tuple(grads)


# ------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("shape", SHAPES)
def test_stack_forward(gb, shape):
    from gbvst import fs_lib, ops
    y, img, flow, mask, _, _ = _op_inputs(shape)
    xr, wr = _stack_ref64(shape)[:2]
    yn = _nhwc(y, ops)
    yn[..., 3] = 7.0                     # whatever the pad channel of the previous frame holds stays out
    x, w = ops.ruder_stack(yn, _nhwc(img, ops), flow.to(DEV), mask.to(DEV))
    assert x.shape == shape + (8,) and w.shape == shape + (4,)
    _close(_nchw(x, 7, ops), xr, 1e-5, "x")
    _close(_nchw(w, 3, ops), wr, 1e-5, "w")
    assert torch.equal(x[..., 4:7], w[..., :3])
    assert float(x[..., 7].abs().max()) == 0.0 and float(w[..., 3].abs().max()) == 0.0
    assert torch.equal(x[..., :3].cpu(), img.permute(0, 2, 3, 1)) and torch.equal(x[..., 3].cpu(), mask[:, 0])
    assert float(w.abs().max()) > 0.1    # the warp is not vacuous
    # the autograd node and the w-less inference form return the same bits
    x2, w2 = fs_lib.ruder_stack_nhwc(yn, _nhwc(img, ops), flow.to(DEV), mask.to(DEV))
    x3, none = ops.ruder_stack(yn, _nhwc(img, ops), flow.to(DEV), mask.to(DEV), want_w=False)
    assert torch.equal(x2, x) and torch.equal(w2, w) and torch.equal(x3, x) and none is None


@pytest.mark.parametrize("shape", SHAPES)
def test_stack_blank(gb, shape):
    from gbvst import fs_lib, ops
    img = _op_inputs(shape)[1]
    im = _nhwc(img, ops)
    im[..., 3] = 3.0                     # the image's pad channel does not leak into the mask channel
    x, w = ops.ruder_stack(None, im, None, None)
    assert x.shape == shape + (8,) and float(x[..., 3:].abs().max()) == 0.0 and float(w.abs().max()) == 0.0
    assert torch.equal(x[..., :3].cpu(), img.permute(0, 2, 3, 1))
    assert torch.equal(fs_lib.ruder_blank_nhwc(im), x)
    with pytest.raises(ValueError):
        ops.ruder_stack(im, im, None, None)


@pytest.mark.parametrize("shape", SHAPES)
def test_stack_backward(gb, shape):
    from gbvst import ops
    _, _, flow, _, gx, gw = _op_inputs(shape)
    _, _, ref_x, ref_w, ref_both = _stack_ref64(shape)
    gxn, gwn, fl = _nhwc(gx, ops), _nhwc(gw, ops), flow.to(DEV)
    gxn[..., 7] = 9.0                    # only channels 4..6 of gx are read
    got = {}
    for name, a, b, ref in (("gx", gxn, None, ref_x), ("gw", None, gwn, ref_w), ("both", gxn, gwn, ref_both)):
        gy = ops.ruder_stack_bwd(a, b, fl, torch.zeros(shape + (4,), device=DEV))
        _close(_nchw(gy, 3, ops), ref, 1e-5, "d/dy_prev from " + name)
        assert float(gy[..., 3].abs().max()) == 0.0
        got[name] = gy
    both = got["gx"] + got["gw"]
    assert (got["both"] - both).abs().max().item() <= 1e-5 * both.abs().max().item()
    # accumulation: the scatter adds onto what gy_prev holds
    gy = ops.ruder_stack_bwd(None, gwn, fl, got["gx"].clone())
    assert (gy - both).abs().max().item() <= 1e-5 * both.abs().max().item()
    with pytest.raises(ValueError):
        ops.ruder_stack_bwd(None, None, fl, torch.zeros(shape + (4,), device=DEV))


def _temporal_ref64(w, y, mask, scale, gout):
    w, y = w.double().requires_grad_(True), y.double().requires_grad_(True)
    loss = RR.temporal_ref(w, y, mask.double(), scale)
    (loss * gout).backward()
    return loss.detach(), w.grad, y.grad


@pytest.mark.parametrize("shape", SHAPES)
def test_temporal(gb, shape):
    from gbvst import ops
    y, _, _, mask, _, _ = _op_inputs(shape)
    N, H, W = shape
    w = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(975))
    lr, gwr, gyr = _temporal_ref64(w, y, mask, 50.0, 1.7)
    wn, yn = _nhwc(w, ops), _nhwc(y, ops)
    wn[..., 3] = 2.0                     # pad channels take no part
    yn[..., 3] = 5.0
    loss = ops.ruder_temporal(wn, yn, mask.to(DEV), 50.0)
    gw, gy = ops.ruder_temporal_bwd(wn, yn, mask.to(DEV), torch.full((), 1.7, device=DEV), 50.0)
    _close_scalar(loss, lr)
    _close(_nchw(gw, 3, ops), gwr, 1e-5, "d/dw")
    _close(_nchw(gy, 3, ops), gyr, 1e-5, "d/dy")
    assert float(gw[..., 3].abs().max()) == 0.0 and float(gy[..., 3].abs().max()) == 0.0
    gw1, none = ops.ruder_temporal_bwd(wn, yn, mask.to(DEV), torch.full((), 1.7, device=DEV), 50.0, need_y=False)
    assert none is None and torch.equal(gw1, gw)
    # a fractional mask (not assumed binary)
    frac = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(976))
    _close_scalar(ops.ruder_temporal(wn, yn, frac.to(DEV), 50.0), _temporal_ref64(w, y, frac, 50.0, 1.0)[0])


def test_edge_flows(gb):
    from gbvst import ops
    shape = SHAPES[0]
    N, H, W = shape
    # flow == 0 is NOT the identity in the reference (see test_gpu_temporal_style.test_edge_flows): the composed
    # reference decides
    y, img, zero, mask, gx, gw = _op_inputs(shape, 0.0)
    xr, wr, _, _, gref = _stack_ref64(shape, 0.0)
    x, w = ops.ruder_stack(_nhwc(y, ops), _nhwc(img, ops), zero.to(DEV), mask.to(DEV))
    _close(_nchw(x, 7, ops), xr, 1e-5, "zero flow x")
    gy = ops.ruder_stack_bwd(_nhwc(gx, ops), _nhwc(gw, ops), zero.to(DEV), torch.zeros(shape + (4,), device=DEV))
    _close(_nchw(gy, 3, ops), gref, 1e-5, "zero flow d/dy_prev")
    # flow == +1000: every sample invalid -> w == 0, nothing reaches y_prev, loss = scale * mean((m * s * y)^2)
    far = _op_inputs(shape, 1000.0)[2]
    x, w = ops.ruder_stack(_nhwc(y, ops), _nhwc(img, ops), far.to(DEV), mask.to(DEV))
    assert float(w.abs().max()) == 0.0 and float(x[..., 4:].abs().max()) == 0.0
    assert torch.equal(x[..., 3].cpu(), mask[:, 0])
    gy = ops.ruder_stack_bwd(_nhwc(gx, ops), _nhwc(gw, ops), far.to(DEV), torch.zeros(shape + (4,), device=DEV))
    assert float(gy.abs().max()) == 0.0
    loss = ops.ruder_temporal(w, _nhwc(y, ops), mask.to(DEV), 3.0)
    _close_scalar(loss, 3.0 * ((mask.double() * S * y.double()) ** 2).mean())


@pytest.mark.parametrize("shape", SHAPES)
def test_determinism(det, shape):
    ops = det
    y, img, flow, mask, gx, gw = _op_inputs(shape)
    yn, im, fl, mk = _nhwc(y, ops), _nhwc(img, ops), flow.to(DEV), mask.to(DEV)
    gxn, gwn = _nhwc(gx, ops), _nhwc(gw, ops)
    gout = torch.full((), 1.7, device=DEV)

    def run():
        x, w = ops.ruder_stack(yn, im, fl, mk)
        loss = ops.ruder_temporal(w, yn, mk, 5.0)
        tg = ops.ruder_temporal_bwd(w, yn, mk, gout, 5.0)
        gy = ops.ruder_stack_bwd(gxn, gwn, fl, torch.zeros(shape + (4,), device=DEV))
        return x, w, loss, tg[0], tg[1], gy

    a, b = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert float(a[5][..., 3].abs().max()) == 0.0
    ops.set_deterministic(False)
    c = run()
    ops.set_deterministic(True)
    assert all(torch.equal(p, q) for p, q in zip(a[:5], c[:5]))     # forwards and the gather-free backward: one route
    assert (c[5] - a[5]).abs().max().item() <= 1e-5 * a[5].abs().max().item()
    _close(_nchw(a[5], 3, ops), _stack_ref64(shape)[4], 1e-5, "deterministic d/dy_prev")


def test_library_ops_and_autograd(gb):
    """vst::ruder_stack / vst::ruder_temporal pass opcheck's schema, fake-tensor and autograd-registration checks;
    autograd through the operators and through the fs_lib nodes equals the op-level backward."""
    from gbvst import fs_lib, ops
    shape = SHAPES[0]
    y, img, flow, mask, gx, gw = (t.to(DEV) for t in _op_inputs(shape))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    yg = y.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.vst.ruder_stack.default, (yg, img, flow, mask, S), test_utils=utils)
    x, w = torch.ops.vst.ruder_stack(yg, img, flow, mask, S)
    ((x * gx).sum() + (w * gw).sum()).backward()
    yn, im = _nhwc(y, ops), _nhwc(img, ops)
    x0, w0 = ops.ruder_stack(yn, im, flow, mask)
    gxn, gwn = _nhwc(gx, ops), _nhwc(gw, ops)
    gy0 = ops.ruder_stack_bwd(gxn, gwn, flow, torch.zeros(shape + (4,), device=DEV))
    atol = 1e-5 * float(gy0.abs().max())          # fp32 atomics, summation order only
    assert torch.equal(x.detach().cpu(), _nchw(x0, 7, ops)) and torch.equal(w.detach().cpu(), _nchw(w0, 3, ops))
    assert (yg.grad.cpu() - _nchw(gy0, 3, ops)).abs().max().item() <= atol
    # the NHWC autograd node: both output gradients in one scatter; x alone; w alone
    for use_x, use_w in ((True, True), (True, False), (False, True)):
        yv = yn.clone().requires_grad_(True)
        x1, w1 = fs_lib.ruder_stack_nhwc(yv, im, flow, mask)
        assert torch.equal(x1, x0) and torch.equal(w1, w0)
        terms = ([(x1 * gxn).sum()] if use_x else []) + ([(w1 * gwn).sum()] if use_w else [])
        sum(terms).backward()
        want = ops.ruder_stack_bwd(gxn if use_x else None, gwn if use_w else None, flow,
                                   torch.zeros(shape + (4,), device=DEV))
        assert (yv.grad - want).abs().max().item() <= atol
    # the temporal operator
    wg, yg2 = w.detach().clone().requires_grad_(True), y.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.vst.ruder_temporal.default, (wg, yg2, mask, 4.0, S), test_utils=utils)
    loss = torch.ops.vst.ruder_temporal(wg, yg2, mask, 4.0, S)
    (loss * 1.3).backward()
    l0 = ops.ruder_temporal(w0, yn, mask, 4.0)
    gw0, gy1 = ops.ruder_temporal_bwd(w0, yn, mask, torch.full((), 1.3, device=DEV), 4.0)
    assert torch.equal(loss.detach(), l0)
    assert torch.equal(wg.grad.cpu(), _nchw(gw0, 3, ops)) and torch.equal(yg2.grad.cpu(), _nchw(gy1, 3, ops))
    wv, yv = w0.clone().requires_grad_(True), yn.clone().requires_grad_(True)
    l1 = fs_lib.ruder_temporal_nhwc(wv, yv, mask, 4.0)
    torch.autograd.backward(l1, torch.full((), 1.3, device=DEV))
    assert torch.equal(l1.detach(), l0) and torch.equal(wv.grad, gw0) and torch.equal(yv.grad, gy1)


# ------------------------------------------------------------------- FastStyleNet(7, 1)
def _fsn(num_inp, base):
    from gbvst import faststyle
    from oracle import style_ref
    net = faststyle.FastStyleNet(num_inp, 1).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         style_ref.fsn_weights(style_ref.RefFastStyleNet(num_inp), base).items()})
    return net


FSN7_KEYS = ["conv1.conv2d.weight", "res1.conv1.conv2d.weight"]


def _fsn7_inputs():
    x = torch.rand(2, 7, 16, 20, generator=torch.Generator().manual_seed(980))
    return x, R.rand(981, (2, 128, 4, 5)), R.rand(982, (2, 3, 16, 20))


@functools.lru_cache(maxsize=None)
def _fsn7_reference(eps=0.0, seed=0):
    """RefFastStyleNet(7) in fp64 -> (features, image, input gradient, {parameter gradients})."""
    model = RR.nets(eps, seed)[0]
    x, gf, gi = _fsn7_inputs()
    x = x.double().requires_grad_(True)
    feats, img = model(x)
    ((feats * gf.double()).sum() + (img * gi.double()).sum()).backward()
    grads = {k: p.grad.numpy() for k, p in model.named_parameters() if k in FSN7_KEYS}
    return feats.detach(), img.detach(), x.grad, grads


def test_faststylenet7_vs_reference(gb, train_math):
    """The 7-channel input, stored 8-channel-padded, through conv1 (9x9, reflect), its weight gradient and its input
    data gradient (_FastStyleFn.backward's needs_input_grad[0] branch)."""
    from gbvst import ops
    net = _fsn(7, RR.MODEL_SEED)
    net.zero_grad()
    x, gf, gi = _fsn7_inputs()
    fr, ir, dxr, gr = _fsn7_reference()
    xn = _nhwc(x, ops).requires_grad_(True)
    feats, img = net.forward_nhwc(xn)
    ((feats * _nhwc(gf, ops)).sum() + (img * _nhwc(gi, ops)).sum()).backward()
    for name, got, ref in (("features", _nchw(feats.detach(), 128, ops), fr), ("image", _nchw(img.detach(), 3, ops), ir)):
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print(train_math, name, "rel", err)
        assert err < 1e-4, (name, err)
    assert xn.grad.shape == (2, 16, 20, 8) and float(xn.grad[..., 7].abs().max()) == 0.0
    pert = [_fsn7_reference(1e-6, sd) for sd in (0, 1)]
    band = max(_nrel(p[2], dxr) for p in pert)
    err = _nrel(_nchw(xn.grad, 7, ops), dxr)
    print(train_math, "dx nrel", err, "band", band)
    assert err < max(1e-3, band), (err, band)
    params = dict(net.named_parameters())
    for k in FSN7_KEYS:
        band = max(_nrel(p[3][k], gr[k]) for p in pert)
        err = _nrel(params[k].grad, gr[k])
        print(train_math, k, "nrel", err, "band", band)
        assert err < max(1e-3, band), (k, err, band)
    # the NCHW entry takes the 7 channels as they are
    f2, i2 = net(x.to(DEV))
    assert f2.shape == (2, 128, 4, 5) and i2.shape == (2, 3, 16, 20)
    assert float((i2.detach().cpu().double() - ir).abs().max() / ir.abs().max()) < 1e-4


# ----------------------------------------------------------------------------- step level
def _trainer(emph):
    from gbvst import faststyle
    _, style, _, _ = RR.step_inputs()
    return faststyle.Ruder([style], emphasis=emph, lr=1e-3, batch_sz=2, device=DEV, vgg=_vgg(RR.VGG_SEED),
                           model=_fsn(7, RR.MODEL_SEED), pre_style_model=_fsn(3, RR.PRE_SEED))


def _dev_inputs(n_frames):
    from gbvst import ops
    imgs, _, masks, flows = RR.step_inputs()
    return ([ops.nchw_to_nhwc(i.to(DEV)) for i in imgs[:n_frames]], [m.to(DEV) for m in masks],
            [f.to(DEV) for f in flows])


def _check_inputs():
    _, _, masks, flows = RR.step_inputs()
    assert len(masks) == len(flows) == 4
    for f in flows:
        R.assert_off_threshold(f)
    for m in masks:
        assert 0.1 < float((m == 0).float().mean()) < 0.3


def _check_grads(T, n_frames, emph, grads_ref, keys):
    params = dict(T.model.named_parameters())
    pert = [RR.reference_run(n_frames, emph, True, 1e-6, sd, 1)[1] for sd in (0, 1)]
    for k in keys:
        band = max(_nrel(pg[k], grads_ref[k]) for pg in pert)
        err = _nrel(params[k].grad, grads_ref[k])
        print(f"ruder {n_frames} frames {k}: nrel {err:.3e} band {band:.3e}")
        assert err < max(1e-3, band), (k, err, band)


def _losses(T, n_frames, roll):
    T.adam.zero_grad()
    out = T.losses_nhwc(*_dev_inputs(n_frames), roll)
    out[0].backward()
    return np.array([float(v.detach()) for v in out[:-1]]), out[-1]


def test_train_step_vs_reference(gb, train_math):
    """3 frames, roll: two steps with an Adam update between them.  Every loss within 1e-3 relative of the
    reference, in its (total, style, content, temporal) order, and no reference term below 1 % of its total;
    step-0 parameter gradients within max(1e-3, band)."""
    _check_inputs()
    losses_ref, grads_ref = RR.reference_run(3, RR.EMPH, True)
    T = _trainer(RR.EMPH)
    pre0 = T.pre_style_model.flat_param.clone()
    for s in range(2):
        ref = np.array(losses_ref[s])
        assert (np.abs(ref[1:]) >= 0.01 * abs(ref[0])).all(), ref      # the total cannot hide a term
        got, styled2 = _losses(T, 3, True)
        rel = np.abs(got - ref) / np.abs(ref)
        print("ruder step", s, "losses", got, "rel", rel)
        assert got.shape == ref.shape and rel.max() < 1e-3, (s, rel)
        assert styled2.shape == (RR.B, RR.H, RR.W, 4)
        if s == 0:
            _check_grads(T, 3, RR.EMPH, grads_ref, GRAD_KEYS)
        T.adam.step()
    # the gradient stops at styled frame 1: nothing is accumulated for (or learnt by) the pre-style net
    assert float(T.pre_style_model.flat_grad.abs().max()) == 0.0 and torch.equal(T.pre_style_model.flat_param, pre0)


def test_temporal_only_gradients(gb, train_math):
    """alpha = beta = 0: the parameter gradients come solely through the temporal kernel, the net's input channels
    (conv1's data gradient) and two chained warps, so they cannot hide behind the style term."""
    _check_inputs()
    losses_ref, grads_ref = RR.reference_run(3, RR.TEMPORAL_ONLY, True, 0.0, 0, 1)
    T = _trainer(RR.TEMPORAL_ONLY)
    got, _ = _losses(T, 3, True)
    ref = losses_ref[0]
    print("ruder temporal only", got, ref)
    assert abs(got[0] - ref[0]) <= 1e-3 * abs(ref[0]) and abs(got[3] - ref[3]) <= 1e-3 * abs(ref[3])
    assert got[1] == 0.0 and got[2] == 0.0 and ref[1] == 0.0 and ref[2] == 0.0
    _check_grads(T, 3, RR.TEMPORAL_ONLY, grads_ref, GRAD_KEYS)


def test_five_frames(gb, train_math):
    """5 frames, roll, one step: four applications of the net and four warps behind the loss."""
    _check_inputs()
    losses_ref, grads_ref = RR.reference_run(5, RR.EMPH, True, 0.0, 0, 1)
    ref = np.array(losses_ref[0])
    assert (np.abs(ref[1:]) >= 0.01 * abs(ref[0])).all(), ref
    T = _trainer(RR.EMPH)
    got, _ = _losses(T, 5, True)
    rel = np.abs(got - ref) / np.abs(ref)
    print("ruder 5 frames losses", got, "rel", rel)
    assert rel.max() < 1e-3, rel
    _check_grads(T, 5, RR.EMPH, grads_ref, ["conv1.conv2d.weight", "deconv3.conv2d.weight"])
    # 4 frames behave as 3 (fs_ruder.py:58, 66)
    ref4 = np.array(RR.reference_run(4, RR.EMPH, True, 0.0, 0, 1)[0][0])
    ref3 = np.array(RR.reference_run(3, RR.EMPH, True)[0][0])
    assert (np.abs(ref4 - ref3) <= 1e-12 * np.abs(ref3)).all()
    got4, _ = _losses(T, 4, True)
    assert (np.abs(got4 - ref4) / np.abs(ref4)).max() < 1e-3


def test_no_roll(gb, train_math):
    """roll False: frame 2 from the blank input, the temporal value exactly 0.0."""
    losses_ref, _ = RR.reference_run(3, RR.EMPH, False, 0.0, 0, 1)
    ref = np.array(losses_ref[0])
    assert ref[3] == 0.0 and (np.abs(ref[1:3]) >= 0.01 * abs(ref[0])).all(), ref
    T = _trainer(RR.EMPH)
    T.adam.zero_grad()
    out = T.losses_nhwc(*_dev_inputs(3), False)
    out[0].backward()
    got = np.array([float(v) for v in out[:-1]])
    print("ruder no roll", got, ref)
    assert out[3].is_cuda and out[3].dim() == 0 and got[3] == 0.0
    assert (np.abs(got[:3] - ref[:3]) / np.abs(ref[:3])).max() < 1e-3
    assert float(T.model.flat_grad.abs().max()) > 0.0


# ------------------------------------------------------------------------------ interface
def test_train_step_interface(gb):
    """train_step on the reference's layout (imgs list, masks [B,k,H,W], flows [B,2k,H,W]) with k = 2 pairs and 2
    images: the temporal term reads masks[:, -1] (fs_ruder.py:97), the losses come back as detached device scalars
    in the reference's order with styled frame 2, and one Adam update is made (every parameter moves by at most lr
    on the first step).  roll None draws once."""
    imgs, _, masks, flows = RR.step_inputs()
    mk, fl = torch.cat(masks[:2], 1), torch.cat(flows[:2], 1)
    T, U = _trainer(RR.EMPH), _trainer(RR.EMPH)
    p0 = T.model.flat_param.clone()
    losses, styled2 = T.train_step(imgs[:2], mk, fl, roll=True)
    frames, dm, df = _dev_inputs(2)
    out = U.losses_nhwc(frames, dm[:2], df[:2], True)
    assert len(losses) == 4 and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in losses)
    for v, w in zip(losses, out[:-1]):
        assert abs(float(v) - float(w)) <= 1e-5 * abs(float(w))
    one = U.losses_nhwc(frames, dm[:1], df[:1], True)          # the same frames, pair 0's mask as the last plane
    assert abs(float(one[3]) - float(out[3])) > 1e-3 * abs(float(out[3]))
    assert abs(float(one[2]) - float(out[2])) <= 1e-5 * abs(float(out[2]))
    assert styled2.shape == (RR.B, RR.H, RR.W, 4) and not styled2.requires_grad
    assert (styled2 - out[-1]).abs().max().item() <= 1e-4 * 255.0
    step = (T.model.flat_param - p0).abs()
    assert T.itr == 1 and 0.0 < float(step.max()) <= 1e-3 * (1 + 1e-3)
    np.random.seed(77)
    first, second = np.random.random(), np.random.random()
    np.random.seed(77)
    losses, _ = T.train_step(imgs[:2], mk, fl)
    assert np.random.random() == second and T.itr == 2
    assert (float(losses[3]) != 0.0) == (first < 0.5)


def test_inference_entries(gb):
    """infer_method with and without a previous frame (fs_ruder.py:110-121) and the device-resident recurrence
    step stylize_next against model(cat(frame, mask, warp(prev / 255, flow)))."""
    from gbvst import fs_lib, ops
    imgs, _, masks, flows = RR.step_inputs()
    T = _trainer(RR.EMPH)
    first = T.infer_method((imgs[0], None, None))
    assert first.shape == (RR.B, 3, RR.H, RR.W) and not first.requires_grad
    with torch.no_grad():
        want = T.pre_style_model(imgs[0].to(DEV))[1] / 255.0
    assert (first - want).abs().max().item() <= 1e-6
    warped = fs_lib.warp(first, flows[0].to(DEV))
    nxt = T.infer_method((imgs[1], masks[0], warped))
    assert nxt.shape == (RR.B, 3, RR.H, RR.W) and -0.1 <= float(nxt.min()) and float(nxt.max()) <= 1.1
    prev = ops.nchw_to_nhwc((first * 255.0).contiguous())
    got = T.stylize_next(prev, ops.nchw_to_nhwc(imgs[1].to(DEV)), flows[0], masks[0])
    assert got.shape == (RR.B, RR.H, RR.W, 4) and not got.requires_grad
    assert (ops.nhwc_to_nchw(got, 3) - nxt * 255.0).abs().max().item() <= 1e-4 * 255.0
