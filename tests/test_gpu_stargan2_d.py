"""GPU parity of StarGAN v2's discriminator update (gbvst.stargan2: adv_loss, r1_reg, d_losses, compute_d_loss,
DiscriminatorTrainer) and of what it is made of.

Kernels, against fp64: vst_loss_r1 / _bwd (forward 1e-6 of the value: an fp64 sum of fp32 squares rounded once;
backward 1e-6 of max|ref|: two fp32 roundings per element) and vst_loss_bce_logits / _bwd (1e-6: a handful of fp32 /
fp64 operations per sample), with guard bands around every output.
Nodes: each twice-differentiable node's inner Function F against its own backward F^T through
<F(a), b> == <a, F^T(b)> to 1e-5 relative (of the sum of the absolute terms of the inner product, the scale of its
fp32 rounding): the cheapest place a wrong double backward shows.
Losses: d_losses on stargan2_d_ref's case against the fixture the reference's own Solver.compute_d_loss produced
(tests/golden/stargan2_dstep.npz) and against the fp64 reference: losses 1e-4, parameter gradients 1e-3 of max|ref| or
within the fp64 reference's own movement under a 1e-6 relative perturbation of its weights (test_gpu_stargan2's rule),
for the whole loss and for the penalty alone.  compute_d_loss end to end adds the generator's error: the fake term is
held to 1e-4 plus what the fp64 discriminator makes of the measured x_fake difference.
Every figure is printed before it is asserted.
"""
import functools
import types

import numpy as np
import pytest
import torch

import reduction_ref as R
import stargan2_d_ref as DR
import stargan2_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SENTINEL = -12345.678
PAD = 64


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


def _guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=dtype)
    return buf[PAD:PAD + n].view(shape), buf


def _guards_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


# ===================================================================================== kernels
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 64, 64), (2, 129, 67)], ids=lambda s: "x".join(map(str, s)))
def test_r1_kernel_vs_fp64(gb, shape):
    """(3, 64, 64) and (2, 129, 67) have more pixels than one block's 256; (1, 1, 1) has H * W = 1."""
    from gbvst import ops
    B, H, W = shape
    gen = torch.Generator().manual_seed(41)
    g = torch.randn(B, H, W, 4, generator=gen)
    g[..., 3] = 1e3 * (1 + torch.rand(B, H, W, generator=gen))          # finite non-zero garbage in the padding lane
    gout = torch.tensor(0.75)
    gd, goutd = g.to(DEV), gout.to(DEV)
    loss, lbuf = _guarded(())
    u, ubuf = _guarded((B, H, W, 4))
    part = torch.empty(ops.R1_PART_DOUBLES, dtype=F64, device=DEV)
    ops._call("vst_loss_r1", ops._p(gd), ops._p(loss), ops._p(part), B, H * W, ops._stream())
    ops._call("vst_loss_r1_bwd", ops._p(gd), ops._p(goutd), ops._p(u), B, H * W, ops._stream())
    torch.cuda.synchronize()
    assert _guards_intact(lbuf) and _guards_intact(ubuf) and not bool((u == SENTINEL).any())
    g64 = g[..., :3].double()
    want = 0.5 * g64.pow(2).flatten(1).sum(1).mean(0)
    want_u = float(gout) * g64 / B
    e_l = abs(float(loss) - float(want)) / float(want)
    e_u = _rel(u[..., :3], want_u)
    print(f"r1 {shape}: fwd {e_l:.3e} bwd {e_u:.3e} (bar 1e-6)")
    assert e_l <= 1e-6 and e_u <= 1e-6
    assert not bool(u[..., 3].any())                                    # lane 3 written 0
    # twice, and through the wrappers and the §8b names: bit-equal
    assert torch.equal(ops.r1(gd), loss.reshape(())) and torch.equal(ops.r1(gd), ops.r1(gd))
    assert torch.equal(ops.r1_bwd(gd, goutd), u)
    l2 = torch.empty((), device=DEV)
    u2 = torch.empty_like(u)
    ops._call("vst_r1_fwd", ops._p(gd), ops._p(l2), ops._p(part), B, H, W, ops._stream())
    ops._call("vst_r1_bwd", ops._p(gd), ops._p(goutd), ops._p(u2), B, H, W, ops._stream())
    assert torch.equal(l2, loss.reshape(())) and torch.equal(u2, u)


@pytest.mark.parametrize("nd", [1, 2, 3, 5])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_bce_logits_kernel_vs_fp64(gb, B, nd):
    from gbvst import ops
    D = ops.cpad(nd)
    gen = torch.Generator().manual_seed(100 * B + nd)
    z = 3.0 * torch.randn(B, D, generator=gen)
    y = torch.randint(0, nd, (B,), generator=gen)
    special = [0.0, 50.0, -50.0]
    for b in range(B):                                                  # the selected logits include 0 and +-50
        z[b, y[b]] = special[b] if b < 3 else z[b, y[b]]
    if B < 3:
        zs = [z.clone() for _ in special]
        for v, zz in zip(special, zs):
            zz[0, y[0]] = v
    else:
        zs = [z]
    gout = torch.tensor(-1.25)
    for z in zs:
        zd, yd, goutd = z.to(DEV), y.to(DEV), gout.to(DEV)
        v = z.double()[torch.arange(B), y]
        for target in (0, 1):
            loss, lbuf = _guarded(())
            grad, gbuf = _guarded((B, D))
            ops._call("vst_loss_bce_logits", ops._p(zd), ops._p(yd), ops._p(loss), B, D, nd, float(target), ops._stream())
            ops._call("vst_loss_bce_logits_bwd", ops._p(zd), ops._p(yd), ops._p(goutd), ops._p(grad), B, D, nd,
                      float(target), ops._stream())
            torch.cuda.synchronize()
            assert _guards_intact(lbuf) and _guards_intact(gbuf) and not bool((grad == SENTINEL).any())
            want = (v.clamp(min=0) - v * target + torch.log1p(torch.exp(-v.abs()))).mean()
            want_g = torch.zeros(B, D, dtype=F64)
            want_g[torch.arange(B), y] = (torch.sigmoid(v) - target) / B * float(gout)
            e_l = abs(float(loss) - float(want)) / abs(float(want))
            e_g = _rel(grad, want_g) if float(want_g.abs().max()) > 1e-30 else float(grad.abs().max())
            print(f"bce B={B} nd={nd} t={target} z0={float(v[0]):+.0f}: fwd {e_l:.3e} bwd {e_g:.3e} (bar 1e-6)")
            assert e_l <= 1e-6 and e_g <= 1e-6
            off = torch.ones(B, D, dtype=torch.bool)
            off[torch.arange(B), y] = False
            assert not bool(grad.cpu()[off].any())                      # unselected columns: exactly 0
            assert torch.equal(ops.bce_logits(zd, yd, nd, target), loss.reshape(()))
            assert torch.equal(ops.bce_logits_bwd(zd, yd, nd, target, goutd), grad)
            l2, g2 = torch.empty((), device=DEV), torch.empty_like(grad)
            ops._call("vst_bce_logits_fwd", ops._p(zd), ops._p(yd), ops._p(l2), B, D, nd, float(target), ops._stream())
            ops._call("vst_bce_logits_bwd", ops._p(zd), ops._p(yd), ops._p(goutd), ops._p(g2), B, D, nd, float(target),
                      ops._stream())
            assert torch.equal(l2, loss.reshape(())) and torch.equal(g2, grad)


def test_bce_logits_refuses_a_domain_outside_the_head(gb):
    """An id outside [0, nd) is never used as an index: the loss and that row of the gradient are NaN."""
    from gbvst import ops
    z = torch.randn(3, 4).to(DEV)
    y = torch.tensor([0, 3, 1], device=DEV)                             # 3 domains: id 3 is the padding column
    assert bool(torch.isnan(ops.bce_logits(z, y, 3, 1)))
    g = ops.bce_logits_bwd(z, y, 3, 1, torch.ones((), device=DEV))
    assert bool(torch.isnan(g[1]).all()) and bool(torch.isfinite(g[[0, 2]]).all())


def test_library_ops_opcheck_and_double_backward(gb):
    from gbvst import library  # noqa: F401
    gen = torch.Generator().manual_seed(83)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    g = torch.randn(2, 3, 6, 5, generator=gen).to(DEV).requires_grad_(True)
    torch.library.opcheck(torch.ops.vst.r1_penalty.default, (g,), test_utils=utils)
    torch.library.opcheck(torch.ops.vst.r1_penalty_backward.default, (torch.ones((), device=DEV), g), test_utils=utils)
    # the penalty of a gradient field g = A x, differentiated down to A: d/dA 0.5/B sum (A x)^2 = (A x) x^T / B
    A = torch.randn(3, 3, generator=gen).to(DEV).requires_grad_(True)
    x = torch.randn(2, 3, 6, 5, generator=gen).to(DEV)
    field = torch.einsum("ij,bjhw->bihw", A, x).contiguous()
    (u,) = torch.autograd.grad(torch.ops.vst.r1_penalty(field), field, create_graph=True)
    assert _rel(u, field.detach().double() / 2) <= 1e-6
    (gA,) = torch.autograd.grad((u * u).sum(), A)                       # through the backward op's own backward
    want = torch.autograd.grad((torch.einsum("ij,bjhw->bihw", A.double(), x.double()) / 2).pow(2).sum(), A)[0]
    assert _rel(gA, want) <= 1e-5
    logits = torch.randn(4, 3, generator=gen).to(DEV).requires_grad_(True)
    y = torch.tensor([2, 0, 1, 2], device=DEV)
    for target in (0.0, 1.0):
        torch.library.opcheck(torch.ops.vst.bce_logits.default, (logits, y, target), test_utils=utils)
        loss = torch.ops.vst.bce_logits(logits, y, target)
        ref_in = logits.detach().double().requires_grad_(True)
        sel = ref_in[torch.arange(4), y]
        ref = torch.nn.functional.binary_cross_entropy_with_logits(sel, torch.full_like(sel, target))
        assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref))
        (gl,) = torch.autograd.grad(loss, logits)
        assert _rel(gl, torch.autograd.grad(ref, ref_in)[0]) <= 1e-6


# ======================================================================================= nodes
def _dot(a, b):
    """(<a, b>, sum |a b|) in fp64."""
    p = a.detach().double() * b.detach().double()
    return float(p.sum()), float(p.abs().sum())


def _adjoint_error(fa, b, a, ftb):
    """|<F(a), b> - <a, F^T(b)>| relative to the sums of absolute terms."""
    (l, la), (r, ra) = _dot(fa, b), _dot(a, ftb)
    return abs(l - r) / max(la, ra, 1e-30)


def _second(fn, inputs, gouts):
    """F(inputs) under grad mode and its backward applied to gouts: (outputs, input gradients)."""
    inputs = [t.clone().requires_grad_(True) for t in inputs]
    outs = fn(*inputs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    return outs, torch.autograd.grad(outs, inputs, grad_outputs=gouts)


def _conv_mod(M, cin, cout, k, pad, gen):
    m = M.Conv2d(cin, cout, k, stride=1, padding=pad, bias=True)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / (cin * k * k) ** 0.5)
        m.bias.copy_(0.1 * torch.randn(cout, generator=gen))
    return m.to(DEV)


def test_mask_node_is_its_own_adjoint(gb):
    from gbvst import stargan2 as M
    gen = torch.Generator().manual_seed(51)
    y, a, b = (torch.randn(2, 4, 6, 8, generator=gen).to(DEV) for _ in range(3))
    for act in ("lrelu", "relu"):
        (fa,), (ftb,) = _second(lambda t: M._MaskFn.apply(t, y, act), [a], [b])
        e = _adjoint_error(fa, b, a, ftb)
        print(f"mask {act}: adjoint {e:.3e} (bar 1e-5)")
        assert e <= 1e-5
        assert torch.equal(fa, torch.where(y > 0, a, (0.2 if act == "lrelu" else 0.0) * a))


@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0), (4, 0)], ids=["3x3", "1x1", "4x4valid"])
def test_dgrad_node_adjoints(gb, k, pad):
    """dx = conv^T(gz; W): its backward for gz is the forward conv, for W the weight gradient, both checked by the
    adjoint identity of the bilinear form <conv^T(gz; W), b>."""
    from gbvst import stargan2 as M
    gen = torch.Generator().manual_seed(53 + k)
    cin, cout, H, W = 4, 8, 6, 8
    mod = _conv_mod(M, cin, cout, k, pad, gen)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    gz = torch.randn(2, Ho, Wo, cout, generator=gen).to(DEV)
    b = torch.randn(2, H, W, cin, generator=gen).to(DEV)
    ck = M._packs(mod)[1]

    def f(t, w):
        return M._DgradFn.apply(t, w, mod, ck, k, 1, pad, (2, H, W, cin))

    (dx,), (d_gz, d_w) = _second(f, [gz, mod.weight.detach()], [b])
    e_gz = _adjoint_error(dx, b, gz, d_gz)                               # linear in gz
    e_w = _adjoint_error(dx, b, mod.weight, d_w)                         # linear in W: <F_W(gz), b> = <W, d_w>
    want = torch.nn.functional.conv_transpose2d(R.nchw64(gz), mod.weight.detach().double().cpu(), padding=pad)
    e_f = _rel(R.nchw64(dx), want)
    print(f"dgrad {k}x{k}: vs fp64 {e_f:.3e} adjoint gz {e_gz:.3e} W {e_w:.3e} (bar 1e-5)")
    assert e_f <= 1e-5 and e_gz <= 1e-5 and e_w <= 1e-5
    assert tuple(d_gz.shape) == tuple(gz.shape) and tuple(d_w.shape) == tuple(mod.weight.shape)


def test_pool_backward_node_adjoint(gb):
    from gbvst import stargan2 as M
    gen = torch.Generator().manual_seed(57)
    a = torch.randn(2, 4, 6, 8, generator=gen).to(DEV)
    b = torch.randn(2, 8, 12, 8, generator=gen).to(DEV)
    (fa,), (ftb,) = _second(M._PoolBwdFn.apply, [a], [b])
    e = _adjoint_error(fa, b, a, ftb)
    print(f"pool backward: adjoint {e:.3e} (bar 1e-5)")
    assert e <= 1e-5 and tuple(ftb.shape) == tuple(a.shape)


@pytest.mark.parametrize("mode", ["same", "pool", "up"])
def test_merge_backward_node_adjoint(gb, mode):
    from gbvst import ops, stargan2 as M
    gen = torch.Generator().manual_seed(59)
    shape = (2, 4, 6, 8)
    a = torch.randn(shape, generator=gen).to(DEV)
    ba = torch.randn(shape, generator=gen).to(DEV)
    bb = torch.randn(ops._merge_b_shape(shape, mode), generator=gen).to(DEV)
    (ga, gbt), (ft,) = _second(lambda t: M._MergeBwdFn.apply(t, mode), [a], [ba, bb])
    (l1, s1), (l2, s2), (r, s3) = _dot(ga, ba), _dot(gbt, bb), _dot(a, ft)
    e = abs(l1 + l2 - r) / max(s1 + s2, s3)
    print(f"merge backward {mode}: adjoint {e:.3e} (bar 1e-5)")
    assert e <= 1e-5


def test_first_order_nodes_refuse_a_second_differentiation(gb):
    from gbvst import stargan2 as M
    gen = torch.Generator().manual_seed(61)
    x = torch.randn(2, 4, 4, 8, generator=gen).to(DEV).requires_grad_(True)
    h = torch.randn(2, 16, generator=gen).to(DEV).requires_grad_(True)
    y = M._AdaINActFn.apply(x, h)
    (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.pow(2).sum(), h)


# ====================================================================================== losses
@functools.lru_cache(maxsize=None)
def _case():
    """(states, (x_real, z_trg, x_ref), GPU nets with the case's weights)."""
    from gbvst import stargan2 as M
    st = DR.states()
    c = DR.CFG
    nets = types.SimpleNamespace(
        generator=M.Generator(c["generator"]["img_size"], c["generator"]["style_dim"], c["generator"]["max_conv_dim"]),
        mapping_network=M.MappingNetwork(**c["mapping_network"]), style_encoder=M.StyleEncoder(**c["style_encoder"]),
        discriminator=M.Discriminator(**c["discriminator"]))
    for k, net in vars(nets).items():
        net.load_state_dict({n: torch.from_numpy(v) for n, v in st[k].items()})
        net.to(DEV)
    return st, DR.inputs(), nets


GRADS = {"loss": "grads", "reg": "grads_reg"}


@functools.lru_cache(maxsize=None)
def _ref64(mode):
    """The fp64 reference of d_losses on the fixture's x_fake of a mode, computed once."""
    st, (x_real, _, _), _ = _case()
    x_fk = np.load(_golden_path())[mode + "_x_fake"]
    return DR.d_losses(st["discriminator"], x_real, DR.Y_ORG, x_fk, DR.Y_TRG, DR.LAMBDA_REG, F64)


def _golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stargan2_dstep.npz")


def _bands(mode, wrt, ref, eps=1e-6, seeds=(0, 1, 2, 3)):
    """How far the fp64 reference's own gradients move when every weight is scaled by (1 + eps N(0, 1))
    (test_gpu_stargan2._bands)."""
    st, (x_real, _, _), _ = _case()
    x_fk = np.load(_golden_path())[mode + "_x_fake"]
    pb = {}
    for s in seeds:
        gen = torch.Generator().manual_seed(s)
        sp = {k: (torch.from_numpy(v).double() * (1 + eps * torch.randn(v.shape, generator=gen, dtype=F64))).numpy()
              for k, v in st["discriminator"].items()}
        got = DR.d_losses(sp, x_real, DR.Y_ORG, x_fk, DR.Y_TRG, DR.LAMBDA_REG, F64)[GRADS[wrt]]
        for k, rg in ref[GRADS[wrt]].items():
            if float(rg.abs().max()) > 0:
                pb[k] = max(pb.get(k, 0.0), _rel(got[k], rg))
    return pb


def _gpu_d_losses(mode, wrt):
    from gbvst import stargan2 as M
    _, (x_real, _, _), nets = _case()
    D = nets.discriminator
    D.zero_grad(set_to_none=True)
    x_fk = torch.from_numpy(np.load(_golden_path())[mode + "_x_fake"]).to(DEV)
    xr = torch.from_numpy(x_real).to(DEV)
    loss, parts = M.d_losses(D, xr, torch.tensor(DR.Y_ORG, device=DEV), x_fk, torch.tensor(DR.Y_TRG, device=DEV),
                             DR.LAMBDA_REG if wrt == "loss" else 0.0)
    return loss, parts, xr


def _head_key():
    c = DR.CFG["discriminator"]
    return "main.%d" % (len(S.trunk_plan(c["img_size"], c["max_conv_dim"])) + 4)


@pytest.mark.parametrize("wrt", ["loss", "reg"])
@pytest.mark.parametrize("mode", DR.MODES)
def test_d_losses_vs_fixture_and_fp64(gb, golden, mode, wrt):
    """wrt 'loss': the gradients of real + fake + lambda_reg * reg against the fixture and fp64.  wrt 'reg': the
    penalty alone back-propagated against fp64 (the fixture holds the whole loss's gradients), so a penalty error
    cannot hide behind the larger adversarial gradient."""
    from gbvst import stargan2 as M
    g = golden("stargan2_dstep")
    ref = _ref64(mode)
    D = _case()[2].discriminator
    assert list(D.state_dict()) == list(g["keys"])
    if wrt == "loss":
        loss, parts, xr = _gpu_d_losses(mode, wrt)
        loss.backward()
    else:
        # reg alone: the same graph, the penalty's scalar back-propagated
        D.zero_grad(set_to_none=True)
        xr = torch.from_numpy(_case()[1][0]).to(DEV)
        x4 = M._nhwc4(xr).requires_grad_()
        y = torch.tensor(DR.Y_ORG, device=DEV)
        reg = M._R1Fn.apply(M._input_grad(D.forward_nhwc(x4, y), x4, torch.ones(DR.B, device=DEV)).contiguous())
        reg.backward(inputs=list(D.parameters()))
        parts = types.SimpleNamespace(reg=reg.detach())
    torch.cuda.synchronize()
    assert xr.grad is None and not xr.requires_grad
    names = ("real", "fake", "reg") if wrt == "loss" else ("reg",)
    for tag, want in (("fixture", {n: float(g[f"{mode}_{n}"]) for n in names}),
                      ("fp64", {n: float(ref[n]) for n in names})):
        for n in names:
            e = abs(float(getattr(parts, n)) - want[n]) / abs(want[n])
            print(f"{mode}/{wrt} vs {tag}: {n} {float(getattr(parts, n)):.7f} err {e:.3e} (bar 1e-4)")
            assert e <= 1e-4, (tag, n)
    if wrt == "loss":
        assert abs(float(loss) - float(ref["real"] + ref["fake"] + DR.LAMBDA_REG * ref["reg"])) <= \
            1e-4 * abs(float(ref["real"] + ref["fake"] + DR.LAMBDA_REG * ref["reg"]))
    bands = []

    def band(k):
        if not bands:
            bands.append(_bands(mode, wrt, ref))
        return bands[0][k]

    worst, n_zero = 0.0, 0
    for k, p in D.named_parameters():
        rg = ref[GRADS[wrt]][k]
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        if float(rg.abs().max()) == 0:      # the penalty does not depend on the biases: they only move the masks
            assert not bool(got.any()), k
            n_zero += 1
            continue
        cmp = [("fp64", rg, got)]
        if wrt == "loss":
            cmp.append(("fixture", g[f"{mode}_g_{k}"], S.stored(got)))
        for tag, rr, gg in cmp:
            e = _rel(gg, rr)
            worst = max(worst, e)
            if e >= 1e-3:
                print(f"{mode}/{wrt} vs {tag}: {k}: {e:.3e}, the reference's own band {band(k):.3e}")
                assert e < band(k), (tag, k, e, band(k))
    print(f"{mode}/{wrt}: worst parameter gradient {worst:.3e} (bar 1e-3); {n_zero} exactly-zero gradients")
    if wrt == "reg":
        # y_org = [2, 0]: the penalty never selects domain 1, and no bias has a gradient
        hw = D.get_parameter(_head_key() + ".weight").grad
        assert not bool(hw[1].any()) and bool(hw[0].any()) and bool(hw[2].any())
        assert n_zero == sum(1 for k in ref["grads"] if k.endswith(".bias"))
    else:
        assert n_zero == 0


def test_the_unselected_head_row_stays_zero(gb):
    """The real terms alone (adversarial + penalty, y_org = [2, 0]): the head row and bias of domain 1, which no
    sample selects, get exact zeros from the fused gather's dense gradient."""
    from gbvst import stargan2 as M
    _, (x_real, _, _), nets = _case()
    D = nets.discriminator
    D.zero_grad(set_to_none=True)
    x4 = M._nhwc4(torch.from_numpy(x_real).to(DEV)).requires_grad_()
    y = torch.tensor(DR.Y_ORG, device=DEV)
    z = D.head_nhwc(x4)
    sel = torch.zeros_like(z)
    sel[torch.arange(DR.B), y] = 1
    (M._BCEFn.apply(z, y, D.num_domains, 1) + M._R1Fn.apply(M._input_grad(z, x4, sel).contiguous())).backward()
    w, b = (D.get_parameter(_head_key() + s).grad for s in (".weight", ".bias"))
    assert not bool(w[1].any()) and float(b[1]) == 0.0
    assert bool(w[0].any()) and bool(w[2].any()) and float(b[0]) != 0.0 and float(b[2]) != 0.0


def test_public_losses_are_drop_ins(gb):
    """adv_loss / r1_reg with the reference's signatures on NCHW tensors equal d_losses' own terms."""
    from gbvst import stargan2 as M
    _, (x_real, _, _), nets = _case()
    D = nets.discriminator
    ref = _ref64("latent")
    x = torch.from_numpy(x_real).to(DEV).requires_grad_()
    out = D(x, torch.tensor(DR.Y_ORG, device=DEV))
    real, reg = M.adv_loss(out, 1), M.r1_reg(out, x)
    for n, v in (("real", real), ("reg", reg)):
        e = abs(float(v) - float(ref[n])) / abs(float(ref[n]))
        print(f"drop-in {n}: {e:.3e} (bar 1e-4)")
        assert e <= 1e-4
    k = "main.0.weight"                                                  # the layer the whole double backward reaches
    (gk,) = torch.autograd.grad(reg, D.get_parameter(k))
    e = _rel(gk, ref["grads_reg"][k])
    print(f"drop-in r1_reg gradient of {k}: {e:.3e} (bar 1e-3)")
    assert e <= 1e-3


@pytest.mark.parametrize("mode", DR.MODES)
def test_compute_d_loss_end_to_end(gb, golden, mode):
    from gbvst import stargan2 as M
    g = golden("stargan2_dstep")
    st, (x_real, z_trg, x_ref), nets = _case()
    args = types.SimpleNamespace(lambda_reg=DR.LAMBDA_REG)
    xr = torch.from_numpy(x_real).to(DEV)
    kw = dict(z_trg=torch.from_numpy(z_trg).to(DEV)) if mode == "latent" else dict(x_ref=torch.from_numpy(x_ref).to(DEV))
    y_org, y_trg = torch.tensor(DR.Y_ORG, device=DEV), torch.tensor(DR.Y_TRG, device=DEV)
    loss, parts = M.compute_d_loss(nets, args, xr, y_org, y_trg, **kw)
    assert set(parts) == {"real", "fake", "reg"} and all(isinstance(parts[k], float) for k in parts)
    with torch.no_grad():
        s = nets.mapping_network(kw["z_trg"], y_trg) if mode == "latent" else nets.style_encoder(kw["x_ref"], y_trg)
        x_fk = nets.generator(xr, s)
    e_x = _rel(x_fk, g[mode + "_x_fake"])
    # what the generator's error is worth to the fake term: the fp64 discriminator on both images
    with torch.no_grad():
        t = {k: torch.from_numpy(v).double() for k, v in st["discriminator"].items()}
        carried = abs(float(DR.adv_loss(S.discriminator_forward(t, x_fk.double().cpu(), DR.Y_TRG,
                                                                 **DR.CFG["discriminator"]), 0))
                      - float(_ref64(mode)["fake"]))
    print(f"{mode}: x_fake {e_x:.3e}, carried into the fake term {carried:.3e}")
    assert e_x <= 1e-4
    for n in ("real", "fake", "reg"):
        want = float(g[f"{mode}_{n}"])
        tol = 1e-4 * abs(want) + (carried if n == "fake" else 0.0)
        print(f"{mode}: {n} {parts[n]:.7f} fixture {want:.7f} (tolerance {tol:.3e})")
        assert abs(parts[n] - want) <= tol, n
    assert abs(float(loss) - (parts.real + parts.fake + DR.LAMBDA_REG * parts.reg)) <= 1e-6 * abs(float(loss))
    with pytest.raises(NotImplementedError):
        M.compute_d_loss(nets, args, xr, y_org, y_trg, masks=[xr], **kw)
    with pytest.raises(AssertionError):
        M.compute_d_loss(nets, args, xr, y_org, y_trg)


def test_launch_economy(gb, monkeypatch):
    """One d_losses(...).backward() runs at most 3 weight-gradient launches per conv (real pass, fake pass, the
    penalty's double backward); the penalty's first-order sweep runs none."""
    from gbvst import stargan2 as M
    _, (x_real, _, _), nets = _case()
    D = nets.discriminator
    n_convs = sum(1 for m in D.modules() if hasattr(m, "kernel_size"))
    assert n_convs == 12                                                 # 3x3, 4 blocks (3 + 2 + 2 + 2), 4x4, head
    ops = M.ops                          # the module stargan2 calls into, whatever else the session has imported
    calls = []
    real_wgrad = ops.conv2d_wgrad

    def counted(*a, **k):
        calls.append(1)
        return real_wgrad(*a, **k)

    monkeypatch.setattr(ops, "conv2d_wgrad", counted)
    x = torch.from_numpy(x_real).to(DEV).requires_grad_()
    reg = M.r1_reg(D(x, torch.tensor(DR.Y_ORG, device=DEV)), x)
    assert len(calls) == 0 and reg.requires_grad
    del reg
    loss, _, _ = _gpu_d_losses("latent", "loss")
    assert len(calls) == 0
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None for p in D.parameters())
    print(f"conv2d_wgrad launches of one backward: {len(calls)} for {n_convs} convs")
    assert 0 < len(calls) <= 3 * n_convs


def test_d_step_is_adam_on_the_same_gradients(gb):
    import copy
    from gbvst import stargan2 as M
    _, (x_real, z_trg, x_ref), nets0 = _case()
    nets = types.SimpleNamespace(**{k: copy.deepcopy(v) for k, v in vars(nets0).items()})
    args = types.SimpleNamespace(lambda_reg=DR.LAMBDA_REG, lr=1e-4, beta1=0.0, beta2=0.99, weight_decay=1e-4)
    trainer = M.DiscriminatorTrainer(nets, args)
    assert isinstance(trainer.optimizer, torch.optim.Adam)
    before = {k: {n: p.detach().clone() for n, p in net.named_parameters()} for k, net in vars(nets).items()}
    xr = torch.from_numpy(x_real).to(DEV)
    y_org, y_trg = torch.tensor(DR.Y_ORG, device=DEV), torch.tensor(DR.Y_TRG, device=DEV)
    losses = trainer.d_step(xr, y_org, y_trg, z_trg=torch.from_numpy(z_trg).to(DEV))
    assert set(losses) == {"real", "fake", "reg"}
    assert xr.grad is None and not xr.requires_grad
    for k in ("generator", "mapping_network", "style_encoder"):
        for n, p in getattr(nets, k).named_parameters():
            assert p.grad is None and torch.equal(p, before[k][n]), (k, n)
    # a fresh Adam with the same settings on the pre-step parameters and the gradients d_step left behind
    twins = [torch.nn.Parameter(v.clone()) for v in before["discriminator"].values()]
    for t, p in zip(twins, nets.discriminator.parameters()):
        assert p.grad is not None
        t.grad = p.grad.clone()
    torch.optim.Adam(twins, lr=args.lr, betas=[args.beta1, args.beta2], weight_decay=args.weight_decay).step()
    for t, (n, p) in zip(twins, nets.discriminator.named_parameters()):
        assert torch.equal(t.detach(), p.detach()), n
        assert not torch.equal(p.detach(), before["discriminator"][n]), n
    # the second update of an iteration: reference mode, on the moved weights
    losses2 = trainer.d_step(xr, y_org, y_trg, x_ref=torch.from_numpy(x_ref).to(DEV))
    assert all(np.isfinite(losses2[k]) for k in losses2) and losses2.real != losses.real


def test_he_init(gb):
    from gbvst import stargan2 as M
    torch.manual_seed(7)
    D = M.Discriminator(**DR.CFG["discriminator"])
    D.apply(M.he_init)
    for n, p in D.named_parameters():
        if n.endswith(".bias"):
            assert not bool(p.any()), n
    w = D.get_parameter("main.1.conv1.weight")                           # 256 -> 256 3x3: std = sqrt(2 / fan_in)
    assert abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02
