"""CPU-only checks of StarGAN v2's discriminator update (gbvst.stargan2's solver half): the restatement the GPU tests
use (tests/stargan2_d_ref.py, torch's native double backward) reproduces in fp32 the fixture the reference's own
Solver.compute_d_loss produced (tests/golden/stargan2_dstep.npz, tools/gen_golden_stargan2_d.py); the case keeps
the activation margin its seed was scanned for; the new C entries are declared, exported and validate their
arguments on the host; the new vst:: operators propagate fake-tensor shapes; the new Python surface refuses what it
does not carry.

Bars of the fixture comparison: losses 1e-5 relative, gradients 1e-4 of max|ref| per tensor, fp32 on the CPU with the
fixture's thread count.

The activation margin: D's weights and x_real are stargan2_ref.CASES["D"]'s; the seeds of z_trg and x_ref are each the
best of a scan of 240 (stargan2_d_ref.SCAN): 2.23e-7 (latent x_fake) and 2.55e-7 (reference x_fake).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import stargan2_d_ref as DR
import stargan2_ref as S

NEW_SYMBOLS = ["vst_loss_r1", "vst_loss_r1_bwd", "vst_loss_bce_logits", "vst_loss_bce_logits_bwd", "vst_r1_fwd",
               "vst_r1_bwd", "vst_bce_logits_fwd", "vst_bce_logits_bwd"]
NEW_OPS = ["r1_penalty", "r1_penalty_backward", "bce_logits", "bce_logits_backward"]
EINVAL = 1


@pytest.fixture(scope="module")
def case():
    st = DR.states()
    return st, DR.inputs()


def test_fixture_layout(golden, case):
    g = golden("stargan2_dstep")
    shapes = S.shapes("discriminator", **DR.CFG["discriminator"])
    assert list(g["keys"]) == list(shapes)
    for mode in DR.MODES:
        assert g[mode + "_x_fake"].shape == (DR.B, 3, 64, 64) and g[mode + "_x_fake"].dtype == np.float32
        assert {k[len(mode) + 3:] for k in g.files if k.startswith(mode + "_g_")} == set(shapes)
        for n in ("real", "fake", "reg"):
            assert np.isfinite(g[f"{mode}_{n}"]) and g[f"{mode}_{n}"] > 0
    assert not np.array_equal(g["latent_x_fake"], g["reference_x_fake"])


def test_case_keeps_its_activation_margin(golden, case):
    """On the reference alone: the nearest LeakyReLU decision of the fp64 discriminator forward over x_real and both
    x_fake stays the margin away from flipping."""
    g = golden("stargan2_dstep")
    st, (x_real, _, _) = case
    m = DR.margin(st["discriminator"], x_real, [g[mode + "_x_fake"] for mode in DR.MODES])
    print(f"D step: activation margin {m:.3e} (held to {S.MARGIN['D']:.0e})")
    assert m >= S.MARGIN["D"]


@pytest.mark.parametrize("mode", DR.MODES)
def test_restatement_reproduces_reference_fixture(golden, case, mode):
    g = golden("stargan2_dstep")
    st, (x_real, z_trg, x_ref) = case
    threads = torch.get_num_threads()
    torch.set_num_threads(S.FIXTURE_THREADS)
    try:
        fake = DR.x_fake(st, mode, x_real, z_trg, x_ref)
        got = DR.d_losses(st["discriminator"], x_real, DR.Y_ORG, fake, DR.Y_TRG, DR.LAMBDA_REG, torch.float32)
    finally:
        torch.set_num_threads(threads)
    ref_fake = g[mode + "_x_fake"]
    e = float(np.abs(fake.numpy().astype(np.float64) - ref_fake).max() / np.abs(ref_fake).max())
    print(f"{mode}: x_fake {e:.3e} (bar 1e-5)")
    assert e <= 1e-5
    for n in ("real", "fake", "reg"):
        want = float(g[f"{mode}_{n}"])
        e = abs(float(got[n]) - want) / abs(want)
        print(f"{mode}: {n} {float(got[n]):.7f} fixture {want:.7f} err {e:.3e} (bar 1e-5)")
        assert e <= 1e-5, n
    worst = 0.0
    for k, gr in got["grads"].items():
        ref = g[f"{mode}_g_{k}"]
        have = S.stored(gr).numpy().astype(np.float64)
        assert have.shape == ref.shape and np.abs(ref).max() > 0, k
        e = float(np.abs(have - ref).max() / np.abs(ref).max())
        worst = max(worst, e)
        assert e <= 1e-4, (k, e)
    print(f"{mode}: worst parameter gradient {worst:.3e} (bar 1e-4)")


def test_restatement_pieces_vs_stock_ops():
    """adv_loss is binary_cross_entropy_with_logits against a constant; r1_reg of a quadratic has a closed form."""
    import torch.nn.functional as F
    z = torch.tensor([0.0, 50.0, -50.0, 1.5, -0.3], dtype=torch.float64)
    for t in (0, 1):
        assert abs(float(DR.adv_loss(z, t)) - float(F.binary_cross_entropy_with_logits(z, torch.full_like(z, t)))) < 1e-9
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 4, 5, generator=gen, dtype=torch.float64).requires_grad_(True)
    a = torch.randn(2, 3, 4, 5, generator=gen, dtype=torch.float64)
    out = (0.5 * a * x * x).flatten(1).sum(1)                             # d out / d x = a x
    assert abs(float(DR.r1_reg(out, x).detach()) - float(0.5 * (a * x.detach()).pow(2).flatten(1).sum(1).mean())) < 1e-12


def test_python_surface_refuses_what_it_does_not_carry():
    from gbvst import ops, stargan2 as M
    D = M.Discriminator(**DR.CFG["discriminator"])
    x, y = torch.zeros(1, 3, 64, 64), torch.tensor([1])
    for call in (lambda: M.d_losses(D, x, y, x, y, 1.0), lambda: M.adv_loss(torch.zeros(2), 1),
                 lambda: D.forward_nhwc(torch.zeros(1, 64, 64, 4), y), lambda: ops.r1(torch.zeros(1, 2, 2, 4)),
                 lambda: ops.r1_bwd(torch.zeros(1, 2, 2, 4), torch.zeros(())),
                 lambda: ops.bce_logits(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), 3, 1),
                 lambda: ops.bce_logits_bwd(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), 3, 1, torch.zeros(()))):
        with pytest.raises(RuntimeError):                                # no CPU fallback
            call()
    with pytest.raises(ValueError):
        D.forward_nhwc(torch.zeros(1, 32, 32, 4), y)                     # the trunk must end at 1x1
    with pytest.raises(ValueError):
        D.head_nhwc(torch.zeros(1, 64, 64, 8))                           # an NHWC image has 4 lanes
    with pytest.raises(AssertionError):
        M.adv_loss(torch.zeros(2), 0.5)
    with pytest.raises(NotImplementedError):
        M.r1_reg(torch.zeros(2), torch.zeros(2, 8, 4, 4))
    nets = types.SimpleNamespace(discriminator=D)
    args = types.SimpleNamespace(lambda_reg=1.0)
    with pytest.raises(NotImplementedError):
        M.compute_d_loss(nets, args, x, y, y, z_trg=torch.zeros(1, 16), masks=[x])
    with pytest.raises(AssertionError):
        M.compute_d_loss(nets, args, x, y, y)
    with pytest.raises(AssertionError):
        M.compute_d_loss(nets, args, x, y, y, z_trg=torch.zeros(1, 16), x_ref=x)
    tr = M.DiscriminatorTrainer(nets, types.SimpleNamespace(lr=2e-4, beta1=0.0, beta2=0.99, weight_decay=1e-4,
                                                            lambda_reg=1.0))
    pg = tr.optimizer.param_groups[0]
    assert isinstance(tr.optimizer, torch.optim.Adam) and pg["lr"] == 2e-4 and pg["weight_decay"] == 1e-4
    assert list(pg["betas"]) == [0.0, 0.99] and len(pg["params"]) == len(list(D.parameters()))


def test_abi_table_exports_and_host_validation():
    import gbvst
    from gbvst import _lib, ops
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name in ("r1", "r1_bwd", "bce_logits", "bce_logits_bwd"):
        assert callable(getattr(ops, name))
    raw = ctypes.CDLL(gbvst._lib.build())
    header = open(gbvst._lib.REPO + "/include/vst_hip.h").read()
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert s + "(" in header, s
    assert "VST_R1_PART_DOUBLES = %d" % ops.R1_PART_DOUBLES in header
    lib = gbvst._lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def r1f(g=p, loss=p, part=p, B=2, hw=16):
        return lib.vst_loss_r1(g, loss, part, B, hw, None)

    def r1b(g=p, gout=p, u=p, B=2, hw=16):
        return lib.vst_loss_r1_bwd(g, gout, u, B, hw, None)

    def r1f8(g=p, loss=p, part=p, B=2, H=4, W=4):
        return lib.vst_r1_fwd(g, loss, part, B, H, W, None)

    def r1b8(g=p, gout=p, u=p, B=2, H=4, W=4):
        return lib.vst_r1_bwd(g, gout, u, B, H, W, None)

    def bcef(fn):
        def call(z=p, y=p, loss=p, B=2, D=4, nd=3, target=1.0):
            return fn(z, y, loss, B, D, nd, target, None)
        return call

    def bceb(fn):
        def call(z=p, y=p, gout=p, grad=p, B=2, D=4, nd=3, target=1.0):
            return fn(z, y, gout, grad, B, D, nd, target, None)
        return call

    # bad arguments are refused before any launch, with non-NULL host pointers (host memory is never touched)
    for call, required, bad in ((r1f, ("g", "loss", "part"), (dict(B=0), dict(hw=0), dict(B=-1))),
                                (r1b, ("g", "gout", "u"), (dict(B=0), dict(hw=0), dict(hw=-4))),
                                (r1f8, ("g", "loss", "part"), (dict(B=0), dict(H=0), dict(W=0))),
                                (r1b8, ("g", "gout", "u"), (dict(B=0), dict(H=0), dict(W=-1)))):
        for name in required:
            assert call(**{name: None}) == EINVAL, (call.__name__, name)
        for kw in bad:
            assert call(**kw) == EINVAL, (call.__name__, kw)
        assert b"r1" in lib.vst_last_error()
    bad = (dict(B=0), dict(D=0), dict(D=6), dict(nd=0), dict(nd=5), dict(target=0.5), dict(target=-1.0))
    for fn in (lib.vst_loss_bce_logits, lib.vst_bce_logits_fwd):
        for name in ("z", "y", "loss"):
            assert bcef(fn)(**{name: None}) == EINVAL, name
        for kw in bad:
            assert bcef(fn)(**kw) == EINVAL, kw
        assert b"bce_logits" in lib.vst_last_error()
    for fn in (lib.vst_loss_bce_logits_bwd, lib.vst_bce_logits_bwd):
        for name in ("z", "y", "gout", "grad"):
            assert bceb(fn)(**{name: None}) == EINVAL, name
        for kw in bad:
            assert bceb(fn)(**kw) == EINVAL, kw
        assert b"bce_logits_bwd" in lib.vst_last_error()


def test_library_ops_fake_shapes_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gbvst import library  # noqa: F401
    for name in NEW_OPS:
        assert name in library.OPS
        assert getattr(torch.ops.vst, name).default._schema.name == "vst::" + name
    with FakeTensorMode():
        g, s = torch.empty(2, 3, 8, 10), torch.empty(())
        assert torch.ops.vst.r1_penalty(g).shape == ()
        assert torch.ops.vst.r1_penalty_backward(s, g).shape == g.shape
        z, y = torch.empty(2, 3), torch.empty(2, dtype=torch.long)
        assert torch.ops.vst.bce_logits(z, y, 1.0).shape == ()
        assert torch.ops.vst.bce_logits_backward(s, z, y, 0.0).shape == z.shape
    g, s = torch.zeros(2, 3, 8, 10), torch.zeros(())
    z, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.long)
    for call in (lambda: torch.ops.vst.r1_penalty(g), lambda: torch.ops.vst.r1_penalty_backward(s, g),
                 lambda: torch.ops.vst.bce_logits(z, y, 1.0), lambda: torch.ops.vst.bce_logits_backward(s, z, y, 1.0)):
        with pytest.raises(RuntimeError):
            call()
