"""CPU tests of tests/sampling_ref.py, the reference of tests/test_gpu_sampling.py.

  * tier agreement: stock torch fp32 (grid_sample, avg_pool2d, the oracle's upsample_flow) passes the very
    comparison functions the GPU tests call, on every case they run: the bounds hold for the references alone;
  * masks: the masked tight tier reproduces the reference's own fs_lib.warp outputs (tests/golden/style_small.npz),
    every masked case keeps clear of the validity threshold, the fbcheck inputs produce both mask values;
  * the cases discriminate: every mutation of sampling_ref.MUTATIONS (a wrong result of the kind a one-line kernel
    slip gives) is rejected by that same comparison function on a named GPU-test case;
  * the host argument checks of the warp-backward and temporal-loss entry points.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampling_ref as S
from oracle import cpu_ref, raft_ref, style_ref

from sampling_ref import (BWD_CASES, FWD_CASES, LOOKUP_CASES, PYRAMID_CASES, TEMPORAL_CASES, UPSAMPLE_CASES,
                          lookup_case, temporal_case)

F64 = torch.float64


def _torch32_warp(x, flow, align, masked, gout=None):
    """The reference warp (utils/flowtools.py:18-32 / fs_lib.py:5-39 with the align mode passed on) in stock fp32
    torch on NHWC input; with gout also its input gradient."""
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(gout is not None)
    N, C, H, W = xn.shape
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(N, H, W)
    yy = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(N, H, W)
    g = torch.stack([2.0 * (xx + flow[:, 0]) / max(W - 1, 1) - 1.0, 2.0 * (yy + flow[:, 1]) / max(H - 1, 1) - 1.0], -1)
    out = F.grid_sample(xn, g, mode="bilinear", padding_mode="zeros", align_corners=align)
    if masked:
        m = F.grid_sample(torch.ones_like(xn), g, align_corners=align)
        m = torch.where(m < 0.9999, torch.zeros_like(m), m)
        out = out * torch.where(m > 0, torch.ones_like(m), m)
    if gout is None:
        return out.detach().permute(0, 2, 3, 1).contiguous()
    out.backward(gout.permute(0, 3, 1, 2))
    return xn.grad.permute(0, 2, 3, 1).contiguous()


# ================================================================================ tier agreement
@pytest.mark.parametrize("shape,family", FWD_CASES, ids=[f"{'x'.join(map(str, s))}-{f}" for s, f in FWD_CASES])
def test_warp_fwd_tiers_agree(shape, family):
    for align in (False, True):
        for masked in (False, True):
            case = S.warp_case(shape, family, align, masked)
            S.check_warp_fwd(_torch32_warp(case["x"], case["flow"], align, masked), case, "host_fwd")
            (tref, tb, valid), (iref, ib, keep) = case["tight"], case["indep"]
            S.le((tref - iref).abs(), ib, "tight vs independent")
            if masked:
                assert bool((valid == keep).all())


@pytest.mark.parametrize("shape,family", BWD_CASES, ids=[f"{'x'.join(map(str, s))}-{f}" for s, f in BWD_CASES])
def test_warp_bwd_tiers_agree(shape, family):
    for align, masked in ((False, False), (True, False), (False, True), (True, True)):
        case = S.warp_bwd_case(shape, family, align, masked)
        x0 = torch.zeros(shape)
        S.check_warp_bwd(_torch32_warp(x0, case["flow"], align, masked, case["gout"]), case, "host_bwd")
        S.le((case["tight"][0] - case["indep"][0]).abs(), case["indep"][1] + 1e-300, "tight vs independent")


def _torch32_temporal(a, b, flow, mask, lam, cl, gout):
    an = a[..., :cl].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    bn = b[..., :cl].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    loss = cpu_ref.temporal_loss(an, bn, flow, mask, lam)
    (loss * gout).backward()
    ga, gb = torch.zeros_like(a), torch.zeros_like(b)
    ga[..., :cl], gb[..., :cl] = an.grad.permute(0, 2, 3, 1), bn.grad.permute(0, 2, 3, 1)
    return loss.detach(), ga, gb


@pytest.mark.parametrize("shape,cscl", TEMPORAL_CASES, ids=[f"{'x'.join(map(str, s))}-cs{c[0]}cl{c[1]}"
                                                            for s, c in TEMPORAL_CASES])
def test_temporal_tiers_agree(shape, cscl):
    """Stock fp32 torch (mean in its own order, autograd) passes check_temporal.  Its mean is a pairwise fp32 sum,
    within the kernel's (cl + 16) 2 u; its gradient scatters fp32 products like the atomic path."""
    c = temporal_case(shape, cscl, "iid")
    loss, ga, gb = _torch32_temporal(c["a"], c["b"], c["flow"], c["mask"], c["lam"], c["cl"], c["gout"])
    S.check_temporal(loss, ga, gb, c["ref"], None, c["indep"](), "host_temporal")


@pytest.mark.parametrize("geo", PYRAMID_CASES)
def test_pyramid_reference(geo):
    P, H2, W2, ld0, levels = geo
    buf = S.pyramid_buffer(P, H2, W2, ld0, levels, fill=True)       # the levels by fp32 avg_pool2d
    lv = S.pyramid_levels(buf, P, H2, W2, ld0, levels)
    for l, (ref, bound) in enumerate(S.pyramid_ref(buf, P, H2, W2, ld0, levels), 1):
        assert tuple(ref.shape[1:]) == (H2 >> l, W2 >> l)
        S.le((lv[l].double() - ref).abs(), bound, f"pyramid level {l}")


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=["-".join(map(str, c)) for c in LOOKUP_CASES])
def test_lookup_tiers_agree(case):
    """The reference's own lookup (oracle.style_ref.RefCorrBlock.__call__'s loop) in fp32 passes check_lookup."""
    c = lookup_case(*case)
    B, H1, W1, H2, W2, ld0, levels, r, cs = c["geo"]
    P, K = B * H1 * W1, 2 * r + 1
    lv = S.pyramid_levels(c["buf"], P, H2, W2, ld0, levels)
    co = c["coords"].permute(0, 2, 3, 1).reshape(P, 1, 1, 2)
    d = torch.linspace(-r, r, K)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, K, K, 2)
    got = torch.zeros(P, cs)
    for l in range(levels):
        got[:, l * K * K:(l + 1) * K * K] = style_ref.bilinear_sampler(lv[l][:, None], co / 2 ** l + delta).reshape(P, -1)
    S.check_lookup(got.view(B, H1, W1, cs), c["tight"], c["indep"], levels, r, "host_lookup", c["kind"] == "outside")
    S.le((c["tight"][0] - c["indep"][0]).abs(), c["indep"][1], "tight vs independent")


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=["-".join(map(str, c)) for c in UPSAMPLE_CASES])
def test_upsample_reference(case):
    B, h, w, mcs, spike = case
    coords1, mask = S.upsample_inputs(B, h, w, mcs, spike)
    ref, bound = S.upsample_ref(coords1, mask)
    got = raft_ref.upsample_flow(coords1 - raft_ref.coords_grid(B, h, w), mask[..., :576].permute(0, 3, 1, 2).contiguous())
    assert torch.isfinite(got).all()
    S.le((got.double() - ref).abs(), bound, "upsample fp32")
    assert float(bound.max()) <= 100 * S.U * float((8 * (coords1 - raft_ref.coords_grid(B, h, w))).abs().max())


# ================================================================================ masks
def test_masked_tier_reproduces_reference_golden(golden):
    g = golden("style_small")
    x = torch.from_numpy(g["fsw_x"]).permute(0, 2, 3, 1).contiguous()
    gout = torch.from_numpy(g["fsw_gout"]).permute(0, 2, 3, 1).contiguous()
    for case in ("zero", "frac", "oob"):
        flow = torch.from_numpy(g[f"fsw_{case}_flow"])
        ref, bound, valid = S.warp_fwd_tight(x, flow, False, True)
        y = torch.from_numpy(g[f"fsw_{case}_y"]).permute(0, 2, 3, 1).double()
        S.le((y - ref).abs(), bound, f"fsw_{case}_y")
        assert bool((y[~valid] == 0).all())
        dref, dbound, _ = S.warp_bwd_tight(gout, flow, False, True)
        dx = torch.from_numpy(g[f"fsw_{case}_dx"]).permute(0, 2, 3, 1).double()
        S.le((dx - dref).abs(), dbound, f"fsw_{case}_dx")
    assert 0.3 < float((~valid).double().mean()) < 1.0


def test_masked_cases_keep_off_the_threshold():
    """No sample of any masked case has a validity sum in [0.9997, 0.99995]: the excluded share is 0."""
    for shape in sorted({s[:3] for s, _ in FWD_CASES} | {s[:3] for s, _ in BWD_CASES}):
        for family in S.FAMILIES:
            for align in (False, True):
                S.assert_off_threshold(S.make_flow(family, *shape), align)


def test_flow_families():
    N, H, W = 2, 37, 53
    for align in (False, True):
        _, _, _, inb, _ = S.geometry(S.make_flow("far", N, H, W), align)
        assert not any(bool(i.any()) for i in inb)
        cx, cy, w, inb, valid = S.geometry(S.make_flow("sweep", N, H, W), align)
        some = inb[0] | inb[1] | inb[2] | inb[3]
        every = inb[0] & inb[1] & inb[2] & inb[3]
        assert 0.2 < some.mean() < 0.95 and 0.1 < every.mean() < 0.8     # inside and outside
    cx, cy, w, inb, _ = S.geometry(S.make_flow("quarter", N, H, W), True)
    assert (w[0] == 1).mean() > 0.03                                      # exactly on a pixel centre: floor decides
    cx, cy, w, inb, _ = S.geometry(S.make_flow("converge", N, H, W))
    cnt = sum(np.bincount((cy[k] * W + cx[k])[0][inb[k][0]], minlength=H * W) for k in range(4))
    assert cnt.max() > 100                                                # hundreds of contributions on one target
    cx, cy, w, inb, _ = S.geometry(S.make_flow("ident", N, H, W))
    k = np.argmax(np.stack(w), 0)[None]
    xs = np.broadcast_to(np.arange(W)[None, None], (N, H, W))
    ys = np.broadcast_to(np.arange(H)[None, :, None], (N, H, W))
    assert (np.take_along_axis(np.stack(w), k, 0) > 0.9999).all()      # all the weight on the sample's own pixel
    assert (np.take_along_axis(np.stack(cx), k, 0)[0] == xs).all() and (np.take_along_axis(np.stack(cy), k, 0)[0] == ys).all()


def test_fbcheck_inputs_discriminate():
    means = {}
    for shape in S.FBC_SHAPES:
        for pair in S.FBC_PAIRS:
            m = S.fbc_ref(*S.fbc_flows(pair, shape))
            assert m.shape == (shape[0], 1) + shape[1:] and bool(((m == 0) | (m == 1)).all())
            means[(shape, pair)] = float(m.mean())
    assert 0.3 < means[((3, 17, 19), "consistent")] < 1.0 and 0.3 < means[((2, 5, 300), "consistent")] < 1.0
    assert means[((3, 17, 19), "inconsistent")] < 0.3
    assert 0.02 < means[((3, 17, 19), "quarter")] < 0.98


# ================================================================================ the cases discriminate
def _wrong_warp_fwd(shape, family, align, masked, mutate):
    case = S.warp_case(shape, family, align, masked)
    return S.warp_fwd_tight(case["x"], case["flow"], align, masked, mutate)[0].float(), case


def _wrong_warp_bwd(shape, family, align, masked, mutate):
    case = S.warp_bwd_case(shape, family, align, masked)
    return S.warp_bwd_tight(case["gout"], case["flow"], align, masked, mutate)[0].float(), case


def _temporal_mut(shape, cscl, mutate):
    c = temporal_case(shape, cscl, "iid")
    w = S.temporal_tight(c["a"], c["b"], c["flow"], c["mask"], c["lam"], c["cl"], c["gout"], None, mutate)
    return c, w


def _lookup_mut(case, mutate):
    c = lookup_case(*case)
    B, H1, W1, H2, W2, ld0, levels, r, cs = c["geo"]
    wrong = S.lookup_tight(c["buf"], c["coords"], B, H1, W1, H2, W2, ld0, levels, r, cs, mutate)[0].float()
    return lambda: S.check_lookup(wrong, c["tight"], c["indep"], levels, r, "mut")


def _fwd(shape, family, align, masked, mutate):
    wrong, case = _wrong_warp_fwd(shape, family, align, masked, mutate)
    return lambda: S.check_warp_fwd(wrong, case, "mut")


def _bwd(shape, family, align, masked, mutate):
    wrong, case = _wrong_warp_bwd(shape, family, align, masked, mutate)
    return lambda: S.check_warp_bwd(wrong, case, "mut")


def _tloss(shape, cscl, mutate):
    c, w = _temporal_mut(shape, cscl, mutate)
    return lambda: S.check_temporal(w["loss"], None, None, c["ref"], None, None, "mut")


def _tgrad(shape, cscl, mutate):
    c, w = _temporal_mut(shape, cscl, mutate)
    return lambda: S.check_temporal(None, w["ga"].float(), w["gb"].float(), c["ref"], None, None, "mut")


# mutation -> the GPU-test cases (test id in tests/test_gpu_sampling.py, builder) that reject it
REJECTED_BY = {
    "swap_ne_sw": [("test_warp_fwd[3x5x7x8-iid]", lambda m: _fwd((3, 5, 7, 8), "iid", False, False, m)),
                   ("test_warp_fwd[2x37x53x64-sweep]", lambda m: _fwd((2, 37, 53, 64), "sweep", True, True, m)),
                   ("test_warp_bwd[3x5x7x20-iid]", lambda m: _bwd((3, 5, 7, 20), "iid", False, False, m)),
                   ("test_temporal[2x37x53-cs4cl3]", lambda m: _tloss((2, 37, 53), (4, 3), m))],
    "ignore_align": [("test_warp_fwd[3x5x7x8-iid]", lambda m: _fwd((3, 5, 7, 8), "iid", True, False, m)),
                     ("test_warp_fwd[2x9x11x128-quarter]", lambda m: _fwd((2, 9, 11, 128), "quarter", True, True, m)),
                     ("test_warp_bwd[2x37x53x4-converge]", lambda m: _bwd((2, 37, 53, 4), "converge", True, False, m))],
    "chunk0": [("test_warp_fwd[3x5x7x8-iid]", lambda m: _fwd((3, 5, 7, 8), "iid", False, False, m)),
               ("test_warp_fwd[2x37x53x64-iid]", lambda m: _fwd((2, 37, 53, 64), "iid", False, False, m)),
               ("test_warp_fwd[2x9x11x128-ident]", lambda m: _fwd((2, 9, 11, 128), "ident", False, True, m)),
               ("test_warp_fwd[1x6x1x12-quarter]", lambda m: _fwd((1, 6, 1, 12), "quarter", True, False, m))],
    "image_stride_hw": [("test_warp_fwd[3x5x7x8-iid]", lambda m: _fwd((3, 5, 7, 8), "iid", False, False, m)),
                        ("test_warp_fwd[3x1x7x4-quarter]", lambda m: _fwd((3, 1, 7, 4), "quarter", True, False, m)),
                        ("test_temporal[3x5x17-cs8cl5]", lambda m: _tloss((3, 5, 17), (8, 5), m))],
    "swap_hw_norm": [("test_warp_fwd[3x5x7x8-iid]", lambda m: _fwd((3, 5, 7, 8), "iid", False, False, m)),
                     ("test_warp_fwd[1x3x300x4-ident]", lambda m: _fwd((1, 3, 300, 4), "ident", False, False, m)),
                     ("test_warp_bwd[2x37x53x64-sweep]", lambda m: _bwd((2, 37, 53, 64), "sweep", False, True, m)),
                     ("test_temporal[3x1x7-cs4cl1]", lambda m: _tgrad((3, 1, 7), (4, 1), m))],
    "cs_for_cl": [("test_temporal[3x5x17-cs4cl3]", lambda m: _tloss((3, 5, 17), (4, 3), m)),
                  ("test_temporal[3x5x17-cs8cl5]", lambda m: _tgrad((3, 5, 17), (8, 5), m)),
                  ("test_temporal[1x6x1-cs4cl1]", lambda m: _tloss((1, 6, 1), (4, 1), m))],
    "gb_pad_unwritten": [("test_temporal[3x5x17-cs4cl3]", lambda m: _tgrad((3, 5, 17), (4, 3), m)),
                         ("test_temporal[1x1x257-cs8cl5]", lambda m: _tgrad((1, 1, 257), (8, 5), m))],
    "lvl_divisor": [("test_corr_lookup[13-10-3-1-near-0]", lambda m: _lookup_mut((13, 10, 3, 1, "near", 0), m)),
                    ("test_corr_lookup[16-24-4-4-grid-0]", lambda m: _lookup_mut((16, 24, 4, 4, "grid", 0), m))],
    "transpose_window": [("test_corr_lookup[13-10-3-1-near-0]", lambda m: _lookup_mut((13, 10, 3, 1, "near", 0), m)),
                         ("test_corr_lookup[7-9-2-1-border-8]", lambda m: _lookup_mut((7, 9, 2, 1, "border", 8), m))],
}


def test_every_mutation_has_a_case():
    assert set(REJECTED_BY) == set(S.MUTATIONS)


@pytest.mark.parametrize("mutate", S.MUTATIONS)
def test_mutation_is_rejected(mutate):
    """Each listed GPU-test case rejects the mutation through the comparison function the GPU test calls; without
    the mutation the same call passes (the rejection is the mutation's doing)."""
    for test_id, build in REJECTED_BY[mutate]:
        build(None)()
        with pytest.raises(AssertionError):
            build(mutate)()
        print(f"{mutate}: rejected by {test_id}")


# ================================================================================ host argument checks
def test_zero_sized_calls_are_refused_on_host():
    """Every rejection happens before a launch: the non-null pointers below are never dereferenced."""
    import gbvst
    lib = gbvst._lib.load()
    null, p = None, 4096
    for name in ("vst_warp_bwd_input", "vst_warp_masked_bwd_input"):
        fn = getattr(lib, name)
        what = name[4:].encode() + b": bad args"
        # (gout, flow, gx, N, H, W, Cs, align, stream)
        for args in ((p, p, p, 0, 8, 8, 4, 0), (p, p, p, 1, 0, 8, 4, 0), (p, p, p, 1, 8, 0, 4, 0), (p, p, p, -1, 8, 8, 4, 0),
                     (p, p, p, 1, 8, 8, 0, 0), (null, p, p, 1, 8, 8, 4, 0), (p, null, p, 1, 8, 8, 4, 0),
                     (p, p, null, 1, 8, 8, 4, 0)):
            assert fn(*args, null) != 0, (name, args)
            assert what in lib.vst_last_error(), (name, args)
    # (a, b, flow, mask, loss, part, N, H, W, Cs, Cl, lambda, stream)
    for args in ((p, p, p, p, p, p, 0, 8, 8, 4, 3), (p, p, p, p, p, p, 1, 0, 8, 4, 3), (p, p, p, p, p, p, 1, 8, 0, 4, 3),
                 (p, p, p, p, p, p, 1, 8, 8, 4, 0), (p, p, p, p, p, p, 1, 8, 8, 4, -1), (p, p, p, p, p, p, 1, 8, 8, 4, 5),
                 (p, p, p, p, null, p, 1, 8, 8, 4, 3), (p, p, p, p, p, null, 1, 8, 8, 4, 3)):
        assert lib.vst_loss_temporal(*args, 1.0, null) != 0, args
        assert b"loss_temporal: bad args" in lib.vst_last_error(), args
    # (a, b, flow, mask, gout, ga, gb, N, H, W, Cs, Cl, lambda, stream)
    for args in ((p, p, p, p, p, p, p, 0, 8, 8, 4, 3), (p, p, p, p, p, p, p, 1, 0, 8, 4, 3),
                 (p, p, p, p, p, p, p, 1, 8, 0, 4, 3), (p, p, p, p, p, p, p, 1, 8, 8, 4, 0),
                 (p, p, p, p, p, p, p, 1, 8, 8, 4, 5), (p, p, p, p, p, null, null, 1, 8, 8, 4, 3),
                 (p, p, p, p, null, p, p, 1, 8, 8, 4, 3)):
        assert lib.vst_loss_temporal_bwd(*args, 1.0, null) != 0, args
        assert b"loss_temporal_bwd: bad args" in lib.vst_last_error(), args
    # corr_lookup documents that a level smaller than 2x2 is refused: 3 levels of 7x9 end at 1x2
    assert lib.vst_corr_lookup(p, p, p, 1, 4, 4, 7, 9, 64, 3, 1, 28, null) != 0
    assert b"level 2 smaller than 2x2" in lib.vst_last_error()
