"""CPU-only: (a) the fp64 references of tests/reduction_ref.py against float64 autograd of the stock
ops, (b) every InstanceNorm geometry case of the GPU suite really reaches the branch it is listed
for, read off the built library's workspace sizes (host code only), so a later change to red_geom /
fin_cpb cannot silently un-cover a branch, (c) unsupported widths are refused."""
import pytest
import torch
import torch.nn.functional as F

import reduction_ref as R

RTOL = 1e-10


def _g(seed, shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _same(got, ref, what):
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape and err <= RTOL * scale, f"{what}: {err:.3e} of {scale:.3e}"


def _stock_act(z, act, slope):
    return {"none": lambda v: v, "relu": F.relu, "lrelu": lambda v: F.leaky_relu(v, slope)}[act](z)


# ------------------------------------------------------------------- a. reference self-check
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_in_ref_vs_autograd(act):
    N, C, H, W, eps, slope = 2, 5, 4, 3, 1e-5, 0.2
    x = (_g(1, (N, C, H, W), 2.0) + 0.5).requires_grad_(True)
    res, g = _g(2, (N, C, H, W)), _g(3, (N, C, H, W))
    y = _stock_act(F.instance_norm(x, eps=eps), act, slope) + res
    y.backward(g)
    xd = x.detach()
    mean, rstd = R.in_stats(xd, eps)
    _same(R.in_fwd(xd, mean, rstd, act, slope, res), y.detach(), "in_fwd")
    dx, db = R.in_bwd(g, xd, mean, rstd, act, slope)
    _same(dx, x.grad, "in_bwd")
    # the per-channel sum is 0 in exact arithmetic: both sides only carry rounding noise
    assert (db - x.grad.sum(dim=(0, 2, 3))).abs().max().item() <= RTOL * x.grad.abs().sum().item()
    # a supplied decision mask replaces the reference's own decisions
    dxm, _ = R.in_bwd(g, xd, mean, rstd, act, slope, mask=(xd - mean) * rstd > 0)
    _same(dxm, x.grad, "in_bwd(mask)")


@pytest.mark.parametrize("gate", [None, 0.7, -0.4])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_in_affine_ref_vs_autograd(act, gate):
    N, C, H, W, eps, slope, mult = 2, 6, 3, 5, 1e-5, 0.2, 0.9
    x = (_g(4, (N, C, H, W), 2.0) + 0.5).requires_grad_(True)
    gam = (_g(5, (C,), 0.2) + 1).requires_grad_(True)
    bet = _g(6, (C,), 0.2).requires_grad_(True)
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)   # a conv bias in front of the norm
    res, g = _g(7, (N, C, H, W)), _g(8, (N, C, H, W))
    y = _stock_act(F.instance_norm(x + bias.view(1, -1, 1, 1), weight=gam, bias=bet, eps=eps), act, slope)
    gt = None
    if gate is not None:
        gt = torch.tensor(gate, dtype=torch.float64, requires_grad=True)
        u = (mult * gt).abs()
        y = 2 * u / (1 + u) * y
    y = y + res
    y.backward(g)
    xd, gd, bd = x.detach(), gam.detach(), bet.detach()
    mean, rstd = R.in_stats(xd, eps)
    _same(R.in_affine_fwd(xd, mean, rstd, gd, bd, act, slope, gate, mult, res), y.detach(), "affine fwd")
    r = R.in_affine_bwd(g, xd, mean, rstd, gd, bd, act, slope, gate, mult)
    _same(r["dx"], x.grad, "affine dx")
    _same(r["dgamma"], gam.grad, "dgamma")
    _same(r["dbeta"], bet.grad, "dbeta")
    if gate is not None:
        _same(r["dgate"], gt.grad, "dgate")
    assert (r["dbias"] - bias.grad).abs().max().item() <= RTOL * x.grad.abs().sum().item()


@pytest.mark.parametrize("N,HW", [(1, 2), (3, 2), (3, 15)])
def test_running_update_ref_vs_stock(N, HW):
    C, mom, eps = 4, 0.1, 1e-5
    x = _g(9, (N, C, HW, 1), 1.5) + 0.3
    rm, rv = _g(10, (C,)), _g(11, (C,)).abs() + 0.5
    rm_s, rv_s = rm.clone(), rv.clone()
    F.instance_norm(x, running_mean=rm_s, running_var=rv_s, use_input_stats=True, momentum=mom, eps=eps)
    mean, rstd = R.in_stats(x, eps)
    var = 1.0 / rstd ** 2 - eps
    got_m, got_v = R.running_update(mean[:, :, 0, 0], var[:, :, 0, 0], rm, rv, HW, mom)
    _same(got_m, rm_s, "running_mean")
    _same(got_v, rv_s, "running_var")


@pytest.mark.parametrize("cs,cl", [(4, 3), (4, 1), (4, 4), (8, 5)])
def test_loss_refs_vs_autograd(cs, cl):
    N, H, W, scale, gout, t = 2, 3, 5, 2.5, -0.37, 0.9
    a = _g(12, (N, cs, H, W)).requires_grad_(True)
    b = _g(13, (N, cs, H, W))
    mask = (_g(14, (N, 1, H, W)) > 0).double() * 0.6
    ac, bc = a[:, :cl], b[:, :cl]
    stock = {
        "l1": scale * F.l1_loss(ac, bc),
        "masked_l1": scale * (mask * (ac - bc).abs()).mean(),
        "masked_l1_nomask": scale * (ac - bc).abs().mean(),
        "mse_const": scale * F.mse_loss(ac, torch.full_like(ac, t)),
        "mse": scale * F.mse_loss(ac, bc),
    }
    ad = a.detach()
    mine = {
        "l1": R.l1(ad, b, cl, scale, gout),
        "masked_l1": R.masked_l1(ad, b, mask, cl, scale, gout),
        "masked_l1_nomask": R.masked_l1(ad, b, None, cl, scale, gout),
        "mse_const": R.mse_const(ad, t, cl, scale, gout),
        "mse": R.mse(ad, b, cl, scale, gout),
    }
    for k, v in stock.items():
        a.grad = None
        v.backward(torch.tensor(gout, dtype=torch.float64))
        _same(mine[k][0], v.detach(), k)
        _same(mine[k][1], a.grad, k + " grad")
        assert mine[k][1][:, cl:].abs().sum().item() == 0


@pytest.mark.parametrize("cl", [3, 1])
def test_tv_ref_vs_oracle(cl):
    from oracle.style_ref import calc_tv_loss
    img = _g(15, (2, 4, 5, 6), 30.0).requires_grad_(True)   # no flat patch: every r > 0
    v = calc_tv_loss(img[:, :cl])
    v.backward()
    _same(R.tv(img.detach(), cl), v.detach(), "tv")
    _same(R.tv_grad(img.detach(), cl), img.grad, "tv_grad")


def test_tv_ref_flat_patch_is_finite():
    img = _g(16, (1, 4, 6, 6), 30.0)
    img[:, :, 1:4, 1:4] = 2.0
    g = R.tv_grad(img, 3)
    # pixel (2, 2): its own term and the ones above and to its left all have r = 0
    assert torch.isfinite(g).all() and g[0, :3, 2, 2].abs().sum().item() == 0 and g[0, :3, 1, 1].abs().sum().item() > 0


# ----------------------------------------------------------------- b. geometry reachability
@pytest.fixture(scope="module")
def lib():
    import gbvst
    gbvst._lib.build()
    return gbvst._lib.load()


@pytest.mark.parametrize("case", R.IN_CASES, ids=[c[0] for c in R.IN_CASES])
def test_in_case_reaches_its_branch(lib, case):
    _, (N, H, W, C), nsplit, expect = case
    HW = H * W
    # plain IN: N*nsplit*C*{3 doubles} + N*C*{float2 + double} + 256
    b = lib.vst_instnorm_ws_bytes(N, HW, C) - 256 - N * C * 16
    assert b % (N * C * 24) == 0 and b // (N * C * 24) == nsplit
    # affine IN: N*nsplit*C*{4 doubles} + N*C*{float2 + 4 doubles} + 256
    b = lib.vst_instnorm_affine_ws_bytes(N, HW, C) - 256 - N * C * 40
    assert b % (N * C * 32) == 0 and b // (N * C * 32) == nsplit
    g = R.geom(N, HW, C)
    assert g["nsplit"] == nsplit, g
    for k, v in expect.items():
        assert g[k] == v, (k, g)
    if "rows" in expect and expect["rows"][0]:
        assert g["SP"] > 3 * g["PG"]   # the unrolled main loop of the partial kernel runs


def test_in_cases_cover_every_branch():
    """Between them the cases reach both finalize widths with and without the 4-chain loop, the unrolled
    partial loop with a remainder, a short last slice, idle threads, HW < PG and PG = 1."""
    gs = [R.geom(N, H * W, C) for _, (N, H, W, C), _, _ in R.IN_CASES]
    for cpb in (4, 16):
        for fold in (False, True):
            assert any(g["cpb"] == cpb and g["fold"] == fold for g in gs), (cpb, fold)
    assert any(g["rows"][0] and g["rows"][1] for g in gs)
    assert any(g["nsplit"] > 1 and g["tail"] < g["PG"] for g in gs)
    assert any(g["idle"] for g in gs) and any(g["hw_lt_pg"] for g in gs) and any(g["PG"] == 1 for g in gs)
    assert any(g["fold_aff"] for g in gs) and any(not g["fold_aff"] for g in gs)


# --------------------------------------------------------------------- c. unsupported widths
@pytest.mark.parametrize("C", [1028, 6])
def test_unsupported_widths_have_no_workspace(lib, C):
    assert lib.vst_instnorm_ws_bytes(2, 64, C) == 0
    assert lib.vst_instnorm_affine_ws_bytes(2, 64, C) == 0
