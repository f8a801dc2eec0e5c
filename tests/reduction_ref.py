"""fp64 references of the reduction families (InstanceNorm in csrc/norm.hip, the scalar losses in
csrc/loss.hip and csrc/style.hip) and the table of InstanceNorm geometries the tests walk.

Plain torch float64 on CPU tensors; nothing here imports the package or calls F.instance_norm, so
the references share no code with the kernels or with ATen's fp32 path.  Every function takes NCHW
float64 VIEWS of the fp32 tensors the device gets (``nchw64``), so both sides see the same numbers.
tests/test_reduction_ref_host.py checks each reference against float64 autograd of the stock ops.

Conventions the kernels document and the references follow: biased variance; sign(0) = 0; the
activation derivative at 0 is 0 for relu and ``slope`` for lrelu; a total-variation term with r = 0
contributes 0 to the gradient (autograd gives NaN there, so it cannot be the reference).
"""
import torch

F64 = torch.float64


def f32(v):
    """The value a C float parameter receives for the Python number v (eps, slope, momentum ...)."""
    return float(torch.tensor(v, dtype=torch.float32))


def nchw64(t, cl=None):
    """NCHW float64 view of an NHWC fp32 tensor (first cl channels)."""
    v = t.detach().cpu().permute(0, 3, 1, 2).to(F64)
    return v if cl is None else v[:, :cl]


# ------------------------------------------------------------------ InstanceNorm geometry cases
# (id, (N, H, W, C), nsplit, expectations).  nsplit is what the library's workspace size implies;
# the expectations are the branch each case is there to reach, in terms of geom() below:
#   cpb            channels per finalize block (fin_cpb)
#   tail           pixels in the last slice
#   rows           pixel rows per thread in a full slice: (rows in the 4x unrolled loop, remainder)
#   fold           the plain finalize's 4-chain loop runs (nsplit > 3 * 256 / cpb)
#   fold_aff       the affine finalize's 4-chain loop runs (CPB = 64: nsplit > 12)
#   idle           threads of the 256 beyond LP * PG
#   hw_lt_pg       fewer pixels than pixel groups
IN_CASES = [
    ("tail_cpb4", (2, 47, 45, 64), 67, dict(cpb=4, tail=3, fold=False, fold_aff=True, rows=(0, 2))),
    ("fold16_unrolled", (1, 16, 28, 256), 56, dict(cpb=16, fold=True)),
    ("fold4_unrolled", (1, 40, 40, 256), 200, dict(cpb=4, fold=True, fold_aff=True)),
    ("cpb16_wide_grid", (8, 16, 32, 256), 64, dict(cpb=16, fold=True)),
    ("part_unrolled_5", (1, 96, 96, 256), 461, dict(SP=20, rows=(4, 1), tail=16, cpb=4)),
    ("part_unrolled_6", (2, 113, 97, 128), 229, dict(SP=48, rows=(4, 2), tail=17, cpb=4)),
    ("c1024_pg1", (1, 33, 31, 1024), 512, dict(PG=1, SP=2, tail=1, cpb=4, fold_aff=True)),
    ("c1024_unrolled", (1, 50, 42, 1024), 420, dict(PG=1, SP=5, rows=(4, 1))),
    ("lp3", (2, 9, 7, 12), 1, dict(LP=3, PG=85, idle=1, hw_lt_pg=True)),
    ("lp18", (2, 15, 13, 72), 7, dict(LP=18, idle=4, cpb=16, fold_aff=False)),
    ("lp34_cpb4", (1, 50, 41, 136), 147, dict(LP=34, idle=18, cpb=4, tail=6, fold_aff=True)),
    ("tiny_hw", (3, 2, 2, 64), 1, dict(SP=4, hw_lt_pg=True)),
    ("c4", (2, 37, 29, 4), 3, dict(LP=1, PG=256)),
    ("c8", (4, 7, 5, 8), 1, dict(LP=2, PG=128)),
]
IN_CASE = {c[0]: c for c in IN_CASES}


def geom(N, HW, C):
    """The reduction geometry a (N, HW, C) tensor gets, from red_geom's four lines and fin_cpb's rule,
    and what follows from it.  The host test holds its nsplit against the library's."""
    LP = C // 4
    PG = 256 // LP
    SP = min(HW, -(-max(-(-N * HW // 512), 2 * PG) // PG) * PG)
    nsplit = -(-HW // SP)
    cpb = 16 if (-(-C // 16) * N >= 128 or nsplit < 64) else 4
    rows = -(-SP // PG)
    return dict(LP=LP, PG=PG, SP=SP, nsplit=nsplit, cpb=cpb, idle=256 - LP * PG,
                tail=HW - (nsplit - 1) * SP, rows=(rows // 4 * 4, rows % 4),
                fold=nsplit > 3 * (256 // cpb), fold_aff=nsplit > 3 * 4, hw_lt_pg=HW < PG)


# ------------------------------------------------------------------------------- activations
def _pos(z, mask):
    return (z > 0) if mask is None else mask


def act_fwd(z, act, slope, mask=None):
    if act == "none":
        return z
    return torch.where(_pos(z, mask), z, z * (slope if act == "lrelu" else 0.0))


def act_grad(z, act, slope, mask=None):
    """act'(z); at z == 0 relu gives 0 and lrelu gives slope."""
    if act == "none":
        return torch.ones_like(z)
    lo = slope if act == "lrelu" else 0.0
    return torch.where(_pos(z, mask), torch.ones_like(z), torch.full_like(z, lo))


# ------------------------------------------------------------------------------ InstanceNorm
def in_stats(x, eps):
    """Per (n, c) mean and 1 / sqrt(biased variance + eps), shaped [N, C, 1, 1]."""
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def in_fwd(x, mean, rstd, act, slope, residual=None, mask=None):
    """act((x - mean) * rstd) (+ residual).  mask: the x_hat > 0 decisions to use instead of its own."""
    y = act_fwd((x - mean) * rstd, act, slope, mask)
    return y if residual is None else y + residual


def in_bwd(g, x, mean, rstd, act, slope, mask=None):
    """Input gradient of in_fwd and its per-channel sum (the gradient of a conv bias in front)."""
    xh = (x - mean) * rstd
    gz = g * act_grad(xh, act, slope, mask)
    dx = rstd * (gz - gz.mean(dim=(2, 3), keepdim=True) - xh * (gz * xh).mean(dim=(2, 3), keepdim=True))
    return dx, dx.sum(dim=(0, 2, 3))


def gate_scale(gate, gate_mult):
    """s = 2|u| / (1 + |u|), u = gate_mult * gate, and ds/dgate."""
    u = gate_mult * gate
    au = abs(u)
    sgn = (u > 0) - (u < 0)
    return 2 * au / (1 + au), 2.0 / (1 + au) ** 2 * sgn * gate_mult


def in_affine_fwd(x, mean, rstd, gamma, beta, act, slope, gate=None, gate_mult=1.0, residual=None):
    """s * act(gamma * x_hat + beta) (+ residual); gamma, beta [C]; gate a Python float or None."""
    z = (x - mean) * rstd * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    y = act_fwd(z, act, slope)
    if gate is not None:
        y = gate_scale(gate, gate_mult)[0] * y
    return y if residual is None else y + residual


def in_affine_bwd(g, x, mean, rstd, gamma, beta, act, slope, gate=None, gate_mult=1.0):
    """dict: dx, dgamma, dbeta, dgate, dbias (= per-channel sum of dx: the conv-bias gradient), z, and
    the sums of the absolute terms behind dgamma / dbeta / dgate (the scale of their rounding error)."""
    ga = gamma.view(1, -1, 1, 1)
    xh = (x - mean) * rstd
    z = xh * ga + beta.view(1, -1, 1, 1)
    s, ds_dgate = (1.0, 0.0) if gate is None else gate_scale(gate, gate_mult)
    gz = s * g * act_grad(z, act, slope)
    dx = rstd * ga * (gz - gz.mean(dim=(2, 3), keepdim=True) - xh * (gz * xh).mean(dim=(2, 3), keepdim=True))
    ga_terms = g * act_fwd(z, act, slope)
    return dict(dx=dx, dgamma=(gz * xh).sum(dim=(0, 2, 3)), dbeta=gz.sum(dim=(0, 2, 3)),
                dgate=ga_terms.sum() * ds_dgate, dbias=dx.sum(dim=(0, 2, 3)), z=z,
                dgamma_abs=(gz * xh).abs().sum(dim=(0, 2, 3)), dbeta_abs=gz.abs().sum(dim=(0, 2, 3)),
                dgate_abs=ga_terms.abs().sum() * abs(ds_dgate))


def running_update(mean, var_biased, rm, rv, HW, momentum):
    """nn.InstanceNorm2d(track_running_stats=True): batch norm over (1, N*C, HW) with the buffers
    repeated N times, the N copies averaged.  mean, var_biased [N, C]; rm, rv [C]."""
    unb = HW / (HW - 1.0) if HW > 1 else 1.0
    rm_new = ((1 - momentum) * rm.unsqueeze(0) + momentum * mean).mean(dim=0)
    rv_new = ((1 - momentum) * rv.unsqueeze(0) + momentum * var_biased * unb).mean(dim=0)
    return rm_new, rv_new


# ------------------------------------------------------------------------------ scalar losses
# a, b: NCHW views of NHWC tensors with channel stride Cs; only the first cl channels count, the
# gradient of the others is exactly 0.  Each returns (value, gradient scaled by gout).
def _mean_loss(a, cl, terms, dterms, scale, gout):
    k = scale / terms.numel()
    grad = torch.zeros_like(a)
    grad[:, :cl] = gout * k * dterms
    return k * terms.sum(), grad


def l1(a, b, cl, scale, gout=1.0):
    d = a[:, :cl] - b[:, :cl]
    return _mean_loss(a, cl, d.abs(), torch.sign(d), scale, gout)


def masked_l1(a, b, mask, cl, scale, gout=1.0):
    """scale * mean(mask * |a - b|), mask [N, 1, H, W] or None (= 1); the mean is over N*H*W*cl."""
    d = a[:, :cl] - b[:, :cl]
    m = torch.ones_like(d[:, :1]) if mask is None else mask
    return _mean_loss(a, cl, m * d.abs(), m * torch.sign(d), scale, gout)


def mse_const(a, target, cl, scale, gout=1.0):
    d = a[:, :cl] - target
    return _mean_loss(a, cl, d * d, 2 * d, scale, gout)


def mse(a, b, cl, scale, gout=1.0):
    d = a[:, :cl] - b[:, :cl]
    return _mean_loss(a, cl, d * d, 2 * d, scale, gout)


def _tv_terms(img, cl):
    i = img[:, :cl]
    d1 = i[:, :, 1:, :-1] - i[:, :, :-1, :-1]   # I[y+1][x] - I[y][x]
    d2 = i[:, :, :-1, 1:] - i[:, :, :-1, :-1]   # I[y][x+1] - I[y][x]
    return d1, d2, torch.sqrt((d1 * d1).sum(dim=1, keepdim=True) + (d2 * d2).sum(dim=1, keepdim=True))


def tv(img, cl):
    """sum over (n, y < H-1, x < W-1) of r = sqrt(sum_c d1^2 + sum_c d2^2)."""
    return _tv_terms(img, cl)[2].sum()


def tv_grad(img, cl):
    """d tv / d img in closed form; a term with r == 0 contributes 0."""
    d1, d2, r = _tv_terms(img, cl)
    w = torch.where(r > 0, 1.0 / r, torch.zeros_like(r))
    g = torch.zeros_like(img)
    g[:, :cl, :-1, :-1] -= (d1 + d2) * w
    g[:, :cl, 1:, :-1] += d1 * w
    g[:, :cl, :-1, 1:] += d2 * w
    return g
