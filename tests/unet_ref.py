"""CPU reference of the U-Net generators (reference networks.py:436-535 with norm=instance, no dropout) and of
the two skip-connection kernels (vst_instnorm_skip_fwd / _bwd), in any float dtype (the GPU tests use float64).

Written from the semantics, not from the module tree.  UnetSkipConnectionBlock.forward returns
cat([x, model(x)], 1), and both activations around it run IN PLACE: the child's LeakyReLU(0.2) has already
overwritten x when the concatenation is made, and the parent's ReLU then runs over the whole concatenation.  With
z_l the pre-activation output of level l's down path (IN(conv) for the middle levels, the bare conv for level 0):

    d_l   = lrelu(z_l)                       the next down conv's input
    cat   = [lrelu(z_l), IN(u_{l+1})]        what block l + 1 returns
    relu(cat) = [relu(z_l), relu(IN(u))]     what the up conv of block l reads (relu(lrelu(z)) = relu(z))

unet_forward states exactly that with out-of-place ops, so torch autograd gives the gradients; the reference
itself (imported by tools/gen_golden_unet.py) produced tests/golden/unet_small.npz, which test_unet_host.py holds
this restatement against.  Weights come from make_state (numpy's frozen RandomState stream), so none are stored.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import reduction_ref as R

SLOPE, EPS = 0.2, 1e-5
CASES = {"a": (5, 700), "b": (7, 710)}      # tools/gen_golden_unet.py: num_downs, weight seed (ngf 4)
FIXTURE_THREADS = 8                          # ... and the torch thread count it ran with


# ----------------------------------------------------------------------------------- parameters
def level_prefixes(num_downs):
    """[(down conv key prefix, up conv key prefix)] from the outermost block (level 0) inwards, in the reference's
    Sequential numbering: outermost [down, sub, relu, up, tanh], middle [lrelu, down, norm, sub, relu, up, norm],
    innermost [lrelu, down, relu, up, norm]."""
    out, p = [("model.model.0", "model.model.3")], "model.model.1"
    for l in range(1, num_downs):
        inner = l == num_downs - 1
        out.append((p + ".model.1", p + (".model.3" if inner else ".model.5")))
        p += ".model.3"
    return out


def channels(num_downs, ngf):
    return [ngf * min(2 ** l, 8) for l in range(num_downs)]


def unet_shapes(input_nc, output_nc, num_downs, ngf):
    """state_dict key -> shape, in the reference's parameter order (every down conv outermost first, then the up
    convs innermost first)."""
    c = channels(num_downs, ngf)
    pre = level_prefixes(num_downs)
    sh = {}
    for l, (dk, _) in enumerate(pre):
        cin = input_nc if l == 0 else c[l - 1]
        sh[dk + ".weight"], sh[dk + ".bias"] = (c[l], cin, 4, 4), (c[l],)
    for l in range(num_downs - 1, -1, -1):
        uk = pre[l][1]
        cin = c[l] if l == num_downs - 1 else 2 * c[l]
        cout = output_nc if l == 0 else c[l - 1]
        sh[uk + ".weight"], sh[uk + ".bias"] = (cin, cout, 4, 4), (cout,)
    return sh


def normed_bias_keys(num_downs):
    """Biases whose conv feeds an InstanceNorm (exact gradient 0): every one but the outermost down conv's, the
    innermost down conv's and the outermost up conv's."""
    pre = level_prefixes(num_downs)
    return {pre[l][0] + ".bias" for l in range(1, num_downs - 1)} | {pre[l][1] + ".bias" for l in range(1, num_downs)}


def make_state(seed, shapes):
    """Deterministic fp32 weights by name: N(0, 1 / fan) weights with fan = prod(shape[1:]) (activations stay
    O(1) through every level) and N(0, 0.1^2) biases, from one RandomState(seed) stream in key order."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, s in shapes.items():
        v = rs.standard_normal(s)
        sd[k] = (v / np.sqrt(np.prod(s[1:])) if len(s) == 4 else 0.1 * v).astype(np.float32)
    return sd


# -------------------------------------------------------------------------------------- network
def _inorm(x):
    mean, rstd = R.in_stats(x, EPS)
    return (x - mean) * rstd


def _net_inorm(x):
    # the network restatement normalises with the stock operator in every dtype: in fp32 it is then the same
    # sequence of ATen calls as the fixture's generator, which the 1e-6 bar of test_unet_host.py needs (an
    # explicit mean / variance in fp32 lands 1.4e-6 / 5e-6 from the fixture at 128 x 128, its rounding alone)
    return F.instance_norm(x, eps=EPS)


def unet_forward(sd, x, num_downs):
    """sd: key -> tensor (x's dtype).  NCHW in, NCHW out."""
    pre = level_prefixes(num_downs)

    def down(l, a):
        return F.conv2d(a, sd[pre[l][0] + ".weight"], sd[pre[l][0] + ".bias"], stride=2, padding=1)

    def up(l, a):
        return F.conv_transpose2d(a, sd[pre[l][1] + ".weight"], sd[pre[l][1] + ".bias"], stride=2, padding=1)

    z = [down(0, x)]
    for l in range(1, num_downs - 1):
        z.append(_net_inorm(down(l, F.leaky_relu(z[-1], SLOPE))))
    h = down(num_downs - 1, F.leaky_relu(z[-1], SLOPE))
    u = _net_inorm(up(num_downs - 1, F.relu(h)))
    for l in range(num_downs - 2, -1, -1):
        cat = torch.cat([F.leaky_relu(z[l], SLOPE), u], 1)
        u = up(l, F.relu(cat))
        u = torch.tanh(u) if l == 0 else _net_inorm(u)
    return u


class RefUnet(nn.Module):
    """unet_forward over parameters held under the reference's key names (state_dict round trip by name)."""

    def __init__(self, input_nc, output_nc, num_downs, ngf, dtype=torch.float64):
        super().__init__()
        self.num_downs = num_downs
        self.shapes = unet_shapes(input_nc, output_nc, num_downs, ngf)
        self.keys = list(self.shapes)
        self.params = nn.ParameterList([nn.Parameter(torch.zeros(s, dtype=dtype)) for s in self.shapes.values()])

    def load_np(self, sd):
        with torch.no_grad():
            for k, p in zip(self.keys, self.params):
                p.copy_(torch.from_numpy(sd[k]).to(p.dtype))
        return self

    def named(self):
        return dict(zip(self.keys, self.params))

    def forward(self, x):
        return unet_forward(self.named(), x, self.num_downs)


def run_case(sd, x, r, num_downs, dtype):
    """Output, input gradient and parameter gradients of sum(out * r) in dtype; numpy in, tensors out."""
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = unet_forward(t, xt, num_downs)
    (out * torch.from_numpy(r).to(dtype)).sum().backward()
    return out.detach(), xt.grad, {k: v.grad for k, v in t.items()}


# ------------------------------------------------------------------------------ the two kernels
def skip_fwd(y, use_stats, slope=SLOPE):
    """y NCHW float64 -> (d = lrelu(z), skip = relu(z), z), z = IN(y) or y."""
    z = _inorm(y) if use_stats else y
    return R.act_fwd(z, "lrelu", slope), R.act_fwd(z, "relu", 0.0), z


def skip_bwd(g_d, g_s, y, use_stats, slope=SLOPE):
    """(dy, db): g = g_d * lrelu'(z) + g_s * relu'(z) (g_d None: 0), then the IN backward (or dy = g)."""
    if use_stats:
        mean, rstd = R.in_stats(y, EPS)
        z = (y - mean) * rstd
    else:
        z = y
    g = g_s * R.act_grad(z, "relu", 0.0)
    if g_d is not None:
        g = g + g_d * R.act_grad(z, "lrelu", slope)
    if not use_stats:
        return g, g.sum(dim=(0, 2, 3))
    return R.in_bwd(g, y, mean, rstd, "none", 0.0)


# ----------------------------------------------------------------------------------- train step
def ref_cyclegan_unet(ngf, ndf, num_downs, dtype=torch.float64, **kw):
    """oracle.cpu_ref.RefCycleGANCon (its losses, step order and Adam, imported unchanged) with the two
    generators replaced by RefUnet and everything in dtype."""
    from oracle import cpu_ref

    class _Step(cpu_ref.RefCycleGANCon):
        def __init__(self):
            self.G_A = RefUnet(3, 3, num_downs, ngf, dtype)
            self.G_B = RefUnet(3, 3, num_downs, ngf, dtype)
            self.D_A = cpu_ref.RefNLayerDiscriminator(3, ndf).to(dtype)
            self.D_B = cpu_ref.RefNLayerDiscriminator(3, ndf).to(dtype)
            self.lA, self.lB, self.lT, self.lI = (kw.get("lambda_A", 10.0), kw.get("lambda_B", 10.0),
                                                  kw.get("lambda_T", 10.0), kw.get("lambda_idt", 0.5))
            lr, beta1 = kw.get("lr", 2e-4), kw.get("beta1", 0.5)
            self.opt_G = torch.optim.Adam(list(self.G_A.parameters()) + list(self.G_B.parameters()), lr=lr,
                                          betas=(beta1, 0.999))
            self.opt_D = torch.optim.Adam(list(self.D_A.parameters()) + list(self.D_B.parameters()), lr=lr,
                                          betas=(beta1, 0.999))

    return _Step()
