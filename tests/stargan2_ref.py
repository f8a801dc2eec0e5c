"""CPU reference of the StarGAN v2 networks (reference core/model.py with w_hpf = 0) and of the kernels under
them (AdaIN, avg_pool2d(2), the residual merge), in any float dtype (the GPU tests use float64).

Written from the architecture as functions over a ``{state_dict key: tensor}`` mapping, not from the module tree:

    ResBlk(x)         = (sc(x) + conv2(a(pool?(conv1(a(x)))))) / sqrt(2),   a = LeakyReLU(0.2) o [IN(affine)]
                        sc = pool? o [1x1 conv when the channel counts differ]
    AdaIN(x, s)       = (1 + gamma) * IN(x) + beta,   (gamma, beta) = halves of fc(s)
    AdainResBlk(x, s) = (conv2(lrelu(AdaIN2(conv1(up?(lrelu(AdaIN1(x, s)))), s))) + sc(x)) / sqrt(2),
                        sc = [1x1 conv] o up?
    Generator         = to_rgb o decode o encode o from_rgb: log2(img_size) - 4 down / up levels, two bottleneck
                        blocks each way, channels 2^14 / img_size doubling up to max_conv_dim
    StyleEncoder / Discriminator = heads o lrelu o conv4x4 o lrelu o ResBlk(down)^(log2(img_size) - 2) o conv3x3
    MappingNetwork    = 4 shared Linear + ReLU, per domain 3 Linear + ReLU and a Linear

torch autograd gives the gradients.  The reference's own modules (imported by tools/gen_golden_stargan2.py) produced
tests/golden/stargan2_small.npz, which test_stargan2_host.py holds this restatement against.  Weights come from
make_state and inputs from case_inputs (numpy's frozen RandomState stream), so none are stored.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import reduction_ref as R

SLOPE, EPS = 0.2, 1e-5
FIXTURE_THREADS = 8  # the torch thread count tools/gen_golden_stargan2.py ran with

# tools/gen_golden_stargan2.py: kind, constructor arguments, input shape, domain labels, weight seed.  The gradients
# are discontinuous where an activation's input crosses 0, and among a few million inputs some lie within fp32
# rounding of it whatever the seed; each case's seed is the one of a scan over [800, 860) / [810, 822) / [820, 832) /
# [830, 890) whose fp64 forward keeps the largest activation_margin (MARGIN: what test_stargan2_host.py holds it to).
CASES = {
    "G": dict(kind="generator", cfg=dict(img_size=256, style_dim=16, max_conv_dim=8), x=(2, 3, 64, 32), seed=811),
    "E": dict(kind="style_encoder", cfg=dict(img_size=64, style_dim=16, num_domains=3, max_conv_dim=8),
              x=(2, 3, 64, 64), y=[2, 0], seed=815),
    "D": dict(kind="discriminator", cfg=dict(img_size=64, num_domains=3, max_conv_dim=8), x=(2, 3, 64, 64),
              y=[2, 0], seed=831),
    "F": dict(kind="mapping_network", cfg=dict(latent_dim=16, style_dim=16, num_domains=3), x=(2, 16), y=[1, 1],
              seed=868),
}
# the reference's default-size nets (img_size 256, style_dim 64, latent_dim 16, num_domains 2, w_hpf 0)
DEFAULTS = {
    "generator": dict(img_size=256, style_dim=64, max_conv_dim=512),
    "mapping_network": dict(latent_dim=16, style_dim=64, num_domains=2),
    "style_encoder": dict(img_size=256, style_dim=64, num_domains=2, max_conv_dim=512),
    "discriminator": dict(img_size=256, num_domains=2, max_conv_dim=512),
}
MARGIN = {"G": 5e-7, "E": 3e-7, "D": 2e-7, "F": 5e-5}
BIG_ELEMS, BIG_ROWS = 1 << 15, 8


def stored(g):
    """What the fixture keeps of a parameter gradient: all of it, or — for the weights above BIG_ELEMS elements,
    the 64 -> 64 3x3 convs of G, the 256 -> 256 3x3 conv of E and D and the 512 x 512 layers of F — its first
    BIG_ROWS output rows (the size cap of a committed file)."""
    return g[:BIG_ROWS] if int(np.prod(g.shape)) > BIG_ELEMS else g


# ----------------------------------------------------------------------------------- parameters
def _conv(sh, p, cin, cout, k, bias=True):
    sh[p + ".weight"] = (cout, cin, k, k)
    if bias:
        sh[p + ".bias"] = (cout,)


def _lin(sh, p, cin, cout):
    sh[p + ".weight"], sh[p + ".bias"] = (cout, cin), (cout,)


def _resblk(sh, p, cin, cout, normalize):
    _conv(sh, p + ".conv1", cin, cin, 3)
    _conv(sh, p + ".conv2", cin, cout, 3)
    if normalize:
        for n in ("norm1", "norm2"):
            sh[p + "." + n + ".weight"], sh[p + "." + n + ".bias"] = (cin,), (cin,)
    if cin != cout:
        _conv(sh, p + ".conv1x1", cin, cout, 1, bias=False)


def _adainblk(sh, p, cin, cout, style_dim):
    _conv(sh, p + ".conv1", cin, cout, 3)
    _conv(sh, p + ".conv2", cout, cout, 3)
    _lin(sh, p + ".norm1.fc", style_dim, 2 * cin)
    _lin(sh, p + ".norm2.fc", style_dim, 2 * cout)
    if cin != cout:
        _conv(sh, p + ".conv1x1", cin, cout, 1, bias=False)


def generator_plan(img_size, max_conv_dim):
    """[(cin, cout, resample)] of the encoder blocks in order; the decoder is its mirror."""
    d = 2 ** 14 // img_size
    plan = []
    for _ in range(int(math.log2(img_size)) - 4):
        plan.append((d, min(2 * d, max_conv_dim), True))
        d = plan[-1][1]
    return plan + [(d, d, False)] * 2


def trunk_plan(img_size, max_conv_dim):
    d = 2 ** 14 // img_size
    plan = []
    for _ in range(int(math.log2(img_size)) - 2):
        plan.append((d, min(2 * d, max_conv_dim)))
        d = plan[-1][1]
    return plan


def shapes(kind, **cfg):
    """state_dict key -> shape in the reference's key order."""
    sh = {}
    if kind == "generator":
        plan = generator_plan(cfg["img_size"], cfg["max_conv_dim"])
        _conv(sh, "from_rgb", 3, plan[0][0], 3)
        for i, (cin, cout, _) in enumerate(plan):
            _resblk(sh, "encode.%d" % i, cin, cout, True)
        for i, (cin, cout, _) in enumerate(reversed(plan)):
            _adainblk(sh, "decode.%d" % i, cout, cin, cfg["style_dim"])
        d0 = plan[0][0]
        sh["to_rgb.0.weight"], sh["to_rgb.0.bias"] = (d0,), (d0,)
        _conv(sh, "to_rgb.2", d0, 3, 1)
    elif kind == "mapping_network":
        _lin(sh, "shared.0", cfg["latent_dim"], 512)
        for i in (2, 4, 6):
            _lin(sh, "shared.%d" % i, 512, 512)
        for d in range(cfg["num_domains"]):
            for i in (0, 2, 4):
                _lin(sh, "unshared.%d.%d" % (d, i), 512, 512)
            _lin(sh, "unshared.%d.6" % d, 512, cfg["style_dim"])
    elif kind in ("style_encoder", "discriminator"):
        top = "shared" if kind == "style_encoder" else "main"
        plan = trunk_plan(cfg["img_size"], cfg["max_conv_dim"])
        _conv(sh, top + ".0", 3, plan[0][0], 3)
        for i, (cin, cout) in enumerate(plan):
            _resblk(sh, "%s.%d" % (top, i + 1), cin, cout, False)
        dl, n = plan[-1][1], len(plan)
        _conv(sh, "%s.%d" % (top, n + 2), dl, dl, 4)
        if kind == "style_encoder":
            for d in range(cfg["num_domains"]):
                _lin(sh, "unshared.%d" % d, dl, cfg["style_dim"])
        else:
            _conv(sh, "%s.%d" % (top, n + 4), dl, cfg["num_domains"], 1)
    else:
        raise ValueError(kind)
    return sh


def param_count(sh):
    return sum(int(np.prod(s)) for s in sh.values())


def make_state(seed, shapes):
    """Deterministic fp32 weights by name from one RandomState(seed) stream in key order: N(0, 1 / fan) conv and
    linear weights with fan = prod(shape[1:]) (activations stay O(1) through every block), N(0, 0.1^2) biases and
    1 + N(0, 0.1^2) norm weights."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, s in shapes.items():
        v = rs.standard_normal(s)
        if len(s) > 1:
            v = v / np.sqrt(np.prod(s[1:]))
        else:
            v = 0.1 * v + (1.0 if k.endswith(".weight") else 0.0)
        sd[k] = v.astype(np.float32)
    return sd


def case_inputs(seed, shape, out_shape):
    """(x, r): the input (u8 levels mapped to [-1, 1] for images, N(0, 1) for codes) and the upstream gradient r
    (multiples of 1/4 in [-1, 1]) of the loss sum(out * r)."""
    rs = np.random.RandomState(seed)
    if len(shape) == 4:
        x = ((rs.randint(0, 256, shape).astype(np.float32) / 255.0) - 0.5) / 0.5
    else:
        x = rs.standard_normal(shape)
    r = rs.randint(-4, 5, out_shape).astype(np.float32) / 4.0
    return x.astype(np.float32), r


def out_shape(name):
    c = CASES[name]
    B = c["x"][0]
    return {"generator": c["x"], "style_encoder": (B, c["cfg"].get("style_dim")),
            "mapping_network": (B, c["cfg"].get("style_dim")), "discriminator": (B,)}[c["kind"]]


def normed_bias_keys(kind, **cfg):
    """Biases with the exact gradient 0.  In the generator that is every conv bias but to_rgb's: a per-channel
    constant added anywhere on the residual stream is removed by the norm at the head of every residual branch,
    rides the shortcuts (1x1 convs without bias, pooling, upsampling: all keep a constant a constant) and is
    removed at last by to_rgb's InstanceNorm.  The other three nets have no norm."""
    if kind != "generator":
        return set()
    n = len(generator_plan(cfg["img_size"], cfg["max_conv_dim"]))
    return {"from_rgb.bias"} | {"%s.%d.%s.bias" % (s, i, c) for s in ("encode", "decode") for i in range(n)
                                for c in ("conv1", "conv2")}


# -------------------------------------------------------------------------------------- networks
def _c(sd, p, x, pad=0):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), padding=pad)


def _l(sd, p, x):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


_TRACE = None  # activation_margin's record of min|z| / max|z| per activation input


def _note(x):
    if _TRACE is not None:
        a = x.detach().abs()
        _TRACE.append(float(a.min() / a.max()))
    return x


def _lrelu(x):
    return F.leaky_relu(_note(x), SLOPE)


def _relu(x):
    return F.relu(_note(x))


def res_blk(sd, p, x, down):
    norm = p + ".norm1.weight" in sd

    def act(h, n):
        if norm:  # the stock operator in every dtype: in fp32 the fixture's own sequence of ATen calls
            h = F.instance_norm(h, weight=sd["%s.%s.weight" % (p, n)], bias=sd["%s.%s.bias" % (p, n)], eps=EPS)
        return _lrelu(h)

    sc = _c(sd, p + ".conv1x1", x) if p + ".conv1x1.weight" in sd else x
    if down:
        sc = F.avg_pool2d(sc, 2)
    h = _c(sd, p + ".conv1", act(x, "norm1"), 1)
    if down:
        h = F.avg_pool2d(h, 2)
    h = _c(sd, p + ".conv2", act(h, "norm2"), 1)
    return (sc + h) / math.sqrt(2)


def adain(sd, p, x, s):
    h = _l(sd, p + ".fc", s)
    gamma, beta = h[:, :x.shape[1], None, None], h[:, x.shape[1]:, None, None]
    return (1 + gamma) * F.instance_norm(x, eps=EPS) + beta


def adain_res_blk(sd, p, x, s, up):
    h = _lrelu(adain(sd, p + ".norm1", x, s))
    if up:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    h = _c(sd, p + ".conv1", h, 1)
    h = _c(sd, p + ".conv2", _lrelu(adain(sd, p + ".norm2", h, s)), 1)
    sc = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if p + ".conv1x1.weight" in sd:
        sc = _c(sd, p + ".conv1x1", sc)
    return (h + sc) / math.sqrt(2)


def generator_forward(sd, x, s, img_size, max_conv_dim, **_):
    plan = generator_plan(img_size, max_conv_dim)
    h = _c(sd, "from_rgb", x, 1)
    for i, (_, _, rs) in enumerate(plan):
        h = res_blk(sd, "encode.%d" % i, h, rs)
    for i, (_, _, rs) in enumerate(reversed(plan)):
        h = adain_res_blk(sd, "decode.%d" % i, h, s, rs)
    h = F.instance_norm(h, weight=sd["to_rgb.0.weight"], bias=sd["to_rgb.0.bias"], eps=EPS)
    return _c(sd, "to_rgb.2", _lrelu(h))


def _pick(out, y):
    return out[torch.arange(len(y)), torch.as_tensor(y, dtype=torch.long)]


def mapping_forward(sd, z, y, num_domains, **_):
    h = z
    for i in (0, 2, 4, 6):
        h = _relu(_l(sd, "shared.%d" % i, h))
    outs = []
    for d in range(num_domains):
        t = h
        for i in (0, 2, 4):
            t = _relu(_l(sd, "unshared.%d.%d" % (d, i), t))
        outs.append(_l(sd, "unshared.%d.6" % d, t))
    return _pick(torch.stack(outs, 1), y)


def _trunk(sd, top, x, img_size, max_conv_dim):
    n = len(trunk_plan(img_size, max_conv_dim))
    h = _c(sd, top + ".0", x, 1)
    for i in range(n):
        h = res_blk(sd, "%s.%d" % (top, i + 1), h, True)
    return _lrelu(_c(sd, "%s.%d" % (top, n + 2), _lrelu(h))), n


def encoder_forward(sd, x, y, img_size, num_domains, max_conv_dim, **_):
    h, _ = _trunk(sd, "shared", x, img_size, max_conv_dim)
    h = h.flatten(1)
    return _pick(torch.stack([_l(sd, "unshared.%d" % d, h) for d in range(num_domains)], 1), y)


def discriminator_forward(sd, x, y, img_size, max_conv_dim, **_):
    h, n = _trunk(sd, "main", x, img_size, max_conv_dim)
    return _pick(_c(sd, "main.%d" % (n + 4), h).flatten(1), y)


FORWARD = {"generator": generator_forward, "mapping_network": mapping_forward, "style_encoder": encoder_forward,
           "discriminator": discriminator_forward}


def forward(kind, cfg, sd, x, cond):
    """cond: the style code s (generator) or the domain labels y (the others)."""
    return FORWARD[kind](sd, x, cond, **cfg)


def activation_margin(kind, cfg, sd, x, cond):
    """The smallest min|z| / max|z| over the inputs z of every LeakyReLU / ReLU of the fp64 forward: how far the
    nearest activation decision is from flipping (the gradients are discontinuous there)."""
    global _TRACE
    _TRACE = []
    try:
        with torch.no_grad():
            t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}
            forward(kind, cfg, t, torch.from_numpy(x).double(),
                    torch.from_numpy(cond).double() if kind == "generator" else cond)
        return min(_TRACE)
    finally:
        _TRACE = None


def run_case(kind, cfg, sd, x, cond, r, dtype):
    """Output, input gradient, style-code gradient (generator; else None) and parameter gradients of sum(out * r)
    in dtype; numpy in, tensors out."""
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    if kind == "generator":
        cond = torch.from_numpy(cond).to(dtype).requires_grad_(True)
    out = forward(kind, cfg, t, xt, cond)
    (out * torch.from_numpy(r).to(dtype)).sum().backward()
    gp = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in t.items()}
    return out.detach(), xt.grad, (cond.grad if kind == "generator" else None), gp


def style_code(seed, B, style_dim):
    return np.random.RandomState(seed).standard_normal((B, style_dim)).astype(np.float32)


# ------------------------------------------------------------------------------------ the kernels
def adain_fwd(x, h, act, slope=SLOPE):
    """x NCHW float64, h [N, 2C] -> (y, z): z = (1 + gamma) * xhat + beta, y = act(z)."""
    C = x.shape[1]
    mean, rstd = R.in_stats(x, EPS)
    z = (1 + h[:, :C, None, None]) * ((x - mean) * rstd) + h[:, C:, None, None]
    return R.act_fwd(z, act, slope), z


def adain_bwd(g, x, h, act, slope=SLOPE):
    """dict: dx, dh [N, 2C], dbias (the per-channel sum of dx), and the sums of the absolute terms behind dh and
    dbias (the scale of their rounding error)."""
    C = x.shape[1]
    mean, rstd = R.in_stats(x, EPS)
    xh = (x - mean) * rstd
    A = 1 + h[:, :C, None, None]
    z = A * xh + h[:, C:, None, None]
    gz = g * R.act_grad(z, act, slope)
    dx = rstd * A * (gz - gz.mean(dim=(2, 3), keepdim=True) - xh * (gz * xh).mean(dim=(2, 3), keepdim=True))
    return dict(dx=dx, dh=torch.cat([(gz * xh).sum(dim=(2, 3)), gz.sum(dim=(2, 3))], 1),
                dh_abs=torch.cat([(gz * xh).abs().sum(dim=(2, 3)), gz.abs().sum(dim=(2, 3))], 1),
                dbias=dx.sum(dim=(0, 2, 3)), dbias_abs=dx.abs().sum(dim=(0, 2, 3)), z=z)


def merge_fwd(a, b, mode, scale):
    """(a + f(b)) * scale on NCHW tensors; mode 'same' | 'pool' | 'up'."""
    fb = b if mode == "same" else (F.avg_pool2d(b, 2) if mode == "pool" else
                                   b.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))
    return (a + fb) * scale


def merge_bwd(g, mode, scale):
    """(ga, gb) of merge_fwd."""
    if mode == "same":
        gb = g
    elif mode == "pool":
        gb = g.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) / 4
    else:
        gb = 4 * F.avg_pool2d(g, 2)
    return g * scale, gb * scale
