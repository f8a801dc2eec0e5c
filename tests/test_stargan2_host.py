"""CPU-only checks of the StarGAN v2 surface (gbvst.stargan2): the module trees keep the reference's state_dict
keys, shapes and parameter counts (tests/golden/stargan2_small.npz, written by tools/gen_golden_stargan2.py from the
reference's own core/model.py) for the four small cases and the four default-size nets; the CPU reference the GPU
tests use (tests/stargan2_ref.py) reproduces the fixture's outputs and gradients in fp32; what the HIP path does not
carry raises; CheckpointIO writes and reads the reference's ``nets_ema`` file format; the new C entries are declared,
exported and validate their arguments on the host; the new vst:: operators propagate fake-tensor shapes.

Bar of the fixture comparison (test_unet_host.py's): 1e-6 of max|ref| per tensor, fp32 on the CPU.  The biases with
the exact gradient 0 (stargan2_ref.normed_bias_keys) hold rounding noise on both sides; their bar is 1e-6 of the
largest gradient of the case."""
import ctypes
import types

import numpy as np
import pytest
import torch

import reduction_ref as R
import stargan2_ref as S

NEW_SYMBOLS = ["vst_adain_ws_bytes", "vst_adain_fwd", "vst_adain_bwd", "vst_act_fwd", "vst_avgpool2_fwd",
               "vst_avgpool2_bwd", "vst_merge_fwd", "vst_merge_bwd"]
NEW_OPS = ["adain_act", "adain_act_backward", "avg_pool2", "avg_pool2_backward", "merge", "merge_backward"]
EINVAL = 1


def _build(kind, cfg):
    from gbvst import stargan2 as M
    if kind == "generator":
        return M.Generator(cfg["img_size"], cfg["style_dim"], cfg["max_conv_dim"], w_hpf=0)
    return {"mapping_network": M.MappingNetwork, "style_encoder": M.StyleEncoder,
            "discriminator": M.Discriminator}[kind](**cfg)


def _cond(name):
    c = S.CASES[name]
    if c["kind"] == "generator":
        return S.style_code(c["seed"] + 2, c["x"][0], c["cfg"]["style_dim"])
    return c["y"]


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_small_nets_match_reference_layout(golden, name):
    g = golden("stargan2_small")
    c = S.CASES[name]
    shapes = S.shapes(c["kind"], **c["cfg"])
    net = _build(c["kind"], c["cfg"])
    assert list(net.state_dict()) == list(g[name + "_keys"]) == list(shapes)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    assert [k for k, _ in net.named_parameters()] == list(shapes)      # no buffers: every key is a parameter
    assert sum(p.numel() for p in net.parameters()) == int(g[name + "_count"]) == S.param_count(shapes)
    # a reference-layout state loads by name and comes back unchanged
    sd = S.make_state(c["seed"], shapes)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k


@pytest.fixture(scope="module")
def default_sets():
    from gbvst import stargan2 as M
    args = types.SimpleNamespace(img_size=256, style_dim=64, latent_dim=16, num_domains=2, w_hpf=0)
    return M.build_model(args)


@pytest.mark.parametrize("kind", sorted(S.DEFAULTS))
def test_default_nets_match_reference_layout(golden, default_sets, kind):
    g = golden("stargan2_small")
    nets, nets_ema = default_sets
    shapes = S.shapes(kind, **S.DEFAULTS[kind])
    for group in (nets, nets_ema):
        if kind == "discriminator" and group is nets_ema:
            assert set(group) == {"generator", "mapping_network", "style_encoder"}
            continue
        net = getattr(group, kind)
        assert list(net.state_dict()) == list(g["default_%s_keys" % kind])
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
        assert sum(p.numel() for p in net.parameters()) == int(g["default_%s_count" % kind])
    if kind != "discriminator":   # the EMA set holds deep copies: equal values, separate storage
        a, b = getattr(nets, kind), getattr(nets_ema, kind)
        assert a is not b
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q) and p.data_ptr() != q.data_ptr(), k


def test_moving_average_is_the_references_lerp(default_sets):
    from gbvst import stargan2 as M
    a, b = M.MappingNetwork(16, 16, 2), M.MappingNetwork(16, 16, 2)
    want = [torch.lerp(p.data, q.data, 0.999) for p, q in zip(a.parameters(), b.parameters())]
    before = [p.detach().clone() for p in a.parameters()]
    M.moving_average(a, b, beta=0.999)
    for w, q, p, p0 in zip(want, b.parameters(), a.parameters(), before):
        assert torch.equal(q, w) and torch.equal(p, p0)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_stargan2_ref_reproduces_reference_fixture(golden, name):
    g = golden("stargan2_small")
    c = S.CASES[name]
    kind, cfg = c["kind"], c["cfg"]
    shapes = S.shapes(kind, **cfg)
    sd = S.make_state(c["seed"], shapes)
    x, r = S.case_inputs(c["seed"] + 1, c["x"], S.out_shape(name))
    cond = _cond(name)
    # on the reference alone: the case's nearest activation decision keeps the margin its seed was chosen for
    margin = S.activation_margin(kind, cfg, sd, x, cond)
    print(f"{name}: activation margin {margin:.3e} (held to {S.MARGIN[name]:.0e})")
    assert margin >= S.MARGIN[name]
    # fp32 sums depend on how ATen splits a reduction over its threads: run with the fixture's thread count
    threads = torch.get_num_threads()
    torch.set_num_threads(S.FIXTURE_THREADS)
    try:
        out, dx, ds, gp = S.run_case(kind, cfg, sd, x, cond, r, torch.float32)
    finally:
        torch.set_num_threads(threads)

    def err(got, ref):
        return float(np.abs(got.numpy().astype(np.float64) - ref).max())

    assert err(out, g[name + "_out"]) <= 1e-6 * np.abs(g[name + "_out"]).max()
    assert err(dx, g[name + "_dx"]) <= 1e-6 * np.abs(g[name + "_dx"]).max()
    if kind == "generator":
        assert err(ds, g[name + "_ds"]) <= 1e-6 * np.abs(g[name + "_ds"]).max()
    stored = [k[len(name) + 3:] for k in g.files if k.startswith(name + "_g_")]
    assert set(stored) == set(shapes)
    gmax = max(np.abs(g[f"{name}_g_{k}"]).max() for k in stored)
    zero = S.normed_bias_keys(kind, **cfg)
    n_zero = 0
    for k in stored:
        ref = g[f"{name}_g_{k}"]
        got = S.stored(gp[k])
        assert tuple(got.shape) == ref.shape, k
        if not np.any(ref):          # a head of a domain no sample selects: exactly zero on both sides
            assert not bool(got.any()), k
            n_zero += 1
            continue
        assert err(got, ref) <= 1e-6 * (gmax if k in zero else np.abs(ref).max()), k
    if name == "F":                  # domains 0 and 2 of y = [1, 1]: 2 x 4 layers x (weight, bias)
        assert n_zero == 16
    if name == "E":                  # domain 1 of y = [2, 0]
        assert n_zero == 2


def test_kernel_references_vs_autograd():
    """The fp64 references of the AdaIN and merge kernels against float64 autograd of the stock ops."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 8, 5, 4, generator=gen, dtype=torch.float64) * 2 + 0.3).requires_grad_(True)
    h = torch.randn(2, 16, generator=gen, dtype=torch.float64).requires_grad_(True)
    g = torch.randn(2, 8, 5, 4, generator=gen, dtype=torch.float64)
    for act in ("none", "lrelu"):
        z = (1 + h[:, :8, None, None]) * F.instance_norm(x, eps=S.EPS) + h[:, 8:, None, None]
        y = F.leaky_relu(z, 0.2) if act == "lrelu" else z
        yr, _ = S.adain_fwd(x.detach(), h.detach(), act, 0.2)
        assert (yr - y).abs().max() <= 1e-10 * y.abs().max()
        dx, dh = torch.autograd.grad((y * g).sum(), (x, h))
        b = S.adain_bwd(g, x.detach(), h.detach(), act, 0.2)
        assert (b["dx"] - dx).abs().max() <= 1e-10 * dx.abs().max()
        assert (b["dh"] - dh).abs().max() <= 1e-10 * dh.abs().max()
        assert (b["dbias"] - dx.sum(dim=(0, 2, 3))).abs().max() <= 1e-10 * dx.abs().sum()
    a = torch.randn(2, 8, 6, 4, generator=gen, dtype=torch.float64).requires_grad_(True)
    for mode, bs in (("same", (2, 8, 6, 4)), ("pool", (2, 8, 12, 8)), ("up", (2, 8, 3, 2))):
        b = torch.randn(bs, generator=gen, dtype=torch.float64).requires_grad_(True)
        fb = b if mode == "same" else (F.avg_pool2d(b, 2) if mode == "pool" else F.interpolate(b, scale_factor=2))
        out = (a + fb) * 0.7
        assert (S.merge_fwd(a.detach(), b.detach(), mode, 0.7) - out).abs().max() <= 1e-12
        go = torch.randn(out.shape, generator=gen, dtype=torch.float64)
        ga, gb = torch.autograd.grad((out * go).sum(), (a, b))
        ra, rb = S.merge_bwd(go, mode, 0.7)
        assert (ra - ga).abs().max() <= 1e-12 and (rb - gb).abs().max() <= 1e-12


def test_unsupported_configs_and_cpu_tensors_raise():
    from gbvst import ops, stargan2 as M
    with pytest.raises(NotImplementedError):
        M.Generator(256, 16, 8, w_hpf=1)
    with pytest.raises(NotImplementedError):
        M.AdainResBlk(8, 8, 16, w_hpf=1)
    with pytest.raises(NotImplementedError):
        M.build_model(types.SimpleNamespace(img_size=256, style_dim=64, latent_dim=16, num_domains=2, w_hpf=1))
    with pytest.raises(NotImplementedError):
        M.ResBlk(6, 8)                                                   # channels % 4 != 0
    G = M.Generator(256, 16, 8, w_hpf=0)
    x, s = torch.zeros(1, 3, 32, 32), torch.zeros(1, 16)
    with pytest.raises(NotImplementedError):
        G(x, s, masks=[x, x])
    with pytest.raises(RuntimeError):                                    # no CPU fallback
        G(x, s)
    with pytest.raises(ValueError):
        G(torch.zeros(1, 3, 24, 32), s)                                  # not a multiple of 2^4
    with pytest.raises(ValueError):
        G.forward_nhwc(torch.zeros(1, 32, 32, 4), torch.zeros(1, 8))     # style_dim
    E, D, Fm = M.StyleEncoder(64, 16, 3, 8), M.Discriminator(64, 3, 8), M.MappingNetwork(16, 16, 3)
    y = torch.tensor([1])
    for net in (E, D):
        with pytest.raises(ValueError):                                  # these two need img_size inputs
            net(torch.zeros(1, 3, 32, 32), y)
        with pytest.raises(RuntimeError):
            net(torch.zeros(1, 3, 64, 64), y)
    with pytest.raises(RuntimeError):
        Fm(torch.zeros(1, 16), y)
    with pytest.raises(ValueError):
        Fm(torch.zeros(1, 12), y)
    sg = M.StyleGuided(types.SimpleNamespace(generator=G), torch.zeros(1, 16))
    with pytest.raises(RuntimeError):
        sg.forward_eval(x)
    t = torch.zeros(2, 4, 4, 8)
    for call in (lambda: ops.adain_fwd(t, torch.zeros(2, 8, 2), torch.zeros(2, 16)),
                 lambda: ops.adain_bwd(t, t, torch.zeros(2, 8, 2), torch.zeros(2, 16)),
                 lambda: ops.avgpool2(t), lambda: ops.avgpool2_bwd(t), lambda: ops.act_fwd(t, "lrelu", 0.2),
                 lambda: ops.merge(t, t, "same"), lambda: ops.merge_bwd(t, "up")):
        with pytest.raises(RuntimeError):
            call()


def test_checkpoint_io_writes_the_reference_format(golden, tmp_path):
    """'{:06d}_nets_ema.ckpt' holds {name: state_dict} with the reference's names and keys, and loads back."""
    from gbvst import stargan2 as M
    g = golden("stargan2_small")
    nets = {"generator": ("G", _build("generator", S.CASES["G"]["cfg"])),
            "mapping_network": ("F", _build("mapping_network", S.CASES["F"]["cfg"])),
            "style_encoder": ("E", _build("style_encoder", S.CASES["E"]["cfg"]))}
    tmpl = str(tmp_path / "ck" / "{:06d}_nets_ema.ckpt")
    io = M.CheckpointIO(tmpl, **{k: v[1] for k, v in nets.items()})
    fname = io.save(100000)
    assert fname.endswith("100000_nets_ema.ckpt")
    raw = torch.load(fname, map_location="cpu", weights_only=True)
    assert list(raw) == ["generator", "mapping_network", "style_encoder"]
    for name, (case, net) in nets.items():
        assert list(raw[name]) == list(g[case + "_keys"])
    # a file of plain CPU tensors in the reference layout (what the reference's own CheckpointIO saves) loads
    states = {name: {k: torch.from_numpy(v) for k, v in
                     S.make_state(7 + i, S.shapes(S.CASES[case]["kind"], **S.CASES[case]["cfg"])).items()}
              for i, (name, (case, _)) in enumerate(nets.items())}
    torch.save(states, tmpl.format(7))
    io.load(7)
    for name, (_, net) in nets.items():
        for k, v in net.state_dict().items():
            assert torch.equal(v, states[name][k]), (name, k)
    with pytest.raises(AssertionError):
        io.load(8)


def test_abi_table_exports_and_host_validation():
    import gbvst
    from gbvst import _lib, ops
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name in ("adain_fwd", "adain_bwd", "avgpool2", "avgpool2_bwd", "merge", "merge_bwd", "act_fwd"):
        assert callable(getattr(ops, name))
    raw = ctypes.CDLL(gbvst._lib.build())
    header = open(gbvst._lib.REPO + "/include/vst_hip.h").read()
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert s + "(" in header, s
    lib = gbvst._lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def afwd(x=p, stats=p, h=p, y=p, ws=p, N=1, HW=16, C=8, act=2):
        return lib.vst_adain_fwd(x, stats, h, y, ws, N, HW, C, act, 0.2, None)

    def abwd(gy=p, x=p, stats=p, h=p, dx=p, ws=p, N=1, HW=16, C=8, act=2):
        return lib.vst_adain_bwd(gy, x, stats, h, dx, p, p, ws, N, HW, C, act, 0.2, 0, None)

    def mfwd(a=p, b=p, out=p, N=1, H=2, W=2, C=8, mode=0):
        return lib.vst_merge_fwd(a, b, out, N, H, W, C, mode, 0.5, None)

    def mbwd(g=p, ga=p, gb=p, N=1, H=2, W=2, C=8, mode=0):
        return lib.vst_merge_bwd(g, ga, gb, N, H, W, C, mode, 0.5, None)

    def pfwd(x=p, y=p, N=1, H=2, W=2, C=8):
        return lib.vst_avgpool2_fwd(x, y, N, H, W, C, None)

    def pbwd(x=p, y=p, N=1, H=2, W=2, C=8):
        return lib.vst_avgpool2_bwd(x, y, N, H, W, C, None)

    # bad arguments are refused before any launch, with non-NULL host pointers (host memory is never touched)
    for call, required in ((afwd, ("x", "stats", "h", "y", "ws")), (abwd, ("gy", "x", "stats", "h", "dx", "ws")),
                           (mfwd, ("a", "b", "out")), (mbwd, ("g", "ga", "gb")), (pfwd, ("x", "y")),
                           (pbwd, ("x", "y"))):
        for name in required:
            assert call(**{name: None}) == EINVAL, (call.__name__, name)
        for kw in (dict(N=0), dict(C=0), dict(C=6)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
    for call in (afwd, abwd):
        for kw in (dict(HW=0), dict(C=1028), dict(act=1), dict(act=3)):     # relu / tanh are not AdaIN's
            assert call(**kw) == EINVAL, (call.__name__, kw)
        assert b"adain" in lib.vst_last_error()
    for call in (mfwd, mbwd):
        for kw in (dict(mode=3), dict(mode=-1), dict(H=0)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
        assert b"merge" in lib.vst_last_error()
    assert lib.vst_act_fwd(p, p, 6, 2, 0.2, None) == EINVAL and lib.vst_act_fwd(None, p, 8, 2, 0.2, None) == EINVAL


@pytest.mark.parametrize("case", R.IN_CASES + [("gen_widest", (2, 16, 16, 512), None, {})], ids=lambda c: c[0])
def test_adain_ws_bytes_agrees_with_geom(case):
    import gbvst
    gbvst._lib.build()
    lib = gbvst._lib.load()
    _, (N, H, W, C), nsplit, _ = case
    g = R.geom(N, H * W, C)
    assert nsplit is None or g["nsplit"] == nsplit
    # N * nsplit * C * {3 doubles} + N * C * {2 float2 tables + 3 doubles} + 256
    assert lib.vst_adain_ws_bytes(N, H * W, C) == N * g["nsplit"] * C * 24 + N * C * 40 + 256
    assert lib.vst_adain_ws_bytes(N, H * W, C) == lib.vst_cond_instnorm_ws_bytes(N, H * W, C)
    for bad in ((N, H * W, C + 2), (N, H * W, 1028), (0, H * W, C), (N, 0, C)):
        assert lib.vst_adain_ws_bytes(*bad) == 0, bad


def test_library_ops_fake_shapes_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gbvst import library  # noqa: F401
    for name in NEW_OPS:
        assert name in library.OPS
        assert getattr(torch.ops.vst, name).default._schema.name == "vst::" + name
    with FakeTensorMode():
        x, h = torch.empty(2, 16, 8, 10), torch.empty(2, 32)
        assert torch.ops.vst.adain_act(x, h, "lrelu", 0.2).shape == x.shape
        dx, dh = torch.ops.vst.adain_act_backward(x, x, h, "none", 0.2)
        assert dx.shape == x.shape and dh.shape == h.shape
        assert torch.ops.vst.avg_pool2(x).shape == (2, 16, 4, 5)
        assert torch.ops.vst.avg_pool2_backward(x).shape == (2, 16, 16, 20)
        hi, lo = torch.empty(2, 16, 16, 20), torch.empty(2, 16, 4, 5)
        for mode, b in (("same", x), ("pool", hi), ("up", lo)):
            assert torch.ops.vst.merge(x, b, mode, 0.5).shape == x.shape
            ga, gb = torch.ops.vst.merge_backward(x, mode, 0.5)
            assert ga.shape == x.shape and gb.shape == b.shape
    x, h = torch.zeros(2, 16, 8, 10), torch.zeros(2, 32)
    for call in (lambda: torch.ops.vst.adain_act(x, h, "lrelu", 0.2),
                 lambda: torch.ops.vst.adain_act_backward(x, x, h, "lrelu", 0.2),
                 lambda: torch.ops.vst.avg_pool2(x), lambda: torch.ops.vst.avg_pool2_backward(x),
                 lambda: torch.ops.vst.merge(x, x, "same", 0.5), lambda: torch.ops.vst.merge_backward(x, "same", 0.5)):
        with pytest.raises(RuntimeError):
            call()
