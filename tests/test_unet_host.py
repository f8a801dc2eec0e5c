"""CPU-only checks of the U-Net generator surface: the CPU reference the GPU tests use (tests/unet_ref.py)
reproduces the fixture the reference's own UnetGenerator produced (tests/golden/unet_small.npz, written by
tools/gen_golden_unet.py); gbvst.networks.UnetGenerator keeps the reference's module tree, key for key; define_G
builds unet_128 and refuses what the HIP path does not carry; the vst_instnorm_skip_* entries are
declared, exported, validate their arguments on the host and size their workspace from red_geom's geometry.

Bar of the fixture comparison: 1e-6 of max|ref| per tensor, fp32 on the CPU.  The biases in front of an
InstanceNorm have the exact gradient 0; both sides hold rounding noise there, and the bar for them is 1e-6 of the
largest gradient of the case."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import reduction_ref as R
import unet_ref as U

CASES = U.CASES
NEW_SYMBOLS = ["vst_instnorm_skip_ws_bytes", "vst_instnorm_skip_fwd", "vst_instnorm_skip_bwd"]
NEW_OPS = ["instance_norm_skip", "instance_norm_skip_backward"]
EINVAL, EUNSUPPORTED = 1, 2
INST = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_unet_ref_reproduces_reference_fixture(golden, case):
    g = golden("unet_small")
    D, seed = CASES[case]
    shapes = U.unet_shapes(3, 3, D, 4)
    assert list(g[case + "_keys"]) == list(shapes)
    # fp32 sums depend on how ATen splits a reduction over its threads (the weight gradients at one thread land
    # 1.1e-6 from the same machine's 8-thread result): run with the thread count the fixture was generated with
    threads = torch.get_num_threads()
    torch.set_num_threads(U.FIXTURE_THREADS)
    try:
        out, dx, gp = U.run_case(U.make_state(seed, shapes), g[case + "_x"], g[case + "_r"], D, torch.float32)
    finally:
        torch.set_num_threads(threads)

    def err(got, ref):
        return float(np.abs(got.numpy().astype(np.float64) - ref).max())

    assert err(out, g[case + "_out"]) <= 1e-6 * np.abs(g[case + "_out"]).max()
    assert err(dx, g[case + "_dx"]) <= 1e-6 * np.abs(g[case + "_dx"]).max()
    stored = [k[len(case) + 3:] for k in g.files if k.startswith(case + "_g_")]
    assert (set(stored) == set(shapes)) if case == "a" else {k for k in shapes if k.endswith(".bias")} < set(stored)
    gmax = max(np.abs(g[f"{case}_g_{k}"]).max() for k in stored)
    zero = U.normed_bias_keys(D)
    for k in stored:
        ref = g[f"{case}_g_{k}"]
        assert err(gp[k], ref) <= 1e-6 * (gmax if k in zero else np.abs(ref).max()), k


def test_unet_ref_skip_kernels_vs_autograd():
    """The fp64 references of the two kernels against float64 autograd of the stock ops."""
    gen = torch.Generator().manual_seed(3)
    y = (torch.randn(2, 8, 5, 3, generator=gen, dtype=torch.float64) * 2 + 0.3).requires_grad_(True)
    g_d, g_s = (torch.randn(2, 8, 5, 3, generator=gen, dtype=torch.float64) for _ in range(2))
    for use_stats in (True, False):
        z = torch.nn.functional.instance_norm(y, eps=U.EPS) if use_stats else y
        d, s = torch.nn.functional.leaky_relu(z, 0.2), torch.relu(z)
        dr, sr, _ = U.skip_fwd(y.detach(), use_stats)
        assert (dr - d).abs().max() <= 1e-10 * d.abs().max() and (sr - s).abs().max() <= 1e-10 * s.abs().max()
        for gd in (g_d, None):
            (dy,) = torch.autograd.grad((s * g_s).sum() + (0 if gd is None else (d * gd).sum()), y, retain_graph=True)
            got, db = U.skip_bwd(gd, g_s, y.detach(), use_stats)
            assert (got - dy).abs().max() <= 1e-10 * dy.abs().max()
            assert (db - dy.sum(dim=(0, 2, 3))).abs().max() <= 1e-10 * dy.abs().sum()


@pytest.mark.parametrize("case", sorted(CASES))
def test_unetgenerator_matches_reference_layout(golden, case):
    from gbvst import networks
    g = golden("unet_small")
    D, seed = CASES[case]
    net = networks.UnetGenerator(3, 3, D, 4, norm_layer=INST)
    shapes = U.unet_shapes(3, 3, D, 4)
    assert list(net.state_dict()) == list(g[case + "_keys"])
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    assert "model.model.0.weight" in shapes and "model.model.1.model.1.weight" in shapes
    # parameters are views of the flat buffers (FlatNet), in the reference's parameter order
    assert net.flat_param.numel() == sum(int(np.prod(s)) for s in shapes.values())
    assert [k for k, _ in net.named_parameters()] == list(shapes)
    # a reference checkpoint loads by name and comes back unchanged
    sd = U.make_state(seed, shapes)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    # the backward's layer order (outermost up conv first ... outermost down conv last) is the reverse of the
    # parameter order: flat offsets fall along it and end at 0
    base = net.flat_param.data_ptr()
    lv = net._levels()
    order = [up for _, up in lv] + [dn for dn, _ in reversed(lv)]
    offs = [(m.weight.data_ptr() - base) // 4 for m in order]
    assert offs == sorted(offs, reverse=True) and offs[-1] == 0


def test_define_g_builds_unets_and_refuses_the_rest():
    from gbvst import networks
    net = networks.define_G(3, 3, 8, "unet_128", norm="instance", use_dropout=False)
    assert type(net) is networks.UnetGenerator and net.num_downs == 7 and net.ngf == 8 and len(net._levels()) == 7
    # the eight-level net is built from the class (define_G keeps refusing the name 'unet_256', as
    # test_cpu_host.test_unsupported_configs_raise holds it to)
    net = networks.init_net(networks.UnetGenerator(3, 3, 8, 8, norm_layer=INST))
    assert net.num_downs == 8 and len(net._levels()) == 8
    with pytest.raises(NotImplementedError):
        networks.define_G(3, 3, 8, "unet_256", norm="instance")
    # unet_256 at ngf 64: the reference's 54.4 M parameters
    shapes = U.unet_shapes(3, 3, 8, 64)
    assert sum(int(np.prod(s)) for s in shapes.values()) == 54409603
    for kw in (dict(norm="batch"), dict(norm="none"), dict(norm="instance", use_dropout=True)):
        with pytest.raises(NotImplementedError):
            networks.define_G(3, 3, 8, "unet_128", **kw)
    with pytest.raises(NotImplementedError):
        networks.define_G(3, 3, 6, "unet_128", norm="instance")     # ngf % 4 != 0
    with pytest.raises(NotImplementedError):
        networks.define_D(3, 8, "pixel", norm="instance")           # stays out of scope
    net = networks.define_G(3, 3, 4, "unet_128", norm="instance")
    for shape in ((1, 3, 128, 192), (1, 3, 64, 128)):               # not multiples of 2 ** 7
        with pytest.raises(ValueError):
            net(torch.zeros(shape))
    with pytest.raises(ValueError):
        net.forward_nhwc(torch.zeros(1, 64, 128, 4))
    with pytest.raises(RuntimeError):                               # no CPU fallback
        net(torch.zeros(1, 3, 128, 128))


def test_abi_table_exports_and_host_validation():
    import gbvst
    from gbvst import _lib, ops
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name in ("instnorm_skip_fwd", "instnorm_skip_bwd", "convT4s2_fwd"):
        assert callable(getattr(ops, name))
    raw = ctypes.CDLL(gbvst._lib.build())
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
    header = open(gbvst._lib.REPO + "/include/vst_hip.h").read()
    for s in NEW_SYMBOLS:
        assert s + "(" in header, s
    lib = gbvst._lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(y=p, stats=p, d=p, cat=p, N=1, HW=16, C=8, Cs=16, c0=8, slope=0.2):
        return lib.vst_instnorm_skip_fwd(y, stats, d, cat, N, HW, C, Cs, c0, slope, None)

    def bwd(g_d=p, g_cat=p, Cs=16, c0=8, y=p, stats=p, dy=p, db=p, ws=p, N=1, HW=16, C=8):
        return lib.vst_instnorm_skip_bwd(g_d, g_cat, Cs, c0, y, stats, dy, db, 1, ws, N, HW, C, 0.2, None)

    # bad arguments are refused before any launch, with non-NULL host pointers (host memory is never touched)
    for call, required in ((fwd, ("y", "cat")), (bwd, ("g_cat", "y", "dy", "ws"))):
        for name in required:
            assert call(**{name: None}) == EINVAL, (call.__name__, name)
            assert b"instnorm_skip" in lib.vst_last_error()
        for kw in (dict(N=0), dict(HW=0), dict(HW=-3), dict(C=0), dict(Cs=0), dict(c0=-4)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
        for kw in (dict(C=6, Cs=16, c0=0), dict(c0=2), dict(c0=12), dict(Cs=12, c0=8), dict(Cs=18, c0=8),
                   dict(C=1028, Cs=2056, c0=0)):
            assert call(**kw) == EUNSUPPORTED, (call.__name__, kw)
            assert b"instnorm_skip" in lib.vst_last_error()
    assert bwd(ws=None, stats=None) == EINVAL       # a bias gradient alone still needs the workspace


@pytest.mark.parametrize("case", R.IN_CASES + [("map_1x2", (1, 1, 2, 32), 1, {})], ids=lambda c: c[0])
def test_skip_ws_bytes_agrees_with_geom(case):
    import gbvst
    gbvst._lib.build()
    lib = gbvst._lib.load()
    _, (N, H, W, C), nsplit, _ = case
    g = R.geom(N, H * W, C)
    assert g["nsplit"] == nsplit
    # N * nsplit * C * {3 doubles} + N * C * {float2 + double} + 256
    assert lib.vst_instnorm_skip_ws_bytes(N, H * W, C) == N * g["nsplit"] * C * 24 + N * C * 16 + 256
    assert lib.vst_instnorm_skip_ws_bytes(N, H * W, C) == lib.vst_instnorm_ws_bytes(N, H * W, C)
    for bad in ((N, H * W, C + 2), (N, H * W, 1028), (0, H * W, C), (N, 0, C)):
        assert lib.vst_instnorm_skip_ws_bytes(*bad) == 0, bad


def test_library_ops_fake_shapes_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gbvst import library, ops
    for name in NEW_OPS:
        assert name in library.OPS
        assert getattr(torch.ops.vst, name).default._schema.name == "vst::" + name
    with FakeTensorMode():
        y = torch.empty(2, 16, 8, 10)
        d, s = torch.ops.vst.instance_norm_skip(y, True, 0.2)
        assert d.shape == y.shape and s.shape == y.shape
        assert torch.ops.vst.instance_norm_skip_backward(y, y, y, False, 0.2).shape == y.shape
    y = torch.zeros(2, 16, 8, 10)
    with pytest.raises(RuntimeError):
        torch.ops.vst.instance_norm_skip(y, True, 0.2)
    with pytest.raises(RuntimeError):
        torch.ops.vst.instance_norm_skip_backward(y, y, y, True, 0.2)
    yn, cat = torch.zeros(2, 8, 10, 16), torch.zeros(2, 8, 10, 32)
    with pytest.raises(RuntimeError):
        ops.instnorm_skip_fwd(yn, None, cat, 0)
    with pytest.raises(RuntimeError):
        ops.instnorm_skip_bwd(yn, cat, 16, yn, None)
