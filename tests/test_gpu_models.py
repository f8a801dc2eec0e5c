"""End-to-end GPU parity of the HIP networks and the CycleGANCon train step.

* ResnetGenerator / NLayerDiscriminator forward, input grad and every parameter grad against the
  golden vectors the REFERENCE produced (tests/golden/nets_small.npz, ngf=ndf=8, 64x64, B=2).
* Three CycleGANCon optimize_parameters() steps against the reference's own loss dict
  (tests/golden/step_small.npz, pool_size=0) — tolerance 1e-3 relative (north_star), plus G_A's
  output on a probe image after the three steps.
* Full-size generator (ngf=64, 9 blocks) at 256x256 against the CPU oracle, and batch-invariance
  at B=4 (each frame equals its B=1 result: InstanceNorm is per sample).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


@pytest.mark.parametrize("tag", ["G", "D"])
def test_network_vs_reference_golden(gb, golden, tag, train_math):
    from gbvst import networks
    g = golden("nets_small")
    if tag == "G":
        net = networks.define_G(3, 3, 8, "resnet_9blocks", "instance", False, "normal", 0.02, [0])
    else:
        net = networks.define_D(3, 8, "basic", 3, "instance", "normal", 0.02, [0])
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}_w_")}
    net.load_state_dict(sd)
    net.zero_grad()
    x = torch.from_numpy(g[f"{tag}_x"]).to(DEV).requires_grad_(True)
    y = net(x)
    y.backward(torch.from_numpy(g[f"{tag}_gy"]).to(DEV))
    torch.cuda.synchronize()
    assert _rel(y.detach().cpu(), g[f"{tag}_y"]) < 1e-4
    assert _rel(x.grad.cpu(), g[f"{tag}_dx"]) < 1e-4
    for k, p in net.named_parameters():
        ref = g[f"{tag}_g_{k}"]
        real_bias = {"G": ("model.26.bias",), "D": ("model.0.bias", "model.11.bias")}[tag]
        if k.endswith("bias") and k not in real_bias:
            # biases in front of InstanceNorm: exact gradient is 0, both sides are rounding noise
            assert np.abs(p.grad.cpu().numpy()).max() < 1e-3
            continue
        assert _rel(p.grad.cpu(), ref) < 1e-3, k


def _load_step_model(gb, g, pool=0):
    from gbvst.cycle_gan_model import CycleGANModel
    from gbvst.options import default_opt
    opt = default_opt(True, ngf=8, ndf=8, pool_size=pool, gpu_ids=[0])
    m = CycleGANModel(opt)
    for name in ("G_A", "G_B", "D_A", "D_B"):
        pre = f"w_{name}_"
        getattr(m, "net" + name).load_state_dict(
            {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    data = tuple(torch.from_numpy(g[k]) for k in ("real_A", "real_A2", "real_B"))
    data = data + (None, torch.from_numpy(g["mask"]), torch.from_numpy(g["flow"]))
    return m, data


def _oracle_fp64_losses(g):
    """The same 3 steps in float64 on the CPU oracle: measures how far the reference's own fp32
    rounding lets later steps drift (Adam's first steps are ~lr*sign(g), so near-zero gradients
    flip with any change of summation order)."""
    from oracle import cpu_ref
    m = cpu_ref.RefCycleGANCon(ngf=8, ndf=8)
    for name, net in m.nets().items():
        pre = f"w_{name}_"
        cpu_ref.load_np_state(net, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
        net.double()
    m.opt_G = torch.optim.Adam(list(m.G_A.parameters()) + list(m.G_B.parameters()), lr=2e-4, betas=(0.5, 0.999))
    m.opt_D = torch.optim.Adam(list(m.D_A.parameters()) + list(m.D_B.parameters()), lr=2e-4, betas=(0.5, 0.999))
    m.set_input_fc2(*(torch.from_numpy(g[k]).double() for k in ("real_A", "real_A2", "real_B", "mask", "flow")))
    names = [str(n) for n in g["loss_names"]]
    out = []
    for _ in range(g["losses"].shape[0]):
        m.optimize_parameters()
        cur = m.get_current_losses()
        out.append([cur[n] for n in names])
    with torch.no_grad():
        probe = m.G_A(torch.from_numpy(g["probe"]).double()).float().numpy()
    return np.array(out), probe


def test_train_step_vs_reference_golden(gb, golden, train_math):
    """Step 0: every loss within 1e-3 relative (north_star).  Later steps: the largest relative loss
    deviation must stay within 1e-3 or within 3x the largest relative deviation that an
    exact-arithmetic (fp64) run of the same algorithm shows from the fp32 reference at that step
    (measured: both reach ~4e-3 at step 2, on different loss terms — Adam's early steps are
    ~lr*sign(g), so rounding-level gradient differences flip near-zero updates)."""
    g = golden("step_small")
    m, data = _load_step_model(gb, g)
    names = [str(n) for n in g["loss_names"]]
    ref_all = g["losses"]
    l64, probe64 = _oracle_fp64_losses(g)
    band = (np.abs(l64 - ref_all) / np.abs(ref_all)).max(axis=1)
    for s in range(ref_all.shape[0]):
        m.set_input_fc2(data)
        m.optimize_parameters()
        cur = m.get_current_losses()
        got = np.array([cur[n] for n in names])
        rel = np.abs(got - ref_all[s]) / np.abs(ref_all[s])
        tol = 1e-3 if s == 0 else max(1e-3, 3 * band[s])
        assert rel.max() <= tol, (s, rel, band[s])
    with torch.no_grad():
        out = m.forward_eval(torch.from_numpy(g["probe"])).cpu().numpy()
    # G_A(probe) after 3 Adam steps: same rule (1e-3, or 3x the exact-arithmetic deviation)
    dev64 = np.abs(probe64 - g["probe_out"]).max()
    assert np.abs(out - g["probe_out"]).max() <= max(1e-3, 3 * dev64), (np.abs(out - g["probe_out"]).max(), dev64)


def test_full_size_generator_vs_oracle(gb, infer_math):
    from gbvst import networks
    from oracle import cpu_ref, prng
    ref = cpu_ref.RefResnetGenerator(3, 3, 64, 9)
    sd = prng.init_state_dict(cpu_ref.state_shapes(ref), base_seed=77)
    cpu_ref.load_np_state(ref, sd)
    net = networks.define_G(3, 3, 64, "resnet_9blocks", "instance", False, "normal", 0.02, [0])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = torch.from_numpy(prng.uniform_f32(78, (1, 3, 256, 256), -1, 1))
    with torch.no_grad():
        y_ref = ref(x)
        y = net(x.to(DEV)).cpu()
    assert (y - y_ref).abs().max().item() < 1e-3
    # batch invariance at B=4 (per-sample InstanceNorm): frame 2 of a batch == the frame alone, up
    # to fp32 summation order (the batched call may take another tile / K order: 256-row tiles
    # walk K channel-slice-major), i.e. a few ulps of the tanh output after 24 conv + IN layers
    xb = torch.from_numpy(prng.uniform_f32(79, (4, 3, 256, 256), -1, 1)).to(DEV)
    with torch.no_grad():
        yb = net(xb)
        y2 = net(xb[2:3].contiguous())
    assert (yb[2:3] - y2).abs().max().item() < 3e-5


def test_pool_and_plain_step_run(gb, golden):
    """pool_size=50 path (ImagePool) and the plain CycleGAN step (lambda_T=0) execute and stay finite."""
    import random
    random.seed(0)
    g = golden("step_small")
    m, data = _load_step_model(gb, g, pool=50)
    m.opt.lambda_T = 0.0
    m.temporal = False
    m.loss_names = [n for n in m.loss_names if n != "G_T"]
    for _ in range(2):
        m.set_input_fc2(data)
        m.optimize_parameters()
    assert all(np.isfinite(v) for v in m.get_current_losses().values())


# ------------------------------------------------------------------------------------------------
# Full-size C2 step (ngf=ndf=64, 256x256, B=4): the production kernel instantiations of the
# metric's train step — the batched N=8 / N=12 generator calls (256x128 channel-slice-major bf16x6
# forward tiles, the 128x128 + 64x64-tail bf16x3 padded-frame data gradients, the wide channel-major
# weight gradients) — against the CPU oracle on identical counter-PRNG weights and inputs.
FULL_B, FULL_S = 4, 256
_NET_SEEDS = {"G_A": 301, "G_B": 302, "D_A": 303, "D_B": 304}
# biases that feed an InstanceNorm: their exact gradient is 0 and both sides hold rounding noise
_REAL_BIAS = {"G": ("model.26.bias",), "D": ("model.0.bias", "model.11.bias")}


def _full_weights():
    from oracle import cpu_ref, prng
    shapes = {"G": cpu_ref.state_shapes(cpu_ref.RefResnetGenerator(3, 3, 64, 9)),
              "D": cpu_ref.state_shapes(cpu_ref.RefNLayerDiscriminator(3, 64))}
    return {n: prng.init_state_dict(shapes[n[0]], base_seed=s) for n, s in _NET_SEEDS.items()}


def _full_inputs():
    from oracle import cpu_ref, prng
    a, a2, b, mask, flow = cpu_ref.synthetic_batch(FULL_B, FULL_S, FULL_S, seed=4321)
    probe = torch.from_numpy(prng.uniform_f32(4322, (1, 3, FULL_S, FULL_S), -1, 1))
    return (a, a2, b, mask, flow), probe


def _grab(store):
    def hook(nets):
        for net in nets:
            for k, p in net.named_parameters():
                store.setdefault(id(net), {})[k] = p.grad.detach().double().cpu().clone()
    return hook


def _oracle_full_step(dtype):
    from oracle import cpu_ref
    m = cpu_ref.RefCycleGANCon(ngf=64, ndf=64)
    W = _full_weights()
    for name, net in m.nets().items():
        cpu_ref.load_np_state(net, W[name])
        net.to(dtype)
    m.opt_G = torch.optim.Adam(list(m.G_A.parameters()) + list(m.G_B.parameters()), lr=2e-4, betas=(0.5, 0.999))
    m.opt_D = torch.optim.Adam(list(m.D_A.parameters()) + list(m.D_B.parameters()), lr=2e-4, betas=(0.5, 0.999))
    data, probe = _full_inputs()
    m.set_input_fc2(*(t.to(dtype) for t in data))
    grads = {}
    m.optimize_parameters(_grab(grads), _grab(grads))
    losses = m.get_current_losses()
    with torch.no_grad():
        out = m.G_A(probe.to(dtype)).double()
    named = {n: grads[id(net)] for n, net in m.nets().items()}
    return losses, named, out


@pytest.fixture(scope="module")
def full_oracle(golden):
    """fp32 oracle run (the reference arithmetic) live, plus the fp64-vs-fp32 band of the same
    step from tests/golden/full_step_band.npz (oracle/gen_full_step_band.py; the fp64 step takes
    minutes on a CPU): the spread the reference's own rounding gives each quantity."""
    return _oracle_full_step(torch.float32), golden("full_step_band")


def _norm_rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.timeout(900)
def test_full_size_train_step_vs_oracle(gb, full_oracle, train_math):
    """One CycleGANCon optimize_parameters() at the C2 config: every step-0 loss within 1e-3
    relative (north_star); every parameter gradient of G_A/G_B (G step) and D_A/D_B (D step)
    within max(2e-3, 3x the fp64-vs-fp32 oracle band) norm-wise; G_A(probe) after the Adam update
    within max(1e-3, 3x the fp64-vs-fp32 deviation)."""
    from gbvst import ops
    from gbvst.cycle_gan_model import CycleGANModel
    from gbvst.options import default_opt
    # the batched passes must reach the production instantiations under this policy
    if ops.get_conv_math() in ("mixed", "bf16x6"):
        assert ops.conv_plan_fwd(2 * FULL_B, 64, 64, 256, 256, 3, 3, 1, 1, 1, "fwd")[0] == 7
    (l32, g32, p32), band = full_oracle
    m = CycleGANModel(default_opt(True, pool_size=0, gpu_ids=[0]))
    W = _full_weights()
    for name in _NET_SEEDS:
        getattr(m, "net" + name).load_state_dict({k: torch.from_numpy(v) for k, v in W[name].items()})
    data, probe = _full_inputs()
    m.set_input_fc2((data[0], data[1], data[2], None, data[3], data[4]))
    grads = {}
    m.optimize_parameters(_grab(grads), _grab(grads))
    torch.cuda.synchronize()
    cur = m.get_current_losses()
    for k, ref in l32.items():
        assert abs(cur[k] - ref) <= 1e-3 * abs(ref), (k, cur[k], ref)
    for name in _NET_SEEDS:
        got = grads[id(getattr(m, "net" + name))]
        for k, ref in g32[name].items():
            if k.endswith("bias") and k not in _REAL_BIAS[name[0]]:
                assert got[k].abs().max().item() < 1e-3, (name, k)
                continue
            b = float(band[f"band_{name}_{k}"])
            rel = _norm_rel(got[k], ref)
            assert rel <= max(2e-3, 3 * b), (name, k, rel, b)
    with torch.no_grad():
        out = m.forward_eval(probe).double().cpu()
    dev64 = float(band["probe_dev64"])
    err = (out - p32).abs().max().item()
    assert err <= max(1e-3, 3 * dev64), (err, dev64)


def test_graphed_inference_matches_eager(gb):
    """No-grad forwards replay a captured HIP graph (FlatNet.graphed_forward): bit-identical to the
    eager launches, per input shape, and still after a weight update (packs refreshed in place)."""
    from gbvst import networks
    G = networks.define_G(3, 3, 16, "resnet_9blocks", "instance", False, "normal", 0.02, [0])
    D = networks.define_D(3, 16, "basic", 3, "instance", "normal", 0.02, [0])
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for net, shapes in ((G, [(1, 3, 64, 64), (2, 3, 64, 96)]), (D, [(2, 3, 64, 64)])):
            for shp in shapes:
                x = (torch.rand(*shp, generator=g) * 2 - 1).cuda()
                y = net(x)
                assert torch.equal(y, net._forward_eager(x)), shp
                assert torch.equal(net(x), y)           # replay again
            key = next(iter(net._graphs))
            net.flat_param.mul_(1.01)                  # a weight update
            net.bump_version()
            x = (torch.rand(*shapes[0], generator=g) * 2 - 1).cuda()
            y = net(x)
            assert next(iter(net._graphs)) == key      # same captured graph, refreshed packs
            assert torch.equal(y, net._forward_eager(x))


# ------------------------------------------------------------------------------------------------
# The weight-gradient routes and producer forms of one generator (ops.wgrad_route, networks._wgrad_form)
# under every route switch: ngf=32, 2 blocks at 2x3x128x128 is the smallest generator whose layers take
# all four routes (ngf=16 or a 64x64 input loses the NHWC routes).
_ROUTE_ARMS = {
    "default": (),
    "no_wgrad_nhwc": (("ops", "WGRAD_NHWC"),),
    "no_in_planes": (("networks", "IN_PLANES"),),
    "no_wgrad_nhwc_no_in_planes": (("ops", "WGRAD_NHWC"), ("networks", "IN_PLANES")),
    "no_apre_bwd": (("networks", "APRE_BWD"),),
    "no_dgrad_epi": (("networks", "DGRAD_EPI"),),
    "no_wgrad_nhwc_f32": (("ops", "WGRAD_NHWC_F32"),),
    "no_in_xt": (("networks", "IN_XT"),),
}
# not bit-equal to the default arm by construction: DGRAD_EPI=False replaces the IN-backward reduction taken
# in the data gradient's epilogue by a separate reduction pass; APRE_BWD=False stages the data gradient's dy
# operand from fp32 rather than from pre-split planes
_ROUTE_ARMS_OTHER_BITS = ("no_dgrad_epi", "no_apre_bwd")
_ROUTE_NGF, _ROUTE_NB, _ROUTE_SHAPE = 32, 2, (2, 3, 128, 128)


def _route_net_run(gb, net, x0, gy):
    net.zero_grad()
    x = x0.clone().requires_grad_(True)
    y = net(x)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach().cpu(), x.grad.cpu(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.fixture(scope="module")
def route_case(gb):
    """The network, its inputs, the float64 CPU oracle's (y, dx, parameter gradients) and the default arm's
    parameter gradients, computed once."""
    from gbvst import networks, ops
    from oracle import cpu_ref, prng
    ref = cpu_ref.RefResnetGenerator(3, 3, _ROUTE_NGF, _ROUTE_NB)
    sd = prng.init_state_dict(cpu_ref.state_shapes(ref), base_seed=611)
    cpu_ref.load_np_state(ref, sd)
    ref.double()
    x = torch.from_numpy(prng.uniform_f32(612, _ROUTE_SHAPE, -1, 1))
    gy = torch.from_numpy(prng.uniform_f32(613, _ROUTE_SHAPE, -1, 1))
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr.backward(gy.double())
    oracle = (yr.detach().numpy(), xr.grad.numpy(), {k: p.grad.numpy() for k, p in ref.named_parameters()})
    net = networks.ResnetGenerator(3, 3, ngf=_ROUTE_NGF, norm_layer=networks.get_norm_layer('instance'),
                                   n_blocks=_ROUTE_NB).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    prev = ops.set_conv_math("bf16x6")
    try:
        default = _route_net_run(gb, net, x.to(DEV), gy.to(DEV))[2]
    finally:
        ops.set_conv_math(prev)
    return net, x.to(DEV), gy.to(DEV), oracle, default


@pytest.mark.parametrize("arm", list(_ROUTE_ARMS))
def test_generator_routes_vs_oracle(gb, route_case, arm):
    """Every route switch leaves the generator's forward + backward running, within the network bounds of the
    float64 oracle (1e-4 output and input gradient, 1e-3 parameter gradients, relative to max|ref|), and —
    the routes being bit-identical op by op — every parameter gradient bit-equal to the default arm's."""
    from gbvst import networks, ops
    net, x, gy, (y_ref, dx_ref, g_ref), default = route_case
    mods = {"ops": ops, "networks": networks}
    prev_math = ops.set_conv_math("bf16x6")
    prev = [(m, f, getattr(mods[m], f)) for m, f in _ROUTE_ARMS[arm]]
    try:
        # the guard: with every switch on, these layers take the four routes (a planner change must not
        # silently turn this into a test of one route)
        N, ngf = _ROUTE_SHAPE[0], _ROUTE_NGF
        d0 = (N, 128, 128, ngf, 64, 64, 2 * ngf, 3, 3, 2, 1)      # also the last ConvTranspose's equivalent conv
        d1 = (N, 64, 64, 2 * ngf, 32, 32, 4 * ngf, 3, 3, 2, 1)    # also the first ConvTranspose's
        res = (N, 32, 32, 4 * ngf, 32, 32, 4 * ngf, 3, 3, 1, 1)
        assert ops.wgrad_route(*res, True) == ops.WG_NHWC and ops.dgrad_refl_epi_ok(N, 32, 32, 4 * ngf, 4 * ngf)
        assert networks._rb_wgrad_nhwc(N, 32, 32, 4 * ngf)
        assert ops.wgrad_route(*d1) == ops.WG_NHWC_F32 and ops.wgrad_route(*d0) == ops.WG_IMAGES
        for cx in (4, 8):
            assert ops.wgrad_route(N, 128, 128, cx, 128, 128, ngf, 7, 7, 1, 3) == ops.WG_IMAGES
        assert networks.TAP_LAST and ops.tap_conv_wgrad_swap_ok(torch.empty((N, 128, 128, ngf), device="meta"), 7, 3,
                                                                "reflect", co=3)
        for m, f in _ROUTE_ARMS[arm]:
            setattr(mods[m], f, False)
        y, dx, grads = _route_net_run(gb, net, x, gy)
    finally:
        for m, f, v in prev:
            setattr(mods[m], f, v)
        ops.set_conv_math(prev_math)
    e_y, e_dx = _rel(y, y_ref), _rel(dx, dx_ref)
    print(arm, "rel err: y %.3g dx %.3g" % (e_y, e_dx))
    assert e_y < 1e-4 and e_dx < 1e-4, (e_y, e_dx)
    real_bias = "model.%d.bias" % (17 + _ROUTE_NB)  # the last conv's: every other bias feeds an InstanceNorm
    for k, g in grads.items():
        if k.endswith("bias") and k != real_bias:
            # biases in front of InstanceNorm: exact gradient is 0, both sides are rounding noise
            assert g.abs().max().item() < 1e-3, k
        else:
            e = _rel(g.cpu(), g_ref[k])
            print(arm, k, "rel err %.3g" % e)
            assert e < 1e-3, (k, e)
    if arm not in _ROUTE_ARMS_OTHER_BITS:
        diff = [k for k, g in grads.items() if not torch.equal(g, default[k])]
        assert not diff, (arm, {k: (grads[k] - default[k]).abs().max().item() for k in diff})
