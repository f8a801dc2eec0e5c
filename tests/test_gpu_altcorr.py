"""GPU parity of RAFT's alternate_corr path: raft_corr.AlternateCorrBlock (csrc/altcorr.hip: fmap2 pyramid +
on-the-fly window dot products) against the fp64 run of the pinned oracle oracle.style_ref.RefCorrBlock, the
reference-written fixture tests/golden/corr_small.npz, and RAFT / MoGAN end to end.

err(x) = max|x - ref| / max|ref|.  Bounds are 4x the fp32 reference's own error against fp64, computed in the
test: the kernel and the fp32 reference are both fp32 sums of D products, in different orders.  Figures seen
(MI355X): fixture 1.27e-6 vs bound 5.03e-6 (the fp64 oracle is 1.26e-6 from the fixture, which is fp32 itself);
odd sizes / batch 2 1.71e-7 vs bound 1.30e-5 (fp32 reference 3.24e-6); levels 2, radius 3, D 20 1.10e-7 vs
bound 2.69e-6 (fp32 reference 6.72e-7); borders 1.33e-7 vs bound 4.0e-6 (fp32 reference 1.01e-6)."""
import argparse

import numpy as np
import pytest
import torch

from oracle import prng, raft_ref
from oracle.style_ref import RefCorrBlock

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gb():
    import gbvst
    gbvst._lib.load()
    return gbvst


def _rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def _g(seed, shape, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([xs, ys], 0).float()[None].repeat(B, 1, 1, 1)


def _refs(f1, f2, coords, L, r):
    """(fp64 oracle output, err of the fp32 oracle against it)."""
    r64 = RefCorrBlock(f1.double(), f2.double(), L, r)(coords.double())
    r32 = RefCorrBlock(f1, f2, L, r)(coords)
    return r64, _rel(r32, r64)


def _shares(r64, L, r):
    KK = (2 * r + 1) ** 2
    return [float((r64[:, l * KK:(l + 1) * KK] != 0).double().mean()) for l in range(L)]


_CACHE = {}


def _odd_case():
    """2x256x36x44 (levels 36x44, 18x22, 9x11, 4x5), computed once and never modified."""
    if "odd" not in _CACHE:
        f1, f2 = _g(51, (2, 256, 36, 44)), _g(52, (2, 256, 36, 44))
        coords = _grid(2, 36, 44) + _g(53, (2, 2, 36, 44), 3.0)
        _CACHE["odd"] = (f1, f2, coords) + _refs(f1, f2, coords, 4, 4)
    return _CACHE["odd"]


def _alt(f1, f2, L, r):
    from gbvst import raft_corr
    AlternateCorrBlock = raft_corr.AlternateCorrBlock
    return AlternateCorrBlock(f1.to(DEV), f2.to(DEV), L, r)


def test_reference_fixture(gb, golden):
    """corr_small.npz["lookup"] was written by the reference's CorrBlock in fp32; the fp64 oracle is 1.26e-6
    from it, so the bound is about 5e-6."""
    g = golden("corr_small")
    f1, f2, coords = (torch.from_numpy(g[k]) for k in ("f1", "f2", "coords"))
    r64 = RefCorrBlock(f1.double(), f2.double(), 4, 4)(coords.double())
    bound = 4 * _rel(r64, g["lookup"])
    got = _alt(f1, f2, 4, 4)(coords.to(DEV))
    e = _rel(got, g["lookup"])
    print("fixture: err %.3g bound %.3g" % (e, bound))
    assert got.shape == (1, 324, 16, 24)
    assert e <= bound


def test_fp64_oracle_odd_sizes_batch2(gb):
    f1, f2, coords, r64, e32 = _odd_case()
    sh = _shares(r64, 4, 4)
    got = _alt(f1, f2, 4, 4)(coords.to(DEV))
    e = _rel(got, r64)
    print("odd: err %.3g fp32-ref err %.3g shares %s" % (e, e32, sh))
    assert min(sh) >= 0.25, sh  # out-of-range zeros cannot carry the test
    assert e <= 4 * e32
    # per level and per batch item too: a wrong level or batch offset cannot hide behind max|ref|
    for b in range(2):
        for l in range(4):
            assert _rel(got[b:b + 1, l * 81:(l + 1) * 81], r64[b:b + 1, l * 81:(l + 1) * 81]) <= 4 * e32, (b, l)


def test_levels2_radius3_channel_tail(gb):
    f1, f2 = _g(51, (1, 20, 16, 16)), _g(52, (1, 20, 16, 16))
    coords = _grid(1, 16, 16) + _g(53, (1, 2, 16, 16), 2.0)
    r64, e32 = _refs(f1, f2, coords, 2, 3)
    sh = _shares(r64, 2, 3)
    blk = _alt(f1, f2, 2, 3)
    got = blk(coords.to(DEV))
    e = _rel(got, r64)
    print("l2r3: err %.3g fp32-ref err %.3g shares %s" % (e, e32, sh))
    assert got.shape == (1, 98, 16, 16)
    assert min(sh) >= 0.25, sh
    assert e <= 4 * e32
    a = blk.lookup_nhwc(coords.to(DEV))
    b = blk.lookup_nhwc(coords.to(DEV), cs=104)
    assert a.shape == (1, 16, 16, 100) and b.shape == (1, 16, 16, 104)
    assert bool((b[..., 98:] == 0).all()) and bool((a[..., 98:] == 0).all())
    assert torch.equal(a[..., :98], b[..., :98])


def test_borders(gb):
    f1, f2, _, _, _ = _odd_case()
    B, H, W, r = 2, 36, 44, 4
    vx = torch.tensor([-7.5, -0.25, 0.0, 0.5, W - 1.0, W - 0.75, W + 6.0])
    vy = torch.tensor([-7.5, -0.25, 0.0, 0.5, H - 1.0, H - 0.75, H + 6.0])
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ix, iy = ww % 7, (hh + ww // 7) % 7
    coords = torch.stack([vx[ix], vy[iy]], 0)[None].repeat(B, 1, 1, 1).contiguous()
    r64, e32 = _refs(f1, f2, coords, 4, 4)
    got = _alt(f1, f2, 4, 4)(coords.to(DEV)).cpu()
    e = _rel(got, r64)
    print("borders: err %.3g fp32-ref err %.3g" % (e, e32))
    assert e <= 4 * e32
    zero = r64 == 0
    assert bool(zero.any()) and bool((got[zero] == 0).all())
    # integer coordinates: the level-0 window is the plain dot products (zero outside the map)
    K = 2 * r + 1
    f1d, f2d = f1.double(), f2.double()
    scale = float(np.abs(r64.numpy()).max())
    n = 0
    for h in range(H):
        for w in range(W):
            x, y = float(coords[0, 0, h, w]), float(coords[0, 1, h, w])
            if x != int(x) or y != int(y):
                continue
            n += 1
            want = torch.zeros(B, K, K, dtype=torch.float64)
            for a in range(K):
                for c in range(K):
                    xx, yy = int(x) + a - r, int(y) + c - r
                    if 0 <= xx < W and 0 <= yy < H:
                        want[:, a, c] = (f1d[:, :, h, w] * f2d[:, :, yy, xx]).sum(1) / 16.0
            d = (got[:, :K * K, h, w].double() - want.reshape(B, K * K)).abs().max()
            assert float(d) <= 4 * e32 * scale, (h, w, float(d))
    assert n >= 16


def test_deterministic_and_graph_capturable(gb):
    from gbvst import ops
    from gbvst import raft_corr
    AlternateCorrBlock = raft_corr.AlternateCorrBlock
    f1, f2, coords, _, _ = _odd_case()
    blk = _alt(f1, f2, 4, 4)
    c = coords.to(DEV)
    a, b = blk.lookup_nhwc(c, cs=328), blk.lookup_nhwc(c, cs=328)
    assert torch.equal(a, b)
    # pyramid build + lookup captured once, replayed on new inputs
    s1 = ops.nchw_to_nhwc(f1.to(DEV))
    s2 = ops.nchw_to_nhwc(f2.to(DEV))
    sc = c.clone()

    def run():
        return AlternateCorrBlock.from_nhwc(s1, s2, 256, 4, 4).lookup_nhwc(sc, cs=328)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    g.replay()
    assert torch.equal(out, a)
    n1, n2 = _g(61, (2, 256, 36, 44)), _g(62, (2, 256, 36, 44))
    nc = _grid(2, 36, 44) + _g(63, (2, 2, 36, 44), 5.0)
    s1.copy_(ops.nchw_to_nhwc(n1.to(DEV)))
    s2.copy_(ops.nchw_to_nhwc(n2.to(DEV)))
    sc.copy_(nc.to(DEV))
    g.replay()
    eager = _alt(n1, n2, 4, 4).lookup_nhwc(nc.to(DEV), cs=328)
    assert torch.equal(out, eager)
    assert not torch.equal(out, a)


def test_memory_no_volume(gb):
    """1x256x64x96: the volume path's pyramid is 201 MB; this path owns the 2 MB fmap2 pyramid and the 8 MB
    output.  Peak growth must stay under 1/8 of the volume pyramid."""
    from gbvst import ops
    from gbvst import raft_corr
    AlternateCorrBlock = raft_corr.AlternateCorrBlock
    f1 = ops.nchw_to_nhwc(_g(71, (1, 256, 64, 96)).to(DEV))
    f2 = ops.nchw_to_nhwc(_g(72, (1, 256, 64, 96)).to(DEV))
    coords = (_grid(1, 64, 96) + _g(73, (1, 2, 64, 96), 3.0)).to(DEV).contiguous()
    volume_bytes = 4 * ops.corr_pyramid_floats(6144, 64, 96, 6144, 4)
    assert volume_bytes > 200e6
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    blk = AlternateCorrBlock.from_nhwc(f1, f2, 256, 4, 4)
    out = blk.lookup_nhwc(coords, cs=328)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print("memory: grew %d bytes, limit %d" % (grew, volume_bytes // 8))
    assert out.shape == (1, 64, 96, 328)
    assert blk.f1.data_ptr() == f1.data_ptr() and blk.f2.data_ptr() == f2.data_ptr()
    assert grew <= volume_bytes // 8


def _raft(alternate, base=1300, wscale=None):
    from gbvst import raft
    m = raft.RAFT(argparse.Namespace(small=False, alternate_corr=alternate))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = raft_ref.raft_weights(shapes, base) if wscale is None else raft_ref.raft_weights(shapes, base, wscale)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def test_raft_end_to_end(gb, golden, monkeypatch):
    from gbvst import raft
    built = []  # which correlation block each forward built: the flag must select the path
    for cls in (raft.AlternateCorrBlock, raft.CorrBlock):  # the classes raft.forward itself names
        def counted(c, *a, _real=cls.from_nhwc.__func__, **k):
            built.append(c.__name__)
            return _real(c, *a, **k)
        monkeypatch.setattr(cls, "from_nhwc", classmethod(counted))
    g = golden("raft_small")
    m, m0 = _raft(True), _raft(False)
    pads = tuple(int(v) for v in g["pads"])
    i1, i2 = torch.from_numpy(g["img1"]).to(DEV), torch.from_numpy(g["img2"]).to(DEV)
    with torch.no_grad():
        low, up = m(i1, i2, iters=6, test_mode=True, pads=pads)
        preds = m(i1, i2, iters=3, test_mode=False, pads=pads)
        assert built == ["AlternateCorrBlock"] * 2
        low0, up0 = m0(i1, i2, iters=6, test_mode=True, pads=pads)
        assert built[2:] == ["CorrBlock"]
    assert _rel(low, g["low6"]) < 1e-3
    assert _rel(up, g["up6"]) < 1e-3
    assert _rel(torch.stack(preds), g["preds3"]) < 1e-3
    assert _rel(low, low0) < 1e-3 and _rel(up, up0) < 1e-3
    x = [torch.from_numpy(prng.uniform_f32(1501 + i, (2, 3, 128, 160), 0.0, 255.0)).to(DEV) for i in range(4)]
    with torch.no_grad():
        for a, b in ((x[0], x[1]), (x[2], x[3])):
            m.use_graphs = False
            ref = raft.compute_raft(m, a, b, it=5)
            m.use_graphs = True
            got = raft.compute_raft(m, a, b, it=5)
            assert torch.equal(got, ref)
    assert len(m._graphs) == 1  # one shape, one captured graph


def test_mogan_steps_alternate_corr(gb, golden):
    """test_gpu_mogan.py's fixture step with opt.alternate_corr=True through MoGANModel.initRaftModel: the
    E-step and M-step losses meet the same tolerances against mogan_small.npz."""
    from gbvst import mogan_model
    from gbvst import options
    g = golden("mogan_small")
    opt = options.default_opt(True, model="mogan", ngf=8, ndf=8, pool_size=0, gpu_ids=[0], alternate_corr=True)
    m = mogan_model.MoGANModel(opt)
    r = m.raftModel
    assert r.args.alternate_corr is True
    shapes = {k: tuple(v.shape) for k, v in r.state_dict().items()}
    r.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in raft_ref.raft_weights(shapes, 1300, 1e-3).items()})
    seeds = {"G_A": 1500, "G_B": 1501, "D_A": 1502, "D_B": 1503, "M_A": 1504, "M_B": 1505}
    for name, seed in seeds.items():
        net = getattr(m, "net" + name)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in prng.init_state_dict(shapes, base_seed=seed).items()})
    names = list(g["loss_names"])
    imgs = [torch.from_numpy(g["img%d" % i]) for i in range(4)]
    for step in range(2):
        m.set_input_fc2(imgs)
        m.optimize_parameters()
        got = np.array([float(getattr(m, "loss_" + n)) if hasattr(m, "loss_" + n) else np.nan for n in names])
        ref = g["losses"][step]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        k = ~np.isnan(ref)
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-3 if step == 0 else 2e-3, atol=1e-6,
                                   err_msg=f"step {step}")
