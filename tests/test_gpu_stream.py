"""The one-pass streaming and layout kernels on the device, one by one (csrc/raft.hip, style.hip, resblk.hip, misc.hip,
temporal.hip and act_bwd_k of norm.hip), against tests/stream_ref.py: the references, the case table and the
comparison functions.  tests/test_stream_ref_host.py proves on the CPU that stock torch passes every comparison, that
twenty named slips are each rejected and that every row names the branch it is there for.

Every row runs through ops._call with explicit pointers: each output sits in the middle of a buffer filled with one
non-canonical NaN, 64 floats of guard on either side; inputs are coordinate-coded integers where the kernel moves
data, and NaN in every lane the kernel is documented not to read.  Movers, selects and the kernels that state their
operation order are compared on bit patterns; the others per element against fp64 with the counted bounds
c u M(o) of stream_ref (the only other allowances are the device math library's: tanh 5 ulp, exp 3 ulp).  Lanes
outside a write window must still hold the sentinel, zero lanes +0, inputs their bits.  No case is skipped.

The module prints the worst err/bound per kernel and the bit-exact lane counts at its end.
"""
import pytest
import torch

import stream_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    import gbvst
    from gbvst import ops as o
    gbvst._lib.load()
    yield o
    for label, (k, n) in sorted(S.EXACT.items()):
        print(f"{label}: bit-exact on {k} of {n} lanes")
    for label, w in sorted(S.WORST.items()):
        print(f"{label}: worst err/bound {w:.3g}")


@pytest.mark.parametrize("case", S.CASES, ids=S.case_ids())
def test_kernel_row(ops, case):
    """Bits, bounds, poisoned lanes, the write window, the guards and the inputs of one table row."""
    S.check(case, S.run_device(ops, case, DEV))


INPLACE = [c for c in S.CASES if c.inplace is not None]


@pytest.mark.parametrize("case", INPLACE, ids=S.case_ids(INPLACE))
def test_in_place_form_returns_the_same_bits(ops, case):
    """add_relu(out=a) and vst_act_fwd(p, p, ...): the output shares its input's buffer."""
    there = S.run_device(ops, case, DEV)
    here = S.run_device(ops, case, DEV, inplace=True)
    for name in there:
        assert (S.bits(there[name]) == S.bits(here[name])).all(), (case.name, name)
    S.check(case, here, label=case.kernel + " in place")


@pytest.mark.parametrize("hd,xcs,P", [(12, 40, 37), (8, 24, 3)])
def test_gru_update_in_place_on_h_through_the_wrapper(ops, hd, xcs, P):
    """ops.gru_update updates h where it stands and mirrors it into hx[:, :hd]: the bits of the guarded run."""
    case = S.CASE[f"gru_update hd{hd} xcs{xcs} P{P}"]
    want = S.run_device(ops, case, DEV)
    h = torch.from_numpy(case.init["h"].copy()).to(DEV)
    hx = torch.from_numpy(case.init["hx"].copy()).to(DEV)
    ops.gru_update(torch.from_numpy(case.inputs["zr"]).to(DEV), torch.from_numpy(case.inputs["q"]).to(DEV), h, hx)
    assert (S.bits(h.cpu().numpy()) == S.bits(want["h"])).all()
    assert (S.bits(hx.cpu().numpy()) == S.bits(want["hx"])).all()
    assert torch.equal(hx[:, :hd].contiguous().view(torch.int32), h.view(torch.int32))


LAYOUT = [(5, 8), (5, 12), (4, 4), (1, 4)]


@pytest.mark.parametrize("C,cs", LAYOUT)
def test_layout_round_trip_through_the_wrappers(ops, C, cs):
    """ops.nchw_to_nhwc / nhwc_to_nchw (the adaptors every other test trusts), cs > cpad(C) included: each
    direction against the table row's index formula and the round trip back to the input's bits."""
    N, H, W = S.BASE
    case = S.CASE[f"nchw_to_nhwc N{N} H{H} W{W} C{C} cs{cs}"]
    x = torch.from_numpy(case.inputs["x"]).to(DEV)
    y = ops.nchw_to_nhwc(x, cs=cs)
    assert tuple(y.shape) == (N, H, W, cs)
    S.check(case, {"y": y.cpu().numpy()}, label="layout wrappers")
    back = ops.nhwc_to_nchw(y, C)
    assert torch.equal(back.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("how", ["single", "batch", "transposed"])
@pytest.mark.parametrize("mode", S.PACK_MODES)
def test_weight_pack_wrappers_match_the_index_formula(ops, mode, how):
    """ops.weight_pack alone (vst_weight_pack_split), inside PackBatch (vst_weight_pack_batch) and with
    transposed=True: the formulas of the comment above pack_coords, bit for bit, pad lanes +0.  (The bf16 planes
    are pinned in test_gpu_conv_arith.py.)"""
    O, I, R, Sw, Op, Ip = S.pack_geometry(mode)
    w = S.coded(3, (O, I, R, Sw))
    wd = torch.from_numpy(w).to(DEV)
    kw = dict(Op=Op, Ip=Ip, transposed=(how == "transposed"))
    if how == "batch":
        with ops.PackBatch():
            wp = ops.weight_pack(wd, getattr(ops, "PACK_" + mode), **kw)
    else:
        wp = ops.weight_pack(wd, getattr(ops, "PACK_" + mode), **kw)
    want = S.pack_expect(w, mode, Op, Ip)
    assert tuple(wp.shape) == want.shape
    same = S.bits(wp.cpu().numpy()) == S.bits(want)
    k, n = S.EXACT.get("weight_pack " + how, (0, 0))
    S.EXACT["weight_pack " + how] = (k + int(same.sum()), n + same.size)
    assert same.all(), (mode, how, int((~same).sum()))


def test_zero_length_adam_and_axpby_are_no_ops(ops):
    """n == 0 returns OK without a launch and leaves the stream usable."""
    e = torch.empty(0, device=DEV)
    ops.adam_step(e, e, e, e, 1e-3, 0.9, 0.999, 1e-8, 1)
    ops.axpby(e, e, 1.0, 0.0)
    x = torch.ones(4, device=DEV)
    ops.axpby(x, x, 2.0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.full((4,), 3.0))
