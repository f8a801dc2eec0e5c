"""CPU checks of tests/stream_ref.py, the instrument tests/test_gpu_stream.py holds the streaming and layout kernels
to.  No GPU is touched.

  * every reference agrees with stock torch CPU (fp32 ops, fp64 F.interpolate, torch.optim.Adam(foreach=False))
    inside the bounds the device is held to: the bounds hold for an honest fp32 implementation, and the index
    formulas are the permute / pad / cat / flip they claim to be;
  * the two tiers of resize_bilinear agree with each other inside the independent tier's a-priori allowance;
  * the library ulp allowances (tanh 5, exp 3) cover stock torch's tanh, exp and sigmoid on the host;
  * the cases discriminate: every mutation of stream_ref.MUTATIONS, applied to the reference side, is rejected
    by the listed cases through the comparison function the GPU test calls;
  * every table row names the route or branch it is there for, and the copy_channels rows reach both routes of
    the alignment rule;
  * the instruments themselves: coded values are distinct fp32 integers, SENT is a NaN no arithmetic produces, every
    lane a kernel is documented not to read is NaN;
  * the GRU wrappers refuse a zr that is not [P][2*hd] before any launch; zero-length vst_adam_step / vst_axpby
    return OK without a launch.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import stream_ref as S


@pytest.fixture(scope="module")
def stock():
    """The stock-torch result of every case, computed once."""
    return {c.name: c.stock() for c in S.CASES}


@pytest.mark.parametrize("case", S.CASES, ids=S.case_ids())
def test_stock_torch_is_inside_the_bounds(case, stock):
    S.check(case, stock[case.name], stock=True)


def test_worst_stock_ratios_are_printed(stock):
    for c in S.CASES:
        with contextlib.redirect_stdout(io.StringIO()):
            S.check(c, stock[c.name], stock=True)
    for label, w in sorted(S.WORST.items()):
        print(f"stock torch {label}: worst err/bound {w:.3g}")
    assert S.WORST and max(S.WORST.values()) <= 1.0


def test_resize_tiers_agree():
    """The fp32-geometry tier and the fp64 F.interpolate tier differ by no more than the position allowance."""
    for c in S.CASES:
        if c.kernel != "resize_bilinear":
            continue
        b = c.expect()["y"].bounds
        if not b:
            continue        # the identity row: bits
        (y1, t1, r1), (y2, t2, r2) = b
        assert r1 and not r2
        assert bool((np.abs(y1 - y2) <= t2 - t1).all()), c.name


def test_library_ulp_allowances_cover_stock_torch():
    x = torch.linspace(-12, 12, 200001)
    x64 = x.double()
    for name, f, lim in (("tanh", torch.tanh, S.TANH_ULP), ("exp", torch.exp, S.EXP_ULP),
                         ("sigmoid", torch.sigmoid, 4)):        # sigmoid: 8 u = 4 ulp at most (case_gru_reset)
        ref = f(x64).numpy()
        worst = float((np.abs(f(x).double().numpy() - ref) / S.ulp32(ref)).max())
        print(f"{name}: {worst:.3g} ulp over [-12, 12] (allowance {lim})")
        assert worst <= lim


# ============================================================================================ the table itself
ISSUE_KERNELS = {"nchw_to_nhwc", "nhwc_to_nchw", "weight_pack", "raft_prep", "add_relu", "copy_channels",
                 "raft_ctx_split", "raft_flow4", "raft_coords_update", "raft_motion", "gru_reset", "gru_update",
                 "channel_normalize", "channel_normalize_bwd", "scaled_tanh", "scaled_tanh_bwd", "act_fwd", "act_bwd",
                 "upsample2x", "upsample2x_bwd", "maxpool2", "maxpool2_bwd", "gram_sym", "concat_label_nhwc",
                 "resize_bilinear", "adam_step"}


def test_every_row_names_its_branch():
    assert set(S.KERNELS) == ISSUE_KERNELS
    for c in S.CASES:
        assert len(c.why) > 8, c.name
    for k in S.KERNELS:
        whys = [c.why for c in S.CASES if c.kernel == k]
        if k != "weight_pack":       # its shapes are the issue's: 96 to 288 elements, one or two blocks
            assert any("fewer than 64 elements" in w for w in whys), (k, "no row under one wave")
            assert any("partial" in w for w in whys), (k, "no row with a partial last block")
    routes = {c.route for c in S.CASES if c.kernel == "copy_channels"}
    assert routes == {"copy_channels4_k", "copy_channels_k"}
    for c in S.CASES:
        if c.kernel == "copy_channels":
            assert c.route in c.why
    assert S.copy_route(12, 4, 16, 8, 4) == "copy_channels4_k" and S.copy_route(8, 0, 8, 4, 3) == "copy_channels_k"
    assert {c.name.split()[1] for c in S.CASES if c.kernel == "weight_pack"} == set(S.PACK_MODES)


def test_instruments():
    assert np.isnan(np.array([S.SENT], np.uint32).view(np.float32))[0]
    assert S.SENT not in (0x7FC00000, 0xFFC00000, 0x7FFFFFFF)          # not a NaN that 0/0, inf - inf or a library returns
    for c in S.CASES:
        for name, a in list(c.inputs.items()) + list(c.init.items()):
            assert a.dtype == np.float32, (c.name, name)
    v = S.coded(3, (5, 3, 3, 2))
    assert len(np.unique(v)) == v.size and float(v.max()) < 2 ** 24 and bool((v == np.round(v)).all())
    # poisoned lanes: what the kernel is documented not to read is NaN in the inputs the device gets
    c = S.CASE["raft_ctx_split hdim8 cdim4 cs16 xcs28 P37"]
    assert np.isnan(c.inputs["c"][:, 12:]).all() and not np.isnan(c.inputs["c"][:, :12]).any()
    c = S.CASE["raft_motion nout6 ocs8 xcs28 c012 P37"]
    assert np.isnan(c.inputs["out"][:, 6:]).all() and np.isnan(c.inputs["flow4"][:, 2:]).all()
    c = S.CASE["raft_coords_update B2 h5 w7 dcs8"]
    assert np.isnan(c.inputs["delta"][:, 2:]).all()
    c = S.CASE["copy_channels (12,2,16,5,6) npix70"]
    assert np.isnan(c.inputs["src"][:, :2]).all() and np.isnan(c.inputs["src"][:, 8:]).all()
    c = S.CASE["maxpool2 fwd N2 11x13 Cs8 ties"]
    assert np.isnan(c.inputs["x"][:, 10]).all() and np.isnan(c.inputs["x"][:, :, 12]).all()
    for n in ("nhwc_to_nchw N2 H5 W7 C5 cs12", "channel_normalize fwd npix70 Cs8 Cl5 mean d0=255.0",
              "scaled_tanh bwd npix70 Cs8 Cl5"):
        assert np.isnan(S.CASE[n].inputs["x"][..., 5:]).all()
    assert np.isnan(S.CASE["raft_prep 8 B2 H5 W7 pads(1, 2, 0, 3)"].inputs["img"][..., 3:]).all()


def test_maxpool_tie_patterns_put_the_first_maximum_at_each_position():
    c = S.CASE["maxpool2 bwd N1 2x2 Cs4 ties"]
    gx = c.expect()["gx"].bits.view(np.float32)[0].reshape(4, 4)       # [position][channel]
    assert [int(np.flatnonzero(gx[:, k])[0]) for k in range(4)] == [0, 1, 2, 3]
    assert all(int((gx[:, k] != 0).sum()) == 1 for k in range(4))


def test_nan_convention_rows():
    """relu and add_relu map NaN to +0 (torch.relu propagates it); maxpool2 propagates it like ATen."""
    e = S.CASE["act_fwd relu n12 nan"].expect()["y"]
    x = S.CASE["act_fwd relu n12 nan"].inputs["x"]
    assert np.isnan(x).sum() == 4 and bool((e.bits[np.isnan(x)] == 0).all())
    assert bool(torch.isnan(torch.relu(torch.from_numpy(x))[torch.from_numpy(np.isnan(x))]).all())
    e = S.CASE["add_relu n8 nan"].expect()["y"]
    assert bool((e.bits[[1, 2, 3, 5]] == 0).all()) and e.bits[4] == 0x7F800000
    e = S.CASE["maxpool2 fwd N2 11x13 Cs8 nan"].expect()["y"]
    assert int((e.kind == 2).sum()) == 3


# ================================================================================================== mutations
REJECTED_BY = {
    "cs_for_cl": ["nchw_to_nhwc N2 H5 W7 C5 cs8", "nhwc_to_nchw N2 H5 W7 C5 cs12",
                  "channel_normalize fwd npix70 Cs4 Cl3 nomean d0=1.0", "channel_normalize bwd npix70 Cs8 Cl5 mean d0=255.0",
                  "scaled_tanh fwd npix70 Cs8 Cl5", "scaled_tanh bwd npix1 Cs4 Cl3"],
    "swap_hw": ["nchw_to_nhwc N2 H5 W7 C4 cs4", "nhwc_to_nchw N2 H5 W7 C1 cs4", "upsample2x fwd N2 H5 W7 C8",
                "concat_label N2 H5 W7 Cx4 Cl5 cs12"],
    "c0_plus_one": ["copy_channels (12,4,16,8,4) npix70", "copy_channels (12,2,16,5,6) npix70",
                    "copy_channels (8,0,8,4,3) npix70", "raft_motion nout6 ocs8 xcs28 c012 P37",
                    "concat_label N2 H5 W7 Cx3 Cl2 cs8"],
    "pack_rs_transposed": ["weight_pack " + m for m in S.PACK_MODES],
    "ikf_unrotated": ["weight_pack IKF"],
    "nhwc_source_as_nchw": ["raft_prep 4 B2 H5 W7 pads(0, 0, 0, 0)", "raft_prep 8 B2 H5 W7 pads(1, 2, 0, 3)"],
    "gate_halves_swapped": ["gru_reset hd12 xcs40 P37", "gru_reset hd8 xcs24 P3", "gru_update hd12 xcs40 P37",
                            "gru_update hd8 xcs24 P3"],
    "hx_not_rhx": ["raft_ctx_split hdim8 cdim4 cs16 xcs28 P37", "raft_motion nout6 ocs8 xcs28 c012 P1"],
    "tanh_relu_halves_swapped": ["raft_ctx_split hdim8 cdim4 cs16 xcs28 P37", "raft_ctx_split hdim8 cdim4 cs16 xcs28 P1"],
    "pads_lr_swapped": ["raft_prep nchw B2 H5 W7 pads(1, 2, 0, 3)", "raft_prep 4 B2 H5 W7 pads(1, 2, 0, 3)"],
    "replicate_as_reflect": ["raft_prep nchw B2 H5 W7 pads(1, 2, 0, 3)", "raft_prep 8 B2 H2 W7 pads(0, 0, 3, 0)"],
    "flow_xy_swapped": ["raft_flow4 B2 h5 w7", "raft_flow4 B1 h1 w1", "raft_coords_update B2 h5 w7 dcs8",
                        "raft_motion nout6 ocs8 xcs28 c012 P37"],
    "coords_unsubtracted": ["raft_flow4 B2 h5 w7", "raft_flow4 B2 h15 w20"],
    "tie_last_wins": ["maxpool2 bwd N2 11x13 Cs8 ties", "maxpool2 bwd N1 2x2 Cs4 ties"],
    "up2_bwd_three_of_four": ["upsample2x bwd N2 H5 W7 C8", "upsample2x bwd N1 H1 W1 C4"],
    "sym_no_transpose": ["gram_sym C5", "gram_sym C33"],
    "lerp_one_sided": ["adam_step betas(0.0, 0.99) step1 n255", "adam_step betas(0.0, 0.99) step100000 n1025"],
    "eps_inside_sqrt": ["adam_step betas(0.9, 0.999) step7 n255", "adam_step betas(0.5, 0.999) step1 n1025"],
    "no_bias_correction": ["adam_step betas(0.9, 0.999) step1 n1", "adam_step betas(0.0, 0.99) step7 n255"],
    "resize_align_corners": ["resize_bilinear (5,7)->(11,4)", "resize_bilinear (1,7)->(3,14) mult",
                             "resize_bilinear (8,8)->(2,2)"],
}


def test_every_mutation_has_a_case():
    assert set(REJECTED_BY) == set(S.MUTATIONS)
    assert all(n in S.CASE for names in REJECTED_BY.values() for n in names)


@pytest.mark.parametrize("mutate", S.MUTATIONS)
def test_mutation_is_rejected(mutate, stock):
    """Each listed case rejects the mutation through the comparison function the GPU test calls; without the
    mutation the same call passes (the rejection is the mutation's doing)."""
    for name in REJECTED_BY[mutate]:
        c = S.CASE[name]
        S.check(c, stock[name], stock=True)
        with pytest.raises(AssertionError):
            S.check(c, stock[name], mutate=mutate, stock=True)
        print(f"{mutate}: rejected by {name}")


def test_a_written_guard_or_window_is_rejected(stock):
    """One lane outside the write window that lost SENT, and one zero lane that is -0, fail the comparison."""
    c = S.CASE["raft_motion nout6 ocs8 xcs28 c012 P37"]
    got = {k: v.copy() for k, v in stock[c.name].items()}
    got["hx"][3, 11] = 0.0
    with pytest.raises(AssertionError):
        S.check(c, got)
    c = S.CASE["nchw_to_nhwc N2 H5 W7 C5 cs8"]
    got = {k: v.copy() for k, v in stock[c.name].items()}
    got["y"][0, 0, 0, 7] = -0.0
    with pytest.raises(AssertionError):
        S.check(c, got)
    c = S.CASE["scaled_tanh fwd npix70 Cs8 Cl5"]
    got = {k: v.copy() for k, v in stock[c.name].items()}
    got["y"][5, 2] = np.nan
    with pytest.raises(AssertionError):
        S.check(c, got)


# ================================================================================================ the small fixes
def test_gru_wrappers_refuse_a_skewed_zr_before_any_launch():
    """gru_reset_k / gru_update_k index zr as [P][2*hd] and h, q as [P][hd] with no stride argument: a zr of
    padded width, or a q of another shape, is an error of the caller.  CPU tensors: the check comes first."""
    from gbvst import ops
    P, hd = 3, 5                                   # cpad(2 * hd) = 12 != 10
    h, q = torch.zeros(P, hd), torch.zeros(P, hd)
    rhx = torch.zeros(P, 3 * hd)
    with pytest.raises(ValueError, match="gru_reset"):
        ops.gru_reset(torch.zeros(P, ops.cpad(2 * hd)), h, rhx)
    with pytest.raises(ValueError, match="gru_update"):
        ops.gru_update(torch.zeros(P, ops.cpad(2 * hd)), q, h, rhx)
    with pytest.raises(ValueError, match="gru_update"):
        ops.gru_update(torch.zeros(P, 2 * hd), torch.zeros(P, hd + 1), h, rhx)
    with pytest.raises(ValueError, match="gru_reset"):
        ops.gru_reset(torch.zeros(P + 1, 2 * hd), h, rhx)
    with pytest.raises(RuntimeError, match="GPU tensors"):     # a well-shaped call gets as far as the device check
        ops.gru_reset(torch.zeros(P, 2 * hd), h, rhx)


def test_zero_length_adam_and_axpby_return_ok_without_a_launch():
    """n == 0 is a no-op (a zero-block grid is a launch error); the pointers below are never dereferenced and no
    device is needed.  n < 0, step < 1 and null pointers with n > 0 stay errors."""
    import gbvst
    lib = gbvst._lib.load()
    null, p = None, 4096
    assert lib.vst_adam_step(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 1, null) == 0
    assert lib.vst_adam_step(null, null, null, null, 0, 1e-3, 0.9, 0.999, 1e-8, 1, null) == 0    # an empty tensor
    assert lib.vst_axpby(p, p, 0, 1.0, 0.0, null) == 0
    assert lib.vst_axpby(null, null, 0, 1.0, 0.0, null) == 0
    assert lib.vst_adam_step(p, p, p, p, -1, 1e-3, 0.9, 0.999, 1e-8, 1, null) != 0
    assert b"adam_step: bad args" in lib.vst_last_error()
    assert lib.vst_adam_step(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0, null) != 0
    assert lib.vst_adam_step(null, p, p, p, 4, 1e-3, 0.9, 0.999, 1e-8, 1, null) != 0
    assert b"adam_step: null pointer" in lib.vst_last_error()
    assert lib.vst_axpby(p, p, -1, 1.0, 0.0, null) != 0
    assert lib.vst_axpby(null, p, 4, 1.0, 0.0, null) != 0
    assert b"axpby: null pointer" in lib.vst_last_error()
