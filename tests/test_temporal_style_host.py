"""CPU-only checks of the temporal video style surface: the Huang / Reconet trainers exist with the
reference's train_step layout (methods/learning-based/fs_huang.py:28, fs_reconet.py:28), the new C-ABI
entries are declared, exported and validate their arguments on the host, the vst::* operators are
registered with fake implementations, and the CPU reference the GPU tests use restates the composed form."""
import inspect

import pytest
import torch

import temporal_style_ref as R

NEW_SYMBOLS = ["vst_temporal_sqdiff_part_floats", "vst_temporal_sqdiff_fwd", "vst_temporal_sqdiff_bwd",
               "vst_resize_bilinear"]


def test_trainers_exist_with_matching_signatures():
    from gbvst import faststyle
    assert issubclass(faststyle.Huang, faststyle.Johnson) and issubclass(faststyle.Reconet, faststyle.Johnson)
    sig_h = inspect.signature(faststyle.Huang.train_step)
    sig_r = inspect.signature(faststyle.Reconet.train_step)
    assert list(sig_h.parameters) == list(sig_r.parameters) == ["self", "imgs", "masks", "flows"]
    assert list(inspect.signature(faststyle.Huang.losses_nhwc).parameters) == \
        list(inspect.signature(faststyle.Reconet.losses_nhwc).parameters)
    for cls, n in ((faststyle.Huang, 4), (faststyle.Reconet, 5)):
        assert len(inspect.signature(cls.__init__).parameters["emphasis"].default) == n
        assert cls.infer_method is faststyle.Johnson.infer_method and cls.prep_adam is faststyle.Johnson.prep_adam


def test_abi_table_and_host_validation():
    import gbvst
    from gbvst import _lib, fs_lib, ops
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name in ("temporal_sqdiff", "temporal_sqdiff_bwd", "resize_bilinear"):
        assert callable(getattr(ops, name))
    assert callable(fs_lib.temporal_loss_nhwc)
    gbvst._lib.build()
    lib = gbvst._lib.load()
    null = None
    # one double per block of (ceil(W * Cs/4 / 256), H, N), counted in floats
    assert lib.vst_temporal_sqdiff_part_floats(4, 64, 64, 128) >= 2 * 8 * 64 * 4
    assert lib.vst_temporal_sqdiff_part_floats(4, 256, 256, 4) >= 2 * 256 * 4
    assert lib.vst_temporal_sqdiff_fwd(null, null, null, null, null, null, null, null, 1, 8, 8, 4, 3, 1.0, 1.0,
                                       null) != 0
    assert b"bad args" in lib.vst_last_error()
    assert lib.vst_temporal_sqdiff_bwd(null, null, null, null, null, null, null, null, null, 1, 8, 8, 4, 3, 1.0,
                                       1.0, null) != 0
    assert lib.vst_resize_bilinear(null, null, null, 1, 2, 8, 8, 2, 2, null) != 0
    assert b"resize_bilinear" in lib.vst_last_error()


def test_cpu_tensors_refused():
    from gbvst import fs_lib, library  # noqa: F401
    a = torch.zeros(1, 8, 8, 4)
    with pytest.raises(RuntimeError):
        fs_lib.temporal_loss_nhwc(a, a, torch.zeros(1, 2, 8, 8), torch.ones(1, 1, 8, 8), 1.0)
    with pytest.raises(RuntimeError):
        torch.ops.vst.resize_bilinear(torch.zeros(1, 2, 8, 8), 2, 2, None)


def test_library_ops_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gbvst import library
    for name in ("temporal_sqdiff", "temporal_sqdiff_backward", "resize_bilinear"):
        assert name in library.OPS
        assert getattr(torch.ops.vst, name).default._schema.name == "vst::" + name
    with FakeTensorMode():
        f, flow, m = torch.empty(2, 128, 8, 10), torch.empty(2, 2, 8, 10), torch.empty(2, 1, 8, 10)
        assert torch.ops.vst.temporal_sqdiff(f, f, flow, m, 1.0, 1.0, None, None).shape == ()
        ga, gb = torch.ops.vst.temporal_sqdiff_backward(torch.empty(()), f, f, flow, m, 1.0, 1.0, None, None)
        assert ga.shape == f.shape and gb.shape == f.shape
        assert torch.ops.vst.resize_bilinear(torch.empty(2, 2, 32, 40), 8, 10, [0.25, 0.25]).shape == (2, 2, 8, 10)


def test_reference_composition():
    """The helper's composed loss against the formula written out with oracle.style_ref.fs_warp, and its
    threshold guard: a flow that puts a sample's validity sum at 0.9998 is refused."""
    from oracle import style_ref
    a, b = R.rand(1, (2, 3, 12, 20)), R.rand(2, (2, 3, 12, 20))
    i1, i2 = R.rand(3, (2, 3, 12, 20)), R.rand(4, (2, 3, 12, 20))
    flow = R.rand(901, (2, 2, 12, 20), 3.0)
    mask = torch.rand(2, 1, 12, 20, generator=torch.Generator().manual_seed(5))
    assert 0.2 < R.assert_off_threshold(flow) < 0.6
    d = i2 - style_ref.fs_warp(i1, flow)
    r = (0.2126 * d[:, 0] + 0.7152 * d[:, 1] + 0.0722 * d[:, 2]).unsqueeze(1)
    want = 3.0 * ((mask * (b / 255 - style_ref.fs_warp(a / 255, flow) - r)) ** 2).mean()
    got = R.temporal_ref(a, b, flow, mask, 3.0, 1.0 / 255.0, (i1, i2))
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    edge = torch.zeros(1, 2, 12, 20)
    R.assert_off_threshold(edge)
    # sample x = (w + f) W / (W - 1) - 0.5 = -0.0002: 0.0002 of the weight falls outside, validity sum 0.9998
    edge[0, 0, 5, 10] = -10.0 + 19.0 * (-0.0002 + 0.5) / 20.0
    with pytest.raises(AssertionError):
        R.assert_off_threshold(edge)
