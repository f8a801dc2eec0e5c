"""CPU-only checks of the Ruder recurrent video style surface: the trainer exists with the reference's
train_step layout (methods/learning-based/fs_ruder.py:38), the new C-ABI entries are declared, exported and
validate their arguments on the host, the vst::* operators are registered with fake implementations, CPU
tensors are refused, the roll draw is fs_ruder.py:18-19's, and the CPU reference the GPU tests use restates
fs_ruder.py:38-108 for two frames."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ruder_ref as RR

NEW_SYMBOLS = ["vst_ruder_stack_fwd", "vst_ruder_stack_bwd", "vst_ruder_temporal_part_floats",
               "vst_ruder_temporal_fwd", "vst_ruder_temporal_bwd"]
NEW_OPS = ["ruder_stack", "ruder_stack_backward", "ruder_temporal", "ruder_temporal_backward"]


def test_trainer_exists_with_reference_signatures():
    from gbvst import faststyle
    assert issubclass(faststyle.Ruder, faststyle.Johnson)
    sig = inspect.signature(faststyle.Ruder.__init__).parameters
    assert list(sig) == ["self", "style_imgs", "emphasis", "lr", "batch_sz", "device", "vgg", "model",
                         "pre_style_model"]
    assert len(sig["emphasis"].default) == 3 and sig["model"].default is None and sig["pre_style_model"].default is None
    ts = inspect.signature(faststyle.Ruder.train_step).parameters
    assert list(ts) == ["self", "imgs", "masks", "flows", "roll"] and ts["roll"].default is None
    assert list(inspect.signature(faststyle.Ruder.losses_nhwc).parameters) == ["self", "frames", "masks", "flows", "roll"]
    assert list(inspect.signature(faststyle.Ruder.infer_method).parameters) == ["self", "params"]
    assert list(inspect.signature(faststyle.Ruder.stylize_next).parameters) == \
        ["self", "prev_styled_nhwc", "frame_nhwc", "flow", "mask"]
    assert faststyle.Ruder.prep_adam is faststyle.Johnson.prep_adam
    # the len > 2 / len > 4 branches of fs_ruder.py:58-75: 2, 3 or 5 frames are used, 4 behave as 3
    assert [faststyle.Ruder.n_recurrent(n) for n in (2, 3, 4, 5, 6)] == [1, 2, 2, 4, 4]
    with pytest.raises(ValueError):
        faststyle.Ruder.n_recurrent(1)
    doc = faststyle.Ruder.losses_nhwc.__doc__
    assert "masks[-1]" in doc and "style" in doc and "fs_ruder.py:103" in doc
    # multi-style stays shut
    with pytest.raises(NotImplementedError):
        faststyle.FastStyleNet(3, n_styles=2)


def test_abi_table_and_host_validation():
    import gbvst
    from gbvst import _lib, fs_lib, ops
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name in ("ruder_stack", "ruder_stack_bwd", "ruder_temporal", "ruder_temporal_bwd"):
        assert callable(getattr(ops, name))
    for name in ("ruder_stack_nhwc", "ruder_temporal_nhwc", "ruder_blank_nhwc"):
        assert callable(getattr(fs_lib, name))
    gbvst._lib.build()
    lib = gbvst._lib.load()
    null = None
    # one double per block of 256 pixels, counted in floats
    assert lib.vst_ruder_temporal_part_floats(2, 32, 40) >= 2 * 10
    assert lib.vst_ruder_temporal_part_floats(4, 256, 256) >= 2 * 1024
    assert lib.vst_ruder_temporal_part_floats(0, 8, 8) == 0
    calls = {
        "vst_ruder_stack_fwd": lambda n, h, w: lib.vst_ruder_stack_fwd(null, null, null, null, null, null, n, h, w,
                                                                       1.0, null),
        "vst_ruder_stack_bwd": lambda n, h, w: lib.vst_ruder_stack_bwd(null, null, null, null, null, n, h, w, 1.0,
                                                                       null),
        "vst_ruder_temporal_fwd": lambda n, h, w: lib.vst_ruder_temporal_fwd(null, null, null, null, null, n, h, w,
                                                                             1.0, 1.0, null),
        "vst_ruder_temporal_bwd": lambda n, h, w: lib.vst_ruder_temporal_bwd(null, null, null, null, null, null, n,
                                                                             h, w, 1.0, 1.0, null),
    }
    for name, call in calls.items():
        assert call(1, 8, 8) != 0, name
        msg = lib.vst_last_error()
        assert b"bad args" in msg and name[len("vst_"):].encode() in msg, (name, msg)


def test_host_validation_of_shapes():
    """N, H, W < 1 are refused before any launch even with non-NULL pointers (host memory is never touched: the
    checks come first)."""
    import ctypes

    import gbvst
    gbvst._lib.build()
    lib = gbvst._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.vst_ruder_stack_fwd(p, p, p, p, p, p, *shape, 1.0, None) != 0
        assert b"bad args" in lib.vst_last_error()
        assert lib.vst_ruder_stack_bwd(p, p, p, p, p, *shape, 1.0, None) != 0
        assert b"bad args" in lib.vst_last_error()
        assert lib.vst_ruder_temporal_fwd(p, p, p, p, p, *shape, 1.0, 1.0, None) != 0
        assert b"bad args" in lib.vst_last_error()
        assert lib.vst_ruder_temporal_bwd(p, p, p, p, p, p, *shape, 1.0, 1.0, None) != 0
        assert b"bad args" in lib.vst_last_error()
    # y_prev, flow and mask come together (or the blank form: none of them)
    assert lib.vst_ruder_stack_fwd(p, p, None, p, p, p, 1, 2, 2, 1.0, None) != 0
    assert b"bad args" in lib.vst_last_error()


def test_cpu_tensors_refused():
    from gbvst import fs_lib, library  # noqa: F401
    a, flow, m = torch.zeros(1, 8, 8, 4), torch.zeros(1, 2, 8, 8), torch.ones(1, 1, 8, 8)
    with pytest.raises(RuntimeError):
        fs_lib.ruder_stack_nhwc(a, a, flow, m)
    with pytest.raises(RuntimeError):
        fs_lib.ruder_blank_nhwc(a)
    with pytest.raises(RuntimeError):
        fs_lib.ruder_temporal_nhwc(a, a, m, 1.0)
    i = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        torch.ops.vst.ruder_stack(i, i, flow, m, 1.0 / 255.0)
    with pytest.raises(RuntimeError):
        torch.ops.vst.ruder_temporal(i, i, m, 1.0, 1.0 / 255.0)


def test_library_ops_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gbvst import library
    for name in NEW_OPS:
        assert name in library.OPS
        assert getattr(torch.ops.vst, name).default._schema.name == "vst::" + name
    with FakeTensorMode():
        img, flow, m = torch.empty(2, 3, 8, 10), torch.empty(2, 2, 8, 10), torch.empty(2, 1, 8, 10)
        x, w = torch.ops.vst.ruder_stack(img, img, flow, m, 1.0 / 255.0)
        assert x.shape == (2, 7, 8, 10) and w.shape == (2, 3, 8, 10)
        assert torch.ops.vst.ruder_stack_backward(x, w, flow, 1.0 / 255.0).shape == (2, 3, 8, 10)
        assert torch.ops.vst.ruder_temporal(w, img, m, 1.0, 1.0 / 255.0).shape == ()
        gw, gy = torch.ops.vst.ruder_temporal_backward(torch.empty(()), w, img, m, 1.0, 1.0 / 255.0)
        assert gw.shape == w.shape and gy.shape == img.shape


def test_roll_draws_once():
    """fs_ruder.py:18-19, 44: one np.random.random() per step, True iff it is below p."""
    from gbvst import faststyle
    np.random.seed(1234)
    want = [np.random.random() for _ in range(9)]
    np.random.seed(1234)
    got = [faststyle.Ruder.roll(0.5) for _ in range(8)]
    assert got == [v < 0.5 for v in want[:8]] and True in got and False in got
    assert np.random.random() == want[8]       # eight calls consumed exactly eight draws


def test_reference_composition_two_frames():
    """ruder_ref's loss against fs_ruder.py:38-108 written out long-hand for 2 frames (both branches)."""
    from oracle import style_ref
    imgs, style, masks, flows = RR.step_inputs()
    imgs = [i.double() for i in imgs[:2]]
    masks, flows = [m.double() for m in masks], [f.double() for f in flows]
    model, pre, vgg = RR.nets()
    alpha, beta, gamma = 0.7, 0.3, 40.0
    with torch.no_grad():
        grams = [style_ref.gram_matrix(f) for f in vgg(style_ref.normalize(style.double()))]
        (total, sl, cl, tl), styled2 = RR.ruder_losses(model, pre, vgg, grams, imgs, masks, flows,
                                                       (alpha, beta, gamma), True)
        s1 = pre(imgs[0])[1] / 255.0
        w1 = style_ref.fs_warp(s1, flows[0])
        s2 = model(torch.cat((imgs[1], masks[0], w1), 1))[1] / 255.0
        sf, imf = vgg(style_ref.normalize(s2)), vgg(style_ref.normalize(imgs[1]))
        want_c = alpha * F.mse_loss(sf[2], imf[2])
        want_s = beta * sum(((style_ref.gram_matrix(f) - g) ** 2).mean() for f, g in zip(sf, grams))
        want_t = gamma * ((masks[3] * (w1 - s2)) ** 2).mean()       # masks[-1]: the LAST plane, not pair 0's
        for got, want in ((cl, want_c), (sl, want_s), (tl, want_t), (total, want_c + want_s + want_t)):
            assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
        assert torch.equal(styled2, s2)
        assert abs(float(want_t) - float(gamma * ((masks[0] * (w1 - s2)) ** 2).mean())) > 1e-3 * float(want_t)
        x, w = RR.stack_ref(s1 * 255.0, imgs[1], flows[0], masks[0])
        assert torch.allclose(w, w1, rtol=1e-12, atol=0) and x.shape == (RR.B, 7, RR.H, RR.W)
        assert abs(float(RR.temporal_ref(w1, s2 * 255.0, masks[3], gamma)) - float(want_t)) <= 1e-12 * float(want_t)
        # no roll: blank input, zero temporal loss
        (total0, sl0, cl0, tl0), s20 = RR.ruder_losses(model, pre, vgg, grams, imgs, masks, flows,
                                                       (alpha, beta, gamma), False)
        b2 = model(torch.cat((imgs[1], torch.zeros_like(masks[0]), torch.zeros_like(imgs[1])), 1))[1] / 255.0
        assert torch.equal(s20, b2) and float(tl0) == 0.0
        assert abs(float(total0) - float(sl0) - float(cl0)) <= 1e-12 * float(total0)
