"""Host side of RAFT's alternate_corr path (raft_corr.AlternateCorrBlock, csrc/altcorr.hip): the flag is
accepted by raft.RAFT, the three C entries are declared and validate their arguments before any launch
(so these calls run without a GPU, as in test_asan_host.py), and the Python wrapper raises the same
errors CorrBlock does."""
import argparse

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import gbvst
    return gbvst._lib.load()


def test_raft_accepts_alternate_corr():
    from gbvst import raft
    m0 = raft.RAFT(argparse.Namespace(small=False))
    m1 = raft.RAFT(argparse.Namespace(small=False, alternate_corr=True))
    assert list(m1.state_dict().keys()) == list(m0.state_dict().keys())
    assert m1.args.alternate_corr is True and not getattr(m0.args, "alternate_corr", False)
    with pytest.raises(NotImplementedError):
        raft.RAFT(argparse.Namespace(small=True, alternate_corr=True))


def test_raft_flops_alternate_term():
    from gbvst import raft
    B, H, W, it = 2, 440, 1024, 20
    h, w = H // 8, W // 8
    base = raft.raft_flops(B, H, W, it)
    assert raft.raft_flops(B, H, W, it, alternate_corr=False) == base
    alt = raft.raft_flops(B, H, W, it, alternate_corr=True)
    gemm = 2.0 * B * (h * w) ** 2 * 256
    dots = it * B * h * w * 4 * 100 * 256 * 2.0
    assert abs((alt - base) - (dots - gemm)) <= 1e-9 * base


def _floats(B, H, W, Dp, levels):
    return B * Dp * sum((H >> l) * (W >> l) for l in range(1, levels))


def test_symbols_and_pyramid_floats(lib):
    from gbvst import _lib, ops
    for name in ("vst_altcorr_pyramid_floats", "vst_altcorr_pyramid", "vst_altcorr_lookup"):
        assert name in _lib.SIGNATURES
    for geo in ((1, 55, 128, 256, 4), (2, 18, 22, 256, 4)):
        assert lib.vst_altcorr_pyramid_floats(*geo) == _floats(*geo)
        assert ops.altcorr_pyramid_floats(*geo) == _floats(*geo)
    assert lib.vst_altcorr_pyramid_floats(1, 55, 128, 256, 1) == 0
    assert lib.vst_altcorr_pyramid_floats(1, 55, 128, 256, 0) == -1
    assert lib.vst_altcorr_pyramid_floats(1, 55, 128, 256, 9) == -1


def test_bad_arguments_rejected_on_host(lib):
    """Every rejection happens before a launch: the non-null pointers below are never dereferenced."""
    null, p = None, 4096
    # (f1, f2, pyr, coords, out, B, H, W, Dp, D, levels, radius, Cs, stream)
    bad = [
        (null, p, p, p, p, 1, 16, 16, 256, 256, 4, 4, 328),    # null fmap1
        (p, null, p, p, p, 1, 16, 16, 256, 256, 4, 4, 328),    # null fmap2
        (p, p, null, p, p, 1, 16, 16, 256, 256, 4, 4, 328),    # null pyramid with levels > 1
        (p, p, p, null, p, 1, 16, 16, 256, 256, 4, 4, 328),    # null coords
        (p, p, p, p, null, 1, 16, 16, 256, 256, 4, 4, 328),    # null out
        (p, p, p, p, p, 1, 16, 16, 256, 256, 4, 4, 323),       # Cs < 4 * 81
        (p, p, p, p, p, 1, 16, 16, 6, 6, 4, 4, 328),           # Dp % 4 != 0
        (p, p, p, p, p, 1, 16, 16, 8, 9, 4, 4, 328),           # D > Dp
        (p, p, p, p, p, 1, 16, 16, 256, 256, 0, 4, 328),       # levels outside 1..8
        (p, p, p, p, p, 1, 16, 16, 256, 256, 9, 4, 2000),
    ]
    for args in bad:
        assert lib.vst_altcorr_lookup(*args, null) != 0, args
        assert b"bad args" in lib.vst_last_error(), args
    # a 3-level pyramid of an 8x7 map: the coarsest level is 2x1
    assert lib.vst_altcorr_lookup(p, p, p, p, p, 1, 8, 7, 256, 256, 3, 4, 244, null) != 0
    assert b"level 2 smaller than 2x2" in lib.vst_last_error()
    assert lib.vst_altcorr_pyramid(p, p, 1, 8, 7, 256, 3, null) != 0
    assert b"level 2 smaller than 2x2" in lib.vst_last_error()
    for args in ((null, p, 1, 16, 16, 256, 4), (p, null, 1, 16, 16, 256, 4), (p, p, 1, 16, 16, 6, 4),
                 (p, p, 1, 16, 16, 256, 0), (p, p, 1, 16, 16, 256, 9)):
        assert lib.vst_altcorr_pyramid(*args, null) != 0, args
        assert b"bad args" in lib.vst_last_error(), args


def test_wrapper_errors():
    from gbvst import ops
    from gbvst import raft_corr
    AlternateCorrBlock = raft_corr.AlternateCorrBlock
    f = torch.zeros(1, 8, 16, 16)
    with pytest.raises(RuntimeError):  # CPU tensors: no fallback
        AlternateCorrBlock(f, f, 2, 3)
    with pytest.raises(RuntimeError):
        AlternateCorrBlock.from_nhwc(f.permute(0, 2, 3, 1).contiguous(), f.permute(0, 2, 3, 1).contiguous(), 8, 2, 3)
    with pytest.raises(RuntimeError):
        ops.altcorr_pyramid(torch.zeros(1, 16, 16, 8), torch.zeros(512), 2)
    with pytest.raises(RuntimeError):
        ops.altcorr_lookup(torch.zeros(1, 16, 16, 8), torch.zeros(1, 16, 16, 8), torch.zeros(512),
                           torch.zeros(1, 2, 16, 16), 8, 2, 3)
    with pytest.raises(ValueError):
        AlternateCorrBlock(f, torch.zeros(1, 8, 16, 12), 2, 3)
    with pytest.raises(ValueError):
        AlternateCorrBlock(f, torch.zeros(2, 8, 16, 16), 2, 3)
    with pytest.raises(ValueError):  # 8x8 with 4 levels: the coarsest level is 1x1
        AlternateCorrBlock(torch.zeros(1, 8, 8, 8), torch.zeros(1, 8, 8, 8), 4, 4)
