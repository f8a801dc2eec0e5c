"""The memory-contract instrument (tests/mem_guard.py) proven on the CPU: the wrapper takes every call form the
package uses, every seeded slip is rejected (and a correct function passes), the package holds no tensor constructor
the instrument does not wrap, and every workspace row of tests/test_gpu_memory_contract.py has a positive size."""
import ast
import glob
import os

import pytest
import torch

import mem_guard as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, M.PKG_DIR)

_ORIGINALS = {n: getattr(torch, n) for n in M.FACTORIES + M.LIKES}
_ORIGINAL_NEWS = {n: torch.Tensor.__dict__.get(n, None) for n in M.NEWS}
_ORIGINAL_NEW_ATTRS = {n: getattr(torch.Tensor, n) for n in M.NEWS}


def _untouched():
    for n, f in _ORIGINALS.items():
        assert getattr(torch, n) is f, n
    for n in M.NEWS:
        assert torch.Tensor.__dict__.get(n, None) is _ORIGINAL_NEWS[n], n
        assert getattr(torch.Tensor, n) is _ORIGINAL_NEW_ATTRS[n], n


def guard(fill):
    """The instrument on CPU tensors, every caller counted as the package."""
    return M.MemGuard(fill, device="cpu", project=lambda frame: "pkg")


# ------------------------------------------------------------------------------------------------ the wrapper
FORMS = [
    ("empty positional sizes", lambda: torch.empty(3, 5), (3, 5), torch.float32),
    ("empty tuple", lambda: torch.empty((2, 3, 4)), (2, 3, 4), torch.float32),
    ("empty ()", lambda: torch.empty(()), (), torch.float32),
    ("empty int + device", lambda: torch.empty(7, device="cpu"), (7,), torch.float32),
    ("empty device object", lambda: torch.empty((7, 2), device=torch.device("cpu")), (7, 2), torch.float32),
    ("empty uint8", lambda: torch.empty(13, device="cpu", dtype=torch.uint8), (13,), torch.uint8),
    ("empty bf16", lambda: torch.empty((3, 4, 9), device="cpu", dtype=torch.bfloat16), (3, 4, 9), torch.bfloat16),
    ("empty fp64", lambda: torch.empty((5,), dtype=torch.float64, device="cpu"), (5,), torch.float64),
    ("empty int32", lambda: torch.empty((5, 1), dtype=torch.int32), (5, 1), torch.int32),
    ("empty zero elements", lambda: torch.empty((0, 4)), (0, 4), torch.float32),
    ("zeros", lambda: torch.zeros((2, 6), device="cpu"), (2, 6), torch.float32),
    ("zeros positional", lambda: torch.zeros(4, dtype=torch.float64), (4,), torch.float64),
    ("zeros requires_grad", lambda: torch.zeros(4, requires_grad=True), (4,), torch.float32),
    ("ones", lambda: torch.ones((3,), device="cpu"), (3,), torch.float32),
    ("full", lambda: torch.full((4, 2), 2.5, device="cpu"), (4, 2), torch.float32),
    ("full int32", lambda: torch.full((9,), 7, dtype=torch.int32), (9,), torch.int32),
    ("empty_like", lambda: torch.empty_like(torch.randn(3, 5)), (3, 5), torch.float32),
    ("empty_like dtype", lambda: torch.empty_like(torch.randn(3, 5), dtype=torch.bfloat16), (3, 5), torch.bfloat16),
    ("zeros_like", lambda: torch.zeros_like(torch.randn(2, 2, 2)), (2, 2, 2), torch.float32),
    ("ones_like", lambda: torch.ones_like(torch.randn(6)), (6,), torch.float32),
    ("full_like", lambda: torch.full_like(torch.randn(6), 0.2), (6,), torch.float32),
    ("new_empty", lambda: torch.randn(2).new_empty((3, 3)), (3, 3), torch.float32),
    ("new_empty sizes", lambda: torch.randn(2).new_empty(3, 2), (3, 2), torch.float32),
    ("new_empty dtype", lambda: torch.randn(2).new_empty((3,), dtype=torch.float64), (3,), torch.float64),
    ("new_zeros", lambda: torch.randn(2).double().new_zeros(5), (5,), torch.float64),
]


@pytest.mark.parametrize("fill", M.FILLS, ids=M.FILL_NAMES.get)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_wrapper_accepts_every_call_form(form, fill):
    name, make, shape, dtype = form
    try:
        with guard(fill) as mg:
            t = make()
            assert len(mg.allocs) == 1 and not mg.passthrough, (name, mg.passthrough)
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
            if t.numel():       # (an empty tensor reports a null pointer)
                assert t.data_ptr() == mg.allocs[0].buf.data_ptr() + M.GUARD
            # the buffer comes from the allocator at its own alignment (64 bytes on the CPU, 512 on the device);
            # GUARD is a multiple of 256, so the window keeps whatever alignment up to 256 the buffer has
            assert M.GUARD % 256 == 0 and t.data_ptr() % 64 == 0, name
            if t.numel():       # ... so misaligned(256) reports exactly the buffers the allocator itself put off 256
                assert bool(mg.misaligned(256)) == bool(mg.allocs[0].buf.data_ptr() % 256), name
            t.vst_split, t.vst_apl, t.vst_planes_only = "a", "b", True      # the package hangs these on tensors
            assert (t.vst_split, t.vst_apl, t.vst_planes_only) == ("a", "b", True)
            if t.numel():
                b = t.contiguous().view(-1).view(torch.uint8)
                init = {"zeros": 0, "ones": 1, "full": None}
                kind = mg.allocs[0].kind.replace("torch.", "").replace(".new_", "").replace("_like", "")
                if kind == "empty":
                    assert bool((b == fill).all()), name       # an empty allocation holds the fill, not zeros
                elif kind in ("zeros", "ones"):
                    assert bool((t.double() == init[kind]).all()), name
                else:
                    assert bool((t.double() == t.double().view(-1)[0]).all()) and float(t.view(-1)[0]) != 0, name
            if "requires_grad" in name:
                assert t.requires_grad
            mg.check()
    finally:
        _untouched()


def test_unmodelled_keywords_and_other_callers_pass_through():
    with guard(0xFF) as mg:
        out = _ORIGINALS["empty"](4)
        a = torch.empty(4, out=out)                                   # out=: not modelled
        b = torch.empty((2, 2), memory_format=torch.contiguous_format)
        c = torch.empty(3, pin_memory=False)
        with pytest.raises(TypeError):                                # a positional form the wrapper does not parse
            torch.full(2, 3, 1.5)                                     # goes to the original (which refuses it): counted
        assert a.data_ptr() == out.data_ptr() and b.shape == (2, 2) and c.shape == (3,)
        assert len(mg.allocs) == 0 and len(mg.passthrough) == 4, mg.passthrough
        assert "torch.full with 3 positional arguments" in mg.passthrough[3]
        assert all("test_mem_guard_host.py" in p for p in mg.passthrough)
    _untouched()
    # a caller outside the package (the default rule: this test module is neither the package nor a *_ref adaptor)
    with M.MemGuard(0xFF, device="cpu") as mg:
        torch.empty(4)
        torch.zeros(4, device="cpu")
        assert not mg.allocs and not mg.passthrough
    _untouched()
    # the instrument's device filter: a CPU allocation is not guarded by a device instrument and is not counted
    with M.MemGuard(0xFF, device="cuda", project=lambda frame: "pkg") as mg:
        t = torch.empty(4, device="cpu")
        assert not mg.allocs and not mg.passthrough and t.shape == (4,)
    _untouched()


def test_the_frame_rule_names_the_package_and_the_ref_adaptors():
    class F:
        def __init__(self, name, file):
            self.f_globals = {"__name__": name, "__file__": file}
    assert M.project_frame(F(M.PKG_DIR + ".ops", os.path.join(PKG, "ops.py"))) == "pkg"
    assert M.project_frame(F("gbvst.library", os.path.join(PKG, "library.py"))) == "pkg"
    assert M.project_frame(F("conv_ref", os.path.join(REPO, "tests", "conv_ref.py"))) == "ref"
    assert M.project_frame(F("test_gpu_ops", os.path.join(REPO, "tests", "test_gpu_ops.py"))) is None
    assert M.project_frame(F("torch.functional", "/x/torch/functional.py")) is None
    assert M.project_frame(F("my_ref", "/elsewhere/my_ref.py")) is None


def test_constructors_restored_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with guard(0x7F):
            assert torch.empty is not _ORIGINALS["empty"]
            assert torch.Tensor.new_empty is not _ORIGINAL_NEW_ATTRS["new_empty"]
            1 / 0
    _untouched()


# ---------------------------------------------------------------------------------------------- seeded slips
N = 16


def _correct(x, mg):
    ws = torch.empty(N)
    ws.copy_(x * 2)
    y = torch.empty(N)
    y.copy_(ws + 1)
    return y


def _write_past(x, mg):
    y = _correct(x, mg)
    y.as_strided((N + 1,), (1,))[N] = 1.0
    return y


def _write_before(x, mg):
    y = _correct(x, mg)
    torch.as_strided(y, (1,), (1,), y.storage_offset() - 1)[0] = 1.0
    return y


def _stale_ws(x, mg):
    ws = torch.empty(N)
    ws += x * 2               # added into before it is written
    y = torch.empty(N)
    y.copy_(ws + 1)
    return y


def _stale_ws_behind_relu(x, mg):
    ws = torch.empty(N)
    y = torch.empty(N)
    s = ws - x.abs() - 1                                            # -|x| - 1 < 0 over a zeroed workspace
    y.copy_(torch.where(s > 0, s, torch.zeros(())) + x)             # the library's relu: NaN -> +0
    return y


def _lane_unwritten(x, mg):
    y = torch.empty(N)
    y[:N - 1].copy_(x[:N - 1] * 2 + 1)
    return y


def _input_modified(x, mg):
    y = _correct(x, mg)
    x[3] = 0.0
    return y


def _read_past(x, mg):
    y = torch.empty(N)
    y.copy_(x.as_strided((N,), (1,), x.storage_offset() + 1) * 2 + 1)   # x[1:N+1]: the last lane is guard memory
    return y


def run_fills(fn, fills=M.FILLS):
    """The per-row procedure of the device test in small: the function under every fill on a placed input; returns
    the failure messages (guards, inputs, bits across fills)."""
    x0 = torch.arange(1, N + 1, dtype=torch.float32) / 4
    outs, fails = [], []
    for fill in fills:
        with guard(fill) as mg:
            x = mg.place(x0)
            y = fn(x, mg)
            fails += mg.failures()
            outs.append(y.clone().view(torch.int32))
    for o in outs[1:]:
        if not torch.equal(o, outs[0]):
            fails.append("results differ between fills")
    return fails


def test_a_correct_function_passes():
    assert run_fills(_correct) == []
    _untouched()


@pytest.mark.parametrize("slip,word", [(_write_past, "AFTER"), (_write_before, "BEFORE"), (_stale_ws, "differ"),
                                       (_lane_unwritten, "differ"), (_input_modified, "input modified"),
                                       (_read_past, "differ")], ids=lambda v: getattr(v, "__name__", None))
def test_every_seeded_slip_is_rejected(slip, word):
    fails = run_fills(slip)
    assert fails and any(word in f for f in fails), fails
    if word in ("AFTER", "BEFORE", "input modified"):      # the message names the allocation
        assert any("test_mem_guard_host.py:" in f and "(16,)" in f and "float32" in f for f in fails), fails
    _untouched()


def test_the_relu_hidden_stale_read_needs_the_7f_fill():
    """ws - |x| - 1 is negative over zeros and NaN over 0xFF: the relu returns +0 for both, the two runs agree.  Over
    0x7F it is 3.4e38: only that fill shows the read."""
    assert run_fills(_stale_ws_behind_relu, fills=(0x00, 0xFF)) == []
    assert run_fills(_stale_ws_behind_relu, fills=(0xFF,)) == []
    fails = run_fills(_stale_ws_behind_relu)
    assert fails == ["results differ between fills"], fails


def test_unwritten_names_the_lanes_left_alone():
    with guard(0x7F) as mg:
        y = torch.empty((4, 8))
        y[:, :6] = 1.0
        u = mg.unwritten(y).all(dim=-1)
        assert bool(u[:, 6:].all()) and not bool(u[:, :6].any())


# ------------------------------------------------------------------------------------------------ source scan
# constructors that fully initialise what they return (or return no fresh device memory at all)
INITIALISING = {"tensor", "arange", "randn", "rand", "randint", "stack", "cat", "from_numpy", "frombuffer", "meshgrid",
                "lerp", "sqrt", "abs", "mean", "sum", "unsqueeze", "load"}
# torch.<name> that make no tensor
NOT_CONSTRUCTORS = {"device", "Generator", "no_grad", "is_grad_enabled", "is_tensor", "save", "manual_seed",
                    "set_grad_enabled", "enable_grad", "inference_mode", "get_default_dtype", "Size", "dtype"}


def _constructor_calls(path):
    tree = ast.parse(open(path).read(), path)
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute):
            f = n.func
            if isinstance(f.value, ast.Name) and f.value.id == "torch":
                yield "torch." + f.attr, n.lineno
            elif f.attr.startswith("new_"):
                yield "." + f.attr, n.lineno
        if isinstance(n, ast.ImportFrom) and n.module == "torch":
            for a in n.names:       # `from torch import empty` would bind the original before the patch
                if a.name[:1].islower():
                    yield "from torch import " + a.name, n.lineno


def scan(paths):
    unknown, seen = [], set()
    for p in paths:
        for name, line in _constructor_calls(p):
            seen.add(name)
            short = name.split(".")[-1]
            if name in M.WRAPPED:
                continue
            if name.startswith("torch.") and (short in INITIALISING or short in NOT_CONSTRUCTORS):
                continue
            if name.startswith("from torch import ") and short in NOT_CONSTRUCTORS | {"nn", "autograd", "optim"}:
                continue
            unknown.append(f"{os.path.relpath(p, REPO)}:{line} {name}")
    return unknown, seen


def test_the_package_holds_no_constructor_the_instrument_does_not_wrap(tmp_path):
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) > 20
    unknown, seen = scan(files)
    assert not unknown, "tensor constructors the instrument neither wraps nor knows as initialising:\n" + \
        "\n".join(unknown)
    assert {"torch.empty", "torch.empty_like", "torch.zeros", ".new_empty"} <= seen      # the scan sees the calls
    # and it does report: an unknown constructor, a .new_* form and a from-import, with file:line
    bad = tmp_path / "bad.py"
    bad.write_text("import torch\nfrom torch import empty\n\ndef f(x):\n    a = torch.empty_strided((2,), (1,))\n"
                   "    return x.new_tensor([1.0]), torch.zeros(3), a\n")
    unknown, _ = scan([str(bad)])
    assert len(unknown) == 3 and ":5 torch.empty_strided" in unknown[1] and ":6 .new_tensor" in unknown[2] and \
        ":2 from torch import empty" in unknown[0], unknown


# --------------------------------------------------------------------------------------------- workspace rows
@pytest.fixture(scope="module")
def lib():
    import gbvst
    gbvst._lib.build()
    return gbvst._lib.load()


def test_every_workspace_row_has_a_positive_size(lib):
    """A row of the device test that takes a workspace, a `part` buffer or a pyramid cannot silently stop exercising
    it: its size query, asked of the library's host code at the row's shape, is positive."""
    import gbvst
    rows = M.workspace_rows(gbvst._lib.CONSTANTS, gbvst._lib.MATH_MODES)
    assert len(rows) >= 30
    for row, query, args in rows:
        n = int(getattr(lib, query)(*args))
        assert n > 0, (row, query, args, n)
    entries = {r[0].split()[0] for r in rows}
    assert set(M.WS_BYTES_ENTRIES) <= entries, set(M.WS_BYTES_ENTRIES) - entries
