"""References, the case table, comparison functions and named mutations for the one-pass streaming and layout
kernels: the kernels that move, pad, concatenate, pool or apply a pointwise function between the big kernels
(csrc/raft.hip, csrc/style.hip, csrc/resblk.hip, csrc/misc.hip, csrc/temporal.hip and act_bwd_k of csrc/norm.hip).
tests/test_gpu_stream.py feeds the comparison functions with the device's results, tests/test_stream_ref_host.py
with stock torch CPU fp32 results (they must pass: the bounds hold for the references alone) and with deliberately
wrong expectations (`mutate=`, they must be rejected: the cases discriminate).  Nothing here imports the package;
the functions that launch take the package's ``ops`` module as an argument.

Four instruments, applied to every kernel of the table:

  1. coordinate-coded inputs   every element of a mover's input is a distinct integer below 2^24 that encodes its
                               tensor and its linear index (so its n, c, h, w); the expected output is an index
                               formula in numpy and the comparison is on BIT PATTERNS.  N, H, W, C are pairwise
                               distinct and R != S, so any transposition changes bits.
  2. per-element bounds        kernels that compute: |y - y64| <= gamma(c) M(o) + floor, gamma(c) = c u / (1 - c u),
                               u = 2^-24, M(o) the sum of the absolute values of the terms of that output (not
                               |y64|: 1 - t*t, (1-z)h + zq and the lerp cancel), c the count of the kernel's
                               roundings, derived in the docstring of the function that computes the bound, and
                               floor = fp32's smallest normal where a gate can underflow.  Contraction to fma only
                               removes roundings, so a counted bound still holds.  `/` and sqrtf are correctly rounded
                               (the library is built without fast-math) and count as one rounding.  tanhf and expf
                               come from the device math library: their allowance is the OpenCL full-profile limit
                               that library is specified to meet, tanh 5 ulp and exp 3 ulp (1 ulp <= 2 u |y|).
                               Where a kernel states its operation order with __f*_rn (raft_prep, raft_flow4,
                               raft_coords_update), and where an output is one IEEE operation (lrelu's product,
                               relu's select), the expectation is a numpy fp32 restatement, bit for bit.
  3. poisoned unread input     every input lane the kernel is documented not to read holds NaN: padding channels
                               >= Cl, c[:, hdim+cdim:] of raft_ctx_split, out[:, nout:] of raft_motion, delta[:, 2:]
                               of raft_coords_update, flow4's z and w, source channels outside [sc0, sc0+nc), the odd
                               last row / column of a floor-mode maxpool2.  Any NaN in an output lane that is not
                               expected to hold one is a failure.
  4. sentinel footprint        every output sits in the middle of a larger device buffer pre-filled with one
                               non-canonical NaN bit pattern (SENT), GUARD floats on either side (run_device).
                               After the call the guards and every lane outside the documented write window still
                               hold SENT bit for bit, lanes documented as zero hold +0 and every input's bits are
                               unchanged.  In-place forms return the bits of the out-of-place form.

NaN convention: relu (apply_act's and add_relu's) maps NaN to +0 where torch.relu propagates it; lrelu,
tanh and maxpool2 propagate it (in maxpool2 the last NaN of a window in scan order is the argmax, as in ATen).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FLOOR = 2.0 ** -126           # fp32's smallest normal
SENT = 0x7FC5A5A5             # a quiet NaN no arithmetic produces
GUARD = 64                    # sentinel floats on either side of every output
f32, f64, u32 = np.float32, np.float64, np.uint32

MUTATIONS = (
    # addressing
    "cs_for_cl", "swap_hw", "c0_plus_one", "pack_rs_transposed", "ikf_unrotated", "nhwc_source_as_nchw",
    # semantics
    "gate_halves_swapped", "hx_not_rhx", "tanh_relu_halves_swapped", "pads_lr_swapped", "replicate_as_reflect",
    "flow_xy_swapped", "coords_unsubtracted", "tie_last_wins",
    # arithmetic
    "up2_bwd_three_of_four", "sym_no_transpose", "lerp_one_sided", "eps_inside_sqrt", "no_bias_correction",
    "resize_align_corners")

# per label in this process: worst err / bound seen, and (bit-exact lanes, lanes compared on bits)
WORST = {}
EXACT = {}


def gamma(c):
    """c u / (1 - c u): the standard bound of c accumulated roundings (covers the second-order terms)."""
    return c * U / (1.0 - c * U)


def ulp32(y):
    """The fp32 ulp at the exact value |y| (subnormal spacing below the smallest normal)."""
    a = np.maximum(np.abs(np.asarray(y, f64)), FLOOR)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


TANH_ULP, EXP_ULP = 5, 3


def cfloat(v):
    """The value a C float parameter receives for the Python number v."""
    return float(f32(v))


def coded(t, shape, shift=20):
    """Distinct integers (t << shift) + 1 + linear index, exact in fp32 (instrument 1)."""
    n = int(np.prod(shape))
    assert n < (1 << shift) and ((t + 1) << shift) <= (1 << 24)
    return ((t << shift) + 1 + np.arange(n)).astype(f32).reshape(shape)


def sentinel(shape):
    return np.full(shape, SENT, u32).view(f32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def rng(seed):
    return np.random.default_rng(seed)


def randn(seed, shape, scale=1.0):
    return (rng(seed).standard_normal(shape) * scale).astype(f32)


class Exp:
    """What one output tensor must hold after the call.  Starts as `init` (the tensor's content before the call:
    SENT for a pure output), every lane compared on bits; exact() / bound() / isnan() overwrite lanes."""

    def __init__(self, init):
        self.bits = bits(init).copy()
        self.kind = np.zeros(init.shape, np.int8)       # 0 bits, 1 bound, 2 must be NaN
        self.bounds = []                                # [(y64, tol)] over the kind == 1 lanes (all must hold)

    def exact(self, vals, where=None):
        where = np.ones(self.bits.shape, bool) if where is None else np.broadcast_to(where, self.bits.shape)
        v = np.broadcast_to(bits(np.asarray(vals, f32)), self.bits.shape)
        self.bits[where] = v[where]
        self.kind[where] = 0
        nan = where & np.isnan(np.broadcast_to(np.asarray(vals, f32), self.bits.shape))
        self.kind[nan] = 2          # a NaN's payload is not pinned, its presence is
        return self

    def bound(self, y64, tol, where=None, more=False, restated=False):
        where = np.ones(self.bits.shape, bool) if where is None else np.broadcast_to(where, self.bits.shape)
        if not more:
            self.kind[where] = 1
        full_y, full_t = np.zeros(self.bits.shape, f64), np.full(self.bits.shape, np.inf)
        full_y[where] = np.broadcast_to(y64, self.bits.shape)[where]
        full_t[where] = np.broadcast_to(tol, self.bits.shape)[where]
        self.bounds.append((full_y, full_t, restated))
        return self


def window(shape, *slices):
    m = np.zeros(shape, bool)
    m[slices] = True
    return m


class Case:
    """One row of the table.  inputs: name -> fp32 array (read-only operands, poisoned where unread); init:
    name -> fp32 array (outputs and in/out operands before the call; SENT where write-only); call(ops, p): the
    launch, p = name -> device pointer; expect(mutate) -> name -> Exp; stock() -> name -> fp32 array, the same
    operation in stock torch CPU fp32 applied onto copies of init; why: the route or branch the row is there for;
    inplace: (output, input) that may share a buffer; post(got): extra bit relations between outputs."""

    def __init__(self, name, kernel, why, inputs, init, call, expect, stock, inplace=None, post=None):
        self.name, self.kernel, self.why = name, kernel, why
        self.inputs, self.init, self.call, self.expect, self.stock = inputs, init, call, expect, stock
        self.inplace, self.post = inplace, post

    def __repr__(self):
        return self.name


def check(case, got, mutate=None, label=None, stock=False):
    """Hold the results `got` (name -> fp32 array) to case.expect(mutate).  Prints what it measured first.
    stock: got comes from stock torch, which owes nothing to a bound marked `restated`."""
    label = label or case.kernel
    exp = case.expect(mutate)
    fails = []
    for name, e in exp.items():
        g = np.ascontiguousarray(got[name], dtype=f32)
        assert g.shape == e.bits.shape, (case.name, name, g.shape, e.bits.shape)
        b = e.kind == 0
        same = bits(g) == e.bits
        k, n = EXACT.get(label, (0, 0))
        EXACT[label] = (k + int((same & b).sum()), n + int(b.sum()))
        if not bool(same[b].all()):
            i = np.argwhere(b & ~same)[0]
            fails.append(f"{name}: {int((b & ~same).sum())} of {int(b.sum())} lanes differ in bits, first at "
                         f"{tuple(i)}: got {bits(g)[tuple(i)]:#010x} want {e.bits[tuple(i)]:#010x}")
        m = e.kind == 2
        if not bool(np.isnan(g[m]).all()):
            fails.append(f"{name}: {int((~np.isnan(g[m])).sum())} lanes that must be NaN are not")
        m = e.kind == 1
        if m.any():
            if bool(np.isnan(g[m]).any()):
                fails.append(f"{name}: {int(np.isnan(g[m]).sum())} NaN in computed lanes")
            for y64, tol, restated in e.bounds:
                if restated and stock:
                    continue        # holds for an implementation with the kernel's own fp32 geometry only
                with np.errstate(invalid="ignore"):
                    err = np.abs(g.astype(f64) - y64)
                    err = np.where(g.astype(f64) == y64, 0.0, err)[m]      # inf == inf
                    ratio = np.where(tol[m] > 0, err / np.maximum(tol[m], 1e-300), np.where(err > 0, np.inf, 0.0))
                worst = float(np.nanmax(ratio)) if ratio.size else 0.0
                if not np.isfinite(err).all():
                    worst = float("inf")
                print(f"{case.name} {name}: worst err/bound = {worst:.3g}")
                if mutate is None:
                    WORST[label] = max(WORST.get(label, 0.0), worst)
                if not worst <= 1.0:
                    fails.append(f"{name}: worst err/bound {worst:.3g}")
    if case.post is not None:
        msg = case.post(got)
        if msg:
            fails.append(msg)
    assert not fails, f"{case.name}" + (f" [{mutate}]" if mutate else "") + ": " + "; ".join(fails)


def run_device(ops, case, dev="cuda", inplace=False):
    """Launch the case with every output in the middle of a SENT-filled buffer (instrument 4) and return
    name -> fp32 array.  Asserts the guards and the inputs' bits after the call.  inplace: case.inplace's output
    shares the buffer of its input (the buffer then starts as that input)."""
    p, ins, outs = {}, {}, {}
    alias = case.inplace if inplace else None
    for name, a in case.inputs.items():
        if alias and name == alias[1]:
            continue
        ins[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        p[name] = ins[name].data_ptr()
    for name, a in case.init.items():
        src = case.inputs[alias[1]] if alias and name == alias[0] else a
        n = int(np.prod(a.shape))
        assert src.size == n
        buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        buf[GUARD:GUARD + n] = torch.from_numpy(bits(src).view(np.int32).reshape(-1)).to(dev)
        outs[name] = (buf, n, a.shape)
        p[name] = buf.data_ptr() + 4 * GUARD
        if alias and name == alias[0]:
            p[alias[1]] = p[name]
    case.call(ops, p)
    torch.cuda.synchronize()
    sent = SENT
    got = {}
    for name, (buf, n, shape) in outs.items():
        h = buf.cpu().numpy()
        assert (h[:GUARD] == sent).all() and (h[GUARD + n:] == sent).all(), f"{case.name}: guard of {name} written"
        got[name] = h[GUARD:GUARD + n].view(f32).reshape(shape).copy()
    for name, t in ins.items():
        assert (bits(t.cpu().numpy()) == bits(case.inputs[name])).all(), f"{case.name}: input {name} changed"
    return got


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ptr(p, name):
    return p.get(name)


BASE = (2, 5, 7)      # N, H, W of the base image; with Cs = 8 its 560 elements leave a partial third block
TINY = (1, 1, 1)      # fewer than 64 elements, one channel group


# ================================================================================================ layout converters
def case_nchw_to_nhwc(N, H, W, C, cs, why):
    x = coded(1, (N, C, H, W))
    HW = H * W

    def expect(mutate=None):
        n, h, w, c = np.indices((N, H, W, cs))
        pq = w * H + h if mutate == "swap_hw" else h * W + w
        Csrc = cs if mutate == "cs_for_cl" else C
        src = ((n * Csrc + c) * HW + pq) % x.size
        valid = (c < Csrc)
        return {"y": Exp(sentinel((N, H, W, cs))).exact(np.where(valid, x.reshape(-1)[src], f32(0)))}

    def stock():
        return {"y": F.pad(_t(x).permute(0, 2, 3, 1), (0, cs - C)).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_nchw_to_nhwc", p["x"], p["y"], N, C, H, W, cs, ops._stream())

    return Case(f"nchw_to_nhwc N{N} H{H} W{W} C{C} cs{cs}", "nchw_to_nhwc", why, {"x": x},
                {"y": sentinel((N, H, W, cs))}, call, expect, stock)


def case_nhwc_to_nchw(N, H, W, C, cs, why):
    x = coded(2, (N, H, W, cs))
    x[..., C:] = np.nan
    HW = H * W

    def expect(mutate=None):
        n, c, h, w = np.indices((N, C, H, W))
        pq = w * H + h if mutate == "swap_hw" else h * W + w
        stride = C if mutate == "cs_for_cl" else cs
        return {"y": Exp(sentinel((N, C, H, W))).exact(x.reshape(-1)[(n * HW + pq) * stride + c])}

    def stock():
        return {"y": _t(x)[..., :C].permute(0, 3, 1, 2).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_nhwc_to_nchw", p["x"], p["y"], N, C, H, W, cs, ops._stream())

    return Case(f"nhwc_to_nchw N{N} H{H} W{W} C{C} cs{cs}", "nhwc_to_nchw", why, {"x": x},
                {"y": sentinel((N, C, H, W))}, call, expect, stock)


# ====================================================================================================== weight_pack
PACK_MODES = ("KC", "CK", "OK", "IK", "IKF", "SOK")


def pack_shape(mode, R, S, Op, Ip):
    return {"KC": (R, S, Ip, Op), "CK": (R, S, Op, Ip), "OK": (Op, R, S, Ip), "IK": (Ip, R, S, Op),
            "IKF": (Ip, R, S, Op), "SOK": (S * Op, R, 1, Ip)}[mode]


def pack_expect(w, mode, Op, Ip, mutate=None):
    """The formulas of the comment above pack_coords (csrc/misc.hip), element by element: KC out[r][s][i][o],
    CK out[r][s][o][i], OK out[o][r][s][i], IK out[i][r][s][o], IKF = IK with the taps rotated 180 degrees,
    SOK out[s*Op + o][r][0][i]; o >= O and i >= I lanes +0."""
    O, I, R, S = w.shape
    out = np.zeros(pack_shape(mode, R, S, Op, Ip), f32)
    wt = w.reshape(O, I, R * S)
    for idx in np.ndindex(out.shape):
        if mode == "KC":
            r, s, i, o = idx
        elif mode == "CK":
            r, s, o, i = idx
        elif mode == "OK":
            o, r, s, i = idx
        elif mode in ("IK", "IKF"):
            i, r, s, o = idx
            if mode == "IKF" and mutate != "ikf_unrotated":
                r, s = R - 1 - r, S - 1 - s
        else:
            so, r, _, i = idx
            s, o = so // Op, so % Op
        tap = s * R + r if mutate == "pack_rs_transposed" else r * S + s
        if o < O and i < I:
            out[idx] = wt[o, i, tap]
    return out


def pack_stock(w, mode, Op, Ip):
    O, I, R, S = w.shape
    wp = F.pad(_t(w), (0, 0, 0, 0, 0, Ip - I, 0, Op - O))
    if mode == "KC":
        y = wp.permute(2, 3, 1, 0)
    elif mode == "CK":
        y = wp.permute(2, 3, 0, 1)
    elif mode == "OK":
        y = wp.permute(0, 2, 3, 1)
    elif mode == "IK":
        y = wp.permute(1, 2, 3, 0)
    elif mode == "IKF":
        y = wp.flip(2, 3).permute(1, 2, 3, 0)
    else:
        y = wp.permute(3, 0, 2, 1).reshape(S * Op, R, 1, Ip)
    return y.contiguous().numpy()


def pack_geometry(mode):
    """(O, I, R, S, Op, Ip) of the mode's row."""
    return (3, 6, 3, 2, 4, 8) if mode == "SOK" else (5, 3, 3, 2, 8, 4)


def case_weight_pack(mode):
    O, I, R, S, Op, Ip = pack_geometry(mode)
    w = coded(3, (O, I, R, S))
    shape = pack_shape(mode, R, S, Op, Ip)

    def expect(mutate=None):
        return {"out": Exp(sentinel(shape)).exact(pack_expect(w, mode, Op, Ip, mutate))}

    def call(ops, p):
        ops._call("vst_weight_pack", p["w"], p["out"], O, I, R, S, Op, Ip, getattr(ops, "PACK_" + mode), ops._stream())

    return Case(f"weight_pack {mode}", "weight_pack", f"pack_coords' {mode} arm, pad lanes o >= {O} / i >= {I}",
                {"w": w}, {"out": sentinel(shape)}, call, expect, lambda: {"out": pack_stock(w, mode, Op, Ip)})


# ======================================================================================================== raft_prep
def case_raft_prep(B, H, W, src, pads, why):
    """src: 'nchw' or the NHWC channel stride.  Bit-exact: the kernel states __fsub_rn(__fmul_rn(2, __fdiv_rn(x,
    255)), 1), restated in numpy fp32."""
    nhwc = src != "nchw"
    img = coded(1, (B, H, W, src) if nhwc else (B, 3, H, W), shift=12)
    if nhwc:
        img[..., 3:] = np.nan
    l0, r0, t, b = pads
    Hp, Wp = H + t + b, W + l0 + r0

    def expect(mutate=None):
        l = r0 if mutate == "pads_lr_swapped" else l0
        n, hp, wp = np.indices((B, Hp, Wp))
        hh, ww = hp - t, wp - l
        if mutate == "replicate_as_reflect":
            hh, ww = np.abs(hh), np.abs(ww)
            hh, ww = np.where(hh > H - 1, 2 * (H - 1) - hh, hh), np.where(ww > W - 1, 2 * (W - 1) - ww, ww)
        hh, ww = np.clip(hh, 0, H - 1), np.clip(ww, 0, W - 1)
        out = np.zeros((B, Hp, Wp, 4), f32)
        flat = img.reshape(-1)
        for c in range(3):
            if nhwc and mutate != "nhwc_source_as_nchw":
                v = flat[((n * H + hh) * W + ww) * src + c]
            else:
                v = flat[((n * 3 + c) * H + hh) * W + ww]
            with np.errstate(invalid="ignore"):
                out[..., c] = f32(2) * (v / f32(255)) - f32(1)
        return {"out": Exp(sentinel(out.shape)).exact(out)}

    def stock():
        x = _t(img)[..., :3].permute(0, 3, 1, 2) if nhwc else _t(img)
        y = 2 * (F.pad(x, (l0, r0, t, b), mode="replicate") / 255) - 1
        return {"out": F.pad(y.permute(0, 2, 3, 1), (0, 1)).contiguous().numpy()}

    def call(ops, p):
        if nhwc:
            ops._call("vst_raft_prep_nhwc", p["img"], src, p["out"], B, H, W, l0, r0, t, b, ops._stream())
        else:
            ops._call("vst_raft_prep", p["img"], p["out"], B, H, W, l0, r0, t, b, ops._stream())

    return Case(f"raft_prep {src} B{B} H{H} W{W} pads{pads}", "raft_prep", why, {"img": img},
                {"out": sentinel((B, Hp, Wp, 4))}, call, expect, stock)


# ========================================================================================================= add_relu
def case_add_relu(n, why, nan=False):
    """relu(a + b): one rounding (the add; max is exact): c = 1, M = |a| + |b|.  NaN lanes (nan=True) hold +0:
    fmaxf(NaN, 0) = 0, the library's relu convention."""
    a, b = randn(11, (n,)), randn(12, (n,))
    if nan:
        a[1], b[2], a[5], b[5] = np.nan, np.nan, np.nan, np.nan
        a[3], b[3] = -np.inf, 1.0
        a[4], b[4] = np.inf, 1.0

    def expect(mutate=None):
        with np.errstate(invalid="ignore"):
            s = a.astype(f64) + b.astype(f64)
        e = Exp(sentinel((n,)))
        fin = np.isfinite(s)
        e.bound(np.maximum(np.where(fin, s, 0), 0), gamma(1) * (np.abs(a.astype(f64)) + np.abs(b.astype(f64))), fin)
        e.exact(np.where(s == np.inf, f32(np.inf), f32(0)), ~fin)
        return {"y": e}

    def stock():
        s = _t(a) + _t(b)
        return {"y": torch.where(s > 0, s, torch.zeros_like(s)).numpy()}

    def call(ops, p):
        ops._call("vst_add_relu", p["a"], p["b"], p["y"], n, ops._stream())

    return Case(f"add_relu n{n}" + (" nan" if nan else ""), "add_relu", why, {"a": a, "b": b}, {"y": sentinel((n,))},
                call, expect, stock, inplace=("y", "a"))


# ==================================================================================================== copy_channels
def copy_route(scs, sc0, dcs, dc0, nc):
    """The alignment rule of vst_copy_channels: float4 granules when every stride, offset and count is a multiple
    of 4, else one float per thread."""
    return "copy_channels4_k" if all(v % 4 == 0 for v in (scs, sc0, dcs, dc0, nc)) else "copy_channels_k"


def case_copy_channels(scs, sc0, dcs, dc0, nc, npix, why):
    src = coded(4, (npix, scs))
    keep = window(src.shape, slice(None), slice(sc0, sc0 + nc))
    src[~keep] = np.nan

    def expect(mutate=None):
        s0 = sc0 + 1 if mutate == "c0_plus_one" else sc0
        e = Exp(sentinel((npix, dcs)))
        full = np.zeros((npix, dcs), f32)
        full[:, dc0:dc0 + nc] = src[:, s0:s0 + nc]
        return {"dst": e.exact(full, window(full.shape, slice(None), slice(dc0, dc0 + nc)))}

    def stock():
        d = _t(sentinel((npix, dcs)).copy())
        d[:, dc0:dc0 + nc] = _t(src)[:, sc0:sc0 + nc]
        return {"dst": d.numpy()}

    def call(ops, p):
        ops._call("vst_copy_channels", p["src"], scs, sc0, p["dst"], dcs, dc0, nc, npix, ops._stream())

    c = Case(f"copy_channels ({scs},{sc0},{dcs},{dc0},{nc}) npix{npix}", "copy_channels", why, {"src": src},
             {"dst": sentinel((npix, dcs))}, call, expect, stock)
    c.route = copy_route(scs, sc0, dcs, dc0, nc)
    return c


# =================================================================================================== raft_ctx_split
def case_ctx_split(hdim, cdim, cs, xcs, P, why):
    """tanh half -> h and hx[:, :hdim], within TANH_ULP ulp of tanh in fp64 (the library's allowance; the argument
    is the input itself, no rounding of ours); relu half -> hx and rhx[:, hdim:hdim+cdim], bit for bit (a select).
    rhx[:, :hdim] and everything from hdim+cdim on are not written."""
    c = randn(21, (P, cs), 2.0)
    c[0, :3] = (0.0, 30.0, -30.0)
    c[:, hdim + cdim:] = np.nan
    nch = hdim + cdim

    def expect(mutate=None):
        swapped = mutate == "tanh_relu_halves_swapped"
        k = np.arange(nch)
        is_t = (k >= cdim) if swapped else (k < hdim)       # swapped: the first cdim lanes get the relu
        v = c[:, :nch].astype(f64)
        t64, r32 = np.tanh(v), np.maximum(c[:, :nch], f32(0))
        eh, ehx, erhx = Exp(sentinel((P, hdim))), Exp(sentinel((P, xcs))), Exp(sentinel((P, xcs)))
        tol = TANH_ULP * ulp32(t64)
        wt = np.zeros((P, xcs), bool)
        wt[:, :nch] = is_t
        wr = np.zeros((P, xcs), bool)
        wr[:, :nch] = ~is_t
        full_t, full_tol, full_r = np.zeros((P, xcs)), np.zeros((P, xcs)), np.zeros((P, xcs), f32)
        full_t[:, :nch], full_tol[:, :nch], full_r[:, :nch] = t64, tol, r32
        ehx.bound(full_t, full_tol, wt).exact(full_r, wr)
        if mutate != "hx_not_rhx":
            erhx.exact(full_r, wr)
        if swapped:
            full_h = np.zeros((P, hdim), f32)
            full_h[:, :cdim] = r32[:, :cdim]
            eh.exact(full_h, window((P, hdim), slice(None), slice(0, cdim)))
        else:
            eh.bound(t64[:, :hdim], tol[:, :hdim])
        return {"h": eh, "hx": ehx, "rhx": erhx}

    def stock():
        h, hx, rhx = (_t(sentinel(s).copy()) for s in ((P, hdim), (P, xcs), (P, xcs)))
        t, r = torch.tanh(_t(c)[:, :hdim]), torch.relu(_t(c)[:, hdim:nch])
        h[:], hx[:, :hdim], hx[:, hdim:nch], rhx[:, hdim:nch] = t, t, r, r
        return {"h": h.numpy(), "hx": hx.numpy(), "rhx": rhx.numpy()}

    def post(got):
        if not (bits(got["h"]) == bits(got["hx"][:, :hdim])).all():
            return "h and hx[:, :hdim] differ in bits"

    def call(ops, p):
        ops._call("vst_raft_ctx_split", p["c"], cs, hdim, cdim, p["h"], p["hx"], p["rhx"], xcs, P, ops._stream())

    return Case(f"raft_ctx_split hdim{hdim} cdim{cdim} cs{cs} xcs{xcs} P{P}", "raft_ctx_split", why, {"c": c},
                {"h": sentinel((P, hdim)), "hx": sentinel((P, xcs)), "rhx": sentinel((P, xcs))}, call, expect, stock,
                post=post)


# ================================================================================ raft_flow4 / raft_coords_update
def _grid(B, h, w):
    ys, xs = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    return np.broadcast_to(np.stack([xs, ys])[None], (B, 2, h, w)).astype(f32)


def case_flow4(B, h, w, why):
    """flow4[p] = (x1 - x, y1 - y, +0, +0) with __fsub_rn: a numpy fp32 restatement, bit for bit."""
    c1 = (_grid(B, h, w) + randn(31, (B, 2, h, w), 3.0)).astype(f32)
    P = B * h * w

    def expect(mutate=None):
        d = c1 if mutate == "coords_unsubtracted" else c1 - _grid(B, h, w)
        d = d.transpose(0, 2, 3, 1).reshape(P, 2)
        if mutate == "flow_xy_swapped":
            d = d[:, ::-1]
        out = np.zeros((P, 4), f32)
        out[:, :2] = d
        return {"flow4": Exp(sentinel((P, 4))).exact(out)}

    def stock():
        d = (_t(c1) - _t(_grid(B, h, w))).permute(0, 2, 3, 1).reshape(P, 2)
        return {"flow4": F.pad(d, (0, 2)).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_raft_flow4", p["coords1"], p["flow4"], B, h, w, ops._stream())

    return Case(f"raft_flow4 B{B} h{h} w{w}", "raft_flow4", why, {"coords1": c1}, {"flow4": sentinel((P, 4))}, call,
                expect, stock)


def case_coords_update(B, h, w, dcs, why):
    """coords1[n][c] += delta[p][c] with __fadd_rn, c < 2; delta[:, 2:] is not read.  Bit for bit."""
    c1 = (_grid(B, h, w) + randn(32, (B, 2, h, w), 3.0)).astype(f32)
    P = B * h * w
    delta = randn(33, (P, dcs))
    delta[:, 2:] = np.nan

    def expect(mutate=None):
        d = delta[:, :2].reshape(B, h, w, 2).transpose(0, 3, 1, 2)
        if mutate == "flow_xy_swapped":
            d = d[:, ::-1]
        return {"coords1": Exp(c1).exact(c1 + d)}

    def stock():
        return {"coords1": (_t(c1) + _t(delta)[:, :2].reshape(B, h, w, 2).permute(0, 3, 1, 2)).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_raft_coords_update", p["coords1"], p["delta"], dcs, B, h, w, ops._stream())

    return Case(f"raft_coords_update B{B} h{h} w{w} dcs{dcs}", "raft_coords_update", why, {"delta": delta},
                {"coords1": c1}, call, expect, stock)


# ====================================================================================================== raft_motion
def case_motion(nout, ocs, xcs, c0, P, why):
    out = coded(5, (P, ocs))
    out[:, nout:] = np.nan
    fl = coded(6, (P, 4))
    fl[:, 2:] = np.nan

    def expect(mutate=None):
        k0 = c0 + 1 if mutate == "c0_plus_one" else c0
        f2 = fl[:, 1::-1] if mutate == "flow_xy_swapped" else fl[:, :2]
        full = np.zeros((P, xcs), f32)
        full[:, k0:k0 + nout], full[:, k0 + nout:k0 + nout + 2] = out[:, :nout], f2
        win = window((P, xcs), slice(None), slice(k0, k0 + nout + 2))
        ehx, erhx = Exp(sentinel((P, xcs))).exact(full, win), Exp(sentinel((P, xcs)))
        if mutate != "hx_not_rhx":
            erhx.exact(full, win)
        return {"hx": ehx, "rhx": erhx}

    def stock():
        hx, rhx = _t(sentinel((P, xcs)).copy()), _t(sentinel((P, xcs)).copy())
        v = torch.cat([_t(out)[:, :nout], _t(fl)[:, :2]], 1)
        hx[:, c0:c0 + nout + 2], rhx[:, c0:c0 + nout + 2] = v, v
        return {"hx": hx.numpy(), "rhx": rhx.numpy()}

    def call(ops, p):
        ops._call("vst_raft_motion", p["out"], ocs, nout, p["flow4"], p["hx"], p["rhx"], xcs, c0, P, ops._stream())

    return Case(f"raft_motion nout{nout} ocs{ocs} xcs{xcs} c0{c0} P{P}", "raft_motion", why,
                {"out": out, "flow4": fl}, {"hx": sentinel((P, xcs)), "rhx": sentinel((P, xcs))}, call, expect, stock)


# ============================================================================================= gru_reset / gru_update
def _gru_data(hd, P):
    zr = randn(41, (P, 2 * hd), 3.0)
    zr[0, :] = np.resize(np.array([100.0, -100.0, 0.0], f32), 2 * hd)     # sigmoid exactly 1, exactly 0, 0.5
    return zr, randn(42, (P, hd)), np.tanh(randn(43, (P, hd))).astype(f32)


def _sig64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x.astype(f64)))


def case_gru_reset(hd, xcs, P, why):
    """rhx[:, :hd] = sigm(r) * h, r = zr[:, hd:], sigm(x) = __fdiv_rn(1, __fadd_rn(1, expf(-x))).
    e = expf(-x): EXP_ULP ulp <= 6 u relative; its share of 1 + e is e / (1 + e) <= 1, so the sum carries <= 6 u
    from e plus its own u, the quotient one more: sigm = sigma (1 + theta), |theta| <= 8 u.  The product adds one:
    c = 9, M = |sigma h| (a single term), floor for a product that underflows."""
    zr, h, _ = _gru_data(hd, P)

    def expect(mutate=None):
        gate = zr[:, :hd] if mutate == "gate_halves_swapped" else zr[:, hd:]
        y = _sig64(gate) * h.astype(f64)
        e = Exp(sentinel((P, xcs)))
        full_y, full_t = np.zeros((P, xcs)), np.zeros((P, xcs))
        full_y[:, :hd], full_t[:, :hd] = y, gamma(9) * np.abs(y) + FLOOR
        return {"rhx": e.bound(full_y, full_t, window((P, xcs), slice(None), slice(0, hd)))}

    def stock():
        rhx = _t(sentinel((P, xcs)).copy())
        rhx[:, :hd] = torch.sigmoid(_t(zr)[:, hd:]) * _t(h)
        return {"rhx": rhx.numpy()}

    def call(ops, p):
        ops._call("vst_gru_reset", p["zr"], p["h"], p["rhx"], hd, xcs, P, ops._stream())

    return Case(f"gru_reset hd{hd} xcs{xcs} P{P}", "gru_reset", why, {"zr": zr, "h": h}, {"rhx": sentinel((P, xcs))},
                call, expect, stock)


def case_gru_update(hd, xcs, P, why):
    """h' = (1 - z) h + z q, z = sigm(zr[:, :hd]) = sigma (1 + theta), |theta| <= 8 u (case_gru_reset), every
    operation __f*_rn.  1 - z: 8 u sigma from z + u |1 - z|; times h: one more u: <= u (8 sigma + 2 (1 - sigma)) |h|;
    z q: 9 u sigma |q|; the sum: u |h'| <= u ((1 - sigma) |h| + sigma |q|).  Together <= u (8 |h| + 10 sigma |q|):
    c = 10, M = |h| + sigma |q| (the terms (1 - sigma) h, sigma h, sigma q).  h is updated in place and copied to
    hx[:, :hd]: the same bits."""
    zr, h, q = _gru_data(hd, P)

    def expect(mutate=None):
        gate = zr[:, hd:] if mutate == "gate_halves_swapped" else zr[:, :hd]
        z = _sig64(gate)
        y = (1 - z) * h.astype(f64) + z * q.astype(f64)
        tol = gamma(10) * (np.abs(h.astype(f64)) + z * np.abs(q.astype(f64))) + FLOOR
        full_y, full_t = np.zeros((P, xcs)), np.zeros((P, xcs))
        full_y[:, :hd], full_t[:, :hd] = y, tol
        return {"h": Exp(h).bound(y, tol),
                "hx": Exp(sentinel((P, xcs))).bound(full_y, full_t, window((P, xcs), slice(None), slice(0, hd)))}

    def stock():
        hx = _t(sentinel((P, xcs)).copy())
        z = torch.sigmoid(_t(zr)[:, :hd])
        hn = (1 - z) * _t(h) + z * _t(q)
        hx[:, :hd] = hn
        return {"h": hn.numpy(), "hx": hx.numpy()}

    def post(got):
        if not (bits(got["h"]) == bits(got["hx"][:, :hd])).all():
            return "hx[:, :hd] != h in bits"

    def call(ops, p):
        ops._call("vst_gru_update", p["zr"], p["q"], p["h"], p["hx"], hd, xcs, P, ops._stream())

    return Case(f"gru_update hd{hd} xcs{xcs} P{P}", "gru_update", why, {"zr": zr, "q": q},
                {"h": h, "hx": sentinel((P, xcs))}, call, expect, stock, post=post)


# ================================================================================================ channel_normalize
def case_chnorm(npix, Cs, Cl, with_mean, d0, backward, why):
    """forward ((x / d0) - mean[c]) / std[c]: three roundings.  With a = x / d0: the first leaves u |a|, the
    difference u |a - m|, the quotient u |a - m|, all over |s|: <= 3 u (|a| + |m|) / |s|: c = 3, M = (|a| + |m|)/|s|.
    backward (x / std[c]) / d0: c = 2, M = |y64|.  Padding lanes hold +0; x's padding lanes are not read."""
    x = (rng(51).random((npix, Cs)) * (255.0 if d0 > 1 else 1.0)).astype(f32) if not backward else randn(52, (npix, Cs))
    x[:, Cl:] = np.nan
    mean = (rng(53).random(Cs) * 0.5 + 0.2).astype(f32)[:Cl] if with_mean else None
    std = (rng(54).random(Cs) * 0.3 + 0.2).astype(f32)[:Cl]

    def expect(mutate=None):
        a = x[:, :Cl].astype(f64) / d0
        m = mean.astype(f64) if with_mean else np.zeros(Cl)
        s = std.astype(f64)
        if backward:
            y = x[:, :Cl].astype(f64) / s / d0
            tol = gamma(2) * np.abs(y)
        else:
            y = (a - m) / s
            tol = gamma(3) * (np.abs(a) + np.abs(m)) / np.abs(s)
        full_y, full_t = np.zeros((npix, Cs)), np.zeros((npix, Cs))
        full_y[:, :Cl], full_t[:, :Cl] = y, tol
        lanes = window((npix, Cs), slice(None), slice(0, Cl))
        e = Exp(sentinel((npix, Cs))).bound(full_y, full_t, lanes)
        # cs_for_cl: a kernel that takes Cs for Cl computes the padding lanes from x (NaN here) instead of +0
        e.exact(x if mutate == "cs_for_cl" else f32(0), ~lanes)
        return {"y": e}

    def stock():
        xs, s = _t(x)[:, :Cl], _t(std)
        if backward:
            y = (xs / s) / d0
        else:
            y = ((xs / d0) - (_t(mean) if with_mean else 0.0)) / s
        return {"y": F.pad(y, (0, Cs - Cl)).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_channel_normalize", p["x"], p["y"], _ptr(p, "mean"), p["std"], float(d0), npix, Cs, Cl,
                  1 if backward else 0, ops._stream())

    ins = {"x": x, "std": std}
    if with_mean:
        ins["mean"] = mean
    return Case(f"channel_normalize {'bwd' if backward else 'fwd'} npix{npix} Cs{Cs} Cl{Cl} "
                f"{'mean' if with_mean else 'nomean'} d0={d0}", "channel_normalize" + ("_bwd" if backward else ""), why,
                ins, {"y": sentinel((npix, Cs))}, call, expect, stock)


# ====================================================================================================== scaled_tanh
def _stanh_x(npix, Cs, Cl):
    x = randn(61, (npix, Cs), 300.0)
    x[0, :3] = (0.0, 5000.0, -5000.0)      # tanh(5000 / 255) == 1 in fp32: 1 - t*t is exactly 0
    x[:, Cl:] = np.nan
    return x


def case_stanh(npix, Cs, Cl, backward, why):
    """t = tanhf(x / 255): the quotient's rounding moves the argument by u |a|, and a tanh'(a) <= tanh(a), so it
    costs u |t|; the library adds TANH_ULP ulp <= 10 u |t|: t~ = t (1 + theta), |theta| <= 11 u.
    forward t * 150 + 127.5: the product 150 |t| (11 u + u), the sum u |y|: <= 13 u (150 |t| + 127.5): c = 13,
    M = 150 |t| + 127.5.
    backward ((gy * 150) * (1 - t*t)) / 255: t*t carries 22 u + u = 23 u t^2, the difference adds u |1 - t^2|, the
    three other operations 3 u relative: <= u |gy| (150/255) (23 t^2 + 4 (1 - t^2)) <= 27 u |gy| (150/255) (1 + t^2):
    c = 27, M = |gy| (150/255) (1 + t^2), the terms of 1 - t*t (at saturation the result is exactly 0 and y64 is
    ~1e-17 |gy|: far inside).  Padding lanes +0."""
    x = _stanh_x(npix, Cs, Cl)
    gy = randn(62, (npix, Cs))
    gy[:, Cl:] = np.nan

    def expect(mutate=None):
        t = np.tanh(x[:, :Cl].astype(f64) / 255.0)
        if backward:
            g = gy[:, :Cl].astype(f64)
            y = g * 150.0 * (1 - t * t) / 255.0
            tol = gamma(27) * np.abs(g) * (150.0 / 255.0) * (1 + t * t)
        else:
            y = t * 150.0 + 127.5
            tol = gamma(13) * (150.0 * np.abs(t) + 127.5)
        full_y, full_t = np.zeros((npix, Cs)), np.zeros((npix, Cs))
        full_y[:, :Cl], full_t[:, :Cl] = y, tol
        lanes = window((npix, Cs), slice(None), slice(0, Cl))
        e = Exp(sentinel((npix, Cs))).bound(full_y, full_t, lanes)
        e.exact(x if mutate == "cs_for_cl" else f32(0), ~lanes)
        return {"y": e}

    def stock():
        t = torch.tanh(_t(x)[:, :Cl] / 255)
        y = ((_t(gy)[:, :Cl] * 150) * (1 - t * t)) / 255 if backward else t * 150 + 127.5
        return {"y": F.pad(y, (0, Cs - Cl)).contiguous().numpy()}

    def call(ops, p):
        if backward:
            ops._call("vst_scaled_tanh_bwd", p["x"], p["gy"], p["y"], npix, Cs, Cl, ops._stream())
        else:
            ops._call("vst_scaled_tanh_fwd", p["x"], p["y"], npix, Cs, Cl, ops._stream())

    ins = {"x": x, "gy": gy} if backward else {"x": x}
    return Case(f"scaled_tanh {'bwd' if backward else 'fwd'} npix{npix} Cs{Cs} Cl{Cl}",
                "scaled_tanh" + ("_bwd" if backward else ""), why, ins, {"y": sentinel((npix, Cs))}, call, expect,
                stock)


# ================================================================================================ act_fwd / act_bwd
ACTS = (("none", 0.0), ("relu", 0.0), ("lrelu", 0.2), ("tanh", 0.0))
_EDGE = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -120, -2.0 ** -120, 1e-3, -1e-3], f32)


def case_act_fwd(act, slope, n, why, nan=False):
    """none: the input's bits.  relu v > 0 ? v : 0: a select, bit for bit (-0, -inf and NaN -> +0).  lrelu
    v > 0 ? v : v * slope: one IEEE product, bit for bit against numpy fp32.  tanh: TANH_ULP ulp of tanh in fp64."""
    x = randn(71, (n,))
    if n >= 8:
        x[:8] = _EDGE
    else:
        x[:4] = (0.0, -0.0, np.inf, -1e-3)
    if nan:
        x[1::3] = np.nan
    sl = f32(slope)

    def expect(mutate=None):
        e = Exp(sentinel((n,)))
        with np.errstate(invalid="ignore"):
            if act == "none":
                e.exact(x)
            elif act == "relu":
                e.exact(np.where(x > 0, x, f32(0)))
            elif act == "lrelu":
                e.exact(np.where(x > 0, x, x * sl))
            else:
                t = np.tanh(x.astype(f64))
                e.bound(t, TANH_ULP * ulp32(t))
        return {"y": e}

    def stock():
        xs = _t(x)
        y = {"none": lambda: xs.clone(), "relu": lambda: torch.where(xs > 0, xs, torch.zeros_like(xs)),
             "lrelu": lambda: F.leaky_relu(xs, slope), "tanh": lambda: torch.tanh(xs)}[act]()
        return {"y": y.numpy()}

    def call(ops, p):
        ops._call("vst_act_fwd", p["x"], p["y"], n, ops.ACT[act], float(slope), ops._stream())

    return Case(f"act_fwd {act} n{n}" + (" nan" if nan else ""), "act_fwd", why, {"x": x}, {"y": sentinel((n,))}, call,
                expect, stock, inplace=("y", "x"))


def case_act_bwd(act, slope, n, why):
    """dx = gy * act'(y) from the OUTPUT y: none 1, relu y > 0 ? 1 : 0, lrelu y > 0 ? 1 : slope (one IEEE product
    each, bit for bit, the sign of a zero included); tanh gy * (1 - y*y): y*y u y^2, the difference u |1 - y^2|, the
    product u: <= u |gy| (y^2 + 2 |1 - y^2|) <= 2 u |gy| (1 + y^2): c = 2, M = |gy| (1 + y^2)."""
    gy = randn(72, (n,))
    y = randn(73, (n,))
    if act == "tanh":
        y = np.tanh(y).astype(f32)
        y[:4] = (1.0, -1.0, 0.0, -0.0)
    else:
        y[:5] = _EDGE[:5] if act != "relu" else (0.0, -0.0, np.inf, 1e-3, 2.0 ** -120)
    sl = f32(slope)

    def expect(mutate=None):
        e = Exp(sentinel((n,)))
        if act == "tanh":
            g, t = gy.astype(f64), y.astype(f64)
            e.bound(g * (1 - t * t), gamma(2) * np.abs(g) * (1 + t * t))
        else:
            d = {"none": np.ones(n, f32), "relu": np.where(y > 0, f32(1), f32(0)),
                 "lrelu": np.where(y > 0, f32(1), sl)}[act]
            e.exact(gy * d)
        return {"dx": e}

    def stock():
        g, t = _t(gy), _t(y)
        d = {"none": lambda: torch.ones_like(t), "relu": lambda: (t > 0).float(),
             "lrelu": lambda: torch.where(t > 0, torch.ones_like(t), torch.full_like(t, slope)),
             "tanh": lambda: 1 - t * t}[act]()
        return {"dx": (g * d).numpy()}

    def call(ops, p):
        ops._call("vst_act_bwd", p["gy"], p["y"], p["dx"], n, ops.ACT[act], float(slope), ops._stream())

    return Case(f"act_bwd {act} n{n}", "act_bwd", why, {"gy": gy, "y": y}, {"dx": sentinel((n,))}, call, expect, stock)


# ======================================================================================================= upsample2x
def case_up2_fwd(N, H, W, C, why):
    x = coded(7, (N, H, W, C))

    def expect(mutate=None):
        n, oh, ow, c = np.indices((N, 2 * H, 2 * W, C))
        if mutate == "swap_hw":
            src = ((n * W + (ow >> 1)) * H + (oh >> 1)) * C + c
        else:
            src = ((n * H + (oh >> 1)) * W + (ow >> 1)) * C + c
        return {"y": Exp(sentinel((N, 2 * H, 2 * W, C))).exact(x.reshape(-1)[src])}

    def stock():
        y = F.interpolate(_t(x).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        return {"y": y.permute(0, 2, 3, 1).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_upsample2x_fwd", p["x"], p["y"], N, H, W, C, ops._stream())

    return Case(f"upsample2x fwd N{N} H{H} W{W} C{C}", "upsample2x", why, {"x": x},
                {"y": sentinel((N, 2 * H, 2 * W, C))}, call, expect, stock)


def case_up2_bwd(N, H, W, C, why):
    """gx = g00 + g01 + g10 + g11: three adds, c = 3, M = sum |g|."""
    g = randn(81, (N, 2 * H, 2 * W, C))

    def expect(mutate=None):
        q = g.astype(f64).reshape(N, H, 2, W, 2, C)
        parts = [q[:, :, 0, :, 0], q[:, :, 0, :, 1], q[:, :, 1, :, 0], q[:, :, 1, :, 1]]
        if mutate == "up2_bwd_three_of_four":
            parts = parts[:3]
        return {"gx": Exp(sentinel((N, H, W, C))).bound(sum(parts), gamma(3) * np.abs(q).sum(axis=(2, 4)))}

    def stock():
        y = F.avg_pool2d(_t(g).permute(0, 3, 1, 2), 2) * 4
        return {"gx": y.permute(0, 2, 3, 1).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_upsample2x_bwd", p["gy"], p["gx"], N, H, W, C, ops._stream())

    return Case(f"upsample2x bwd N{N} H{H} W{W} C{C}", "upsample2x_bwd", why, {"gy": g}, {"gx": sentinel((N, H, W, C))},
                call, expect, stock)


# ========================================================================================================= maxpool2
TIE_PATTERNS = ((1, 1, 1, 1), (0, 1, 1, 1), (0, 0, 1, 1), (0, 0, 0, 1))     # the first maximum at position 0, 1, 2, 3


def _maxpool_x(N, H, W, Cs, data):
    Ho, Wo = H // 2, W // 2
    if data == "coded":
        x = coded(10, (N, H, W, Cs))
    else:
        x = (rng(91).integers(-3, 4, (N, H, W, Cs)) / 2.0).astype(f32)      # half-integers: frequent ties
        for k, pat in enumerate(TIE_PATTERNS):                               # window (0, 0, 0), channel k
            x[0, 0:2, 0:2, k] = np.array(pat, f32).reshape(2, 2) * 2.5
        if data == "nan":
            x[0, 0, 0, 0] = np.nan                       # NaN first, larger values after it: NaN stays
            if Wo > 1:
                x[0, 1, 2, 1] = x[0, 0, 3, 1] = np.nan   # two NaNs in one window: the later one is the argmax
            x[N - 1, 2 * Ho - 1, 2 * Wo - 1, Cs - 1] = np.nan    # NaN last
    x[:, 2 * Ho:], x[:, :, 2 * Wo:] = np.nan, np.nan     # floor mode: the odd last row / column is not read
    return x


def _maxpool_scan(x, N, H, W, Cs, mutate):
    """The scan (0,0), (0,1), (1,0), (1,1): a later element wins if strictly greater or NaN (ATen's CPU rule)."""
    Ho, Wo = H // 2, W // 2
    b = [x[:, i:2 * Ho:2, j:2 * Wo:2] for i in (0, 1) for j in (0, 1)]
    m, am = b[0].copy(), np.zeros(b[0].shape, np.int8)
    with np.errstate(invalid="ignore"):
        for k in (1, 2, 3):
            pick = ((b[k] >= m) if mutate == "tie_last_wins" else (b[k] > m)) | np.isnan(b[k])
            m, am = np.where(pick, b[k], m), np.where(pick, k, am)
    return m, am


def case_maxpool_fwd(N, H, W, Cs, data, why):
    x = _maxpool_x(N, H, W, Cs, data)
    Ho, Wo = H // 2, W // 2

    def expect(mutate=None):
        return {"y": Exp(sentinel((N, Ho, Wo, Cs))).exact(_maxpool_scan(x, N, H, W, Cs, mutate)[0])}

    def stock():
        y = F.max_pool2d(_t(x).permute(0, 3, 1, 2), 2)
        return {"y": y.permute(0, 2, 3, 1).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_maxpool2_fwd", p["x"], p["y"], N, H, W, Cs, ops._stream())

    return Case(f"maxpool2 fwd N{N} {H}x{W} Cs{Cs} {data}", "maxpool2", why, {"x": x},
                {"y": sentinel((N, Ho, Wo, Cs))}, call, expect, stock)


def case_maxpool_bwd(N, H, W, Cs, data, why):
    """gx = gy of the window at its argmax, +0 elsewhere (the unread odd row / column included): bit for bit."""
    x = _maxpool_x(N, H, W, Cs, "ties" if data == "coded" else data)
    Ho, Wo = H // 2, W // 2
    gy = coded(11, (N, Ho, Wo, Cs))

    def expect(mutate=None):
        _, am = _maxpool_scan(x, N, H, W, Cs, mutate)
        gx = np.zeros((N, H, W, Cs), f32)
        for k in range(4):
            gx[:, k // 2:2 * Ho:2, k % 2:2 * Wo:2] = np.where(am == k, gy, f32(0))
        return {"gx": Exp(sentinel((N, H, W, Cs))).exact(gx)}

    def stock():
        xs = _t(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.max_pool2d(xs, 2).backward(_t(gy).permute(0, 3, 1, 2))
        return {"gx": xs.grad.permute(0, 2, 3, 1).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_maxpool2_bwd", p["gy"], p["x"], p["gx"], N, H, W, Cs, ops._stream())

    return Case(f"maxpool2 bwd N{N} {H}x{W} Cs{Cs} {data}", "maxpool2_bwd", why, {"gy": gy, "x": x},
                {"gx": sentinel((N, H, W, Cs))}, call, expect, stock)


# ========================================================================================================= gram_sym
def case_gram_sym(C, why):
    """S = (dG + dG^T) * scale: two roundings, c = 2, M = (|dG| + |dG^T|) scale."""
    dG = randn(101, (C, C))
    scale = cfloat(1.0 / 7.0)

    def expect(mutate=None):
        d = dG.astype(f64)
        other = d if mutate == "sym_no_transpose" else d.T
        return {"S": Exp(sentinel((C, C))).bound((d + other) * scale, gamma(2) * (np.abs(d) + np.abs(d.T)) * scale)}

    def stock():
        return {"S": ((_t(dG) + _t(dG).t()) * scale).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_gram_sym", p["dG"], p["S"], C, scale, ops._stream())

    return Case(f"gram_sym C{C}", "gram_sym", why, {"dG": dG}, {"S": sentinel((C, C))}, call, expect, stock)


# ================================================================================================ concat_label_nhwc
def case_concat_label(N, H, W, Cx, Cl, cs, why):
    x, lab = coded(8, (N, Cx, H, W)), coded(9, (N, Cl))

    def expect(mutate=None):
        n, h, w, c = np.indices((N, H, W, cs))
        pq = w * H + h if mutate == "swap_hw" else h * W + w
        k0 = Cx + 1 if mutate == "c0_plus_one" else Cx      # the label block one lane late
        vx = x.reshape(-1)[((n * Cx + np.minimum(c, Cx - 1)) * H * W + pq)]
        vl = lab.reshape(-1)[n * Cl + np.clip(c - k0, 0, Cl - 1)]
        y = np.where(c < Cx, vx, np.where((c >= k0) & (c < k0 + Cl), vl, f32(0)))
        return {"y": Exp(sentinel((N, H, W, cs))).exact(y.astype(f32))}

    def stock():
        y = torch.cat([_t(x), _t(lab)[:, :, None, None].expand(N, Cl, H, W)], 1).permute(0, 2, 3, 1)
        return {"y": F.pad(y, (0, cs - Cx - Cl)).contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_concat_label_nhwc", p["x"], p["label"], p["y"], N, Cx, Cl, H, W, cs, ops._stream())

    return Case(f"concat_label N{N} H{H} W{W} Cx{Cx} Cl{Cl} cs{cs}", "concat_label_nhwc", why, {"x": x, "label": lab},
                {"y": sentinel((N, H, W, cs))}, call, expect, stock)


# ================================================================================================== resize_bilinear
def _resize_geom(Hi, Ho, align):
    """The kernel's source row and weights in fp32 (csrc/temporal.hip is compiled with contraction off):
    f = sh (o + 0.5) - 0.5 clamped at 0, y0 = min(int(f), Hi - 1), y1 = y0 + (y0 < Hi - 1), l = f - y0, h = 1 - l."""
    o = np.arange(Ho, dtype=f32)
    if align:        # MUTATION resize_align_corners
        f = (f32(Hi - 1) / f32(max(Ho - 1, 1))) * o
    else:
        f = (f32(Hi) / f32(Ho)) * (o + f32(0.5)) - f32(0.5)
    f = np.where(f < 0, f32(0), f).astype(f32)
    y0 = np.minimum(f.astype(np.int64), Hi - 1)
    y1 = y0 + (y0 < Hi - 1)
    l = (f - y0.astype(f32)).astype(f32)
    return y0, y1, l, (f32(1) - l).astype(f32)


def case_resize(Hi, Wi, Ho, Wo, with_mult, why, N=2, C=3):
    """Two tiers, as tests/sampling_ref.py.  tight: rows, columns and weights from the fp32 restatement, products
    and sums in fp64; a corner's value passes a product, a sum, a product and a sum (and the multiplier): c = 4 (5),
    M = sum |w_i x_i| |mult|.  independent: F.interpolate in fp64; on top of the tight bound it allows for the fp32
    source position (the scale's division, a product, a difference: |df| <= 3 u (Hi + 1), likewise in x), which
    moves the value by at most |df| times the largest step between neighbours, <= 2 max |x| of the plane.
    Same size and no multiplier: weights 1 and 0, exact: the input's bits."""
    x = randn(111, (N, C, Hi, Wi), 4.0)
    mult = np.array([0.5, 2.0, 1.25], f32)[:C] if with_mult else None

    def expect(mutate=None):
        align = mutate == "resize_align_corners"
        y0, y1, ly, hy = _resize_geom(Hi, Ho, align)
        x0, x1, lx, hx = _resize_geom(Wi, Wo, align)
        X = x.astype(f64)
        ly, hy = ly.astype(f64)[:, None], hy.astype(f64)[:, None]
        lx, hx = lx.astype(f64)[None, :], hx.astype(f64)[None, :]
        g = lambda yy, xx: X[:, :, yy][:, :, :, xx]
        terms = [hy * hx * g(y0, x0), hy * lx * g(y0, x1), ly * hx * g(y1, x0), ly * lx * g(y1, x1)]
        m = mult.astype(f64)[None, :, None, None] if with_mult else 1.0
        y = sum(terms) * m
        M = sum(np.abs(t) for t in terms) * np.abs(m)
        e = Exp(sentinel((N, C, Ho, Wo)))
        if (Hi, Wi) == (Ho, Wo) and not with_mult and not align:
            return {"y": e.exact(x)}
        tol = gamma(5 if with_mult else 4) * M
        e.bound(y, tol, restated=True)
        yi = F.interpolate(_t(X), size=(Ho, Wo), mode="bilinear", align_corners=align).numpy() * m
        pos = 3 * U * ((Hi + 1) + (Wi + 1)) * 2 * np.abs(X).max(axis=(2, 3), keepdims=True) * np.abs(m)
        e.bound(yi, tol + pos, more=True)
        return {"y": e}

    def stock():
        y = F.interpolate(_t(x), size=(Ho, Wo), mode="bilinear", align_corners=False)
        if with_mult:
            y = y * _t(mult)[None, :, None, None]
        return {"y": y.contiguous().numpy()}

    def call(ops, p):
        ops._call("vst_resize_bilinear", p["x"], _ptr(p, "mult"), p["y"], N, C, Hi, Wi, Ho, Wo, ops._stream())

    ins = {"x": x, "mult": mult} if with_mult else {"x": x}
    return Case(f"resize_bilinear ({Hi},{Wi})->({Ho},{Wo})" + (" mult" if with_mult else ""), "resize_bilinear", why,
                ins, {"y": sentinel((N, C, Ho, Wo))}, call, expect, stock)


# ======================================================================================================== adam_step
ADAM_LR, ADAM_EPS = 2e-4, 1e-8


def case_adam(betas, step, n, why):
    """One step from arbitrary fp32 states.  The reference is fp64 with the scalars as the C ABI receives them
    (cfloat) and the two bias corrections rounded to float as the host code does; torch.optim.Adam gets the same
    scalars (it would otherwise form 1 - beta in double from the unrounded beta: 1 - 0.999 and 1 - float(0.999)
    differ by 1.3e-5 relative, the cancellation's doing, not a rounding of the kernel's).  w = 1 - b1, 1 - b2: exact
    for these betas (Sterbenz), counted as a rounding all the same.
      m' (either arm of the lerp: w, a difference, a product with w or 1 - w, a sum): c = 4,
         M_m = |m| + w (|g| + |m|) for w < 0.5, else |g| + (1 - w) (|g| + |m|); b1 = 0: m' == g bit for bit.
      v' = v b2 + (1 - b2) (g g): at most four roundings on a term: c = 4, M_v = v' (every term >= 0).
      p' = p - (lr / bc1) (m' / denom), denom = sqrtf(v') / bc2 + eps: v' 4 u, its root 2 u + u, the quotient u, the
         sum u: denom <= 5 u relative; m' 4 u M_m; the quotient, lr / bc1 and the product 3 u: the update carries
         <= u s (4 M_m + 8 |m'|) / denom <= 12 u s M_m / denom, the final difference u |p'|: c = 13,
         M_p = |p| + s M_m / denom, s = lr / bc1.
    Elements with g = m = v = 0 leave p's bits unchanged."""
    b1, b2 = cfloat(betas[0]), cfloat(betas[1])
    lr, eps = cfloat(ADAM_LR), cfloat(ADAM_EPS)
    r = rng(121 + n)
    p0, g = randn(122, (n,)), randn(123, (n,), 0.1)
    m0 = (r.standard_normal(n) * 0.05).astype(f32)
    v0 = (r.random(n) * 0.01).astype(f32)
    zero = np.arange(n) % 7 == 3
    g[zero], m0[zero], v0[zero] = 0, 0, 0
    small = np.arange(n) % 7 == 5          # sqrt(v') of the order of eps: where eps sits decides the step
    g[small], m0[small], v0[small] = g[small] * f32(1e-6), m0[small] * f32(1e-4), f32(1e-14)
    one_minus = lambda b: float(f32(1) - f32(b))

    def expect(mutate=None):
        G, M0, V0, P0 = (a.astype(f64) for a in (g, m0, v0, p0))
        w = one_minus(b1)
        m1 = M0 + w * (G - M0)
        Mm = np.abs(M0) + w * (np.abs(G) + np.abs(M0)) if w < 0.5 else np.abs(G) + (1 - w) * (np.abs(G) + np.abs(M0))
        v1 = V0 * b2 + one_minus(b2) * G * G
        bc1 = float(f32(1.0 - b1 ** step))
        bc2s = float(f32(np.sqrt(1.0 - b2 ** step)))
        if mutate == "no_bias_correction":
            bc1, bc2s = 1.0, 1.0
        denom = np.sqrt(v1 / (bc2s * bc2s) + eps) if mutate == "eps_inside_sqrt" else np.sqrt(v1) / bc2s + eps
        s = lr / bc1
        p1 = P0 - s * (m1 / denom)
        em, ev, ep = Exp(m0), Exp(v0), Exp(p0)
        if b1 == 0.0:
            em.exact((m0 + (g - m0)) if mutate == "lerp_one_sided" else g)
        else:
            em.bound(m1, gamma(4) * Mm)
        ev.bound(v1, gamma(4) * v1)
        Mp = np.abs(P0) + s * Mm / denom
        ep.bound(p1, gamma(13) * Mp, ~zero)
        ep.exact(p0, zero)
        return {"p": ep, "m": em, "v": ev}

    def stock():
        pt = _t(p0.copy()).requires_grad_(True)
        opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        opt.state[pt] = dict(step=torch.tensor(float(step - 1)), exp_avg=_t(m0.copy()), exp_avg_sq=_t(v0.copy()))
        pt.grad = _t(g.copy())
        opt.step()
        st = opt.state[pt]
        return {"p": pt.detach().numpy(), "m": st["exp_avg"].numpy(), "v": st["exp_avg_sq"].numpy()}

    def call(ops, pp):
        ops._call("vst_adam_step", pp["p"], pp["g"], pp["m"], pp["v"], n, ADAM_LR, betas[0], betas[1], ADAM_EPS, step,
                  ops._stream())

    return Case(f"adam_step betas{betas} step{step} n{n}", "adam_step", why, {"g": g}, {"p": p0, "m": m0, "v": v0},
                call, expect, stock)


# ======================================================================================================== the table
def _build_cases():
    N, H, W = BASE
    cs_ = []
    part = "560 elements: two full 256-thread blocks and a partial third"
    tiny = "fewer than 64 elements: one partial wave"
    for fn in (case_nchw_to_nhwc, case_nhwc_to_nchw):
        cs_ += [fn(N, H, W, 5, 8, "pad lanes 5..7; " + part),
                fn(N, H, W, 5, 12, "cs > cpad(C): a whole padding channel group"),
                fn(N, H, W, 4, 4, "no padding lane"),
                fn(N, H, W, 1, 4, "one logical channel"),
                fn(1, 1, 1, 1, 4, tiny)]
    cs_ += [case_weight_pack(m) for m in PACK_MODES]
    for src in ("nchw", 4, 8):
        srcwhy = "raft_prep_k" if src == "nchw" else f"raft_prep_nhwc_k, source stride {src}"
        cs_ += [case_raft_prep(N, H, W, src, (1, 2, 0, 3), srcwhy + ": unequal pads on every side; partial last block"),
                case_raft_prep(N, H, W, src, (0, 0, 0, 0), srcwhy + ": no padding"),
                case_raft_prep(N, 2, W, src, (0, 0, 3, 0), srcwhy + ": a pad larger than the image (H = 2)")]
    cs_ += [case_raft_prep(1, 1, 1, "nchw", (0, 0, 0, 0), tiny), case_raft_prep(1, 1, 1, 4, (0, 0, 0, 0), tiny)]
    cs_ += [case_add_relu(4, "one float4: " + tiny), case_add_relu(1100, "275 float4s: a partial second block"),
            case_add_relu(8, "NaN convention: relu(NaN) = +0", nan=True)]
    for args, why in (((12, 4, 16, 8, 4, 70), "float4 route: every stride, offset and count 4-aligned"),
                      ((12, 2, 16, 5, 6, 70), "scalar route: unaligned offsets; 420 elements: a partial second block"),
                      ((8, 0, 8, 4, 3, 70), "scalar route only because nc % 4 != 0"),
                      ((12, 4, 16, 8, 4, 1), "float4 route, " + tiny)):
        cs_.append(case_copy_channels(*args, why + " -> " + copy_route(*args[:5])))
    cs_ += [case_ctx_split(8, 4, 16, 28, 37, "both halves; 444 elements: a partial second block"),
            case_ctx_split(8, 4, 16, 28, 1, tiny)]
    cs_ += [case_flow4(2, 5, 7, "70 pixels, two images"), case_flow4(1, 1, 1, tiny),
            case_flow4(2, 15, 20, "600 pixels: a partial third block")]
    cs_ += [case_coords_update(2, 5, 7, 4, "delta stride 4"), case_coords_update(2, 5, 7, 8, "delta stride 8"),
            case_coords_update(2, 15, 20, 4, "600 pixels: a partial third block"),
            case_coords_update(1, 1, 1, 4, tiny)]
    cs_ += [case_motion(6, 8, 28, 12, 37, "window [12, 20) of both buffers; 296 elements: a partial second block"),
            case_motion(6, 8, 28, 12, 1, tiny)]
    for fn in (case_gru_reset, case_gru_update):
        cs_ += [fn(12, 40, 37, "xcs > 3 hd; gates at +-100 and 0; 444 elements: a partial second block"),
                fn(8, 24, 3, "xcs == 3 hd; " + tiny)]
    for Cs, Cl in ((4, 3), (8, 5)):
        for mean in (True, False):
            for d0 in (255.0, 1.0):
                cs_.append(case_chnorm(70, Cs, Cl, mean, d0, False,
                                       f"{'mean' if mean else 'mean == NULL'} arm, d0 {d0}, {Cs - Cl} padding lanes"
                                       + ("; " + part if Cs == 8 else "; a partial second block")))
        for d0 in (255.0, 1.0):
            cs_.append(case_chnorm(70, Cs, Cl, True, d0, True, f"BWD = 1, d0 {d0}, {Cs - Cl} padding lanes"))
        cs_ += [case_stanh(70, Cs, Cl, False, "BWD = 0: saturation and 0"),
                case_stanh(70, Cs, Cl, True, "BWD = 1: 1 - t*t exactly 0 at saturation")]
    cs_ += [case_chnorm(1, 4, 3, True, 255.0, False, tiny), case_chnorm(1, 4, 3, True, 255.0, True, tiny),
            case_stanh(1, 4, 3, False, tiny), case_stanh(1, 4, 3, True, tiny)]
    for act, slope in ACTS:
        cs_ += [case_act_fwd(act, slope, 4, f"{act}: one float4, " + tiny),
                case_act_fwd(act, slope, 1100, f"{act}: +-0, +-inf and values either side of 0; a partial second block"),
                case_act_bwd(act, slope, 5, f"{act}: " + tiny),
                case_act_bwd(act, slope, 1100, f"{act}: +-0 and values either side of 0; a partial fifth block")]
    cs_.append(case_act_fwd("relu", 0.0, 12, "NaN convention: relu(NaN) = +0", nan=True))
    cs_ += [case_up2_fwd(N, H, W, 8, "560 input float4 x 4 outputs; a partial last block"), case_up2_fwd(1, 1, 1, 4, tiny),
            case_up2_bwd(N, H, W, 8, "140 float4 threads"), case_up2_bwd(1, 1, 1, 4, tiny),
            case_up2_bwd(N, H, W, 16, "280 float4 threads: a partial second block")]
    cs_ += [case_maxpool_fwd(2, 11, 13, 8, "coded", "floor mode (odd H and W); addressing; 480 outputs"),
            case_maxpool_fwd(2, 11, 13, 8, "ties", "floor mode; a window per tie pattern"),
            case_maxpool_fwd(2, 11, 13, 8, "nan", "NaN convention: a NaN in the window wins"),
            case_maxpool_fwd(1, 2, 2, 4, "ties", "one window per channel, " + tiny),
            case_maxpool_bwd(2, 11, 13, 8, "ties", "floor mode; the first maximum gets the gradient; 2288 threads"),
            case_maxpool_bwd(2, 11, 13, 8, "nan", "NaN convention: the last NaN of the window is the argmax"),
            case_maxpool_bwd(1, 2, 2, 4, "ties", "one window per channel, " + tiny)]
    cs_ += [case_gram_sym(5, "25 elements: " + tiny.split(":")[0]), case_gram_sym(33, "1089 elements: a partial fifth block")]
    cs_ += [case_concat_label(N, H, W, 3, 2, 8, "x | label | 3 zero lanes; " + part),
            case_concat_label(N, H, W, 3, 2, 12, "cs > cpad(Cx + Cl)"),
            case_concat_label(N, H, W, 4, 5, 12, "label block starts 4-aligned and crosses a group"),
            case_concat_label(1, 1, 1, 3, 2, 8, tiny)]
    for (hi, wi), (ho, wo), why in (((5, 7), (5, 7), "same size: weights 1 and 0"),
                                    ((5, 7), (11, 4), "up in H, down in W; clamped first and last rows; 264 outputs: a partial second block"),
                                    ((1, 7), (3, 14), "one source row: y1 == y0 everywhere"),
                                    ((8, 8), (2, 2), "4x down: half-integer source positions, " + tiny.split(":")[0])):
        for mult in (False, True):
            cs_.append(case_resize(hi, wi, ho, wo, mult, why + ("; per-channel multiplier" if mult else "; mult == NULL")))
    for betas, why in (((0.9, 0.999), "the w < 0.5 arm of the lerp"), ((0.5, 0.999), "w == 0.5: the other arm"),
                       ((0.0, 0.99), "w == 1: m' == g bit for bit")):
        for step in (1, 7, 100000):
            for n in (1, 255, 1025):
                size = {1: tiny, 255: "one block less a thread", 1025: "a partial fifth block"}[n]
                cs_.append(case_adam(betas, step, n, f"{why}; step {step}; n {n}: {size}"))
    return cs_


CASES = _build_cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES), "case names must be unique"
KERNELS = sorted({c.kernel for c in CASES})


def case_ids(cases=None):
    return [c.name.replace(" ", "_") for c in (CASES if cases is None else cases)]
