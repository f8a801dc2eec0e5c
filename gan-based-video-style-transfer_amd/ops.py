"""Tensor-level wrappers over the C ABI (include/vst_hip.h).

Every function launches on torch's current HIP stream, takes/returns torch tensors that live on the
GPU, and raises on a non-zero status.  Activations are NHWC fp32 with a channel stride that is a
multiple of 4 (``cpad``); images are NHWC4.  There is no CPU fallback: a CPU tensor is an error.
"""
import ctypes
import os
import threading

import torch

from . import _lib

_C = _lib.CONSTANTS  # the VST_* enum values of include/vst_hip.h
ACT = {"none": _C["VST_ACT_NONE"], "relu": _C["VST_ACT_RELU"], "lrelu": _C["VST_ACT_LRELU"], "tanh": _C["VST_ACT_TANH"]}
PAD = {"zero": _C["VST_PAD_ZERO"], "reflect": _C["VST_PAD_REFLECT"]}
PACK_KC, PACK_CK, PACK_OK, PACK_IK, PACK_IKF, PACK_SOK = (
    _C["VST_PACK_" + n] for n in ("KC", "CK", "OK", "IK", "IKF", "SOK"))
# the conv kernels consume: forward conv -> PACK_OK, data-gradient / transposed conv -> PACK_IK
PACK_FWD, PACK_DGRAD = PACK_OK, PACK_IK
EUNSUPPORTED = _C["VST_EUNSUPPORTED"]
IN_EPS = 1e-5


def cpad(c):
    return (c + 3) // 4 * 4


def lib():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev_check(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise RuntimeError("vst ops require GPU tensors (no CPU fallback)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("vst ops require contiguous float32 tensors")


def _call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        _lib.check(rc, name)


# ------------------------------------------------------------------------------------ layout
def nchw_to_nhwc(x, cs=None):
    _dev_check(x)
    N, C, H, W = x.shape
    cs = cs or cpad(C)
    y = torch.empty((N, H, W, cs), device=x.device, dtype=torch.float32)
    _call("vst_nchw_to_nhwc", _p(x), _p(y), N, C, H, W, cs, _stream())
    return y


def nhwc_to_nchw(x, c):
    _dev_check(x)
    N, H, W, cs = x.shape
    y = torch.empty((N, c, H, W), device=x.device, dtype=torch.float32)
    _call("vst_nhwc_to_nchw", _p(x), _p(y), N, c, H, W, cs, _stream())
    return y


def _pack_shape(mode, O, I_, R, S, Op=None, Ip=None):
    Op, Ip = Op or cpad(O), Ip or cpad(I_)
    return {PACK_KC: (R, S, Ip, Op), PACK_CK: (R, S, Op, Ip), PACK_OK: (Op, R, S, Ip),
            PACK_IK: (Ip, R, S, Op), PACK_IKF: (Ip, R, S, Op), PACK_SOK: (S * Op, R, 1, Ip)}[mode]


class PackBatch:
    """A network's weight packs as ONE launch (vst_weight_pack_batch).  Inside ``with PackBatch()``
    every weight_pack / convT3s2_phase_packs call allocates its outputs and records a job instead of
    launching; leaving the block packs them all.  ``run()`` re-packs every recorded job in place
    from the (updated) weights — after an optimizer step the pack set is refreshed by one kernel
    instead of one launch per pack.  The job sources are the live parameter tensors (views into the
    network's flat buffer), so the outputs stay valid objects across refreshes."""
    _active = None
    REC = 168  # sizeof(PackJob), include/vst_hip.h

    def __init__(self):
        self.jobs, self.blocks, self.copies, self._dev = [], 0, [], None

    def __enter__(self):
        self._prev, PackBatch._active = PackBatch._active, self
        return self

    def __exit__(self, *exc):
        PackBatch._active = self._prev
        if exc[0] is None and self.jobs:
            self.run()
        return False

    def add(self, w, mode, O, I_, R, S, strides, tr=None, ts=None, Op=None, Ip=None):
        import struct
        Op, Ip = Op or cpad(O), Ip or cpad(I_)
        shape = _pack_shape(mode, O, I_, R, S, Op, Ip)
        out = torch.empty(shape, device=w.device, dtype=torch.float32)
        split = torch.empty((3,) + shape, device=w.device, dtype=torch.bfloat16)
        out.vst_split = split
        total = out.numel()
        tr = list(tr) if tr is not None else [-1]  # -1: identity tap map (any R / S)
        ts = list(ts) if ts is not None else [-1]
        if len(tr) > 8 or len(ts) > 8:
            raise ValueError("PackBatch: explicit tap maps need R, S <= 8")
        rec = struct.pack("<3Q8i2q4q8i8i", w.data_ptr(), out.data_ptr(), split.data_ptr(), O, I_, R, S,
                          Op, Ip, mode, 0, total, self.blocks, *strides,
                          *(tr + [0] * (8 - len(tr))), *(ts + [0] * (8 - len(ts))))
        self.jobs.append((rec, w, out, split))
        self.blocks += (total + 255) // 256
        self._dev = None
        return out

    def copy_into(self, dst, src):
        """dst[:n] = src on every run (padded bias vectors)."""
        self.copies.append((dst, src))
        dst[:src.numel()].copy_(src)

    def run(self):
        if self._dev is None:
            buf = b"".join(j[0] for j in self.jobs)
            self._dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(self.jobs[0][1].device)
        _call("vst_weight_pack_batch", _p(self._dev), len(self.jobs), self.blocks, _stream())
        for dst, src in self.copies:
            dst[:src.numel()].copy_(src)


def weight_pack(w, mode, transposed=False, Op=None, Ip=None):
    """Pack a PyTorch conv weight for the GEMM kernels (see vst_weight_pack).  For a
    ConvTranspose2d weight [Ci][Co][R][S] pass transposed=True: dims are then (O=Ci, I=Co).
    Op / Ip: padded channel counts (default cpad; 8 lets a 3-channel side use the split-bf16
    kernels, whose K chunks are 8 channels deep)."""
    _dev_check(w)
    O, I_, R, S = w.shape
    Op, Ip = Op or cpad(O), Ip or cpad(I_)
    pb = PackBatch._active
    if pb is not None:
        return pb.add(w, mode, O, I_, R, S, (I_ * R * S, R * S, S, 1), Op=Op, Ip=Ip)
    shape = _pack_shape(mode, O, I_, R, S, Op, Ip)
    out = torch.empty(shape, device=w.device, dtype=torch.float32)
    # the split-arithmetic conv paths read the pack as three bf16 planes (written in the same pass)
    split = torch.empty((3,) + shape, device=w.device, dtype=torch.bfloat16)
    _call("vst_weight_pack_split", _p(w), _p(out), _p(split), O, I_, R, S, Op, Ip, mode, _stream())
    out.vst_split = split
    return out


# --------------------------------------------------------------------------------------- conv
class LaunchProbe:
    """Measurement hook (bench.py): HIP events around the launches of one conv op ("fwd" =
    vst_conv2d_fwd, "wgrad" = vst_conv2d_wgrad) of one shape (N, H, W, Cx, Cop, R, stride, pad,
    pad_mode), recorded on the stream the op is launched on.  every: events around one matching launch in
    `every` (`seen` counts them all) — an event pair costs the stream a few microseconds of idle time between
    kernels, so timing all 108 probed launches of a C2 step would add ~1 ms to the very step being measured;
    a stride coprime to the per-step launch count (36) samples every launch position over the steps."""

    def __init__(self, key, every=1):
        self.key, self.events, self.steps, self.every, self.seen = key, [], 1, max(1, int(every)), 0

    def mean_ms(self):
        torch.cuda.synchronize()
        t = [a.elapsed_time(b) for a, b in self.events]
        return sum(t) / len(t) if t else float("nan")


_probes = []


def set_launch_probes(probes):
    global _probes
    _probes = list(probes)


def _probe_begin(op, key):
    for p in _probes:
        if p.key == (op, key):
            p.seen += 1
            if (p.seen - 1) % p.every:
                return None
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            return p, ev
    return None


def _probe_end(h):
    if h is not None:
        p, ev = h
        ev[1].record()
        p.events.append(ev)


# Split-K tails of x6 forward grids (the workspace of vst_conv2d_fwd_ex); False keeps the small-tile tails.  (Module
# flags like this one are route selectors the tests flip in-process to compare routes; they are not read from the
# environment.)
FWD_SPLITK = True
# conv2d_fwd_hw with the split-K plans of the square convs' workspace path (RAFT's SepConvGRU convs);
# False: the one-launch plans
FWD_HW_SPLITK = True

# Planner answers the step asks for again and again are kept under keys that hold EVERY input of the answer: the
# inputs given here (shape, arithmetic mode, the route switches read) and the calling thread's tile override — the C
# override is thread_local and autograd runs the backward on its own thread, so debug_set_tiles mirrors it here.
_plan_memo = {}
_tiles = threading.local()


def _memo(plan, *inputs):
    key = (plan.__name__, inputs, getattr(_tiles, "v", None))
    r = _plan_memo.get(key)
    if r is None:
        r = _plan_memo[key] = plan(*inputs)
    return r


def _fwd_ex(x, wp, bias, cop, R, S, stride, pad_h, pad_w, pad_mode, act, slope, role, ws, sq=False, out=None,
            co_real=None, stats=False):
    """The one forward-conv launch (vst_conv2d_fwd_ex): y, or (y, part, nsplit) with stats.  ws: whether a workspace
    is asked for (vst_conv2d_fwd_ex_ws_bytes) —
      conv2d_fwd / conv2d_fwd_in:  FWD_SPLITK and S == R (sq: the answer memoized, the launch probed);
      their co_real < cop path:    only for the head (cop == 4), no flag;
      conv2d_fwd_hw:               FWD_HW_SPLITK."""
    _dev_check(x, wp, bias)
    N, H, W, Cx = x.shape
    Ho = (H + 2 * pad_h - R) // stride + 1
    Wo = (W + 2 * pad_w - S) // stride + 1
    y = out if out is not None else torch.empty((N, Ho, Wo, cop), device=x.device)
    m = _math(role)
    co = cop if co_real is None else int(co_real)
    nb = 0
    if ws:
        q = (N, H, W, Cx, cop, R, S, stride, pad_h, pad_w, PAD[pad_mode], m, co)
        nb = _memo(lib().vst_conv2d_fwd_ex_ws_bytes, *q) if sq else int(lib().vst_conv2d_fwd_ex_ws_bytes(*q))
    wsb = torch.empty((nb + 3) // 4, device=x.device) if nb else None
    part = nsplit = None
    if stats:
        part = torch.empty((N * max(1, Ho * Wo // 32) * cop * 2,), device=x.device, dtype=torch.float64)
        nsplit = ctypes.c_int(0)
    h = _probe_begin("fwd", (N, H, W, Cx, cop, R, stride, pad_h, pad_mode)) if _probes and sq else None
    _call("vst_conv2d_fwd_ex", _p(x), _p(wp), _p(getattr(wp, "vst_split", None)), _p(bias), _p(y), N, H, W, Cx, cop,
          R, S, stride, pad_h, pad_w, PAD[pad_mode], ACT[act], float(slope), m, co, _p(part),
          ctypes.addressof(nsplit) if stats else None, _p(wsb), nb, _stream())
    _probe_end(h)
    return (y, part, nsplit.value) if stats else y


def conv2d_fwd(x, wp, bias, cop, R, S, stride, pad, pad_mode="zero", act="none", slope=0.0,
               out=None, role="fwd", co_real=None):
    """co_real: the real output channels when cop pads them (the PatchGAN head: 1 of 4)."""
    if co_real is not None and co_real < cop:
        return _fwd_ex(x, wp, bias, cop, R, S, stride, pad, pad, pad_mode, act, slope, role, cop == 4, out=out,
                       co_real=co_real)
    return _fwd_ex(x, wp, bias, cop, R, S, stride, pad, pad, pad_mode, act, slope, role, FWD_SPLITK and S == R,
                   sq=True, out=out)


def conv2d_fwd_in(x, wp, bias, cop, R, S, stride, pad, pad_mode="zero", role="fwd"):
    """A conv that feeds an InstanceNorm: (y, stats).  The split-bf16 kernels emit the statistics
    partials from their epilogue (part / nsplit of vst_conv2d_fwd_ex) and one small fold finalizes them; other
    paths (fp32 policy, 4-channel inputs, image sizes not a multiple of 32 pixels) fall back to
    instnorm_stats(y).  Same stats layout as instnorm_stats."""
    y, part, nsplit = _fwd_ex(x, wp, bias, cop, R, S, stride, pad, pad, pad_mode, "none", 0.0, role,
                              FWD_SPLITK and S == R, sq=True, stats=True)
    if nsplit == 0:
        return y, instnorm_stats(y)
    N, Ho, Wo, _ = y.shape
    stats = torch.empty((N, cop, 2), device=x.device)
    _call("vst_instnorm_finalize", _p(part), _p(stats), N, Ho * Wo, cop, nsplit, IN_EPS, _stream())
    return y, stats


def conv2d_tfwd(x, wp, bias, Ho, Wo, cx, R, S, stride, pad, act="none", slope=0.0,
                pad_mode="zero", addend=None, role="bwd", co_real=None):
    """Transposed conv / data gradient (vst_conv2d_tfwd).  pad_mode='reflect' (stride 1) is the
    exact gradient of ReflectionPad2d(pad)+conv; addend is added in the epilogue.  co_real: the real
    channels of x when Cy pads them (vst_conv2d_tfwd_co: the PatchGAN head's data gradient)."""
    _dev_check(x, wp, bias, addend)
    N, Hi, Wi, Cy = x.shape
    y = torch.empty((N, Ho, Wo, cx), device=x.device)
    if co_real is not None and co_real < Cy:
        _call("vst_conv2d_tfwd_co", _p(x), _p(wp), _p(bias), _p(addend), _p(y), N, Hi, Wi, Cy, Ho, Wo, cx,
              R, S, stride, pad, PAD[pad_mode], ACT[act], float(slope), _math(role), int(co_real), _stream())
        return y
    _call("vst_conv2d_tfwd", _p(x), _p(wp), _p(bias), _p(addend), _p(y), N, Hi, Wi, Cy, Ho, Wo, cx,
          R, S, stride, pad, PAD[pad_mode], ACT[act], float(slope), _math(role), _stream())
    return y


# The four routes of a conv's weight gradient (wgrad_route).  The kernel, and which operand images the layer's
# producers (the IN apply of x, the IN backward of dy) may write for it, follow from the route alone:
#   WG_NHWC      vst_conv2d_wgrad_nhwc: x NHWC fp32, dy as its NHWC bf16 planes (``dy.vst_apl``), and only those
#   WG_NHWC_F32  vst_conv2d_wgrad_nhwc_f32 (its im2col form for short output rows included): x and dy NHWC fp32
#   WG_IMAGES    vst_conv2d_wgrad_pre on the split-bf16 kernel (WPLAN_BF): the producers may supply x's padded
#                channel-major image (x_t) and dy's channel-major bf16 planes (dy_planes)
#   WG_PLAIN     everything else: vst_conv2d_wgrad_pre / _bias, no producer image
WG_NHWC, WG_NHWC_F32, WG_IMAGES, WG_PLAIN = 0, 1, 2, 3
# False sends the shapes of WG_NHWC / WG_NHWC_F32 / the im2col form of WG_NHWC_F32 to the routes below them
WGRAD_NHWC = True
WGRAD_NHWC_F32 = True
WGRAD_IM2COL = True


def wgrad_route(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, pad, dy_nhwc_planes=False, role="bwd"):
    """The route (WG_*) of this conv's weight gradient.  dy_nhwc_planes: dy exists only as its NHWC bf16 planes
    (the planes-only backward chain) — such a dy can take WG_NHWC and never WG_NHWC_F32.  role: or an arithmetic's
    name.  The C planners' answer under the calling thread's tile override and the three switches above."""
    return _memo(_wgrad_route, N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, pad, _math(role), bool(dy_nhwc_planes),
                 WGRAD_NHWC, WGRAD_NHWC_F32, WGRAD_IM2COL)


def wgrad_nhwc_ok(N, H, W, Cx, Ho, Wo, Cyp, R, stride, pad, math="bwd"):
    """Does a planes-only dy take WG_NHWC at this shape (math: an arithmetic's name, or a role of the policy)?"""
    return wgrad_route(N, H, W, Cx, Ho, Wo, Cyp, R, R, stride, pad, True, math) == WG_NHWC


def wgrad_nhwc_f32_ok(N, H, W, Cx, Ho, Wo, Cyp, R, stride, pad, math="bwd"):  # ... and an fp32 dy WG_NHWC_F32?
    return wgrad_route(N, H, W, Cx, Ho, Wo, Cyp, R, R, stride, pad, False, math) == WG_NHWC_F32


def _wgrad_route(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, pad, m, dy_nhwc_planes, nhwc, nhwc_f32, im2col):
    geom = (N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, pad, m)
    if R == S and dy_nhwc_planes:
        if nhwc and lib().vst_conv2d_wgrad_nhwc_ok(*geom):
            return WG_NHWC
    elif R == S and nhwc_f32 and (lib().vst_conv2d_wgrad_nhwc_ok(*geom) or
                                  (im2col and lib().vst_conv2d_wgrad_nhwc_f32_ok(*geom))):
        return WG_NHWC_F32
    return WG_IMAGES if _wgrad_plan(*geom[:10], m)[0] == WPLAN_BF else WG_PLAIN


def conv2d_wgrad(x, dy, dw, db, R, S, stride, pad, pad_mode, co, ci, so, si, accumulate=True,
                 role="bwd", dy_planes=None, x_t=None):
    """dw (+)= weight gradient written with strides (so, si) — see vst_conv2d_wgrad; db (if not
    None) (+)= per-channel sum of dy (the bias gradient).  dy_planes: dy's bf16 plane image made by
    instnorm_act_bwd(..., planes=True), x_t: x's padded channel-major image made by
    instnorm_act_fwd(..., cp=...): those images have one reader, vst_conv2d_wgrad_pre, which then runs.
    Otherwise the kernel is wgrad_route's, for dy as it arrived (planes-only: ``dy.vst_planes_only``)."""
    _dev_check(x, dy)
    N, H, W, Cx = x.shape
    _, Ho, Wo, Cyp = dy.shape
    geom = (N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, pad)
    planes_only = getattr(dy, "vst_planes_only", False)
    images = x_t is not None or dy_planes is not None
    route = WG_IMAGES if images else wgrad_route(*geom, dy_nhwc_planes=planes_only, role=role)
    if planes_only and route == WG_NHWC and db is not None:
        raise RuntimeError("conv2d_wgrad: the bias gradient of a planes-only dy comes from its IN backward")
    if planes_only and route != WG_NHWC and dy_planes is None:
        raise RuntimeError("conv2d_wgrad: dy has NHWC planes only and this shape needs its fp32 image / plane copy")
    m, acc = _math(role), 1 if accumulate else 0
    key = (N, H, W, Cx, Cyp, R, stride, pad, pad_mode)
    if route in (WG_NHWC, WG_NHWC_F32):
        name = "vst_conv2d_wgrad_nhwc" if route == WG_NHWC else "vst_conv2d_wgrad_nhwc_f32"
        nbytes = int(getattr(lib(), name + "_ws_bytes")(*geom, m))
        ws = torch.empty((nbytes + 3) // 4, device=x.device)
        h = _probe_begin("wgrad", key) if _probes else None
        _call(name, _p(x), _p(dy.vst_apl if route == WG_NHWC else dy), _p(dw), _p(ws), nbytes, *geom, PAD[pad_mode],
              co, ci, so, si, acc, m, _stream())
        _probe_end(h)
        if db is not None:
            channel_sum(dy, db, co, accumulate)
        return
    nbytes = lib().vst_conv2d_wgrad_ws_bytes(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride)
    ws = torch.empty((nbytes + 3) // 4, device=x.device)
    h = _probe_begin("wgrad", key) if _probes else None
    if db is not None and not images:
        # the weight and bias gradient in one fused pass where a route takes the shape (vst_conv2d_wgrad_bias)
        rc = lib().vst_conv2d_wgrad_bias(_p(x), _p(dy), _p(dw), _p(db), _p(ws), nbytes, *geom, PAD[pad_mode], co, ci,
                                         so, si, acc, m, _stream())
        if rc == 0:
            _probe_end(h)
            return
        if rc != EUNSUPPORTED:
            _lib.check(rc, "vst_conv2d_wgrad_bias")
    _call("vst_conv2d_wgrad_pre", _p(x), _p(x_t), _p(dy), _p(dy_planes), _p(dw), _p(ws), nbytes, *geom, PAD[pad_mode],
          co, ci, so, si, acc, m, _stream())
    _probe_end(h)
    if db is not None:
        channel_sum(dy, db, co, accumulate)


# Conv GEMM arithmetic by role (see VST_MATH_* in include/vst_hip.h).  The default policy, bf16x6,
# runs EVERY conv — training forwards, data gradients, weight gradients, inference — with the
# fp32-equivalent three-plane bf16 split (dropped product terms <= 2^-24 relative).  "mixed" (the
# round-1 default) keeps the forwards at bf16x6 — the forward rounding decides ReLU masks, and a mask
# flipped by a 1e-5 perturbation changes which gradients exist (measured on the reference-golden G:
# bf16x3 forward => 6e-3 input-grad error, bf16x6 forward => 1e-7) — but runs data/weight gradients
# and inference-only forwards at bf16x3 (~2^-16 relative products, ~1e-5 relative gradient error):
# narrower than fp32, so it is a separately labelled option.  VST_CONV_MATH / set_conv_math:
# bf16x6 (default) | mixed | fp32 (v_mfma_f32_32x32x2_f32) | bf16x3.
_POLICIES = {"mixed": {"fwd": "bf16x6", "infer": "bf16x3", "bwd": "bf16x3"},
             "fp32": {"fwd": "fp32", "infer": "fp32", "bwd": "fp32"},
             "bf16x3": {"fwd": "bf16x3", "infer": "bf16x3", "bwd": "bf16x3"},
             "bf16x6": {"fwd": "bf16x6", "infer": "bf16x6", "bwd": "bf16x6"}}
_policy_name = os.environ.get("VST_CONV_MATH", "bf16x6")
if _policy_name not in _POLICIES:
    raise ValueError("VST_CONV_MATH must be one of %s" % sorted(_POLICIES))


def set_conv_math(policy):
    """Select the conv arithmetic policy (fp32 | bf16x3 | bf16x6 | mixed); returns the previous."""
    global _policy_name
    if policy not in _POLICIES:
        raise ValueError(policy)
    prev, _policy_name = _policy_name, policy
    return prev


def get_conv_math():
    return _policy_name


# Deterministic debug switch: the warp input gradients (warp_bwd_nhwc,
# warp_masked_bwd_nhwc, the temporal loss's ga) run the atomic-free sort + ordered-gather path
# (vst_warp_bwd_input_det) instead of the fp32-atomic scatter, so two runs agree bit for bit.
_deterministic = os.environ.get("VST_DETERMINISTIC", "0") == "1"


def set_deterministic(flag):
    """Select the deterministic warp backward (True) or the atomic scatter (False); returns the previous."""
    global _deterministic
    prev, _deterministic = _deterministic, bool(flag)
    return prev


def _warp_bwd_det(gout, flow, gx, align_corners, masked, negate, cl):
    N, H, W, C = gout.shape
    ws = torch.empty(lib().vst_warp_bwd_det_ws_bytes(N, H, W), device=gout.device, dtype=torch.uint8)
    _call("vst_warp_bwd_input_det", _p(gout), _p(flow), _p(gx), _p(ws), ws.numel(), N, H, W, C, cl,
          int(align_corners), int(masked), int(negate), _stream())


def _math(role):
    """VST_MATH_* of a role of the current policy ('fwd' | 'infer' | 'bwd'), or of an arithmetic named outright."""
    return _lib.MATH_MODES[role if role in _lib.MATH_MODES else _POLICIES[_policy_name][role]]


def debug_set_tiles(fprop=-1, tconv=-1, wgrad=-1):
    """Force GEMM tiles for calls from this host thread (vst_debug_set_tiles; -1 = automatic)."""
    _tiles.v = (int(fprop), int(tconv), int(wgrad))
    lib().vst_debug_set_tiles(*_tiles.v)


PLAN_RK, PLAN_SKINNY, PLAN_C4_DIRECT = _C["VST_PLAN_RK"], _C["VST_PLAN_SKINNY"], _C["VST_PLAN_C4_DIRECT"]
TILE_NAMES = {0: "128x128 (8 waves of 64x32)", 1: "128x64", 2: "128x128 (4 waves of 64x64)", 3: "64x128",
              4: "128x128 BK64", 5: "128x64 BK64", 6: "64x64", 7: "256x128 (8 waves of 64x64)", 8: "64x64 BK64",
              9: "128x128 BK16 (4 waves of 64x64, 2 blocks/CU at x6)",
              PLAN_RK: "fp32 [row][k] kernel", PLAN_SKINNY: "VALU skinny kernel",
              PLAN_C4_DIRECT: "4-channel patch-staged direct kernel"}


WPLAN_BF = _C["VST_WPLAN_BF"]  # the split-bf16 kernel over channel-major operand images
WPLAN_NAMES = {_C["VST_WPLAN_GENERIC"]: "conv_wgrad_k (NHWC operands)", _C["VST_WPLAN_RK"]: "copies + conv_wgrad_rk_k",
               WPLAN_BF: "copies + conv_wgrad_bf_k", _C["VST_WPLAN_SKINNY"]: "skinny VALU",
               _C["VST_WPLAN_BF_PADW"]: "Wo-padded copies + conv_wgrad_bf_k"}


def conv_plan_wgrad(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, math):
    """Host-only query (vst_conv_plan_wgrad): (path, tile kind, nsplit) of vst_conv2d_wgrad."""
    return _wgrad_plan(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, _math(math))


def _wgrad_plan(N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, m):
    import ctypes
    path, kind, ns = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _call("vst_conv_plan_wgrad", N, H, W, Cx, Ho, Wo, Cyp, R, S, stride, m, ctypes.addressof(path),
          ctypes.addressof(kind), ctypes.addressof(ns))
    return path.value, kind.value, ns.value


def conv_plan_fwd_tail(N, H, W, Cx, Cop, R, S, stride, pad, math):
    """Host-only: split-K count of the x6 tail launch vst_conv2d_fwd_ex runs for this shape (0: none)."""
    import ctypes
    m = _math(math)
    ks = ctypes.c_int(0)
    _call("vst_conv_plan_fwd_tail", N, H, W, Cx, Cop, R, S, stride, pad, m, ctypes.addressof(ks))
    return ks.value


def conv_plan_fwd(N, H, W, Cx, Cop, R, S, stride, pad_h, pad_w, math, with_tail=False):
    """Host-only query (vst_conv_plan_fwd): (tile kind, tail-split row[, tail kind]) vst_conv2d_fwd
    would use for this shape under `math` ('fp32' | 'bf16x3' | 'bf16x6', or a role of the current
    policy)."""
    import ctypes
    m = _math(math)
    kind, ms, tk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _call("vst_conv_plan_fwd", N, H, W, Cx, Cop, R, S, stride, pad_h, pad_w, m, ctypes.addressof(kind),
          ctypes.addressof(ms), ctypes.addressof(tk))
    return (kind.value, ms.value, tk.value) if with_tail else (kind.value, ms.value)


def channel_sum(x, db, cl, accumulate=True):
    """db[c] (+)= sum over pixels of x[..., c] (bias gradient)."""
    _dev_check(x)
    cs = x.shape[-1]
    nhw = x.numel() // cs
    nbytes = lib().vst_channel_sum_ws_bytes(nhw, cs)
    ws = torch.empty((nbytes + 3) // 4, device=x.device)
    _call("vst_channel_sum", _p(x), _p(db), _p(ws), nhw, cs, cl, 1 if accumulate else 0, _stream())


# ReflectionPad2d(1) + 3x3 data gradients as the interior conv + border GEMM (vst_conv2d_dgrad_refl)
# instead of the conv over the zero-padded frame + reflect fold; False keeps the fold.
DGRAD_BORDER = True


def conv2d_dgrad_s1(dy, ikf, H, W, cx, R, pad, pad_mode="zero", addend=None, role="bwd"):
    """Data gradient of a stride-1 conv as a FORWARD conv (the split-bf16 MFMA fprop kernel with
    pre-split weights).  Reflect padding, 3x3 / pad 1: the interior dx = conv(dy, rot180(W)^T, zero
    pad 1) (+ addend in its epilogue) plus the padded border positions' GEMM added into rows / columns
    1 and H-2 / W-2 (vst_conv2d_dgrad_refl).  Other reflect cases: dx_full = conv(dy, rot180(W)^T,
    zero pad R-1) over the padded input frame [H+2p][W+2p], then the reflect fold (+ addend).  Zero
    padding p <= R-1: dx = conv(dy, rot180(W)^T, zero pad R-1-p) directly (+ addend).  ikf:
    VST_PACK_IKF pack."""
    _dev_check(dy, ikf, addend)
    if pad_mode == "reflect" and DGRAD_BORDER and R == 3 and pad == 1 and getattr(ikf, "vst_split", None) is not None:
        N, Hy, Wy, Cy = dy.shape
        m = _math(role)
        nb = int(lib().vst_conv2d_dgrad_refl_ws_bytes(N, H, W, Cy, cx, m)) if (Hy, Wy) == (H, W) else 0
        if nb:
            dx = torch.empty((N, H, W, cx), device=dy.device)
            ws = torch.empty((nb + 3) // 4, device=dy.device)
            h = _probe_begin("dgrad", (N, H, W, Cy, cx, R, 1, pad, pad_mode)) if _probes else None
            _call("vst_conv2d_dgrad_refl", _p(dy), _p(ikf.vst_split), _p(addend), _p(dx), _p(ws), nb, N, H, W, Cy, cx,
                  m, _stream())
            _probe_end(h)
            return dx
    if pad_mode == "reflect":
        dxp = conv2d_fwd(dy, ikf, None, cx, R, R, 1, R - 1, "zero", role=role)
        return reflect_fold(dxp, pad, addend)
    if pad > R - 1:
        raise NotImplementedError("conv2d_dgrad_s1: zero padding must be <= R-1")
    dx = conv2d_fwd(dy, ikf, None, cx, R, R, 1, R - 1 - pad, "zero", role=role)
    if addend is not None:
        axpby(addend, dx, 1.0, 1.0)
    return dx


# The data gradient of ReflectionPad2d(p) + Conv2d(C -> 4, 7x7) (the generator's last layer) as the
# zero-pad-p conv of dy on the direct 4-channel kernel + the reflect-fold frame (vst_c4_dgrad_frame),
# instead of the conv over the (H+2p) x (W+2p) padded frame + reflect_fold.  False: that route.
C4_DGRAD = True


def c4_dgrad_reflect_ok(dy, cx, R, pad, role="bwd"):
    N, H, W, C = dy.shape
    return (C4_DGRAD and C == 4 and cx % 16 == 0 and R == 2 * pad + 1 and H > 2 * pad + 1 and W > 2 * pad + 1
            and conv_plan_fwd(N, H, W, 4, cx, R, R, 1, pad, pad, role)[0] == PLAN_C4_DIRECT)


def c4_dgrad_reflect(dy, ikf, H, W, cx, R, pad, role="bwd"):
    """dx of ReflectionPad2d(pad) + Conv2d(cx -> 4, R x R) from the 4-channel dy (ikf: VST_PACK_IKF):
    the interior dxp[i+pad][j+pad] as the zero-pad-pad forward conv over dy (the direct 4-channel
    kernel), then vst_c4_dgrad_frame adds the reflect-fold terms of the padded frame's border."""
    _dev_check(dy, ikf)
    N = dy.shape[0]
    dx = conv2d_fwd(dy, ikf, None, cx, R, R, 1, pad, "zero", role=role)
    _call("vst_c4_dgrad_frame", _p(dy), _p(ikf), _p(dx), N, H, W, cx, R, pad, _stream())
    return dx


def conv2d_dgrad_refl_in(dy, ikf, H, W, cx, y_in, stats, act="relu", slope=0.0, addend=None, db=None,
                         accumulate_db=True, planes=False, role="bwd", apre=False):
    """ReflectionPad2d(1) + 3x3 data gradient (conv2d_dgrad_s1's interior conv + border GEMM) fused with
    the InstanceNorm(+act) backward of the layer below it: returns (g, dy_in[, dy_in_planes]) — g = the
    data gradient (+ addend), dy_in = instnorm_act_bwd(g, y_in, stats, act) — or None when the fused route
    does not support the shape / arithmetic.  The IN partials are taken by the data gradient's GEMM
    epilogue and border add (vst_conv2d_dgrad_refl_epi_part: no partial pass; x6 arithmetic, H W % 32 ==
    0); dy's pre-split planes (``dy.vst_apl``) are its A operand when present, and apre
    writes dy_in as planes only."""
    _dev_check(dy, ikf, addend, y_in, stats)
    if not DGRAD_BORDER or getattr(ikf, "vst_split", None) is None:
        return None
    N, Hy, Wy, Cy = dy.shape
    C = y_in.shape[-1]
    if (Hy, Wy) != (H, W) or cx != C:
        return None
    m = _math(role)
    nb = int(lib().vst_conv2d_dgrad_refl_in_epi_ws_bytes(N, H, W, Cy, C, m))
    if not nb:
        return None
    g = torch.empty((N, H, W, C), device=dy.device)
    dyi = torch.empty_like(g)
    ws = torch.empty((nb + 3) // 4, device=dy.device)
    pl, ldp = None, 0
    if planes:
        ldp = lib().vst_cp_ld(N * H * W)
        pl = torch.empty((3, C, ldp), device=dy.device, dtype=torch.bfloat16)
    if apre:  # dy_in as NHWC planes only (instnorm_act_bwd(apre=True))
        dyi.vst_apl = torch.empty((3, dyi.numel()), device=dy.device, dtype=torch.bfloat16)
        dyi.vst_planes_only = True
    h = _probe_begin("dgrad", (N, H, W, Cy, C, 3, 1, 1, "reflect")) if _probes else None
    _call("vst_conv2d_dgrad_refl_epi_part", _p(dy), _p(getattr(dy, "vst_apl", None)), _p(ikf.vst_split),
          _p(addend), _p(g), _p(y_in), _p(stats), _p(ws), nb, N, H, W, Cy, C, ACT[act], float(slope), m, _stream())
    _probe_end(h)
    _call("vst_instnorm_act_bwd_epi_tail", _p(g), _p(y_in), _p(stats), _p(dyi), _p(db), _p(ws), N, H, W, C, ACT[act],
          float(slope), 1 if accumulate_db else 0, _p(pl), ldp, _p(getattr(dyi, "vst_apl", None)), _stream())
    return (g, dyi, pl) if planes else (g, dyi)


def dgrad_refl_epi_ok(N, H, W, Cy, Cx, role="bwd"):
    """Does conv2d_dgrad_refl_in take this shape (vst_conv2d_dgrad_refl_in_epi_ws_bytes > 0)?"""
    return DGRAD_BORDER and int(lib().vst_conv2d_dgrad_refl_in_epi_ws_bytes(N, H, W, Cy, Cx, _math(role))) > 0


def reflect_fold(dxp, p, addend=None):
    _dev_check(dxp, addend)
    N, Hp, Wp, C = dxp.shape
    H, W = Hp - 2 * p, Wp - 2 * p
    dx = torch.empty((N, H, W, C), device=dxp.device)
    _call("vst_reflect_fold", _p(dxp), _p(addend), _p(dx), N, H, W, C, p, _stream())
    return dx


# --------------------------------------------------------------------------------- instnorm
def _in_ws(N, HW, C, device):
    nbytes = lib().vst_instnorm_ws_bytes(N, HW, C)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def instnorm_stats(y):
    _dev_check(y)
    N, H, W, C = y.shape
    stats = torch.empty((N, C, 2), device=y.device)
    ws = _in_ws(N, H * W, C, y.device)
    _call("vst_instnorm_stats", _p(y), _p(stats), _p(ws), N, H * W, C, IN_EPS, _stream())
    return stats


def instnorm_act_fwd(y, stats, act="relu", slope=0.0, residual=None, cp=None, xpl=None):
    """a = act(IN(y)) (+ residual).  cp = (pad, pad_mode, stride) of the conv that consumes a:
    returns (a, a_t) where a_t is a's padded channel-major image for that conv's x6 weight gradient
    (vst_instnorm_act_fwd_cp; conv2d_wgrad(x_t=a_t)).  xpl = (pad, pad_mode, wx): returns (a, planes),
    a's padded image as the bf16 planes [3][C][ld] with wx zero columns per row
    (vst_instnorm_act_fwd_planes; tap_conv_wgrad_swap(x_pl=planes))."""
    _dev_check(y, stats, residual)
    N, H, W, C = y.shape
    a = torch.empty_like(y)
    if xpl is not None:
        pad, mode, wx = xpl
        ld = lib().vst_cp_ld(N * (H + 2 * pad) * (W + 2 * pad + wx))
        pl = torch.empty((3, C, ld), device=y.device, dtype=torch.bfloat16)
        _call("vst_instnorm_act_fwd_planes", _p(y), _p(stats), _p(residual), _p(a), _p(pl), N, H, W, C, ACT[act],
              float(slope), pad, PAD[mode], wx, _stream())
        return a, pl
    if cp is not None:
        pad, mode, st = cp
        at = torch.empty((C, lib().vst_cp_ld(N * (H + 2 * pad) * (W + 2 * pad))), device=y.device)
        _call("vst_instnorm_act_fwd_cp", _p(y), _p(stats), _p(residual), _p(a), _p(at), N, H, W, C, ACT[act],
              float(slope), pad, PAD[mode], st, _stream())
        return a, at
    _call("vst_instnorm_act_fwd", _p(y), _p(stats), _p(residual), _p(a), N, H * W, C, ACT[act],
          float(slope), _stream())
    return a


def instnorm_act_bwd(ga, y, stats, act="relu", slope=0.0, db=None, accumulate_db=True, planes=False, apre=False):
    """dy = backward of act(IN(y)); db (if given) (+)= sum of dy per channel (conv-bias grad).
    planes=True: returns (dy, dy_planes) — the apply pass also writes dy's three bf16 planes
    [3][C][vst_cp_ld(N*H*W)], the x6 weight gradient's operand image (conv2d_wgrad(dy_planes=...)).
    apre: dy is written ONLY as its NHWC bf16 planes ``dy.vst_apl`` (the pre-split A operand of the data
    gradient that consumes it, conv2d_dgrad_refl_in) — dy's fp32 values are NOT written (dy.vst_planes_only):
    its readers must take the planes (the weight gradient: dy_planes; the data gradient: vst_apl)."""
    _dev_check(ga, y, stats)
    N, H, W, C = y.shape
    dy = torch.empty_like(y)
    ws = _in_ws(N, H * W, C, y.device)
    pl, ldp = None, 0
    if planes:
        ldp = lib().vst_cp_ld(N * H * W)
        pl = torch.empty((3, C, ldp), device=y.device, dtype=torch.bfloat16)
    if apre:
        dy.vst_apl = torch.empty((3, dy.numel()), device=y.device, dtype=torch.bfloat16)
        dy.vst_planes_only = True
        _call("vst_instnorm_act_bwd_planes_apre", _p(ga), _p(y), _p(stats), _p(dy), _p(db), _p(ws), N, H * W, C,
              ACT[act], float(slope), 1 if accumulate_db else 0, _p(pl), ldp, _p(dy.vst_apl), _stream())
        return (dy, pl) if planes else dy
    _call("vst_instnorm_act_bwd_planes", _p(ga), _p(y), _p(stats), _p(dy), _p(db), _p(ws), N, H * W, C,
          ACT[act], float(slope), 1 if accumulate_db else 0, _p(pl), ldp, _stream())
    return (dy, pl) if planes else dy


def _skip_check(y, stats, cat, c0):
    if y.dim() != 4 or cat.dim() != 4 or cat.shape[:3] != y.shape[:3]:
        raise ValueError("instnorm_skip: y %s and cat %s must be NHWC over the same pixels" %
                         (tuple(y.shape), tuple(cat.shape)))
    N, H, W, C = y.shape
    if stats is not None and tuple(stats.shape) != (N, C, 2):
        raise ValueError("instnorm_skip: stats %s is not [N, C, 2] of y %s" % (tuple(stats.shape), tuple(y.shape)))
    if c0 < 0 or c0 + C > cat.shape[-1]:
        raise ValueError("instnorm_skip: channels [%d, %d) lie outside cat's %d" % (c0, c0 + C, cat.shape[-1]))
    return N, H * W, C, cat.shape[-1]


def instnorm_skip_fwd(y, stats, cat, c0, want_d=True, slope=0.2):
    """The U-Net skip connection's forward (vst_instnorm_skip_fwd): z = IN(y) (stats None: z = y);
    relu(z) goes into channels [c0, c0 + C) of the concatenation buffer cat, and d = lrelu(z) is returned
    (want_d=False: None — the up norm's apply into its half of cat)."""
    _dev_check(y, stats, cat)
    N, HW, C, Cs = _skip_check(y, stats, cat, c0)
    d = torch.empty_like(y) if want_d else None
    _call("vst_instnorm_skip_fwd", _p(y), _p(stats), _p(d), _p(cat), N, HW, C, Cs, int(c0), float(slope), _stream())
    return d


def instnorm_skip_bwd(g_d, g_cat, c0, y, stats, db=None, accumulate_db=True, slope=0.2):
    """Backward of instnorm_skip_fwd (vst_instnorm_skip_bwd): g = g_d * lrelu'(z) + g_cat[..., c0:c0 + C] *
    relu'(z) (g_d None: the second term alone), then the IN backward (stats None: dy = g).  db (if given)
    (+)= the per-channel sum of dy.  Returns dy."""
    _dev_check(g_d, g_cat, y, stats, db)
    N, HW, C, Cs = _skip_check(y, stats, g_cat, c0)
    if g_d is not None and g_d.shape != y.shape:
        raise ValueError("instnorm_skip_bwd: g_d %s does not match y %s" % (tuple(g_d.shape), tuple(y.shape)))
    if db is not None and db.numel() != C:
        raise ValueError("instnorm_skip_bwd: db has %d entries for %d channels" % (db.numel(), C))
    dy = torch.empty_like(y)
    ws = None
    if stats is not None or db is not None:
        nbytes = lib().vst_instnorm_skip_ws_bytes(N, HW, C)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=y.device)
    _call("vst_instnorm_skip_bwd", _p(g_d), _p(g_cat), Cs, int(c0), _p(y), _p(stats), _p(dy), _p(db),
          1 if accumulate_db else 0, _p(ws), N, HW, C, float(slope), _stream())
    return dy


def act_bwd(gy, y, act, slope=0.0):
    _dev_check(gy, y)
    dx = torch.empty_like(y)
    _call("vst_act_bwd", _p(gy), _p(y), _p(dx), y.numel(), ACT[act], float(slope), _stream())
    return dx


# ------------------------------------------------------------------------------------- flow
def warp_nhwc(x, flow, align_corners=False):
    _dev_check(x, flow)
    N, H, W, C = x.shape
    out = torch.empty_like(x)
    _call("vst_warp_fwd", _p(x), _p(flow), _p(out), N, H, W, C, int(align_corners), _stream())
    return out


def warp_bwd_nhwc(gout, flow, align_corners=False):
    _dev_check(gout, flow)
    N, H, W, C = gout.shape
    gx = torch.zeros_like(gout)
    if _deterministic:
        _warp_bwd_det(gout, flow, gx, align_corners, False, False, C)
        return gx
    _call("vst_warp_bwd_input", _p(gout), _p(flow), _p(gx), N, H, W, C, int(align_corners), _stream())
    return gx


def fbcheck(ff, bf):
    _dev_check(ff, bf)
    N, _, H, W = bf.shape
    mask = torch.empty((N, 1, H, W), device=bf.device)
    _call("vst_fbcheck", _p(ff), _p(bf), _p(mask), N, H, W, _stream())
    return mask


# ----------------------------------------------------------------------------------- losses
def _part(npix, device):
    return torch.empty(lib().vst_loss_part_floats(npix), device=device)


def loss_temporal(a, b, flow, mask, lam, cl=3):
    _dev_check(a, b, flow, mask)
    N, H, W, Cs = a.shape
    loss = torch.empty((), device=a.device)
    _call("vst_loss_temporal", _p(a), _p(b), _p(flow), _p(mask), _p(loss), _p(_part(N * H * W, a.device)),
          N, H, W, Cs, cl, float(lam), _stream())
    return loss


def loss_temporal_bwd(a, b, flow, mask, gout, ga, gb, lam, cl=3):
    N, H, W, Cs = a.shape
    if _deterministic and ga is not None:   # gb first, then ga -= its ordered scatter
        gbuf = gb if gb is not None else torch.empty_like(a)
        _call("vst_loss_temporal_bwd", _p(a), _p(b), _p(flow), _p(mask), _p(gout), None, _p(gbuf), N, H, W,
              Cs, cl, float(lam), _stream())
        _warp_bwd_det(gbuf, flow, ga, False, False, True, cl)
        return
    _call("vst_loss_temporal_bwd", _p(a), _p(b), _p(flow), _p(mask), _p(gout), _p(ga), _p(gb), N, H, W,
          Cs, cl, float(lam), _stream())


def loss_l1(a, b, scale, cl=3):
    _dev_check(a, b)
    npix = a.numel() // a.shape[-1]
    loss = torch.empty((), device=a.device)
    _call("vst_loss_l1", _p(a), _p(b), _p(loss), _p(_part(npix, a.device)), npix, a.shape[-1], cl,
          float(scale), _stream())
    return loss


def loss_l1_bwd(a, b, gout, scale, cl=3):
    npix = a.numel() // a.shape[-1]
    g = torch.empty_like(a)
    _call("vst_loss_l1_bwd", _p(a), _p(b), _p(gout), _p(g), npix, a.shape[-1], cl, float(scale), _stream())
    return g


def loss_mse_const(a, target, scale=1.0, cl=1):
    _dev_check(a)
    npix = a.numel() // a.shape[-1]
    loss = torch.empty((), device=a.device)
    _call("vst_loss_mse_const", _p(a), float(target), _p(loss), _p(_part(npix, a.device)), npix,
          a.shape[-1], cl, float(scale), _stream())
    return loss


def loss_mse_const_bwd(a, target, gout, scale=1.0, cl=1):
    npix = a.numel() // a.shape[-1]
    g = torch.empty_like(a)
    _call("vst_loss_mse_const_bwd", _p(a), float(target), _p(gout), _p(g), npix, a.shape[-1], cl,
          float(scale), _stream())
    return g


R1_PART_DOUBLES = _C["VST_R1_PART_DOUBLES"]


def _r1_check(what, g):
    _dev_check(g)
    if g.dim() != 4 or g.shape[-1] != 4:
        raise ValueError("%s: the image gradient is NHWC [B, H, W, 4], got %s" % (what, tuple(g.shape)))


def r1(g):
    """r1_reg of the NHWC-4 image gradient g: 0.5 / B * sum over h, w and the three real lanes of g^2
    (vst_loss_r1; fp64 accumulation in a fixed order)."""
    _r1_check("r1", g)
    B, H, W, _ = g.shape
    loss = torch.empty((), device=g.device)
    part = torch.empty(R1_PART_DOUBLES, dtype=torch.float64, device=g.device)
    _call("vst_loss_r1", _p(g), _p(loss), _p(part), B, H * W, _stream())
    return loss


def r1_bwd(g, gout):
    """gout * g / B with lane 3 zeroed (vst_loss_r1_bwd); gout a device scalar."""
    _r1_check("r1_bwd", g)
    _dev_check(gout)
    if gout.numel() != 1:
        raise ValueError("r1_bwd: gout is a scalar, got %s" % (tuple(gout.shape),))
    B, H, W, _ = g.shape
    u = torch.empty_like(g)
    _call("vst_loss_r1_bwd", _p(g), _p(gout), _p(u), B, H * W, _stream())
    return u


def _bce_check(what, z, y, nd, target):
    _dev_check(z)
    if z.dim() != 2 or z.shape[1] % 4 or not 0 < nd <= z.shape[1]:
        raise ValueError("%s: logits are [B, cpad(num_domains)] with %d domains, got %s" % (what, nd, tuple(z.shape)))
    if not y.is_cuda or y.dtype != torch.int64 or not y.is_contiguous() or tuple(y.shape) != (z.shape[0],):
        raise ValueError("%s: domain ids are a contiguous int64 device tensor [%d]" % (what, z.shape[0]))
    if target not in (0, 1):
        raise ValueError("%s: target must be 0 or 1, got %r" % (what, target))


def bce_logits(z, y, nd, target):
    """mean_b softplus(-+z[b, y[b]]): binary_cross_entropy_with_logits of the selected domain's logit against the
    constant target (vst_loss_bce_logits)."""
    _bce_check("bce_logits", z, y, nd, target)
    loss = torch.empty((), device=z.device)
    _call("vst_loss_bce_logits", _p(z), _p(y), _p(loss), z.shape[0], z.shape[1], int(nd), float(target), _stream())
    return loss


def bce_logits_bwd(z, y, nd, target, gout):
    """The dense [B, D] gradient of bce_logits: (sigmoid(z) - target) / B * gout in column y[b], zeros elsewhere
    (vst_loss_bce_logits_bwd)."""
    _bce_check("bce_logits_bwd", z, y, nd, target)
    _dev_check(gout)
    grad = torch.empty_like(z)
    _call("vst_loss_bce_logits_bwd", _p(z), _p(y), _p(gout), _p(grad), z.shape[0], z.shape[1], int(nd), float(target),
          _stream())
    return grad


# -------------------------------------------------------------------------------- optimizer
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    _dev_check(p, g, m, v)
    _call("vst_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1),
          float(beta2), float(eps), int(step), _stream())


def axpby(x, y, a, b):
    _dev_check(x, y)
    _call("vst_axpby", _p(x), _p(y), x.numel(), float(a), float(b), _stream())


# ------------------------------------------------------------- learning-based style path
def warp_masked_nhwc(x, flow, align_corners=False):
    """fs_lib.warp (methods/learning-based/fs_lib.py:5-39): warp * grid_sample(ones) validity."""
    _dev_check(x, flow)
    N, H, W, C = x.shape
    out = torch.empty_like(x)
    _call("vst_warp_masked_fwd", _p(x), _p(flow), _p(out), N, H, W, C, int(align_corners), _stream())
    return out


def warp_masked_bwd_nhwc(gout, flow, align_corners=False):
    _dev_check(gout, flow)
    N, H, W, C = gout.shape
    gx = torch.zeros_like(gout)
    if _deterministic:
        _warp_bwd_det(gout, flow, gx, align_corners, True, False, C)
        return gx
    _call("vst_warp_masked_bwd_input", _p(gout), _p(flow), _p(gx), N, H, W, C, int(align_corners),
          _stream())
    return gx


def _tsq_args(a, b, flow, mask, cl, inputs):
    N, H, W, Cs = a.shape
    i1, i2 = inputs if inputs is not None else (None, None)
    _dev_check(a, b, flow, mask, i1, i2)
    if b.shape != a.shape or flow.shape != (N, 2, H, W) or mask.numel() != N * H * W:
        raise ValueError("temporal_sqdiff: a/b %s %s, flow %s, mask %s do not match" %
                         (tuple(a.shape), tuple(b.shape), tuple(flow.shape), tuple(mask.shape)))
    if inputs is not None and (i1.shape != (N, H, W, 4) or i2.shape != (N, H, W, 4)):
        raise ValueError("temporal_sqdiff: the input frames must be NHWC4 of the frames' size")
    return N, H, W, Cs, (Cs if cl is None else cl), i1, i2


def temporal_sqdiff(a, b, flow, mask, scale, cl=None, ab_scale=1.0, inputs=None):
    """scale * mean((mask * (s*b - fs_lib.warp(s*a, flow) - r))^2) over the cl logical channels of NHWC a, b
    (fs_huang.py:55-56, fs_reconet.py:61-69); s = ab_scale; inputs = (i1, i2) NHWC4 frames: r = their
    luminance-weighted warped difference (fs_reconet.py:66-67), else 0.  One fused pass; device scalar."""
    N, H, W, Cs, cl, i1, i2 = _tsq_args(a, b, flow, mask, cl, inputs)
    loss = torch.empty((), device=a.device)
    part = torch.empty(lib().vst_temporal_sqdiff_part_floats(N, H, W, Cs), device=a.device)
    _call("vst_temporal_sqdiff_fwd", _p(a), _p(b), _p(flow), _p(mask), _p(i1), _p(i2), _p(loss), _p(part),
          N, H, W, Cs, cl, float(scale), float(ab_scale), _stream())
    return loss


def temporal_sqdiff_bwd(a, b, flow, mask, gout, ga, gb, scale, cl=None, ab_scale=1.0, inputs=None):
    """Gradients of temporal_sqdiff: gb written (pad channels 0), ga ACCUMULATED (zero it first); either may
    be None.  Deterministic mode: gb first, then ga from the ordered scatter of -gb through valid samples."""
    N, H, W, Cs, cl, i1, i2 = _tsq_args(a, b, flow, mask, cl, inputs)
    _dev_check(gout, ga, gb)
    args = (N, H, W, Cs, cl, float(scale), float(ab_scale), _stream())
    if _deterministic and ga is not None:
        gbuf = gb if gb is not None else torch.empty_like(a)
        _call("vst_temporal_sqdiff_bwd", _p(a), _p(b), _p(flow), _p(mask), _p(i1), _p(i2), _p(gout), None,
              _p(gbuf), *args)
        _warp_bwd_det(gbuf, flow, ga, False, True, True, cl)
        return
    _call("vst_temporal_sqdiff_bwd", _p(a), _p(b), _p(flow), _p(mask), _p(i1), _p(i2), _p(gout), _p(ga), _p(gb),
          *args)


def ruder_stack(y_prev, img, flow, mask, s=1.0 / 255.0, want_w=True):
    """The Ruder net's next input (fs_ruder.py:52): x [N,H,W,8] = (img rgb, mask, fs_lib.warp(s * y_prev, flow)
    rgb, 0) and w [N,H,W,4] = the same warped values (None unless want_w), in one pass.  y_prev: the previous
    styled frame, NHWC4 0..255; img NHWC4 [0,1]; flow [N,2,H,W]; mask [N,1,H,W].  y_prev = flow = mask = None:
    the blank form of fs_ruder.py:78 (channels 3..7 of x and w zero)."""
    _dev_check(y_prev, img, flow, mask)
    if img.dim() != 4 or img.shape[-1] != 4:
        raise ValueError("ruder_stack: img must be NHWC4, got %s" % (tuple(img.shape),))
    N, H, W, _ = img.shape
    given = [t is not None for t in (y_prev, flow, mask)]
    if any(given) != all(given):
        raise ValueError("ruder_stack: y_prev, flow and mask are given together or not at all (the blank form)")
    if all(given) and (y_prev.shape != img.shape or flow.shape != (N, 2, H, W) or mask.numel() != N * H * W):
        raise ValueError("ruder_stack: y_prev %s, img %s, flow %s, mask %s do not match" %
                         (tuple(y_prev.shape), tuple(img.shape), tuple(flow.shape), tuple(mask.shape)))
    x = torch.empty((N, H, W, 8), device=img.device, dtype=torch.float32)
    w = torch.empty((N, H, W, 4), device=img.device, dtype=torch.float32) if want_w else None
    _call("vst_ruder_stack_fwd", _p(y_prev), _p(img), _p(flow), _p(mask), _p(x), _p(w), N, H, W, float(s), _stream())
    return x, w


def ruder_stack_bwd(gx, gw, flow, gy_prev, s=1.0 / 255.0):
    """The one scatter of the Ruder recurrence: gy_prev (NHWC4, ACCUMULATED: zero it first) += s * scatter(valid
    corner weights * (gx[..., 4:7] + gw)); gx [N,H,W,8] (the net's input gradient) or gw [N,H,W,4] (from the
    temporal loss) may be None.  Deterministic mode: the combined gradient is written once and scattered in order."""
    _dev_check(gx, gw, flow, gy_prev)
    N, H, W, _ = gy_prev.shape
    if gx is None and gw is None:
        raise ValueError("ruder_stack_bwd: neither gx nor gw given")
    if gy_prev.shape != (N, H, W, 4) or flow.shape != (N, 2, H, W) or \
            (gx is not None and gx.shape != (N, H, W, 8)) or (gw is not None and gw.shape != (N, H, W, 4)):
        raise ValueError("ruder_stack_bwd: gx %s, gw %s, flow %s, gy_prev %s do not match" %
                         (None if gx is None else tuple(gx.shape), None if gw is None else tuple(gw.shape),
                          tuple(flow.shape), tuple(gy_prev.shape)))
    if _deterministic:
        gbuf = torch.empty_like(gy_prev)
        _call("vst_ruder_stack_bwd", _p(gx), _p(gw), _p(flow), None, _p(gbuf), N, H, W, float(s), _stream())
        _warp_bwd_det(gbuf, flow, gy_prev, False, True, False, 3)
        return gy_prev
    _call("vst_ruder_stack_bwd", _p(gx), _p(gw), _p(flow), _p(gy_prev), None, N, H, W, float(s), _stream())
    return gy_prev


def _ruder_temporal_args(w, y, mask):
    _dev_check(w, y, mask)
    if w.dim() != 4 or w.shape[-1] != 4 or y.shape != w.shape or mask.numel() != w.numel() // 4:
        raise ValueError("ruder_temporal: w %s, y %s, mask %s do not match (NHWC4 images, one mask plane)" %
                         (tuple(w.shape), tuple(y.shape), tuple(mask.shape)))
    return w.shape[:3]


def ruder_temporal(w, y, mask, scale, ab_scale=1.0 / 255.0):
    """scale * mean((mask * (w - s*y))^2) over the 3 image channels (fs_ruder.py:97): w the warped previous
    frame a ruder_stack returned, y the styled frame (NHWC4, 0..255), s = ab_scale.  Device scalar."""
    N, H, W = _ruder_temporal_args(w, y, mask)
    loss = torch.empty((), device=w.device)
    part = torch.empty(lib().vst_ruder_temporal_part_floats(N, H, W), device=w.device)
    _call("vst_ruder_temporal_fwd", _p(w), _p(y), _p(mask), _p(loss), _p(part), N, H, W, float(scale),
          float(ab_scale), _stream())
    return loss


def ruder_temporal_bwd(w, y, mask, gout, scale, ab_scale=1.0 / 255.0, need_w=True, need_y=True):
    """(gw, gy) of ruder_temporal times the device scalar gout, NHWC4 with pad channel 0 (None if not needed)."""
    N, H, W = _ruder_temporal_args(w, y, mask)
    _dev_check(gout)
    if not (need_w or need_y):
        return None, None
    gw = torch.empty_like(w) if need_w else None
    gy = torch.empty_like(y) if need_y else None
    _call("vst_ruder_temporal_bwd", _p(w), _p(y), _p(mask), _p(gout), _p(gw), _p(gy), N, H, W, float(scale),
          float(ab_scale), _stream())
    return gw, gy


_MULT_CACHE = {}


def resize_bilinear(x, size, mult=None):
    """F.interpolate(x, size=size, mode='bilinear', align_corners=False) of NCHW planes, channel c times
    mult[c] (a sequence of C floats or None): the flow / mask resize of fs_reconet.py:57-60."""
    _dev_check(x)
    N, C, Hi, Wi = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    m = None
    if mult is not None:
        key = (tuple(float(v) for v in mult), str(x.device))
        if len(key[0]) != C:
            raise ValueError("resize_bilinear: one multiplier per channel")
        if key not in _MULT_CACHE:
            _MULT_CACHE[key] = torch.tensor(key[0], device=x.device, dtype=torch.float32)
        m = _MULT_CACHE[key]
    y = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    _call("vst_resize_bilinear", _p(x), _p(m), _p(y), N, C, Hi, Wi, Ho, Wo, _stream())
    return y


def instnorm_affine_fwd(y, stats, gamma, beta, act="none", gate=None, gate_mult=1.0, residual=None,
                        slope=0.0):
    """s * act(gamma * IN(y) + beta) + residual (vst_instnorm_affine_fwd); gamma/beta padded to C."""
    _dev_check(y, stats, gamma, beta, gate, residual)
    N, H, W, C = y.shape
    out = torch.empty_like(y)
    _call("vst_instnorm_affine_fwd", _p(y), _p(stats), _p(gamma), _p(beta), _p(gate), float(gate_mult),
          _p(residual), _p(out), N, H * W, C, ACT[act], float(slope), _stream())
    return out


def instnorm_affine_bwd(g, y, stats, gamma, beta, act="none", gate=None, gate_mult=1.0, dgamma=None,
                        dbeta=None, dgate=None, dbias=None, accumulate=True, slope=0.0):
    _dev_check(g, y, stats, gamma, beta, gate)
    N, H, W, C = y.shape
    dx = torch.empty_like(y)
    nbytes = lib().vst_instnorm_affine_ws_bytes(N, H * W, C)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=y.device)
    _call("vst_instnorm_affine_bwd", _p(g), _p(y), _p(stats), _p(gamma), _p(beta), _p(gate),
          float(gate_mult), _p(dx), _p(dgamma), _p(dbeta), _p(dgate), _p(dbias), _p(ws), N, H * W, C,
          ACT[act], float(slope), 1 if accumulate else 0, _stream())
    return dx


def style_ids(s_id, N, S, device):
    """The device int32 [N] style ids the conditional-norm kernels read, from a Python int, a 0-dim tensor
    (long or float: truncated as ``.long()`` does; one style for the batch) or a length-N sequence / 1-D tensor
    (one style per sample).  Values that arrive on the host are range-checked here (ValueError); a device
    tensor is converted on the device without a copy back, and the kernels clamp what they read."""
    if torch.is_tensor(s_id):
        if s_id.dim() > 1 or (s_id.dim() == 1 and s_id.numel() != N):
            raise ValueError("style id: a scalar or %d ids, got shape %s" % (N, tuple(s_id.shape)))
        if s_id.is_cuda:
            return s_id.detach().to(torch.int64).to(torch.int32).expand(N).contiguous()
        s_id = s_id.detach().to(torch.int64).tolist()
    try:
        ids = [int(v) for v in s_id]
    except TypeError:
        ids = [int(s_id)] * N
    if len(ids) != N:
        raise ValueError("style id: a scalar or %d ids, got %d" % (N, len(ids)))
    if min(ids) < 0 or max(ids) >= S:
        raise ValueError("style id %s outside [0, %d)" % (ids if len(set(ids)) > 1 else ids[0], S))
    return torch.tensor(ids, dtype=torch.int32, device=device)


def _cond_check(y, stats, sid, embed, bn_w, bn_b, act):
    _dev_check(y, stats, embed, bn_w, bn_b)
    N, C = y.shape[0], y.shape[-1]
    if not sid.is_cuda or sid.dtype != torch.int32 or not sid.is_contiguous() or tuple(sid.shape) != (N,):
        raise RuntimeError("cond_instnorm: sid must be a contiguous int32 GPU tensor of %d ids" % N)
    S, Cl = embed.shape[0], bn_w.numel()
    if y.dim() != 4 or tuple(stats.shape) != (N, C, 2) or tuple(embed.shape) != (S, 2 * Cl) or \
            bn_b.numel() != Cl or not 0 < Cl <= C or S < 1:
        raise ValueError("cond_instnorm: y NHWC with stats [N, C, 2], embed [S, 2*Cl] and bn weight / bias [Cl], "
                         "Cl <= %d" % C)
    if act not in ("none", "relu"):
        raise ValueError("cond_instnorm: act must be 'none' or 'relu'")
    return S, Cl


def cond_instnorm_fwd(y, stats, sid, embed, bn_w, bn_b, act="none"):
    """act(ge * (bn_w * IN(y) + bn_b) + be), {ge, be} = the halves of embed[sid[n]] (vst_cond_instnorm_fwd).
    sid: device int32 [N] (style_ids); embed [S, 2*Cl], bn_w / bn_b [Cl], Cl <= C real channels."""
    S, Cl = _cond_check(y, stats, sid, embed, bn_w, bn_b, act)
    N, H, W, C = y.shape
    out = torch.empty_like(y)
    ws = torch.empty((N, C, 2), device=y.device)
    _call("vst_cond_instnorm_fwd", _p(y), _p(stats), _p(sid), _p(embed), _p(bn_w), _p(bn_b), _p(out), _p(ws),
          N, H * W, C, Cl, S, ACT[act], _stream())
    return out


def cond_instnorm_bwd(g, y, stats, sid, embed, bn_w, bn_b, act="none", dembed=None, dbn_w=None, dbn_b=None,
                      dbias=None, accumulate=True):
    """dx of cond_instnorm_fwd; dembed [S, 2*Cl] (every row), dbn_w, dbn_b, dbias [Cl] written or accumulated."""
    S, Cl = _cond_check(y, stats, sid, embed, bn_w, bn_b, act)
    _dev_check(g, dembed, dbn_w, dbn_b, dbias)
    N, H, W, C = y.shape
    if g.shape != y.shape or (dembed is not None and dembed.numel() != S * 2 * Cl) or \
            any(t is not None and t.numel() != Cl for t in (dbn_w, dbn_b, dbias)):
        raise ValueError("cond_instnorm_bwd: g as y, dembed [S, 2*Cl], dbn_w / dbn_b / dbias [Cl]")
    dx = torch.empty_like(y)
    nbytes = lib().vst_cond_instnorm_ws_bytes(N, H * W, C)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=y.device)
    _call("vst_cond_instnorm_bwd", _p(g), _p(y), _p(stats), _p(sid), _p(embed), _p(bn_w), _p(bn_b), _p(dx),
          _p(dembed), _p(dbn_w), _p(dbn_b), _p(dbias), _p(ws), N, H * W, C, Cl, S, ACT[act],
          1 if accumulate else 0, _stream())
    return dx


def _adain_check(y, stats, h, act):
    _dev_check(y, stats, h)
    if y.dim() != 4 or tuple(stats.shape) != (y.shape[0], y.shape[-1], 2) or \
            tuple(h.shape) != (y.shape[0], 2 * y.shape[-1]):
        raise ValueError("adain: y NHWC [N, H, W, C] with stats [N, C, 2] and h [N, 2*C], got %s, %s, %s" %
                         (tuple(y.shape), tuple(stats.shape), tuple(h.shape)))
    if act not in ("none", "lrelu"):
        raise ValueError("adain: act must be 'none' or 'lrelu'")


def _adain_ws(N, HW, C, device):
    nbytes = lib().vst_adain_ws_bytes(N, HW, C)
    if nbytes == 0:
        raise ValueError("adain: C = %d is not a multiple of 4 up to 1024" % C)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def adain_fwd(y, stats, h, act="none", slope=0.2):
    """act((1 + gamma) * IN(y) + beta), {gamma, beta} = the halves of h[n] (vst_adain_fwd); h [N, 2*C] is the
    style projection fc(s), stats from instnorm_stats."""
    _adain_check(y, stats, h, act)
    N, H, W, C = y.shape
    out = torch.empty_like(y)
    ws = torch.empty((N, C, 2), device=y.device)
    _call("vst_adain_fwd", _p(y), _p(stats), _p(h), _p(out), _p(ws), N, H * W, C, ACT[act], float(slope), _stream())
    return out


def adain_bwd(g, y, stats, h, act="none", slope=0.2, dh=None, dbias=None, accumulate=False):
    """dx of adain_fwd; dh [N, 2*C] and dbias [C] (the bias gradient of the conv that made y), each optional,
    written or accumulated."""
    _adain_check(y, stats, h, act)
    _dev_check(g, dh, dbias)
    N, H, W, C = y.shape
    if g.shape != y.shape or (dh is not None and dh.shape != h.shape) or (dbias is not None and dbias.numel() != C):
        raise ValueError("adain_bwd: g as y, dh as h, dbias [C]")
    dx = torch.empty_like(y)
    ws = _adain_ws(N, H * W, C, y.device)
    _call("vst_adain_bwd", _p(g), _p(y), _p(stats), _p(h), _p(dx), _p(dh), _p(dbias), _p(ws), N, H * W, C, ACT[act],
          float(slope), 1 if accumulate else 0, _stream())
    return dx


def act_fwd(x, act, slope=0.0):
    """act(x) of a tensor whose element count is a multiple of 4 (vst_act_fwd; backward: act_bwd)."""
    _dev_check(x)
    y = torch.empty_like(x)
    _call("vst_act_fwd", _p(x), _p(y), x.numel(), ACT[act], float(slope), _stream())
    return y


def avgpool2(x):
    """F.avg_pool2d(x, 2) of NHWC x with even H and W (vst_avgpool2_fwd)."""
    _dev_check(x)
    N, H, W, C = x.shape
    if H % 2 or W % 2 or C % 4:
        raise ValueError("avgpool2: even H and W and C %% 4 == 0, got %s" % (tuple(x.shape),))
    y = torch.empty((N, H // 2, W // 2, C), device=x.device)
    _call("vst_avgpool2_fwd", _p(x), _p(y), N, H // 2, W // 2, C, _stream())
    return y


def avgpool2_bwd(gy):
    _dev_check(gy)
    N, H, W, C = gy.shape
    gx = torch.empty((N, 2 * H, 2 * W, C), device=gy.device)
    _call("vst_avgpool2_bwd", _p(gy), _p(gx), N, H, W, C, _stream())
    return gx


MERGE = {"same": _C["VST_MERGE_SAME"], "pool": _C["VST_MERGE_POOL"], "up": _C["VST_MERGE_UP"]}


def _merge_b_shape(a_shape, mode):
    N, H, W, C = a_shape
    if mode not in MERGE:
        raise ValueError("merge: mode must be one of %s" % sorted(MERGE))
    if mode == "up" and (H % 2 or W % 2):
        raise ValueError("merge 'up': a must have even H and W, got %s" % (tuple(a_shape),))
    return {"same": (N, H, W, C), "pool": (N, 2 * H, 2 * W, C), "up": (N, H // 2, W // 2, C)}[mode]


def merge(a, b, mode="same", scale=2 ** -0.5):
    """(a + f(b)) * scale, NHWC (vst_merge_fwd): f = identity ('same'), avg_pool2d(., 2) ('pool': b at twice a's
    resolution) or nearest 2x upsampling ('up': b at half a's resolution)."""
    _dev_check(a, b)
    if a.dim() != 4 or a.shape[-1] % 4 or tuple(b.shape) != _merge_b_shape(a.shape, mode):
        raise ValueError("merge %r: a %s and b %s do not fit (C %% 4 == 0)" % (mode, tuple(a.shape), tuple(b.shape)))
    lo = b if mode == "up" else a
    out = torch.empty_like(a)
    _call("vst_merge_fwd", _p(a), _p(b), _p(out), lo.shape[0], lo.shape[1], lo.shape[2], lo.shape[3], MERGE[mode],
          float(scale), _stream())
    return out


def merge_bwd(g, mode="same", scale=2 ** -0.5):
    """(ga, gb) of merge from out's gradient g, one pass over g (vst_merge_bwd)."""
    _dev_check(g)
    bs = _merge_b_shape(g.shape, mode)
    ga, gb = torch.empty_like(g), torch.empty(bs, device=g.device)
    lo = bs if mode == "up" else g.shape
    _call("vst_merge_bwd", _p(g), _p(ga), _p(gb), lo[0], lo[1], lo[2], lo[3], MERGE[mode], float(scale), _stream())
    return ga, gb


def upsample2x(x):
    _dev_check(x)
    N, H, W, C = x.shape
    y = torch.empty((N, 2 * H, 2 * W, C), device=x.device)
    _call("vst_upsample2x_fwd", _p(x), _p(y), N, H, W, C, _stream())
    return y


def upsample2x_bwd(gy):
    _dev_check(gy)
    N, H2, W2, C = gy.shape
    gx = torch.empty((N, H2 // 2, W2 // 2, C), device=gy.device)
    _call("vst_upsample2x_bwd", _p(gy), _p(gx), N, H2 // 2, W2 // 2, C, _stream())
    return gx


def scaled_tanh(x, cl=3):
    _dev_check(x)
    y = torch.empty_like(x)
    _call("vst_scaled_tanh_fwd", _p(x), _p(y), x.numel() // x.shape[-1], x.shape[-1], cl, _stream())
    return y


def scaled_tanh_bwd(x, gy, cl=3):
    _dev_check(x, gy)
    gx = torch.empty_like(x)
    _call("vst_scaled_tanh_bwd", _p(x), _p(gy), _p(gx), x.numel() // x.shape[-1], x.shape[-1], cl,
          _stream())
    return gx


def channel_normalize(x, mean, std, d0=1.0, cl=3, backward=False):
    """((x / d0) - mean[c]) / std[c] (backward: (x / std[c]) / d0); mean/std device tensors [cl]."""
    _dev_check(x, mean, std)
    y = torch.empty_like(x)
    _call("vst_channel_normalize", _p(x), _p(y), _p(mean), _p(std), float(d0),
          x.numel() // x.shape[-1], x.shape[-1], cl, 1 if backward else 0, _stream())
    return y


def maxpool2(x):
    _dev_check(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), device=x.device)
    _call("vst_maxpool2_fwd", _p(x), _p(y), N, H, W, C, _stream())
    return y


def maxpool2_bwd(gy, x):
    _dev_check(gy, x)
    N, H, W, C = x.shape
    gx = torch.empty_like(x)
    _call("vst_maxpool2_bwd", _p(gy), _p(x), _p(gx), N, H, W, C, _stream())
    return gx


def loss_mse(a, b, scale=1.0, cl=None, out=None, accumulate=False):
    """scale * mean((a - b)^2) over the cl logical channels (default all)."""
    _dev_check(a, b)
    cs = a.shape[-1]
    npix = a.numel() // cs
    loss = out if out is not None else torch.zeros((), device=a.device)
    _call("vst_loss_mse", _p(a), _p(b), _p(loss), _p(_part(npix, a.device)), npix, cs, cl or cs,
          float(scale), 1 if accumulate else 0, _stream())
    return loss


def loss_mse_bwd(a, b, gout, scale=1.0, cl=None, grad=None):
    cs = a.shape[-1]
    npix = a.numel() // cs
    acc = grad is not None
    g = grad if acc else torch.empty_like(a)
    _call("vst_loss_mse_bwd", _p(a), _p(b), _p(gout), _p(g), npix, cs, cl or cs, float(scale),
          1 if acc else 0, _stream())
    return g


def loss_tv(img, scale=1.0, cl=3):
    _dev_check(img)
    N, H, W, C = img.shape
    loss = torch.zeros((), device=img.device)
    _call("vst_loss_tv", _p(img), _p(loss), _p(_part(N * (H - 1) * (W - 1), img.device)), N, H, W, C, cl,
          float(scale), 0, _stream())
    return loss


def loss_tv_bwd(img, gout, scale=1.0, cl=3):
    N, H, W, C = img.shape
    g = torch.empty_like(img)
    _call("vst_loss_tv_bwd", _p(img), _p(gout), _p(g), N, H, W, C, cl, float(scale), _stream())
    return g


def gram(f, role="fwd"):
    """G[b] = F_b^T F_b / (h*w) for NHWC features f [B][h][w][C] -> [B][C][C]
    (fast_style_transfer.py:813-817).  Each G[b] is the weight gradient of a 1x1 conv whose input
    and output gradient are both F_b, i.e. the split-K MFMA wgrad kernel."""
    _dev_check(f)
    B, h, w, C = f.shape
    G = torch.empty((B, C, C), device=f.device)
    for b in range(B):
        fb = f[b:b + 1]
        conv2d_wgrad(fb, fb, G[b], None, 1, 1, 1, 0, "zero", C, C, C, 1, accumulate=False, role=role)
    axpby(G, G, 1.0 / (h * w), 0.0)
    return G


def split_planes(wp):
    """Attach the bf16 split planes (vst_weight_split) the split-arithmetic conv paths read."""
    split = torch.empty((3,) + tuple(wp.shape), device=wp.device, dtype=torch.bfloat16)
    _call("vst_weight_split", _p(wp), _p(split), wp.numel(), _stream())
    wp.vst_split = split
    return wp


def gram_bwd(f, dG, role="bwd"):
    """dF_b = F_b (dG_b + dG_b^T) / (h*w): a 1x1 conv of F_b with weight S_b (vst_gram_sym)."""
    _dev_check(f, dG)
    B, h, w, C = f.shape
    df = torch.empty_like(f)
    for b in range(B):
        S = torch.empty((C, 1, 1, C), device=f.device)
        _call("vst_gram_sym", _p(dG[b]), _p(S), C, float(1.0 / (h * w)), _stream())
        split_planes(S)
        conv2d_fwd(f[b:b + 1], S, None, C, 1, 1, 1, 0, out=df[b:b + 1], role=role)
    return df


def corr_pyramid_floats(P, H2, W2, ld0, levels):
    return lib().vst_corr_pyramid_floats(P, H2, W2, ld0, levels)


def corr_pyramid(pyr, P, H2, W2, ld0, levels):
    _call("vst_corr_pyramid", _p(pyr), P, H2, W2, ld0, levels, _stream())


def corr_lookup(pyr, coords, B, H1, W1, H2, W2, ld0, levels, radius, cs=None):
    """cs: the output channel stride (default cpad; the padded channels are written as zeros)."""
    _dev_check(pyr, coords)
    K = 2 * radius + 1
    cs = cs or cpad(levels * K * K)
    out = torch.empty((B, H1, W1, cs), device=pyr.device)
    _call("vst_corr_lookup", _p(pyr), _p(coords), _p(out), B, H1, W1, H2, W2, ld0, levels, radius, cs,
          _stream())
    return out


def altcorr_pyramid_floats(B, H, W, Dp, levels):
    """Floats of the pooled fmap2 levels 1..levels-1 (-1 for levels outside 1..8)."""
    return lib().vst_altcorr_pyramid_floats(B, H, W, Dp, levels)


def altcorr_pyramid(f2, pyr, levels):
    """Fill pyr (altcorr_pyramid_floats floats) with the 2x2 average-pooled levels of NHWC f2."""
    _dev_check(f2, pyr)
    B, H, W, Dp = f2.shape
    _call("vst_altcorr_pyramid", _p(f2), _p(pyr), B, H, W, Dp, levels, _stream())


def altcorr_lookup(f1, f2, pyr, coords, D, levels, radius, cs=None):
    """AlternateCorrBlock window features [B, H, W, cs] from NHWC f1, f2 [B, H, W, Dp] and f2's pooled levels;
    cs: the output channel stride (default cpad; the padded channels are written as zeros)."""
    _dev_check(f1, f2, pyr, coords)
    B, H, W, Dp = f1.shape
    K = 2 * radius + 1
    cs = cs or cpad(levels * K * K)
    out = torch.empty((B, H, W, cs), device=f1.device)
    _call("vst_altcorr_lookup", _p(f1), _p(f2), _p(pyr), _p(coords), _p(out), B, H, W, Dp, D, levels, radius, cs,
          _stream())
    return out


# -------------------------------------------------------------------------------- StarGAN
def concat_label_nhwc(x, label, cs=None):
    """NCHW x [N,Cx,H,W] + label [N,Cl] -> NHWC [N,H,W,cs] (StarGAN model.py:59-64)."""
    _dev_check(x, label)
    N, Cx, H, W = x.shape
    Cl = label.shape[1]
    cs = cs or cpad(Cx + Cl)
    y = torch.empty((N, H, W, cs), device=x.device)
    _call("vst_concat_label_nhwc", _p(x), _p(label), _p(y), N, Cx, Cl, H, W, cs, _stream())
    return y


def instnorm_running_update(stats, running_mean, running_var, HW, momentum=0.1):
    _dev_check(stats, running_mean, running_var)
    N, C, _ = stats.shape
    _call("vst_instnorm_running_update", _p(stats), _p(running_mean), _p(running_var), N, C, HW,
          float(momentum), IN_EPS, _stream())


def instnorm_stats_from_running(running_mean, running_var, N):
    _dev_check(running_mean, running_var)
    C = running_mean.numel()
    stats = torch.empty((N, C, 2), device=running_mean.device)
    _call("vst_instnorm_stats_from_running", _p(running_mean), _p(running_var), _p(stats), N, C, IN_EPS,
          _stream())
    return stats


# -------------------------------------------------------------------------------- formats
def fc2_unpack(raw):
    """raw float32 [B,H,W,9] FC2 block on the device -> (img1 NHWC4, img2 NHWC4, mask [B,1,H,W],
    flow [B,2,H,W]) as the CycleGANCon step consumes them (fc2_dataset.py:35-41)."""
    _dev_check(raw)
    B, H, W, nine = raw.shape
    if nine != 9 or raw.dtype != torch.float32 or not raw.is_contiguous():
        raise ValueError("fc2_unpack: expected contiguous float32 [B,H,W,9]")
    img1 = torch.empty((B, H, W, 4), device=raw.device)
    img2 = torch.empty((B, H, W, 4), device=raw.device)
    mask = torch.empty((B, 1, H, W), device=raw.device)
    flow = torch.empty((B, 2, H, W), device=raw.device)
    _call("vst_fc2_unpack", _p(raw), _p(img1), _p(img2), _p(mask), _p(flow), B, H, W, _stream())
    return img1, img2, mask, flow


def u8_image_to_nhwc4(x):
    """uint8 [B,H,W,3] on the device -> ToTensor + Normalize(0.5, 0.5) as float32 NHWC4."""
    if not x.is_cuda:
        raise RuntimeError("vst ops require GPU tensors (no CPU fallback)")
    if x.dtype != torch.uint8 or x.shape[-1] != 3 or not x.is_contiguous():
        raise ValueError("u8_image_to_nhwc4: expected contiguous uint8 [..., 3]")
    y = torch.empty(tuple(x.shape[:-1]) + (4,), device=x.device)
    _call("vst_u8_image_to_nhwc4", _p(x), _p(y), x.numel() // 3, _stream())
    return y


# ----------------------------------------------------------------------------------- RAFT
def conv2d_fwd_hw(x, wp, bias, cop, R, S, stride, pad_h, pad_w, act="none", role="fwd"):
    """Forward conv with separate row / column zero padding (RAFT's SepConvGRU (1,5) / (5,1) convs)."""
    return _fwd_ex(x, wp, bias, cop, R, S, stride, pad_h, pad_w, "zero", act, 0.0, role, FWD_HW_SPLITK)


def raft_prep(img, pads, nhwc=False, out=None):
    """[B,3,H,W] NCHW (or NHWC [B,H,W,Cs>=3] with nhwc=True) -> replicate pad (l, r, t, b) +
    2*(x/255)-1 -> NHWC4 (written into ``out`` when given)."""
    _dev_check(img, out)
    l, r, t, b = pads
    if nhwc:
        B, H, W, cs = img.shape
    else:
        B, C, H, W = img.shape
        if C != 3:
            raise ValueError("raft_prep: expected 3-channel images")
    shape = (B, H + t + b, W + l + r, 4)
    if out is None:
        out = torch.empty(shape, device=img.device)
    elif tuple(out.shape) != shape:
        raise ValueError("raft_prep: out has shape %s, expected %s" % (tuple(out.shape), shape))
    if nhwc:
        _call("vst_raft_prep_nhwc", _p(img), cs, _p(out), B, H, W, l, r, t, b, _stream())
        return out
    _call("vst_raft_prep", _p(img), _p(out), B, H, W, l, r, t, b, _stream())
    return out


def add_relu(a, b, out=None):
    _dev_check(a, b, out)
    y = out if out is not None else torch.empty_like(a)
    _call("vst_add_relu", _p(a), _p(b), _p(y), a.numel(), _stream())
    return y


def copy_channels(src, src_c0, dst, dst_c0, nc):
    _dev_check(src, dst)
    npix = src.numel() // src.shape[-1]
    if dst.numel() // dst.shape[-1] != npix:
        raise ValueError("copy_channels: pixel counts differ")
    _call("vst_copy_channels", _p(src), src.shape[-1], src_c0, _p(dst), dst.shape[-1], dst_c0, nc, npix, _stream())


def raft_ctx_split(c, hdim, cdim, h, hx, rhx):
    _dev_check(c, h, hx, rhx)
    npix = c.numel() // c.shape[-1]
    _call("vst_raft_ctx_split", _p(c), c.shape[-1], hdim, cdim, _p(h), _p(hx), _p(rhx), hx.shape[-1], npix,
          _stream())


def raft_flow4(coords1, flow4):
    _dev_check(coords1, flow4)
    B, _, h, w = coords1.shape
    _call("vst_raft_flow4", _p(coords1), _p(flow4), B, h, w, _stream())


def raft_motion(out, nout, flow4, hx, rhx, c0):
    _dev_check(out, flow4, hx, rhx)
    npix = out.numel() // out.shape[-1]
    _call("vst_raft_motion", _p(out), out.shape[-1], nout, _p(flow4), _p(hx), _p(rhx), hx.shape[-1], c0, npix,
          _stream())


def _gru_check(what, zr, h, q=None):
    """The GRU kernels take no channel strides: zr is [P][2*hd] and h, q are [P][hd], densely packed (a conv
    output whose padded width is not 2*hd would be read skewed)."""
    hd = h.shape[-1]
    if zr.shape[-1] != 2 * hd or zr.numel() != 2 * h.numel():
        raise ValueError("%s: zr %s must be [..., 2*hd] over h's pixels, h is %s"
                         % (what, tuple(zr.shape), tuple(h.shape)))
    if q is not None and tuple(q.shape) != tuple(h.shape):
        raise ValueError("%s: q %s and h %s differ" % (what, tuple(q.shape), tuple(h.shape)))


def gru_reset(zr, h, rhx):
    _gru_check("gru_reset", zr, h)
    _dev_check(zr, h, rhx)
    hd = h.shape[-1]
    _call("vst_gru_reset", _p(zr), _p(h), _p(rhx), hd, rhx.shape[-1], h.numel() // hd, _stream())


def gru_update(zr, q, h, hx):
    _gru_check("gru_update", zr, h, q)
    _dev_check(zr, q, h, hx)
    hd = h.shape[-1]
    _call("vst_gru_update", _p(zr), _p(q), _p(h), _p(hx), hd, hx.shape[-1], h.numel() // hd, _stream())


def raft_coords_update(coords1, delta):
    _dev_check(coords1, delta)
    B, _, h, w = coords1.shape
    _call("vst_raft_coords_update", _p(coords1), _p(delta), delta.shape[-1], B, h, w, _stream())


def raft_upsample(coords1, mask):
    _dev_check(coords1, mask)
    B, _, h, w = coords1.shape
    out = torch.empty((B, 2, 8 * h, 8 * w), device=coords1.device)
    _call("vst_raft_upsample", _p(coords1), _p(mask), mask.shape[-1], _p(out), B, h, w, _stream())
    return out


def loss_masked_l1(a, b, mask, scale, cl):
    """scale * mean(mask * |a - b|) over cl logical channels of NHWC a, b; mask [B,1,H,W] / [B,H,W] or None."""
    _dev_check(a, b, mask)
    npix = a.numel() // a.shape[-1]
    loss = torch.empty((), device=a.device)
    _call("vst_loss_masked_l1", _p(a), _p(b), _p(mask), _p(loss), _p(_part(npix, a.device)), npix, a.shape[-1], cl,
          float(scale), _stream())
    return loss


def loss_masked_l1_bwd(a, b, mask, gout, scale, cl):
    _dev_check(a, b, mask, gout)
    npix = a.numel() // a.shape[-1]
    grad = torch.empty_like(a)
    _call("vst_loss_masked_l1_bwd", _p(a), _p(b), _p(mask), _p(gout), _p(grad), npix, a.shape[-1], cl, float(scale),
          _stream())
    return grad


# ----------------------------------------------------------------------- tap-GEMM convolutions
# VST_TAP_CHUNK_MB > 0 runs the tap GEMMs' R*R*4-wide intermediates (411 MB for 8 images at 256^2,
# 7x7) in chunks of images sized for the 256 MB Infinity Cache, each chunk overwriting one buffer.
# Off by default: the C2 step A/B measured 63.15-63.27 ms with 128 MB chunks, 64.12 with 64 MB,
# 62.85-62.87 in one pass (the smaller GEMM launches lose more than the cache hits save).
TAP_CHUNK_BYTES = 0
# tap_conv_wgrad: the folded dy written as the x6 wgrad's bf16 planes (vst_tapfold_planes);
# False writes the fp32 D and lets the wgrad copy it into planes.
TAP_PLANES = True
# The generator's last-layer weight gradient as the swapped GEMM (tap_conv_wgrad_swap); False:
# the R x 1 form (tap_conv_wgrad_h).
TAP_SWAP = True


def _tap_chunks(N, per_image_bytes):
    n = N if TAP_CHUNK_BYTES <= 0 else max(1, min(N, TAP_CHUNK_BYTES // max(1, per_image_bytes)))
    return [(i, min(N, i + n)) for i in range(0, N, n)]


def tap_conv_fwd(x, ck, bias, R, pad, pad_mode="zero", act="none", slope=0.0, role="fwd"):
    """'same' conv with <= 4 output channels on the MFMA kernel (see vst_tapsum_fwd): ck is the
    VST_PACK_CK pack [R][S][4][Ci] of the weight, bias padded to 4 (or None); returns NHWC4."""
    _dev_check(x, ck, bias)
    N, H, W, Cx = x.shape
    if ck.shape != (R, R, 4, Cx):
        raise ValueError("tap_conv_fwd: CK pack shape %s does not match R=%d, Cx=%d" % (tuple(ck.shape), R, Cx))
    y = torch.empty((N, H, W, 4), device=x.device)
    chunks = _tap_chunks(N, H * W * R * R * 16)
    zbuf = torch.empty((chunks[0][1], H, W, R * R * 4), device=x.device)
    for a, b in chunks:
        z = conv2d_fwd(x[a:b], ck, None, R * R * 4, 1, 1, 1, 0, "zero", role=role, out=zbuf[:b - a])
        _call("vst_tapsum_fwd", _p(z), R * R * 4, _p(bias), _p(y[a:b]), b - a, H, W, R, R, pad, PAD[pad_mode],
              ACT[act], float(slope), _stream())
    return y


def tap_conv_fwd_h(x, sok, bias, R, pad, pad_mode="zero", act="none", slope=0.0, role="fwd"):
    """The same conv as tap_conv_fwd with the (r, ci) contraction on the matrix cores and only the column
    taps summed afterwards (vst_tapconv_h_fwd): sok = the VST_PACK_SOK pack [S*4][R][1][Ci]."""
    _dev_check(x, sok, bias)
    N, H, W, Cx = x.shape
    if sok.shape != (R * 4, R, 1, Cx):
        raise ValueError("tap_conv_fwd_h: SOK pack shape %s does not match R=%d, Cx=%d" % (tuple(sok.shape), R, Cx))
    Ho, Wo = H + 2 * pad - R + 1, W + 2 * pad - R + 1
    y = torch.empty((N, Ho, Wo, 4), device=x.device)
    z = torch.empty((N, Ho, W, R * 4), device=x.device)
    _call("vst_tapconv_h_fwd", _p(x), _p(sok), _p(getattr(sok, "vst_split", None)), _p(bias), _p(z), _p(y), N, H, W,
          Cx, R, pad, PAD[pad_mode], ACT[act], float(slope), _math(role), _stream())
    return y


def tap_conv_wgrad_bf_ok(x, R, role="bwd"):
    """Does tap_conv_wgrad's own GEMM (the 1x1 weight gradient of the 4 R R folded dy channels against x) run on
    the split-bf16 kernel, which reads x's unpadded channel-major image (x_t) and the folded dy as planes?"""
    N, H, W, Cx = x.shape
    return conv_plan_wgrad(N, H, W, Cx, H, W, R * R * 4, 1, 1, 1, role)[0] == WPLAN_BF


def tap_conv_wgrad(x, dy, dw, R, pad, pad_mode="zero", accumulate=True, role="bwd", x_t=None):
    """dw [Co<=4][Ci][R][R] (+)= weight gradient of tap_conv_fwd given dy NHWC4 (pre-activation).
    x_t: x's unpadded channel-major image (instnorm_act_fwd(cp=(0, "zero", 1))) for the x6 path."""
    _dev_check(x, dy, dw)
    N, H, W, Cx = x.shape
    Co, Ci = dw.shape[0], dw.shape[1]
    K = R * R * 4
    if TAP_PLANES and TAP_CHUNK_BYTES <= 0 and tap_conv_wgrad_bf_ok(x, R, role):
        # D straight as the x6 wgrad's bf16 planes (vst_tapfold_planes): no fp32 D, no plane copy
        P = N * H * W
        ldp = lib().vst_cp_ld(P)
        pl = torch.empty((3, K, ldp), device=x.device, dtype=torch.bfloat16)
        _call("vst_tapfold_planes", _p(dy), _p(pl), ldp, N, H, W, R, R, pad, PAD[pad_mode], _stream())
        t = torch.empty((K, Ci), device=x.device)
        nbytes = lib().vst_conv2d_wgrad_ws_bytes(N, H, W, Cx, H, W, K, 1, 1, 1)
        ws = torch.empty((nbytes + 3) // 4, device=x.device)
        _call("vst_conv2d_wgrad_pre", _p(x), _p(x_t), _p(pl), _p(pl), _p(t), _p(ws), nbytes, N, H, W, Cx, H, W, K, 1, 1, 1,
              0, PAD["zero"], K, Ci, Ci, 1, 0, _math(role), _stream())
        _call("vst_tap_wgrad_scatter", _p(t), _p(dw), Co, Ci, R, R, 1 if accumulate else 0, _stream())
        return
    chunks = _tap_chunks(N, H * W * R * R * 16)
    dbuf = torch.empty((chunks[0][1], H, W, R * R * 4), device=x.device)
    t = torch.empty((R * R * 4, Ci), device=x.device)
    for a, b in chunks:
        d = dbuf[:b - a]
        _call("vst_tapfold", _p(dy[a:b]), _p(d), b - a, H, W, R, R, pad, PAD[pad_mode], _stream())
        conv2d_wgrad(x[a:b], d, t, None, 1, 1, 1, 0, "zero", R * R * 4, Ci, Ci, 1, accumulate=a > 0, role=role)
    _call("vst_tap_wgrad_scatter", _p(t), _p(dw), Co, Ci, R, R, 1 if accumulate else 0, _stream())


def tap_conv_wgrad_h_ok(x, R, pad, pad_mode, role="bwd"):
    """Does tap_conv_wgrad_h take this shape: a reflect 'same' conv whose R x 1 wgrad frame (W+R+1 wide)
    runs on the x6 split-bf16 kernel without padded rows."""
    N, H, W, Cx = x.shape
    return (pad_mode == "reflect" and 2 * pad == R - 1 and pad + 1 < min(H, W) and
            conv_plan_wgrad(N, H, W, Cx, H + 2, W + R + 1, 4 * R, R, 1, 1, role)[0] == WPLAN_BF)


def tap_conv_wgrad_h(x, dy, dw, R, pad, pad_mode="reflect", accumulate=True, role="bwd", x_t=None):
    """tap_conv_wgrad as the R x 1 conv's weight gradient (vst_tapshift_planes): dy's column-shifted copies
    as 4R channels over the (H+2) x (W+R+1) frame, x padded by pad+1.  x_t: x's channel-major image padded
    by pad+1, reflect (instnorm_act_fwd(cp=(pad + 1, "reflect", 1))), or None."""
    _dev_check(x, dy, dw)
    N, H, W, Cx = x.shape
    Co, Ci = dw.shape[0], dw.shape[1]
    K = 4 * R
    Ho, Wo = H + 2, W + R + 1
    ldp = lib().vst_cp_ld(N * Ho * Wo)
    pl = torch.empty((3, K, ldp), device=x.device, dtype=torch.bfloat16)
    _call("vst_tapshift_planes", _p(dy), _p(pl), ldp, N, H, W, R, _stream())
    t = torch.empty((K, Ci, R), device=x.device)
    nbytes = lib().vst_conv2d_wgrad_ws_bytes(N, H, W, Cx, Ho, Wo, K, R, 1, 1)
    ws = torch.empty((nbytes + 3) // 4, device=x.device)
    _call("vst_conv2d_wgrad_pre", _p(x), _p(x_t), _p(pl), _p(pl), _p(t), _p(ws), nbytes, N, H, W, Cx, Ho, Wo, K, R, 1,
          1, pad + 1, PAD["reflect"], K, Ci, Ci * R, R, 0, _math(role), _stream())
    _call("vst_tap_wgrad_scatter_h", _p(t), _p(dw), Co, Ci, R, R, 1 if accumulate else 0, _stream())


def tap_swap_geom(W, R):
    """(wx, frame width) of tap_conv_wgrad_swap: the (W+R-1)-wide reflect-padded x rows get wx zero
    columns so that every row is whole 8-pixel chunks."""
    wx = (8 - (W + R - 1) % 8) % 8
    return wx, W + R - 1 + wx


def tap_conv_wgrad_swap_ok(x, R, pad, pad_mode, role="bwd", co=4):
    """Does tap_conv_wgrad_swap take this shape: a reflect 'same' conv whose swapped GEMM (the R x R wgrad
    of the dy channels against x's padded frame as Ci outputs) runs on the x6 split-bf16 kernel.  co: the
    layer's real output channels — vst_tap_wgrad_swap runs the GEMM over 3 dy channels when co <= 3, 4
    otherwise, and the plan is queried with that same count."""
    N, H, W, Cx = x.shape
    wx, Wq = tap_swap_geom(W, R)
    cx = 3 if co <= 3 else 4
    return (TAP_SWAP and pad_mode == "reflect" and 2 * pad == R - 1 and pad < min(H, W) and Cx % 4 == 0 and
            conv_plan_wgrad(N, H, W + wx, cx, H + R - 1, Wq, Cx, R, R, 1, role)[0] == WPLAN_BF)


def tap_conv_wgrad_swap(x, dy, dw, R, pad, pad_mode="reflect", accumulate=True, role="bwd", x_pl=None, db=None):
    """tap_conv_wgrad with the GEMM's roles swapped (vst_tap_wgrad_swap): M = R*R*3 (tap, co) rows of the
    zero-padded dy against x's reflect-padded frame as Cx columns.  x_pl: that frame's bf16 planes as the
    IN apply writes them (instnorm_act_fwd(xpl=(pad, "reflect", wx))); None: made here from x."""
    _dev_check(x, dy, dw)
    N, H, W, Cx = x.shape
    Co, Ci = dw.shape[0], dw.shape[1]
    if pad_mode != "reflect" or 2 * pad != R - 1:
        raise NotImplementedError("tap_conv_wgrad_swap: reflect 'same' convs only")
    if tuple(dy.shape) != (N, H, W, 4) or Co > 4 or Ci != Cx:
        raise ValueError("tap_conv_wgrad_swap: dy %s / dw %s do not match x %s" % (tuple(dy.shape), tuple(dw.shape),
                                                                               tuple(x.shape)))
    if x_pl is None:  # the identity IN (mean 0, rstd 1): a == x, plus the planes
        st = torch.zeros((N, Cx, 2), device=x.device)
        st[..., 1] = 1.0
        _, x_pl = instnorm_act_fwd(x, st, "none", xpl=(pad, "reflect", tap_swap_geom(W, R)[0]))
    ld = lib().vst_tap_wgrad_swap_ld(N, H, W, R)
    if x_pl.shape != (3, Cx, ld) or x_pl.dtype != torch.bfloat16:
        raise ValueError("tap_conv_wgrad_swap: x planes %s do not match (3, %d, %d) bf16" % (tuple(x_pl.shape), Cx, ld))
    nbytes = lib().vst_tap_wgrad_swap_ws_bytes(N, H, W, Cx, R)
    ws = torch.empty((nbytes + 3) // 4, device=x.device)
    # db: the bias gradient (+)= the channel sums of dy, taken by the same pass (vst_tap_wgrad_swap_db)
    _call("vst_tap_wgrad_swap_db", _p(dy), _p(x_pl), _p(dw), _p(db), _p(ws), nbytes, N, H, W, Cx, R, Co,
          1 if accumulate else 0, _math(role), _stream())


def tap_conv_dgrad(dy, kc, R, pad, pad_mode="zero", role="bwd"):
    """Data gradient (NHWC4) of a 'same' conv with <= 4 input channels: kc = VST_PACK_KC pack
    [R][R][4][Cy] of its weight (see vst_tapgather)."""
    _dev_check(dy, kc)
    N, H, W, Cy = dy.shape
    if kc.shape != (R, R, 4, Cy):
        raise ValueError("tap_conv_dgrad: KC pack shape %s does not match R=%d, Cy=%d" % (tuple(kc.shape), R, Cy))
    y = torch.empty((N, H, W, 4), device=dy.device)
    chunks = _tap_chunks(N, H * W * R * R * 16)
    zbuf = torch.empty((chunks[0][1], H, W, R * R * 4), device=dy.device)
    for a, b in chunks:
        z = conv2d_fwd(dy[a:b], kc, None, R * R * 4, 1, 1, 1, 0, "zero", role=role, out=zbuf[:b - a])
        _call("vst_tapgather", _p(z), _p(y[a:b]), b - a, H, W, R, R, pad, PAD[pad_mode], _stream())
    return y


def dgrad_sok_pack(w, ci_real=None):
    """VST_PACK_SOK pack of the data gradient of a conv with <= 4 input channels, w [Co][Ci][R][S]: the
    conv dy -> dx over the taps rotated 180 deg, w_d[o = ci][i = co][r][s] = w[co][ci][R-1-r][S-1-s].
    ci_real: only the first ci_real (<= 4) input channels' gradient (the others' is not wanted)."""
    Co, Ci, R, S = w.shape
    Ci = ci_real or Ci
    pb = PackBatch._active
    if pb is not None:  # straight from w: transposed strides + reversed tap maps
        return pb.add(w, PACK_SOK, Ci, Co, R, S, (R * S, w.shape[1] * R * S, S, 1), list(range(R - 1, -1, -1)),
                      list(range(S - 1, -1, -1)), Op=4)
    return weight_pack(w.detach()[:, :Ci].permute(1, 0, 2, 3).flip(2, 3).contiguous(), PACK_SOK, Op=4)


def tap_conv_dgrad_h(dy, sokd, R, pad, pad_mode="zero", role="bwd"):
    """Data gradient (NHWC4) of a 'same' conv with <= 4 input channels via vst_tapconv_h_fwd: the full
    correlation of dy with the rotated taps (sokd = dgrad_sok_pack(w); zero pad R-1), then the reflect fold
    (reflect padding) or the interior crop (zero padding)."""
    _dev_check(dy, sokd)
    if pad_mode == "reflect" and pad != (R - 1) // 2:
        raise NotImplementedError("tap_conv_dgrad_h: reflect padding %d with R=%d (only 'same', (R-1)/2)" % (pad, R))
    full = tap_conv_fwd_h(dy, sokd, None, R, R - 1, "zero", role=role)
    if pad_mode == "reflect":
        return reflect_fold(full, pad)
    o = R - 1 - pad
    return full[:, o:full.shape[1] - o, o:full.shape[2] - o].contiguous()


def convT3s2_phase_packs(wt):
    """Phase weight packs of a ConvTranspose2d(k=3, stride=2, padding=1, output_padding=1) weight
    wt [Ci][Co][3][3]: output parity a (rows) / b (cols) uses taps k=1 (even) or k=(2, 0) at input
    offsets (0, +1) (odd).  Returns the VST_PACK_OK packs of the 1x1, 1x2, 2x1, 2x2 phase convs."""
    pb = PackBatch._active
    if pb is not None:  # packed straight from wt (transposed view + tap maps), no copies
        Ci, Co = wt.shape[0], wt.shape[1]
        st = (9, Co * 9, 3, 1)  # logical [o = co][i = ci][a][b] of wt[ci][co][kh][kw]
        return [pb.add(wt, PACK_OK, Co, Ci, 1 + a, 1 + b, st, [2, 0] if a else [1], [2, 0] if b else [1])
                for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
    wc = wt.detach().permute(1, 0, 2, 3)  # [Co][Ci][kh][kw]
    odd = torch.tensor([2, 0], device=wt.device)
    ev = torch.tensor([1], device=wt.device)
    packs = []
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = wc.index_select(2, odd if a else ev).index_select(3, odd if b else ev).contiguous()
        packs.append(weight_pack(w, PACK_OK))
    return packs


def conv4s2_dgrad_phase_packs(w):
    """Phase packs of the data gradient of Conv2d(k=4, stride 2, padding 1) with weight w [Co][Ci][4][4]:
    output parity a (rows) / b (cols) = a 2x2 conv over dy (padding 1) with taps (3, 1) (even) or
    (2, 0) (odd) of w read as [out = ci][in = co] (VST_PACK_OK packs, PackBatch tap maps)."""
    Co, Ci = w.shape[0], w.shape[1]
    maps = ([3, 1], [2, 0])
    pb = PackBatch._active
    if pb is not None:
        st = (16, Ci * 16, 4, 1)  # logical [o = ci][i = co][r][s] of w[co][ci][kh][kw]
        return [pb.add(w, PACK_OK, Ci, Co, 2, 2, st, maps[a], maps[b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
    wc = w.detach().permute(1, 0, 2, 3)
    packs = []
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ra, cb = torch.tensor(maps[a], device=w.device), torch.tensor(maps[b], device=w.device)
        packs.append(weight_pack(wc.index_select(2, ra).index_select(3, cb).contiguous(), PACK_OK))
    return packs


# the four phases in one launch stored interleaved (vst_conv4s2_dgrad); False: images + interleave
C4S2_GROUPED = True


def conv4s2_dgrad_grouped(N, Hd, Wd, Cy, cop, role="bwd", split=True):
    """Does conv4s2_dgrad run its one grouped launch (vst_conv4s2_dgrad) for this shape?  split: the packs carry
    their bf16 planes.  A grid of fewer than half a CU round of 128x128 phase tiles (the StarGAN discriminator's
    deep layers: 100 rows x 1024 channels per phase at B = 4, K = 8192) runs as four split-K forwards + the
    interleave instead."""
    small = 4 * (-(-N * (Hd + 1) * (Wd + 1) // 128)) * (-(-cop // 128)) < 128
    return bool(C4S2_GROUPED and _math(role) != _lib.MATH_MODES["fp32"] and Cy % 32 == 0 and cop != 4 and not small
                and split)


def conv4s2_dgrad(dy, packs, cop, role="bwd"):
    """Data gradient of Conv2d(k=4, s=2, p=1) onto a (2*Hd) x (2*Wd) input via four 2x2 phase convs
    (padding 1, outputs (Hd+1) x (Wd+1)) + vst_interleave_phases_full."""
    _dev_check(dy)
    N, Hd, Wd, Cy = dy.shape
    m = _math(role)
    split = all(getattr(wp, "vst_split", None) is not None for wp in packs)
    if conv4s2_dgrad_grouped(N, Hd, Wd, Cy, cop, role, split):
        # one launch, stored straight into the interleaved gradient (vst_conv4s2_dgrad)
        y = torch.empty((N, 2 * Hd, 2 * Wd, cop), device=dy.device)
        _call("vst_conv4s2_dgrad", _p(dy), *[_p(wp.vst_split) for wp in packs], _p(y), N, Hd, Wd, Cy, cop, m,
              _stream())
        return y
    outs = [conv2d_fwd(dy, wp, None, cop, 2, 2, 1, 1, "zero", role=role) for wp in packs]
    y = torch.empty((N, 2 * Hd, 2 * Wd, cop), device=dy.device)
    _call("vst_interleave_phases_full", _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(y), N, Hd, Wd,
          cop, _stream())
    return y


def convT4s2_fwd(x, packs, bias, cop, act="none", role="fwd"):
    """ConvTranspose2d(k=4, s=2, p=1) forward on NHWC x [N, H, W, Cx] -> [N, 2H, 2W, cop].  It is, operand for
    operand, the data gradient of Conv2d(k=4, s=2, p=1) with the transposed weight [Ci][Co][4][4] read as that
    conv's [Co][Ci]: packs = conv4s2_dgrad_phase_packs(weight).  Without a bias and an activation it is
    conv4s2_dgrad itself (the grouped launch where that route takes the shape); with them the four 2x2 phase convs
    carry them in their epilogues (each output pixel belongs to exactly one phase) ahead of the interleave."""
    _dev_check(x, bias)
    if bias is None and act == "none":
        return conv4s2_dgrad(x, packs, cop, role=role)
    N, H, W, _ = x.shape
    outs = [conv2d_fwd(x, wp, bias, cop, 2, 2, 1, 1, "zero", act=act, role=role) for wp in packs]
    y = torch.empty((N, 2 * H, 2 * W, cop), device=x.device)
    _call("vst_interleave_phases_full", _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(y), N, H, W, cop,
          _stream())
    return y


# ConvTranspose2d phase convs storing straight into the interleaved output (vst_conv2d_fwd_phase)
# instead of four phase images + vst_interleave_phases; False keeps the latter.
CONVT_DIRECT = True
# ... and all four in one launch (vst_conv2d_convT_s2) where Cx % 32 == 0; False: one per phase.
CONVT_GROUPED = True


def convT3s2_route(Cx, cop, role="fwd", split=True):
    """The form convT3s2_fwd runs: 'grouped' (vst_conv2d_convT_s2, all four phases in one launch), 'phase'
    (vst_conv2d_fwd_phase per phase) or 'images' (phase images + vst_interleave_phases).  split: the packs carry
    their bf16 planes."""
    if not (CONVT_DIRECT and _math(role) != _lib.MATH_MODES["fp32"] and Cx % 8 == 0 and cop != 4 and split):
        return "images"
    return "grouped" if CONVT_GROUPED and Cx % 32 == 0 else "phase"


def convT3s2_fwd(x, packs, bias, cop, act="none", role="fwd"):
    """ConvTranspose2d(k=3, s=2, p=1, op=1) forward on NHWC x via four phase convs, stored straight into
    the interleaved output (split-bf16 math) or as phase images + interleave."""
    _dev_check(x, bias)
    N, H, W, Cx = x.shape
    m = _math(role)
    route = convT3s2_route(Cx, cop, role, all(getattr(wp, "vst_split", None) is not None for wp in packs))
    if route != "images":
        y = torch.empty((N, 2 * H, 2 * W, cop), device=x.device)
        if route == "grouped":
            _call("vst_conv2d_convT_s2", _p(x), *[_p(wp.vst_split) for wp in packs], _p(bias), _p(y), N, H, W, Cx,
                  cop, ACT[act], 0.0, m, _stream())
            return y
        for (a, b), wp in zip(((0, 0), (0, 1), (1, 0), (1, 1)), packs):
            _call("vst_conv2d_fwd_phase", _p(x), _p(wp.vst_split), _p(bias), _p(y), N, H, W, Cx, cop, a, b, ACT[act],
                  0.0, m, _stream())
        return y
    outs = []
    for (a, b), wp in zip(((0, 0), (0, 1), (1, 0), (1, 1)), packs):
        outs.append(conv2d_fwd_hw(x, wp, bias, cop, 1 + a, 1 + b, 1, a, b, act=act, role=role))
    y = torch.empty((N, 2 * H, 2 * W, cop), device=x.device)
    _call("vst_interleave_phases", _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(y), N, H, W, cop,
          _stream())
    return y


_ROUTE_FLAGS = ("FWD_SPLITK", "FWD_HW_SPLITK", "DGRAD_BORDER", "C4_DGRAD", "TAP_CHUNK_BYTES", "TAP_PLANES", "TAP_SWAP",
                "C4S2_GROUPED", "CONVT_DIRECT", "CONVT_GROUPED")
# the forward-route switches of networks.py (the generator's / discriminator's layer routes)
_NET_ROUTE_FLAGS = ("C8_EDGES", "C4_FWD", "DGRAD_AS_FPROP", "TAP_LAST", "TAP_H", "CONVT_PHASES", "IN_XT", "D_CO1")


def route_flags():
    """The module-level route switches that change which kernels a forward launches (tests and tools
    flip them in-process): part of FlatNet.graphed_forward's capture key."""
    import sys
    g = globals()
    net = sys.modules.get(__name__.rsplit(".", 1)[0] + ".networks")
    return tuple(g[n] for n in _ROUTE_FLAGS) + (tuple(getattr(net, n) for n in _NET_ROUTE_FLAGS) if net else ())


_lib.apply_route_overrides(__name__, globals())
