"""unet_256 training passes for a kernel trace, the per-kernel summary of that trace, and the per-layer table.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python3 tools/unet_trace.py run [steps]
    python3 tools/unet_trace.py sum OUT/.../p_kernel_trace.csv [steps] > profiles/unet_step_summary.txt
    python3 tools/unet_trace.py layers [steps] > profiles/unet_layertable.jsonl

run: 3 warm-up passes, then `steps` passes (forward + backward with trainable weights) of
UnetGenerator(3, 3, 8, ngf=64) (unet_256's net) at B = 4, 256 x 256, all in the one traced process.  Each pass also launches the plain
InstanceNorm apply kernels (ops.instnorm_act_fwd / instnorm_act_bwd) once at the two widest skip levels, 4 x 128 x
128 x 64 and 4 x 64 x 64 x 128, so the comparison the skip kernels are held to has both sides at the same shape in
the same trace.  sum: per (kernel, grid) count, MEDIAN and mean time and the share of a pass, then that comparison.
layers: HIP events around every conv-family and skip op of a pass (outermost call), keyed by op and shapes, with the
route the op took — the baseline of the small-spatial (weight-streaming) follow-up; also frames/s of the pass next
to resnet_9blocks' at the same batch, for information.
"""
import csv
import json
import os
import statistics
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, B, SIZE, NGF = 3, 4, 256, 64
LEVELS = ((SIZE // 2, NGF), (SIZE // 4, 2 * NGF))     # (map side, channels) of the two widest skip levels
# (new kernel, the plain kernel it is measured against, bytes per element new / old)
PAIRS = (("skip_apply_k", "in_apply_k", 12, 8), ("skip_bwd_apply_k", "in_bwd_apply_k", 16, 12))


def _net(name="unet_256"):
    import torch
    from gbvst import _lib, networks
    _lib.load()
    torch.manual_seed(11)
    if name == "unet_256":      # define_G does not offer this name yet: the class, initialised as define_G would
        inst = networks.get_norm_layer("instance")
        return networks.init_net(networks.UnetGenerator(3, 3, 8, NGF, norm_layer=inst), "normal", 0.02, [0])
    return networks.define_G(3, 3, NGF, name, "instance", False, "normal", 0.02, [0])


def _compare_launches(ops, bufs):
    for y, st, g in bufs:
        ops.instnorm_act_fwd(y, st, "relu")
        ops.instnorm_act_bwd(g, y, st, "relu")


def _pass(net, x, r):
    net.zero_grad()
    (net(x) * r).sum().backward()


def run(steps):
    import torch
    from gbvst import ops
    net = _net()
    dev = net.flat_param.device
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(B, 3, SIZE, SIZE, generator=g) * 2 - 1).to(dev)
    r = torch.randn(B, 3, SIZE, SIZE, generator=g).to(dev)
    bufs = []
    for side, c in LEVELS:
        y = torch.randn(B, side, side, c, generator=g).to(dev)
        bufs.append((y, ops.instnorm_stats(y), torch.randn(B, side, side, c, generator=g).to(dev)))
    for _ in range(WARMUP + steps):
        _pass(net, x, r)
        _compare_launches(ops, bufs)
    torch.cuda.synchronize()
    print("passes", WARMUP + steps)


def summarise(path, steps, top=45):
    d = defaultdict(list)
    for row in csv.DictReader(open(path)):
        name = row["Kernel_Name"].split("(")[0].replace("void ", "")
        d[(name, int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))].append(
            int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    total = steps + WARMUP
    tot = sum(sum(v) for v in d.values())
    print("unet_256 (ngf %d) forward + backward, B=%d, %dx%d: %d passes traced (%d warm-up included in the counts)"
          % (NGF, B, SIZE, SIZE, total, WARMUP))
    print("total kernel time %.1f ms (%.2f ms/pass, the comparison launches included)" % (tot / 1e6, tot / 1e6 / total))
    for (name, gx, gy), v in sorted(d.items(), key=lambda kv: -sum(kv[1]))[:top]:
        print("%-88s g=%8d,%4d n=%5d med=%8.1fus avg=%8.1fus /pass=%6.2fms %5.1f%%" %
              (name[-88:], gx, gy, len(v), statistics.median(v) / 1e3, sum(v) / len(v) / 1e3, sum(v) / 1e6 / total,
               100 * sum(v) / tot))
    print("\nskip kernels against the plain InstanceNorm apply kernels at the same shape, medians over this trace")
    print("(bar: the byte ratio x 1.10; the skip forward here is the one with both outputs, grid = one thread per float4):")
    for side, c in LEVELS:
        grid = B * side * side * c // 4
        at = {name.split("::")[-1]: ts for (name, gx, _), ts in d.items() if gx in (grid, grid // 256)}
        for new, old, bn, bo in PAIRS:
            ref = [t for k, ts in at.items() if k.split("<")[0] == old for t in ts]
            mo = statistics.median(ref) / 1e3 if ref else float("nan")
            # the variant the bar is set for: both outputs / both gradients (template arguments <STATS, true>)
            for k in sorted(k for k in at if k.split("<")[0] == new):
                mn = statistics.median(at[k]) / 1e3
                full = k.replace(" ", "").endswith(",true>")
                ratio, bar = mn / mo, bn / bo * 1.10
                print("  %d x %3d x %3d x %3d  %-30s med %7.2f us (n=%3d)  %-15s med %7.2f us (n=%3d)  ratio %.3f  %s"
                      % (B, side, side, c, k, mn, len(at[k]), old, mo, len(ref), ratio,
                         ("bar %.3f  %s" % (bar, "ok" if ratio <= bar else "MISSED")) if full else "(one output: no bar)"))


def layers(steps):
    import torch
    from gbvst import ops
    rec, on = defaultdict(list), [False]
    depth = [0]

    def shape(t):
        return "x".join(str(int(s)) for s in t.shape)

    def describe(name, a, k):
        if name in ("conv2d_fwd", "conv2d_fwd_in"):
            x, _, _, cop, R, S, st, pad = a[:8]
            N, H, W, Cx = x.shape
            nb = ops.FWD_SPLITK and S == R and ops.lib().vst_conv2d_fwd_ex_ws_bytes(
                N, H, W, Cx, cop, R, S, st, pad, pad, ops.PAD["zero"], ops._math(k.get("role", "fwd")), cop)
            return "%s -> %d k%d s%d" % (shape(x), cop, R, st), "split-K" if nb else "one pass"
        if name in ("conv4s2_dgrad", "convT4s2_fwd"):
            x, packs, cop = a[0], a[1], a[2] if name == "conv4s2_dgrad" else a[3]
            N, Hd, Wd, Cy = x.shape
            plain = name == "conv4s2_dgrad" or (a[2] is None and k.get("act", "none") == "none")
            small = 4 * (-(-N * (Hd + 1) * (Wd + 1) // 128)) * (-(-cop // 128)) < 128
            grouped = plain and ops.C4S2_GROUPED and Cy % 32 == 0 and cop != 4 and not small
            return "%s -> %d" % (shape(x), cop), "grouped phases" if grouped else "4 phase convs + interleave"
        if name == "conv2d_wgrad":
            x, dy = a[0], a[1]
            R, S, st, pad = a[4:8]
            N, H, W, Cx = x.shape
            route = ops.wgrad_route(N, H, W, Cx, dy.shape[1], dy.shape[2], dy.shape[3], R, S, st, pad)
            return "x %s dy %s" % (shape(x), shape(dy)), {ops.WG_NHWC: "nhwc planes", ops.WG_NHWC_F32: "nhwc f32 / im2col",
                                                          ops.WG_IMAGES: "channel-major images", ops.WG_PLAIN: "plain"}[route]
        if name == "conv2d_tfwd":
            return "%s -> %dx%dx%d" % (shape(a[0]), a[3], a[4], a[5]), "transposed kernel"
        if name == "instnorm_skip_fwd":
            return "%s into %d at %d" % (shape(a[0]), a[2].shape[-1], a[3]), \
                ("stats" if a[1] is not None else "no stats") + (", d" if k.get("want_d", True) else "")
        if name == "instnorm_skip_bwd":
            return "%s from %d at %d" % (shape(a[3]), a[1].shape[-1], a[2]), \
                ("stats" if a[4] is not None else "no stats") + (", g_d" if a[0] is not None else "")
        return shape(a[0]), ""

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **k):
            if not on[0] or depth[0]:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            depth[0] += 1
            e0.record()
            try:
                out = fn(*a, **k)
            finally:
                depth[0] -= 1
            e1.record()
            rec[(name,) + describe(name, a, k)].append((e0, e1))
            return out
        setattr(ops, name, f)

    for name in ("conv2d_fwd", "conv2d_fwd_in", "conv4s2_dgrad", "convT4s2_fwd", "conv2d_wgrad", "conv2d_tfwd",
                 "instnorm_skip_fwd", "instnorm_skip_bwd", "instnorm_stats", "act_bwd", "channel_sum"):
        wrap(name)
    g = torch.Generator().manual_seed(7)
    fps = {}
    for which in ("unet_256", "resnet_9blocks"):
        net = _net(which)
        dev = net.flat_param.device
        x = (torch.rand(B, 3, SIZE, SIZE, generator=g) * 2 - 1).to(dev)
        r = torch.randn(B, 3, SIZE, SIZE, generator=g).to(dev)
        for _ in range(WARMUP):
            _pass(net, x, r)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            _pass(net, x, r)
        t1.record()
        torch.cuda.synchronize()
        fps[which] = B * steps / (t0.elapsed_time(t1) * 1e-3)
        if which == "unet_256":
            on[0] = True
            for _ in range(steps):
                _pass(net, x, r)
            torch.cuda.synchronize()
            on[0] = False
        del net
    rows = []
    for (name, lab, route), evs in rec.items():
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
        rows.append({"op": name, "layer": lab, "route": route, "calls_per_pass": len(us) / steps,
                     "us": round(statistics.median(us), 1)})
    rows.sort(key=lambda r: -r["us"] * r["calls_per_pass"])
    for row in rows:
        print(json.dumps(row))
    print(json.dumps({"pass": "forward + backward, B=%d, %dx%d, ngf %d" % (B, SIZE, SIZE, NGF),
                      "frames_per_s": {k: round(v, 1) for k, v in fps.items()},
                      "ops_us_per_pass": round(sum(r["us"] * r["calls_per_pass"] for r in rows), 1)}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "run"
    if mode == "sum":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    elif mode == "layers":
        layers(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
