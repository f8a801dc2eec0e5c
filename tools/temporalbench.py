"""Temporal video style path timings at 256^2, B = 4 frame pairs, standalone:
  (a) ms per Reconet.train_step / Huang.train_step (median over steps, host clock around a device synchronise);
  (b) the fused masked-warp squared-difference loss (fs_lib.temporal_loss_nhwc: one kernel each way) against the
      same loss composed from what the package had before it — fs_lib.warp_nhwc + torch elementwise ops + .mean(),
      forward + backward through autograd on both arms — for the feature form (4x64x64x128) and the output form
      with the input term (4x256x256x4).  The arms alternate sample by sample (HIP events around `inner` calls
      each); medians, the achieved bytes/s over the algorithmic byte count, and the arms' agreement are printed.
`python tools/temporalbench.py [steps] [samples] [inner]` prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _median_ms(fns, samples, inner, warm=3):
    """Median ms per call of each fn, the fns alternating sample by sample."""
    for fn in fns:
        for _ in range(warm):
            fn()
    ts = [[] for _ in fns]
    for _ in range(samples):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def algorithmic_bytes(N, H, W, Cs, inputs):
    """Least traffic of forward + backward: each pass reads a, b, flow, mask (and the two NHWC4 input frames) once;
    the backward writes ga and gb once."""
    t = N * H * W * Cs * 4
    side = N * H * W * 4 * (2 + 1) + (2 * N * H * W * 4 * 4 if inputs else 0)
    return 2 * (2 * t + side) + 2 * t


def fused_vs_composed(dev, N, H, W, Cs, cl, inputs, ab_scale, samples, inner):
    from gbvst import fs_lib
    g = torch.Generator().manual_seed(11)
    a = torch.randn(N, H, W, Cs, generator=g)
    b = torch.randn(N, H, W, Cs, generator=g)
    if cl < Cs:
        a[..., cl:] = 0
        b[..., cl:] = 0
    a, b = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    flow = (torch.randn(N, 2, H, W, generator=g) * 3.0).to(dev)
    mask = torch.rand(N, 1, H, W, generator=g).to(dev)
    ins = None
    if inputs:
        ins = tuple(torch.rand(N, H, W, 4, generator=g).to(dev) for _ in range(2))
    mask_l = mask.view(N, H, W, 1)
    scale = 10.0

    def fused():
        a.grad = b.grad = None
        loss = fs_lib.temporal_loss_nhwc(a, b, flow, mask, scale, inputs=ins, ab_scale=ab_scale, cl=cl)
        loss.backward()
        return loss

    def composed():
        a.grad = b.grad = None
        d = b * ab_scale - fs_lib.warp_nhwc(a * ab_scale, flow)
        if ins is not None:
            di = ins[1] - fs_lib.warp_nhwc(ins[0], flow)
            d = d - (0.2126 * di[..., 0] + 0.7152 * di[..., 1] + 0.0722 * di[..., 2]).unsqueeze(-1)
        loss = scale * ((mask_l * d)[..., :cl] ** 2).mean()
        loss.backward()
        return loss

    lf = fused()
    gaf, gbf = a.grad.clone(), b.grad.clone()
    lc = composed()
    agree = {"loss_rel": abs(float(lf) - float(lc)) / abs(float(lc)),
             "ga_rel": float((gaf - a.grad).abs().max() / a.grad.abs().max()),
             "gb_rel": float((gbf - b.grad).abs().max() / b.grad.abs().max())}
    (tf, tc), (rf, rc) = _median_ms([fused, composed], samples, inner)
    nbytes = algorithmic_bytes(N, H, W, Cs, inputs)
    return {"shape": [N, H, W, Cs], "input_term": bool(inputs), "fused_ms": round(tf, 4), "composed_ms": round(tc, 4),
            "fused_range_ms": [round(v, 4) for v in rf], "composed_range_ms": [round(v, 4) for v in rc],
            "speedup": round(tc / tf, 2), "algorithmic_mb": round(nbytes / 1e6, 2),
            "fused_gb_per_s": round(nbytes / (tf * 1e-3) / 1e9, 1), "agreement": {k: float("%.2e" % v) for k, v in agree.items()}}


def train_step_ms(dev, cls, steps, B=4, S=256):
    g = torch.Generator().manual_seed(7)
    T = cls([torch.rand(1, 3, S, S, generator=g)], lr=1e-3, batch_sz=B, device=dev)
    imgs = [torch.rand(B, 3, S, S, generator=g).to(dev) for _ in range(2)]
    masks = (torch.rand(B, 1, S, S, generator=g) < 0.8).float().to(dev)
    flows = (torch.randn(B, 2, S, S, generator=g) * 3.0).to(dev)
    for _ in range(2):
        T.train_step(imgs, masks, flows)
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.train_step(imgs, masks, flows)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_per_step": round(statistics.median(ts), 3), "range_ms": [round(min(ts), 3), round(max(ts), 3)]}


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("temporalbench needs a HIP device (no CPU timing)")
    dev = torch.device("cuda:0")
    from gbvst import _lib, faststyle
    _lib.load()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 31
    inner = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    out = {"reconet": train_step_ms(dev, faststyle.Reconet, steps), "huang": train_step_ms(dev, faststyle.Huang, steps),
           "feature_form": fused_vs_composed(dev, 4, 64, 64, 128, 128, False, 1.0, samples, inner),
           "output_form": fused_vs_composed(dev, 4, 256, 256, 4, 3, True, 1.0 / 255.0, samples, inner)}
    print(json.dumps(out))
