"""Developer: RAFT's two correlation paths side by side — raft_corr.CorrBlock (all-pairs volume + pyramid,
role "infer" as RAFT uses it) against raft_corr.AlternateCorrBlock (fmap2 pyramid + on-the-fly window dots) —
at RAFT's feature-map sizes, plus compute_raft(it=20) at 440x1024 with the flag off and on, alternating.

One process; each path runs after its own warm-up; times are device events around synchronised work (medians
of `reps` windows).  Fails without a GPU.  Prints one JSON line.  usage: altcorr_bench.py [reps]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gbvst  # noqa: E402
from gbvst import raft, raft_corr  # noqa: E402

FMAPS = [(1, 256, 55, 128), (8, 256, 55, 128), (1, 256, 136, 240)]
L, R, CS, ITERS = 4, 4, 328, 20
FP32_VECTOR_PEAK = 157.3e12  # MI355X fp32 vector FLOP/s


def timed(fn, reps, inner=1):
    """Median ms of one fn() over `reps` event-timed windows of `inner` calls, after a warm-up window."""
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / inner)
    return float(np.median(t))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    del keep
    return int(grew)


def corr_case(shape, reps):
    B, D, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(7)
    f1 = torch.randn((B, H, W, D), device="cuda", generator=g)
    f2 = torch.randn((B, H, W, D), device="cuda", generator=g)
    coords = (raft_corr.coords_grid(B, H, W) + torch.randn((B, 2, H, W), device="cuda", generator=g) * 3.0).contiguous()
    builders = {"volume": lambda: raft_corr.CorrBlock.from_nhwc(f1, f2, D, L, R, role="infer"),
                "alternate": lambda: raft_corr.AlternateCorrBlock.from_nhwc(f1, f2, D, L, R)}
    out = {"fmap": list(shape)}
    for name, build in builders.items():
        def full():
            blk = build()
            for _ in range(ITERS):
                blk.lookup_nhwc(coords, cs=CS)

        def once():
            blk = build()
            return blk, blk.lookup_nhwc(coords, cs=CS)

        blk = build()
        r = {"build_ms": timed(build, reps),
             "lookup_ms": timed(lambda: blk.lookup_nhwc(coords, cs=CS), reps, inner=10),
             "build_plus_20_lookups_ms": timed(full, reps)}
        del blk
        r["peak_bytes"] = peak_bytes(once)
        out[name] = r
    flops = 2.0 * B * H * W * L * (2 * R + 2) ** 2 * D
    out["alternate"]["lookup_flops"] = flops
    out["alternate"]["lookup_tflops"] = flops / (out["alternate"]["lookup_ms"] * 1e-3) / 1e12
    out["alternate"]["lookup_share_of_fp32_vector_peak"] = out["alternate"]["lookup_tflops"] * 1e12 / FP32_VECTOR_PEAK
    out["faster_build_plus_20"] = min(("volume", "alternate"), key=lambda k: out[k]["build_plus_20_lookups_ms"])
    return out


def raft_case(reps):
    from oracle import raft_ref
    models = {}
    for flag in (False, True):
        m = raft.RAFT(argparse.Namespace(small=False, alternate_corr=flag))
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in raft_ref.raft_weights(shapes, 1300).items()})
        models[flag] = m.to("cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(11)
    i1 = torch.rand((1, 3, 436, 1024), device="cuda", generator=g) * 255
    i2 = torch.rand((1, 3, 436, 1024), device="cuda", generator=g) * 255
    t = {False: [], True: []}
    flows = {}
    for flag in (False, True):  # warm-up + graph capture
        flows[flag] = raft.compute_raft(models[flag], i1, i2, it=ITERS)
    torch.cuda.synchronize()
    for _ in range(reps):  # alternate the two in the same run
        for flag in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            raft.compute_raft(models[flag], i1, i2, it=ITERS)
            b.record()
            torch.cuda.synchronize()
            t[flag].append(a.elapsed_time(b))
    d = (flows[True] - flows[False]).abs().max().item() / (flows[False].abs().max().item() + 1e-30)
    return {"image": [1, 3, 436, 1024], "padded": [440, 1024], "iters": ITERS,
            "volume_ms": float(np.median(t[False])), "alternate_ms": float(np.median(t[True])),
            "flow_rel_diff": d}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    if not torch.cuda.is_available():
        raise SystemExit("altcorr_bench: needs a HIP device")
    gbvst._lib.load()
    with torch.no_grad():
        res = {"tool": "altcorr_bench", "levels": L, "radius": R, "cs": CS, "lookups": ITERS, "reps": reps,
               "source_stamp": gbvst._lib.source_stamp(), "corr": [corr_case(s, reps) for s in FMAPS],
               "raft": raft_case(reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
