"""StarGAN v2 latent-guided inference on the MI355X: latency, and the workload of a kernel trace.

    python tools/stargan2_trace.py time [H W ...]       one JSON line per size: ms/frame of
                                                        StyleGuided.from_latent(nets, z, y).forward_eval(img) at B = 1
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/stargan2_trace.py run H W REPS
                                                        WARM + REPS forwards for the profiler; summarise the CSV with
                                                        tools/profsum.py CSV <REPS + WARM>

Default-size nets (build_model: img_size 256, style_dim 64, latent_dim 16, 2 domains; the generator is fully
convolutional, so any H, W that are multiples of 16 run), seeded random weights, fp32-equivalent conv arithmetic (the
default policy).  ``time``: WARM warm-up calls per size, then ROUNDS rounds of REPS calls, each call timed by a host
clock around the call and a device synchronise; reported are the median over all timed calls and the medians of the
best and worst round (the spread).  The style code is computed once (the mapping network is not in the timed call),
as the reference's evaluation does per video.  No GPU: the tool fails, it measures nothing on a CPU.
"""
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, REPS, ROUNDS = 5, 30, 3


def model():
    import gbvst
    from gbvst import stargan2 as M
    gbvst._lib.load()
    torch.manual_seed(0)
    args = types.SimpleNamespace(img_size=256, style_dim=64, latent_dim=16, num_domains=2, w_hpf=0)
    _, ema = M.build_model(args)
    nets = types.SimpleNamespace(**{k: v.to("cuda") for k, v in ema.items()})
    z = torch.randn(1, 16, device="cuda")
    return M.StyleGuided.from_latent(nets, z, torch.tensor([1], device="cuda"))


def call(sg, img):
    t0 = time.perf_counter()
    sg.forward_eval(img)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stargan2_trace: needs a HIP device")
    mode, rest = sys.argv[1], [int(v) for v in sys.argv[2:]]
    sg = model()
    if mode == "run":
        H, W, reps = rest
        img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
        for _ in range(WARM + reps):
            call(sg, img)
        return
    sizes = list(zip(rest[0::2], rest[1::2])) or [(256, 256), (432, 1024)]
    from gbvst import _lib, ops
    for H, W in sizes:
        img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
        for _ in range(WARM):
            call(sg, img)
        rounds = [[call(sg, img) for _ in range(REPS)] for _ in range(ROUNDS)]
        meds = sorted(statistics.median(r) for r in rounds)
        print(json.dumps({"what": "StarGAN v2 latent-guided generator inference, B=1, default-size nets", "H": H,
                          "W": W, "ms_per_frame_median": round(statistics.median(sum(rounds, [])), 3),
                          "round_medians_ms": [round(m, 3) for m in meds], "calls": REPS * ROUNDS,
                          "timing": "host clock around forward_eval + device synchronise, per call",
                          "math": ops.get_conv_math(), "source_stamp": _lib.source_stamp(),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
