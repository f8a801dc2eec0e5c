"""Dumoulin multi-style train steps for a kernel trace, and the per-kernel summary of that trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python3 tools/dumoulin_trace.py run [steps]
    python3 tools/dumoulin_trace.py sum OUT/.../p_kernel_trace.csv [steps] > profiles/dumoulin_step_summary.txt

run: 3 warm-up steps, then `steps` steps of Dumoulin.train_step at B = 4, 256 x 256, 3 styles (style ids 0, 1, 2 in
turn), all in the one traced process.  sum: per (kernel, grid) count, MEDIAN and mean time and the share of a step,
then the comparison the conditional-norm apply kernels are held to: their median at conv3 (4 x 64 x 64 x 128) against
in_aff_apply_k / in_aff_bwd_apply_k at the residual blocks, the same shape in the same trace.
"""
import csv
import os
import statistics
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, B, SIZE, N_STYLES = 3, 4, 256, 3
# conv3 / residual-block activations: B x 64 x 64 x 128 floats, one thread per float4
APPLY_GRID = B * (SIZE // 4) * (SIZE // 4) * 128 // 4
PAIRS = (("cond_apply_k", "in_aff_apply_k"), ("cond_bwd_apply_k", "in_aff_bwd_apply_k"))


def run(steps):
    import torch
    from gbvst import _lib, faststyle
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    styles = [torch.rand(1, 3, SIZE, SIZE, generator=g) for _ in range(N_STYLES)]
    D = faststyle.Dumoulin(styles, lr=1e-3, batch_sz=B, device=dev)
    x = torch.rand(B, 3, SIZE, SIZE, generator=g).to(dev)
    for i in range(WARMUP + steps):
        D.train_step(x, style_id=i % N_STYLES)
    torch.cuda.synchronize()
    print("steps", WARMUP + steps)


def summarise(path, steps, top=60):
    d = defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        key = (name, int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
        d[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = steps + WARMUP
    tot = sum(sum(v) for v in d.values())
    print("Dumoulin.train_step, B=%d, %dx%d, %d styles: %d steps traced (%d warm-up included in the counts)" %
          (B, SIZE, SIZE, N_STYLES, total, WARMUP))
    print("total kernel time %.1f ms (%.2f ms/step)" % (tot / 1e6, tot / 1e6 / total))
    for (name, gx, gy), v in sorted(d.items(), key=lambda kv: -sum(kv[1]))[:top]:
        print("%-88s g=%8d,%4d n=%5d med=%8.1fus avg=%8.1fus /step=%6.2fms %5.1f%%" %
              (name[-88:], gx, gy, len(v), statistics.median(v) / 1e3, sum(v) / len(v) / 1e3, sum(v) / 1e6 / total,
               100 * sum(v) / tot))
    print("\napply kernels at %d x 64 x 64 x 128 (grid %d threads), medians over this trace:" % (B, APPLY_GRID))
    for new, old in PAIRS:
        med = {}
        for want in (new, old):
            v = [t for (name, gx, _), ts in d.items()
                 if name.split("::")[-1] == want and gx in (APPLY_GRID, APPLY_GRID // 256) for t in ts]
            med[want] = (statistics.median(v) / 1e3, len(v)) if v else (float("nan"), 0)
        print("  %-18s med %7.2f us (n=%d)   %-20s med %7.2f us (n=%d)   ratio %.3f" %
              (new, *med[new], old, *med[old], med[new][0] / med[old][0]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sum":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    else:
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
