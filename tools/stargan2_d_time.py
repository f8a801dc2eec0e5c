"""StarGAN v2 discriminator update on the MI355X: step time against stock PyTorch, and the workload of a kernel trace.

    python tools/stargan2_d_time.py time [B]            JSON lines: ms/step of the D update at the default size
                                                        (img_size 256, 2 domains, B = 8: the reference's batch_size)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/stargan2_d_time.py run ours REPS
                                                        WARM + REPS updates for the profiler; summarise the CSV with
                                                        tools/profsum.py CSV <REPS + WARM>

What is timed, with x_fake given (a fixed random image batch, so both sides run the same arithmetic and the generator
is not in it): zero_grad, the three losses (real, fake, R1 with lambda_reg = 1), backward, Adam(lr 1e-4, betas
(0, 0.99), weight_decay 1e-4), and one .tolist() of the three losses — the reference's host sync.
  ours    gbvst.stargan2.d_losses on the HIP kernels, backward restricted to D's parameters (what d_step does)
  stock   the same step by tests/stargan2_d_ref.py (functional D, torch's native double backward) in fp32 on the GPU
  d_step  DiscriminatorTrainer.d_step in latent mode: ours plus the mapping network and the generator forward
WARM warm-up steps, then ROUNDS rounds of REPS steps, each timed by a host clock around the step and a device
synchronise; reported are the median over all timed steps and the round medians.  No GPU: the tool fails.
"""
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
WARM, REPS, ROUNDS = 3, 10, 3
ARGS = types.SimpleNamespace(img_size=256, style_dim=64, latent_dim=16, num_domains=2, w_hpf=0, lambda_reg=1.0, lr=1e-4,
                             beta1=0.0, beta2=0.99, weight_decay=1e-4)


def setup(B):
    import gbvst
    from gbvst import stargan2 as M
    gbvst._lib.load()
    torch.manual_seed(0)
    nets, _ = M.build_model(ARGS)
    for net in nets.values():
        net.apply(M.he_init)
        net.to("cuda")
    x_real, x_fake = (torch.rand(B, 3, 256, 256, device="cuda") * 2 - 1 for _ in range(2))
    y_org, y_trg = (torch.randint(0, 2, (B,), device="cuda") for _ in range(2))
    return M, nets, x_real, x_fake, y_org, y_trg, torch.randn(B, 16, device="cuda")


def ours_step(M, nets, trainer, x_real, x_fake, y_org, y_trg):
    D = nets.discriminator
    loss, parts = M.d_losses(D, x_real, y_org, x_fake, y_trg, ARGS.lambda_reg)
    trainer.optimizer.zero_grad()
    loss.backward(inputs=list(D.parameters()))
    trainer.optimizer.step()
    return torch.stack([parts.real, parts.fake, parts.reg]).tolist()


def stock(nets):
    """(step, params): the discriminator's weights as plain tensors under stock PyTorch ops and their Adam."""
    import stargan2_d_ref as DR
    import stargan2_ref as S
    t = {k: v.detach().clone().requires_grad_(True) for k, v in nets.discriminator.state_dict().items()}
    opt = torch.optim.Adam(list(t.values()), lr=ARGS.lr, betas=[ARGS.beta1, ARGS.beta2], weight_decay=ARGS.weight_decay)
    cfg = S.DEFAULTS["discriminator"]

    def step(x_real, x_fake, y_org, y_trg):
        xr = x_real.detach().clone().requires_grad_(True)
        out = S.discriminator_forward(t, xr, y_org, **cfg)
        real, reg = DR.adv_loss(out, 1), DR.r1_reg(out, xr)
        fake = DR.adv_loss(S.discriminator_forward(t, x_fake, y_trg, **cfg), 0)
        opt.zero_grad()
        (real + fake + ARGS.lambda_reg * reg).backward(inputs=list(t.values()))
        opt.step()
        return torch.stack([real.detach(), fake.detach(), reg.detach()]).tolist()
    return step


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stargan2_d_time: needs a HIP device")
    mode = sys.argv[1]
    B = int(sys.argv[2]) if mode == "time" and len(sys.argv) > 2 else 8
    M, nets, x_real, x_fake, y_org, y_trg, z_trg = setup(B)
    trainer = M.DiscriminatorTrainer(nets, ARGS)
    stock_step = stock(nets)
    steps = {"ours": lambda: ours_step(M, nets, trainer, x_real, x_fake, y_org, y_trg),
             "stock": lambda: stock_step(x_real, x_fake, y_org.tolist(), y_trg.tolist()),
             "d_step": lambda: trainer.d_step(x_real, y_org, y_trg, z_trg=z_trg)}
    if mode == "run":
        for _ in range(WARM + int(sys.argv[3])):
            timed(steps[sys.argv[2]])
        return
    from gbvst import _lib, ops
    first = {k: timed(fn)[1] for k, fn in (("ours", steps["ours"]), ("stock", steps["stock"]))}
    print(json.dumps({"first_step_losses": first}), flush=True)      # the same weights and inputs: the same losses
    for name, fn in steps.items():
        for _ in range(WARM):
            timed(fn)
        rounds = [[timed(fn)[0] for _ in range(REPS)] for _ in range(ROUNDS)]
        print(json.dumps({"what": "StarGAN v2 discriminator update, default-size D, x_fake given" if name != "d_step"
                          else "DiscriminatorTrainer.d_step, latent mode (mapping network + generator forward included)",
                          "step": name, "B": B, "ms_per_step_median": round(statistics.median(sum(rounds, [])), 3),
                          "round_medians_ms": sorted(round(statistics.median(r), 3) for r in rounds),
                          "steps": REPS * ROUNDS, "timing": "host clock around the step + device synchronise, per step",
                          "math": ops.get_conv_math(), "source_stamp": _lib.source_stamp(),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
