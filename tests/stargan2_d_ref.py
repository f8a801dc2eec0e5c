"""CPU reference of StarGAN v2's discriminator update (reference core/solver.py: adv_loss, r1_reg, compute_d_loss),
restated over stargan2_ref's functional networks with torch's native double backward, in any float dtype.

    adv_loss(logits, t) = mean softplus(-logits) (t = 1) | mean softplus(logits) (t = 0)
    r1_reg(out, x)      = 0.5 * mean_b sum_{c,h,w} (d sum(out) / d x)^2
    loss                = adv_loss(D(x_real, y_org), 1) + adv_loss(D(x_fake, y_trg), 0) + lambda_reg * r1_reg(...)
    x_fake              = G(x_real, F(z_trg, y_trg))   (latent mode)   |   G(x_real, E(x_ref, y_trg))   (reference mode)

tools/gen_golden_stargan2_d.py ran the reference's own Solver.compute_d_loss on the same weights and inputs and wrote
tests/golden/stargan2_dstep.npz; test_stargan2_d_host.py holds this restatement against it.

The case: D = stargan2_ref.CASES["D"]'s geometry (img_size 64, 3 domains, max_conv_dim 8: both shortcut kinds), batch 2,
with the matching tiny Generator(64, 16, 8), StyleEncoder(64, 16, 3, 8) and MappingNetwork(16, 16, 3).  The gradients
jump where a LeakyReLU input crosses 0.  The discriminator's weights and x_real are CASES["D"]'s own (seed 831 / 832:
that forward keeps its scanned margin already); the seeds of z_trg and x_ref, which decide the two x_fake, are each the
one of a scan over SCAN (gen_golden_stargan2_d.py --scan) whose fp64 discriminator forward over that mode's x_fake
keeps the largest activation margin.  The host test holds the smallest of the three to stargan2_ref.MARGIN["D"].
"""
import numpy as np
import torch
import torch.nn.functional as F

import stargan2_ref as S

CFG = {
    "discriminator": S.CASES["D"]["cfg"],
    "generator": dict(img_size=64, style_dim=16, max_conv_dim=8),
    "style_encoder": S.CASES["E"]["cfg"],
    "mapping_network": S.CASES["F"]["cfg"],
}
SEEDS = {"discriminator": S.CASES["D"]["seed"], "x_real": S.CASES["D"]["seed"] + 1, "generator": 961,
         "style_encoder": 962, "mapping_network": 963, "latent": 1084, "reference": 1081}
B = 2
Y_ORG, Y_TRG = [2, 0], [1, 2]
LAMBDA_REG = 1.0
MODES = ("latent", "reference")
SCAN = range(1000, 1240)


def states():
    """{kind: {key: fp32 array}} of the four nets."""
    return {k: S.make_state(SEEDS[k], S.shapes(k, **CFG[k])) for k in CFG}


def inputs(latent=None, reference=None):
    """x_real [B, 3, 64, 64] (u8 levels in [-1, 1]), z_trg [B, 16], x_ref [B, 3, 64, 64]; latent / reference override
    the seeds of z_trg / x_ref (the scan)."""
    x_real, _ = S.case_inputs(SEEDS["x_real"], (B, 3, 64, 64), (B,))
    z_trg, _ = S.case_inputs(latent or SEEDS["latent"], (B, CFG["mapping_network"]["latent_dim"]), (B,))
    x_ref, _ = S.case_inputs(reference or SEEDS["reference"], (B, 3, 64, 64), (B,))
    return x_real, z_trg, x_ref


def _t(sd, dtype, grad=False):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(grad) for k, v in sd.items()}


def x_fake(st, mode, x_real, z_trg, x_ref, dtype=torch.float32):
    """The generator's output of a mode, without gradients (numpy in, tensor out)."""
    with torch.no_grad():
        xr = torch.from_numpy(x_real).to(dtype)
        if mode == "latent":
            s = S.mapping_forward(_t(st["mapping_network"], dtype), torch.from_numpy(z_trg).to(dtype), Y_TRG,
                                  **CFG["mapping_network"])
        else:
            s = S.encoder_forward(_t(st["style_encoder"], dtype), torch.from_numpy(x_ref).to(dtype), Y_TRG,
                                  **CFG["style_encoder"])
        return S.generator_forward(_t(st["generator"], dtype), xr, s, **CFG["generator"])


def adv_loss(logits, target):
    assert target in (0, 1)
    return F.softplus(-logits if target else logits).mean()


def r1_reg(d_out, x_in):
    (g,) = torch.autograd.grad(d_out.sum(), x_in, create_graph=True)
    return 0.5 * g.pow(2).flatten(1).sum(1).mean(0)


def d_losses(sd, x_real, y_org, x_fk, y_trg, lambda_reg, dtype):
    """dict(real, fake, reg: detached scalars; grads: {key: d (real + fake + lambda_reg * reg) / d parameter};
    grads_reg: the same of the penalty alone) of the discriminator state sd.  A parameter the quantity does not
    depend on (the penalty's biases: they only move the masks) gets zeros."""
    t = _t(sd, dtype, grad=True)
    xr = torch.as_tensor(x_real).to(dtype).requires_grad_(True)
    out = S.discriminator_forward(t, xr, y_org, **CFG["discriminator"])
    real, reg = adv_loss(out, 1), r1_reg(out, xr)
    fake = adv_loss(S.discriminator_forward(t, torch.as_tensor(x_fk).to(dtype), y_trg, **CFG["discriminator"]), 0)

    def grads(q):
        gs = torch.autograd.grad(q, list(t.values()), allow_unused=True, retain_graph=True)
        return {k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(t.items(), gs)}

    return dict(real=real.detach(), fake=fake.detach(), reg=reg.detach(), grads_reg=grads(reg),
                grads=grads(real + fake + lambda_reg * reg))


def margin(sd, x_real, fakes):
    """The smallest activation margin of the fp64 discriminator forward over x_real and every x_fake."""
    c = CFG["discriminator"]
    ms = [S.activation_margin("discriminator", c, sd, np.asarray(x_real, np.float32), Y_ORG)]
    ms += [S.activation_margin("discriminator", c, sd, np.asarray(f, np.float32), Y_TRG) for f in fakes]
    return min(ms)
