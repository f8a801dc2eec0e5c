"""CPU reference of the Ruder recurrent train step for tests/test_gpu_ruder.py and tests/test_ruder_host.py.

The reference's own train_method cannot run without a GPU (its fs_lib.warp calls .cuda()), so the loss graph
of methods/learning-based/fs_ruder.py:38-108 is composed here, line by line, from the oracle pieces that
tests/test_oracle_golden.py pins to the reference (oracle.style_ref.fs_warp, RefFastStyleNet(7) for the
recurrent net, RefFastStyleNet(3) for the frozen pre-style net, RefVGG, gram_matrix, normalize).  Evaluated
in fp64 (temporal_style_ref.reference_run says why).  Everything is computed once per configuration
(functools caches) and shared between the tests."""
import functools

import torch
import torch.nn.functional as F

from oracle import style_ref
from temporal_style_ref import VGG_SEED, rand

# The recurrent FastStyleNet(7) / the pre-style FastStyleNet(3), and how MODEL_SEED was chosen.
# At 32x40 a layer's gradient is a sum over as few as 1e4 activations, so ONE ReLU or max-pool decision (in the net or
# in the VGG) that lands on the other side moves a parameter gradient by 1e-3 .. 2e-2 norm-wise, and among the ~4e6
# decisions of a step some always sit within 1e-6 (relative) of their threshold: for every seed 570..590 a
# 1 + 1e-6 N(0,1) scaling of the weights moves the reference's own full-emphasis gradients by 1.5e-3 .. 1.1e-2.  What
# differs between seeds is how near the nearest decisions are, and no test may hinge on how a forward pass rounds: as
# with the warp's validity threshold, the seed is changed, never the band.
#   1. On this CPU reference alone, seeds 570..630 were scanned for gradients that respond smoothly (GRAD_KEYS move by
#      < 2e-4) to 1 + 3e-7 N(0,1) scalings, four perturbation seeds, in the 3-frame, 5-frame and temporal-only runs:
#      571 575 578 581 587 590 596 600 603 609 619 621 625 630 do; the others move by 1e-3 .. 2e-2 (570: 9.7e-3).
#   2. fp32 convolutions round each sum of ~600..1200 products to ~1e-6 of its magnitude, more than a 3e-7 weight
#      scaling moves it, so (1) does not settle it: on an MI355X the step-0 gradients of these fourteen seeds were
#      measured against this reference under every conv policy (fp32, bf16x6, mixed) in the three runs.  Wherever no
#      decision differed the GPU agrees to 3e-6 .. 2e-5; ten of the fourteen had at least one of the nine cases across
#      a decision (1e-3 .. 1.1e-2; e.g. 587: 3 frames 9.2e-3 under every policy, 5 frames and temporal-only 3e-6).
#      619 has the largest margin: its worst case of the nine is 1.4e-4, and 1.4e-4 is also what its own reference
#      moves under the 3e-7 scalings (decisions of little weight).  609, 621, 625 stay below 1e-3 too (7.1e-4, 8.9e-4,
#      5.2e-4).  The bands the tests assert are unchanged (1e-6, two seeds, as the sibling train-step tests take them).
MODEL_SEED, PRE_SEED = 619, 540
B, H, W = 2, 32, 40
N_FRAMES = 5
# (alpha, beta, gamma): chosen on the CPU reference so that every term is at least 1 % of the total at both
# steps of the 3-frame run and at step 0 of the 5-frame run (asserted in the tests).  Unit weights give, on these
# seeded weights (3 frames, roll): content 6.17, style 94.8, temporal 0.0385 (5 frames: 6.21, 94.8, 0.0383;
# 2 frames: 5.97, 94.8, 0.0377; no roll: 5.97, 94.8, 0).
EMPH = (1.0, 0.1, 100.0)
# alpha = beta = 0: the gradients come through the temporal kernel, the net's input channels and the warps alone
TEMPORAL_ONLY = (0.0, 0.0, 100.0)


def step_inputs():
    """5 frames, the style image, 4 mask planes [B,1,H,W] and 4 flow planes [B,2,H,W]."""
    imgs = [torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(580 + i)) for i in range(N_FRAMES)]
    style = torch.rand(1, 3, 40, 40, generator=torch.Generator().manual_seed(562))
    masks = [(torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(590 + i)) < 0.8).float()
             for i in range(N_FRAMES - 1)]
    flows = [rand(600 + i, (B, 2, H, W), 3.0) for i in range(N_FRAMES - 1)]
    return imgs, style, masks, flows


def stack_ref(y_prev, img, flow, mask, s=1.0 / 255.0):
    """fs_ruder.py:50-52 on NCHW tensors: (cat(img, mask, w), w), w = fs_lib.warp(s * y_prev, flow)."""
    w = style_ref.fs_warp(y_prev * s, flow)
    return torch.cat((img, mask, w), 1), w


def temporal_ref(w, y, mask, scale, s=1.0 / 255.0):
    """fs_ruder.py:97: scale * mean((mask * (w - s * y))^2)."""
    return scale * ((mask * (w - y * s)) ** 2).mean()


def ruder_losses(model, pre, vgg, grams, imgs, masks, flows, emph, roll):
    """fs_ruder.py:38-108 with masks / flows already split into planes; returns the reference's tuple
    (total, style, content, temporal) -- style before content, fs_ruder.py:103 -- and styled frame 2 / 255."""
    alpha, beta, gamma = emph
    if roll:
        with torch.no_grad():          # Adam covers self.model only: nothing is learnt through the pre-style net
            _, styled_img1 = pre(imgs[0])
        styled_img1 = styled_img1 / 255.0
        warped1 = style_ref.fs_warp(styled_img1, flows[0])
        _, styled_img2 = model(torch.cat((imgs[1], masks[0], warped1), 1))
        styled_img2 = styled_img2 / 255.0
        loss_img, loss_styled, loss_warped = imgs[1], styled_img2, warped1
        if len(imgs) > 2:
            warped2 = style_ref.fs_warp(styled_img2, flows[1])
            _, styled_img3 = model(torch.cat((imgs[2], masks[1], warped2), 1))
            styled_img3 = styled_img3 / 255.0
            loss_img, loss_styled, loss_warped = imgs[2], styled_img3, warped2
        if len(imgs) > 4:
            warped3 = style_ref.fs_warp(styled_img3, flows[2])
            _, styled_img4 = model(torch.cat((imgs[3], masks[2], warped3), 1))
            styled_img4 = styled_img4 / 255.0
            warped4 = style_ref.fs_warp(styled_img4, flows[3])
            _, styled_img5 = model(torch.cat((imgs[4], masks[3], warped4), 1))
            styled_img5 = styled_img5 / 255.0
            loss_img, loss_styled, loss_warped = imgs[4], styled_img5, warped4
    else:
        _, styled_img2 = model(torch.cat((imgs[1], 0.0 * masks[0], 0.0 * imgs[1]), 1))
        styled_img2 = styled_img2 / 255.0
        loss_img, loss_styled, loss_warped = imgs[1], styled_img2, styled_img2
    styled_features = vgg(style_ref.normalize(loss_styled))
    img_features = vgg(style_ref.normalize(loss_img))
    content = alpha * F.mse_loss(styled_features[2], img_features[2])
    style = 0
    for i, gs in enumerate(grams):
        style = style + ((style_ref.gram_matrix(styled_features[i]) - gs) ** 2).mean()
    style = style * beta
    if roll:
        temporal = gamma * ((masks[-1] * (loss_warped - loss_styled)) ** 2).mean()
    else:
        temporal = torch.zeros((), dtype=loss_styled.dtype)
    return (content + style + temporal, style, content, temporal), styled_img2


def nets(eps=0.0, seed=0):
    """(model, pre-style model, vgg) in fp64 from the seeded weights, scaled by 1 + eps N(0,1) if eps."""
    model = style_ref.RefFastStyleNet(7)
    style_ref.load_np(model, style_ref.fsn_weights(model, MODEL_SEED))
    pre = style_ref.RefFastStyleNet(3)
    style_ref.load_np(pre, style_ref.fsn_weights(pre, PRE_SEED))
    vgg = style_ref.RefVGG("vgg16")
    style_ref.load_np(vgg, style_ref.vgg_weights(vgg, VGG_SEED))
    model, pre, vgg = model.double(), pre.double(), vgg.double()
    if eps:
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in list(model.parameters()) + list(pre.parameters()) + list(vgg.parameters()):
                p.mul_(1 + eps * torch.randn(p.shape, generator=gen).double())
    return model, pre, vgg


@functools.lru_cache(maxsize=None)
def reference_run(n_frames=3, emph=EMPH, roll=True, eps=0.0, seed=0, steps=2):
    """``steps`` reference train steps on the first ``n_frames`` frames (all 4 mask / flow planes are passed, as
    the reference's loader does, so the temporal term reads masks[-1]) with torch.optim.Adam(lr 1e-3) on the
    recurrent model between them: ([[total, style, content, temporal] per step], step-0 parameter gradients)."""
    imgs, style, masks, flows = step_inputs()
    imgs = [i.double() for i in imgs[:n_frames]]
    masks, flows = [m.double() for m in masks], [f.double() for f in flows]
    model, pre, vgg = nets(eps, seed)
    with torch.no_grad():
        grams = [style_ref.gram_matrix(f) for f in vgg(style_ref.normalize(style.double()))]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses, grads = [], None
    for s in range(steps):
        opt.zero_grad()
        ls, _ = ruder_losses(model, pre, vgg, grams, imgs, masks, flows, emph, roll)
        ls[0].backward()
        losses.append([float(v.detach()) for v in ls])
        if s == 0:
            grads = {k: p.grad.clone().numpy() for k, p in model.named_parameters()}
        opt.step()
    return losses, grads
