"""Generate tests/golden/stargan2_small.npz by importing the READ-ONLY reference.

TEST INFRASTRUCTURE ONLY — build container only (the GPU box never runs this); the output is data.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_stargan2.py

Imported from the reference tree: methods/GAN-based/StarGANv2AdvCon/core/model.py (Generator, MappingNetwork,
StyleEncoder, Discriminator), fp32 on the CPU.  The module imports ``munch`` (not installed) and ``core.wing``
(the FAN of the w_hpf > 0 path, unused at w_hpf = 0): both are replaced by in-memory stubs before the import.
Weights are tests/stargan2_ref.make_state(seed, shapes) by name, inputs and upstream gradients
stargan2_ref.case_inputs(seed + 1, ...), the generator's style code stargan2_ref.style_code(seed + 2, ...): the
tests regenerate all of them, so none is stored.

Cases (stargan2_ref.CASES):
  G  Generator(256, style_dim=16, max_conv_dim=8, w_hpf=0), input 2x3x64x32 (bottleneck 4x2), s 2x16
  E  StyleEncoder(64, 16, num_domains=3, max_conv_dim=8), input 2x3x64x64, y = [2, 0]
  D  Discriminator(64, 3, max_conv_dim=8), input 2x3x64x64, y = [2, 0]
  F  MappingNetwork(16, 16, 3), z 2x16, y = [1, 1]
Stored per case: the state_dict key list and parameter count, the output, the input gradient of sum(out * r) (and
ds for G) and every parameter gradient, the all-zero ones of F's domains 0 and 2 included — as stargan2_ref.stored
keeps them: of the 64 -> 64 3x3 weights of G, the 256 -> 256 3x3 weight of E and D and the 512 x 512 weights of F
the first BIG_ROWS output rows
(the whole would take the file past the 1 MiB cap of a committed file).
Also the key lists and parameter counts of the four default-size nets (stargan2_ref.DEFAULTS).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "stargan2_small.npz")
sys.path.insert(0, os.path.join(REPO, "tests"))
import stargan2_ref as S  # noqa: E402

CLASS = {"generator": "Generator", "mapping_network": "MappingNetwork", "style_encoder": "StyleEncoder",
         "discriminator": "Discriminator"}


def reference_model():
    munch = types.ModuleType("munch")
    munch.Munch = dict
    wing = types.ModuleType("core.wing")
    wing.FAN = object
    core = types.ModuleType("core")
    core.wing = wing
    sys.modules.update({"munch": munch, "core": core, "core.wing": wing})
    path = os.path.join(REF, "methods", "GAN-based", "StarGANv2AdvCon", "core", "model.py")
    spec = importlib.util.spec_from_file_location("core.model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(model, kind, cfg):
    if kind == "generator":
        return model.Generator(cfg["img_size"], cfg["style_dim"], cfg["max_conv_dim"], w_hpf=0)
    return getattr(model, CLASS[kind])(**cfg)


def main():
    torch.set_num_threads(S.FIXTURE_THREADS)
    model = reference_model()
    out = {}
    for name, c in S.CASES.items():
        kind, cfg = c["kind"], c["cfg"]
        net = build(model, kind, cfg)
        keys = list(net.state_dict())
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        want = S.shapes(kind, **cfg)
        assert keys == list(want) and shapes == want, name
        sd = S.make_state(c["seed"], shapes)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        x, r = S.case_inputs(c["seed"] + 1, c["x"], S.out_shape(name))
        xt = torch.from_numpy(x).requires_grad_(True)
        if kind == "generator":
            st = torch.from_numpy(S.style_code(c["seed"] + 2, c["x"][0], cfg["style_dim"])).requires_grad_(True)
            y = net(xt, st)
        else:
            y = net(xt, torch.tensor(c["y"], dtype=torch.long))
        (y * torch.from_numpy(r)).sum().backward()
        out.update({f"{name}_keys": np.array(keys), f"{name}_count": np.int64(sum(p.numel() for p in net.parameters())),
                    f"{name}_out": y.detach().numpy(), f"{name}_dx": xt.grad.numpy()})
        if kind == "generator":
            out[f"{name}_ds"] = st.grad.numpy()
        for k, p in net.named_parameters():
            g = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().astype(np.float32)
            out[f"{name}_g_{k}"] = S.stored(g)
    for kind, cfg in S.DEFAULTS.items():
        net = build(model, kind, cfg)
        assert list(net.state_dict()) == list(S.shapes(kind, **cfg)), kind
        out[f"default_{kind}_keys"] = np.array(list(net.state_dict()))
        out[f"default_{kind}_count"] = np.int64(sum(p.numel() for p in net.parameters()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), len(out), "arrays")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
