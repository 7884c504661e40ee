#!/usr/bin/env python3
"""G9: ResNet-50-IBN-a / -b golden vectors from the IMPORTED reference backbones (build container only).

    python tests/golden/gen_golden_ibn.py     # writes tests/golden/g9_ibn.npz

Both backbones of models/imagenet/resnet_ibn_cnsn.py (`resnet50_ibn_a`, `resnet50_ibn_b`, pos='post', cnsn_type='sn') on
G6's input (4,3,224,224) with the name-seeded fill of gen_golden_fill.fill_by_name(model, 3): state_dict keys and shapes;
train- then eval-mode logits (fp32, fp64); one training step of a fresh model with loss (logits * w).sum() — logits, the
gradients of a few IBN / InstanceNorm parameters, conv1 and fc rows 0-3, and running statistics after it.  Inputs, seeds
and results only — no reference source, no checkpoint."""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True   # the reference tree is read-only material: leave no __pycache__ in it

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
np.int = int

from tests.golden.gen_golden_fill import fill_by_name  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):          # the reference prints per site
    from models.imagenet.resnet_ibn_cnsn import resnet50_ibn_a, resnet50_ibn_b  # noqa: E402

torch.set_num_threads(8)

SEED = 3
FC_ROWS = 4
BUILD = {"a": resnet50_ibn_a, "b": resnet50_ibn_b}
GRADS = {"a": ["layer1.0.bn1.IN.weight", "layer1.0.bn1.BN.weight", "layer3.5.bn1.IN.bias", "conv1.weight", "fc.weight"],
         "b": ["bn1.weight", "layer1.2.IN.weight", "layer2.3.IN.bias", "conv1.weight", "fc.weight"]}
RUNNING = {"a": ["layer1.0.bn1.BN.running_var", "layer3.5.bn1.BN.running_mean", "layer4.2.cnsn.selfnorm.g_bn.running_var"],
           "b": ["layer1.0.bn1.running_var", "layer2.3.bn3.running_mean", "layer4.2.cnsn.selfnorm.g_bn.running_var"]}


class Cfg:
    active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"


def make(v, dt):
    with contextlib.redirect_stdout(io.StringIO()):
        m = BUILD[v](Cfg)
    return fill_by_name(m, SEED).to(dt)


def main():
    x = torch.from_numpy(np.load(os.path.join(HERE, "g6_models.npz"))["r50_x"])
    w = torch.randn(4, 1000, generator=torch.Generator().manual_seed(6009), dtype=torch.float64)
    out = {"w": w.numpy(), "fc_rows": np.array(FC_ROWS), "seed": np.array(SEED)}
    for v in BUILD:
        out[f"{v}_keys"] = np.array([f"{k}|{tuple(t.shape)}" for k, t in make(v, torch.float32).state_dict().items()])
        out[f"{v}_grad_names"] = np.array(GRADS[v])
        out[f"{v}_running_names"] = np.array(RUNNING[v])
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            m = make(v, dt).train()
            with torch.no_grad():
                out[f"{v}_{tag}_train"] = m(x.to(dt)).numpy()
                m.eval()
                out[f"{v}_{tag}_eval"] = m(x.to(dt)).numpy()
            m = make(v, dt).train()                       # the step: a fresh model
            logits = m(x.to(dt))
            (logits * w.to(dt)).sum().backward()
            params, state = dict(m.named_parameters()), m.state_dict()
            out[f"{v}_{tag}_step_logits"] = logits.detach().numpy()
            for k in GRADS[v]:
                gr = params[k].grad
                out[f"{v}_{tag}_grad_{k}"] = (gr[:FC_ROWS] if k == "fc.weight" else gr).numpy()
            for k in RUNNING[v]:
                out[f"{v}_{tag}_{k}"] = state[k].numpy()
    path = os.path.join(HERE, "g9_ibn.npz")
    np.savez_compressed(path, **out)
    print("g9_ibn.npz", os.path.getsize(path), "bytes")
    for k in sorted(out):
        if out[k].dtype.kind == "f":
            print(k, out[k].shape, float(np.abs(out[k]).max()))


if __name__ == "__main__":
    main()
