#!/usr/bin/env python3
"""G6b: one training step of the IMPORTED reference ResNet-50 (+SN, pos=post) — gradients, not only logits (build container only).

    python tests/golden/gen_golden_models_grad.py     # writes tests/golden/g6b_r50_grad.npz

G6's input `r50_x` (4,3,224,224) and G6's name-seeded fill (`fill_by_name(r50, 2)`), train mode with grad enabled, the fixed
scalar loss (logits * w).sum() with a seeded `w` stored in the fixture; fp64 (the truth) and fp32 (its noise).  Stored: the
logits; the gradients of fc.weight (classes 0-3: the whole matrix is 16 MB in fp64), layer4.2's bn3 and SelfNorm gate,
layer4.0's downsample BatchNorm2d, layer1.0's SelfNorm gate and the stem convolution; three running variances after the
step.  Arrays only — no reference source, no checkpoint."""
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

from tests.golden.gen_golden_fill import fill_by_name  # noqa: E402
from tests.golden.gen_golden_models import resnet50  # noqa: E402  (G6's generator imports the reference)

torch.set_num_threads(8)

FC_ROWS = 4
GRADS = ["fc.weight", "layer4.2.bn3.weight", "layer4.2.bn3.bias", "layer4.2.cnsn.selfnorm.g_fc.weight", "layer4.0.downsample.1.weight",
         "layer1.0.cnsn.selfnorm.g_fc.weight", "conv1.weight"]
RUNNING = ["layer2.1.bn3.running_var", "layer3.0.downsample.1.running_var", "layer4.2.cnsn.selfnorm.g_bn.running_var"]


def main():
    x = torch.from_numpy(np.load(os.path.join(HERE, "g6_models.npz"))["r50_x"])
    w = torch.randn(4, 1000, generator=torch.Generator().manual_seed(6002), dtype=torch.float64)
    out = {"w": w.numpy(), "grad_names": np.array(GRADS), "running_names": np.array(RUNNING), "fc_rows": np.array(FC_ROWS)}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with contextlib.redirect_stdout(io.StringIO()):
            class Cfg:
                active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"
            r50 = resnet50(Cfg)
        fill_by_name(r50, 2).to(dt).train()
        logits = r50(x.to(dt))
        (logits * w.to(dt)).sum().backward()
        params, state = dict(r50.named_parameters()), r50.state_dict()
        out[f"{tag}_logits"] = logits.detach().numpy()
        for k in GRADS:
            gr = params[k].grad
            out[f"{tag}_grad_{k}"] = (gr[:FC_ROWS] if k == "fc.weight" else gr).numpy()
        for k in RUNNING:
            out[f"{tag}_{k}"] = state[k].numpy()
    path = os.path.join(HERE, "g6b_r50_grad.npz")
    np.savez_compressed(path, **out)
    print("g6b_r50_grad.npz", os.path.getsize(path), "bytes")
    for k in sorted(out):
        if out[k].dtype.kind == "f":
            print(k, out[k].shape, float(np.abs(out[k]).max()))


if __name__ == "__main__":
    main()
