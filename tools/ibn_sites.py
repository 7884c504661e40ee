#!/usr/bin/env python3
"""The IBN layers of ResNet-50-IBN-a / -b at N = 256, bf16, channels-last: forward and backward of each site in three versions,
timed with device events —
  fused   this library's single launch (callers/ibn.py -> functional.IBNorm, cnsn_forward_ibn / cnsn_backward_ibn)
  today   this library's IBN / InstanceNorm2d path before it (CNSN_NHWC_FUSED=0: split, plane-statistics kernels, MIOpen
          BatchNorm2d, cat, ReLU)
  torch   what the reference runs: torch.split + nn.InstanceNorm2d + nn.BatchNorm2d + torch.cat + ReLU
— and the model line: a ResNet-50-IBN-a and -b training step at bs 256, bf16 autocast, channels-last, in images/s, with this
library's IBN layers and with torch's own.

    python tools/ibn_sites.py [--iters 20] [--only fused|today|torch] [--no-model] [--csv DIR]

Needed bytes per site: forward 3 tensor passes (+2 with the addend), backward 5 (+2) — csrc/cnsn_nhwc_ibn_kernels.h.  Kernel
times and bytes come from runs of their own: `rocprofv3 --kernel-trace --stats` and `rocprofv3 --pmc FETCH_SIZE` /
`--pmc WRITE_SIZE` around `--only fused --iters 3 --no-model`."""
import argparse
import csv
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SITES = [("a", "layer1.i.bn1", (256, 64, 56, 56), 32, False), ("a", "layer2.0.bn1", (256, 128, 56, 56), 64, False),
         ("a", "layer2.i.bn1", (256, 128, 28, 28), 64, False), ("a", "layer3.0.bn1", (256, 256, 28, 28), 128, False),
         ("a", "layer3.i.bn1", (256, 256, 14, 14), 128, False), ("b", "bn1 (stem)", (256, 64, 112, 112), 64, False),
         ("b", "layer1.2.IN", (256, 256, 56, 56), 256, True), ("b", "layer2.3.IN", (256, 512, 28, 28), 512, True)]
PEAK = 8.0e12


def set_fused(on):
    from cnsn_amd import _ffi
    if on:
        os.environ.pop("CNSN_NHWC_FUSED", None)
    else:
        os.environ["CNSN_NHWC_FUSED"] = "0"
    _ffi.reload_env()


class TorchIBN(nn.Module):
    """the reference's layer (models/imagenet/resnet_ibn_cnsn.py:24-44; nn.InstanceNorm2d alone when half == C) + the ReLU"""

    def __init__(self, c, half):
        super().__init__()
        self.half = half
        self.IN = nn.InstanceNorm2d(half, affine=True)
        self.BN = nn.BatchNorm2d(c - half) if half < c else None

    def forward_act(self, x, addend=None, relu=True):
        if addend is not None:
            x = x + addend
        if self.BN is None:
            y = self.IN(x)
        else:
            s = torch.split(x, self.half, 1)
            y = torch.cat((self.IN(s[0].contiguous()), self.BN(s[1].contiguous())), 1)
        return torch.relu(y) if relu else y

    def forward(self, x):
        return self.forward_act(x, relu=False)


def layer(version, c, half):
    from cnsn_amd.callers import IBN, InstanceNorm2d
    if version == "torch":
        return TorchIBN(c, half)
    return InstanceNorm2d(c, affine=True) if half == c else IBN(c)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def time_site(version, shape, half, addend, iters):
    dev = torch.device("cuda")
    c = shape[1]
    set_fused(version != "today")
    m = layer(version, c, half).to(dev).train()
    x = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_()
    a = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last) if addend else None
    gy = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    fwd, bwd, route = [], [], None
    for i in range(iters + 3):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        y = m.forward_act(x, a, relu=True)
        e1.record()
        route = type(y.grad_fn).__name__
        y.backward(gy)
        e2.record()
        torch.cuda.synchronize()
        if i >= 3:
            fwd.append(e0.elapsed_time(e1))
            bwd.append(e1.elapsed_time(e2))
        x.grad = None
        del y
    set_fused(True)
    return median(fwd), median(bwd), route


def model_step(variant, torch_layers, iters):
    from cnsn_amd.callers import IBN, InstanceNorm2d, resnet50_ibn_a, resnet50_ibn_b

    class Cfg:
        active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"
    m = (resnet50_ibn_a if variant == "a" else resnet50_ibn_b)(Cfg)
    if torch_layers:       # torch's own IBN layers in place of this library's
        for name, mod in list(m.named_modules()):
            if isinstance(mod, (IBN, InstanceNorm2d)):
                parent = m.get_submodule(name.rsplit(".", 1)[0]) if "." in name else m
                c = mod.num_features if isinstance(mod, InstanceNorm2d) else mod.half + mod.BN.num_features
                setattr(parent, name.rsplit(".", 1)[-1], TorchIBN(c, c if isinstance(mod, InstanceNorm2d) else mod.half))
    m = m.cuda().to(memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    x = torch.randn(256, 3, 224, 224, device="cuda").contiguous(memory_format=torch.channels_last)
    tgt = torch.randint(0, 1000, (256,), device="cuda")
    times = []
    for i in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = nn.functional.cross_entropy(m(x), tgt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    ms = median(times)
    return ms, 256 / (ms / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["fused", "today", "torch"])
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/ibn_sites.py measures on the GPU"
    import cnsn_amd  # noqa: F401
    versions = [args.only] if args.only else ["fused", "today", "torch"]
    rows = []
    for v, site, shape, half, addend in SITES:
        n, c, h, w = shape
        tensor = n * c * h * w * 2
        need_f, need_b = (5 if addend else 3) * tensor, (7 if addend else 5) * tensor
        for ver in versions:
            f, b, route = time_site(ver, shape, half, addend, args.iters)
            row = dict(backbone=v, site=site, shape="x".join(map(str, shape)), half=half, addend=int(addend), version=ver, route=route,
                       fwd_ms=round(f, 4), bwd_ms=round(b, 4), fwd_bwd_ms=round(f + b, 4),
                       frac_hbm_fwd=round(need_f / (f / 1e3) / PEAK, 3), frac_hbm_bwd=round(need_b / (b / 1e3) / PEAK, 3))
            rows.append(row)
            print(row, flush=True)
            torch.cuda.empty_cache()
    model = []
    if not args.no_model:
        for v in ("a", "b"):
            for torch_layers in (False, True):
                ms, ips = model_step(v, torch_layers, args.iters)
                r = dict(backbone=f"resnet50_ibn_{v}", layers="torch" if torch_layers else "cnsn_amd", ms_per_step=round(ms, 2),
                         images_per_s=round(ips, 1))
                model.append(r)
                print(r, flush=True)
                torch.cuda.empty_cache()
    if args.csv:
        os.makedirs(args.csv, exist_ok=True)
        for name, data in (("ibn_sites.csv", rows), ("ibn_model.csv", model)):
            if data:
                with open(os.path.join(args.csv, name), "w", newline="") as fh:
                    wr = csv.DictWriter(fh, fieldnames=list(data[0]))
                    wr.writeheader()
                    wr.writerows(data)


if __name__ == "__main__":
    main()
