#!/usr/bin/env python3
"""`relu(bn(x))` on dense NCHW tensors at the sites of the workloads that stay in NCHW — WideResNet-40-2 at bs 128 (fp32) and the
dilated FCN-ResNet50 backbone at bs 16, 512x512 (bf16) — training: forward and backward of each layer in two versions, timed with
device events in the SAME process, the two alternating, after a warm-up of every shape —
  fused   this library's two plain launches per direction (callers/bn_act.py with CNSN_BN_ACT_NCHW=1 ->
          functional.BatchNormActNCHW, cnsn_forward_bn_act_nchw / cnsn_backward_bn_act_nchw)
  plain   the statements before it (the default): torch's nn.BatchNorm2d (MIOpen) + nn.ReLU(inplace=True)
Every (site, version) is measured `--rounds` times (`--iters` calls each, median); the table gives the median of the rounds and
their spread (max - min), which is what a difference has to exceed.

    python tools/bn_act_nchw_sites.py [--iters 20] [--rounds 5] [--only fused|plain] [--family wrn|fcn] [--csv DIR]

Needed bytes per site: forward 3 tensor passes, backward 5 (csrc/cnsn_nchw_bn_kernels.h).  Kernel times and bytes come from runs of
their own: `rocprofv3 --kernel-trace --stats` and `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` around
`--only fused --iters 3 --rounds 1`."""
import argparse
import csv
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, BF16 = torch.float32, torch.bfloat16
SITES = [("wrn", "block1 bn2", (128, 32, 32, 32), F32), ("wrn", "conv1 / block1.0 bn1", (128, 16, 32, 32), F32),
         ("wrn", "block2 bn2", (128, 64, 16, 16), F32), ("wrn", "block3 bn2", (128, 128, 8, 8), F32),
         ("fcn", "stem bn1", (16, 64, 256, 256), BF16), ("fcn", "layer1 bn3-wide", (16, 256, 128, 128), BF16),
         ("fcn", "layer3 (dilated)", (16, 1024, 64, 64), BF16), ("fcn", "layer4 (dilated)", (16, 2048, 64, 64), BF16)]
PEAK = 8.0e12


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


class Site:
    def __init__(self, shape, dtype):
        dev = torch.device("cuda")
        self.bn = nn.BatchNorm2d(shape[1]).to(dev).train()
        self.x = torch.randn(shape, device=dev, dtype=dtype).requires_grad_()
        self.gy = torch.randn(shape, device=dev, dtype=dtype)

    def run(self, fused, iters):
        from cnsn_amd.callers import _sites, bn_act
        was = _sites.FUSE_BN_ACT_NCHW
        _sites.FUSE_BN_ACT_NCHW = fused
        fwd, bwd, route = [], [], None
        for _ in range(iters):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            y = bn_act(self.bn, self.x)
            e1.record()
            route = type(y.grad_fn).__name__
            y.backward(self.gy)
            e2.record()
            torch.cuda.synchronize()
            fwd.append(e0.elapsed_time(e1))
            bwd.append(e1.elapsed_time(e2))
            self.x.grad = self.bn.weight.grad = self.bn.bias.grad = None      # (as zero_grad(set_to_none=True) leaves them)
            del y
        _sites.FUSE_BN_ACT_NCHW = was
        return median(fwd), median(bwd), route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["fused", "plain"])
    ap.add_argument("--family", choices=["wrn", "fcn"])
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bn_act_nchw_sites.py measures on the GPU"
    versions = [args.only] if args.only else ["fused", "plain"]
    rows = []
    for fam, name, shape, dtype in SITES:
        if args.family and fam != args.family:
            continue
        s = Site(shape, dtype)                                   # (one site at a time: the FCN tensors are 0.5 GB each)
        for ver in versions:                                     # warm-up, both versions
            s.run(ver == "fused", 3)
        got = {ver: [] for ver in versions}
        for _ in range(args.rounds):                             # the two alternating
            for ver in versions:
                got[ver].append(s.run(ver == "fused", args.iters))
        tensor = s.x.numel() * s.x.element_size()
        for ver in versions:
            f, b = [g[0] for g in got[ver]], [g[1] for g in got[ver]]
            t = [g[0] + g[1] for g in got[ver]]
            row = dict(family=fam, site=name, shape="x".join(map(str, shape)), dtype=str(dtype)[6:], version=ver, route=got[ver][0][2],
                       fwd_ms=round(median(f), 4), bwd_ms=round(median(b), 4), fwd_bwd_ms=round(median(t), 4),
                       spread_ms=round(max(t) - min(t), 4), frac_hbm_fwd=round(3 * tensor / (median(f) / 1e3) / PEAK, 3),
                       frac_hbm_bwd=round(5 * tensor / (median(b) / 1e3) / PEAK, 3))
            rows.append(row)
            print(row, flush=True)
        del s
        torch.cuda.empty_cache()
    if args.csv:
        os.makedirs(args.csv, exist_ok=True)
        with open(os.path.join(args.csv, "bn_act_nchw_sites.csv"), "w", newline="") as fh:
            wr = csv.DictWriter(fh, fieldnames=list(rows[0]))
            wr.writeheader()
            wr.writerows(rows)


if __name__ == "__main__":
    main()
