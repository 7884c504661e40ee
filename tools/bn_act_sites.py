#!/usr/bin/env python3
"""`relu(bn(x))` at the sites a ResNet-50 runs at bs 256, bf16, channels-last, training: forward and backward of each layer in
two versions, timed with device events in the SAME process, the two alternating, after a warm-up of every shape —
  fused   this library's single launch (callers/bn_act.py -> functional.BatchNormAct, cnsn_forward_bn_act / cnsn_backward_bn_act)
  plain   the statements before it (CNSN_BN_ACT=0): torch's nn.BatchNorm2d (MIOpen) + nn.ReLU(inplace=True)
Every (site, version) is measured `--rounds` times (`--iters` calls each, median); the table gives the median of the rounds and
their spread (max - min), which is what a difference has to exceed.

    python tools/bn_act_sites.py [--iters 20] [--rounds 5] [--only fused|plain] [--mode 2] [--csv DIR]

`--mode`: CNSN_NHWC_FUSED for the fused version (2: wherever the kernels apply — what the AUTO rule is derived from; 1: AUTO).
Needed bytes per site: forward 3 tensor passes, backward 5 (csrc/cnsn_nhwc_bn_kernels.h).  Kernel times and bytes come from runs
of their own: `rocprofv3 --kernel-trace --stats` and `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` around
`--only fused --iters 3 --rounds 1`."""
import argparse
import csv
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SITES = [("stem bn1", (256, 64, 112, 112), 1), ("layer1 bn1/bn2", (256, 64, 56, 56), 6), ("layer2.0 bn1", (256, 128, 56, 56), 1),
         ("layer2 bn1/bn2", (256, 128, 28, 28), 7), ("layer3.0 bn1", (256, 256, 28, 28), 1), ("layer3 bn1/bn2", (256, 256, 14, 14), 11),
         ("layer4.0 bn1", (256, 512, 14, 14), 1), ("layer4 bn1/bn2", (256, 512, 7, 7), 5)]
PEAK = 8.0e12


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


class Site:
    def __init__(self, shape):
        dev = torch.device("cuda")
        cl = torch.channels_last
        self.bn = nn.BatchNorm2d(shape[1]).to(dev).train()
        self.x = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=cl).requires_grad_()
        self.gy = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=cl)

    def run(self, fused, iters):
        from cnsn_amd.callers import _sites, bn_act
        _sites.FUSE_BN_ACT = fused
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
        _sites.FUSE_BN_ACT = True
        return median(fwd), median(bwd), route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["fused", "plain"])
    ap.add_argument("--mode", default="2")
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bn_act_sites.py measures on the GPU"
    from cnsn_amd import _ffi
    os.environ["CNSN_NHWC_FUSED"] = args.mode
    _ffi.reload_env()
    versions = [args.only] if args.only else ["fused", "plain"]
    sites = [(name, shape, count, Site(shape)) for name, shape, count in SITES]
    for _, _, _, s in sites:                                     # warm-up of every shape, both versions
        for ver in versions:
            s.run(ver == "fused", 3)
    rows = []
    for name, shape, count, s in sites:
        got = {ver: [] for ver in versions}
        for _ in range(args.rounds):                             # the two alternating
            for ver in versions:
                got[ver].append(s.run(ver == "fused", args.iters))
        tensor = s.x.numel() * 2
        for ver in versions:
            f, b = [g[0] for g in got[ver]], [g[1] for g in got[ver]]
            t = [g[0] + g[1] for g in got[ver]]
            row = dict(site=name, shape="x".join(map(str, shape)), layers=count, version=ver, route=got[ver][0][2],
                       fwd_ms=round(median(f), 4), bwd_ms=round(median(b), 4), fwd_bwd_ms=round(median(t), 4),
                       spread_ms=round(max(t) - min(t), 4), frac_hbm_fwd=round(3 * tensor / (median(f) / 1e3) / PEAK, 3),
                       frac_hbm_bwd=round(5 * tensor / (median(b) / 1e3) / PEAK, 3))
            rows.append(row)
            print(row, flush=True)
    if len(versions) == 2:
        total = {ver: sum(r["fwd_bwd_ms"] * r["layers"] for r in rows if r["version"] == ver) for ver in versions}
        print({"per_step_ms_all_33_layers": {k: round(v, 3) for k, v in total.items()}}, flush=True)
    if args.csv:
        os.makedirs(args.csv, exist_ok=True)
        with open(os.path.join(args.csv, "bn_act_sites.csv"), "w", newline="") as fh:
            wr = csv.DictWriter(fh, fieldnames=list(rows[0]))
            wr.writeheader()
            wr.writerows(rows)


if __name__ == "__main__":
    main()
