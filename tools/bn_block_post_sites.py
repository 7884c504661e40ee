#!/usr/bin/env python3
"""The ResNet-50 bottleneck tails at pos='residual' (bs 256, bf16, channels-last) through `CNSN.forward_bn_block`:
bn3 + SelfNorm + add + ReLU (`add_mode="post"`, all four site shapes) and bn3 + SelfNorm (`add_mode="none"`, the IBN-b blocks:
56x56 and 28x28) — the single launch (CNSN_BN_BLOCK=1) against the un-fused sequence (CNSN_BN_BLOCK=0: nn.BatchNorm2d + the
op's own launches), alternating, HIP events; median and min..max of the repeats.  `model`: one ResNet-50-IBN-b pos='residual'
training step (bs 256, 224x224, bf16 autocast, channels-last, SGD) with the switch on and off instead.  `once <mode> <i>
<on|off>`: a few calls of one site and nothing else, for a profiler.  (measurement aid; profiles/r09_bn_block_post.md)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cnsn_amd  # noqa: E402
from cnsn_amd import functional as F_  # noqa: E402

dev = torch.device("cuda:0")
CL = torch.channels_last
SITES = ((256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7))
CASES = [("post", i) for i in range(4)] + [("none", 0), ("none", 1)]


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}..{max(v):.3f})"


def site(mode, shape):
    t = lambda: torch.randn(shape, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)  # noqa: E731
    c, b, gy = t().requires_grad_(), t().requires_grad_(), t()
    m = cnsn_amd.CNSN(None, cnsn_amd.SelfNorm(shape[1])).to(dev).train()
    bn = torch.nn.BatchNorm2d(shape[1]).to(dev).train()

    def call():
        c.grad = b.grad = None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        y = m.forward_bn_block(c, bn, b if mode == "post" else None, relu=mode == "post", add_mode=mode)
        ev[1].record()
        y.backward(gy)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
    return call


def sites():
    print("| site | mode | single launch fwd ms | bwd ms | un-fused fwd ms | bwd ms | tensor MB |")
    print("|---|---|---|---|---|---|---|")
    for mode, i in CASES:
        shape = SITES[i]
        call = site(mode, shape)
        times = {True: ([], []), False: ([], [])}
        for rep in range(24):                       # alternating; the first four of each are warm-up
            for fused in (True, False):
                F_._BN_BLOCK = fused
                f, b = call()
                if rep >= 4:
                    times[fused][0].append(f)
                    times[fused][1].append(b)
        print(f"| {shape} | {mode} | {spread(times[True][0])} | {spread(times[True][1])} | {spread(times[False][0])} | "
              f"{spread(times[False][1])} | {shape[0] * shape[1] * shape[2] * shape[3] * 2 / 1e6:.0f} |", flush=True)


def model():
    from cnsn_amd.callers import ResNet50IBNCNSN
    torch.manual_seed(0)
    net = ResNet50IBNCNSN(ibn_cfg=("b", "b", None, None), cnsn_type="sn", pos="residual").to(dev).to(memory_format=CL).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    x = torch.randn(256, 3, 224, 224, device=dev).contiguous(memory_format=CL)
    yl = torch.randint(0, 1000, (256,), device=dev)

    def step():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(net(x), yl)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    times = {True: [], False: []}
    for rep in range(14):                           # alternating; the first four of each are warm-up
        for fused in (True, False):
            F_._BN_BLOCK = fused
            t = step()
            if rep >= 4:
                times[fused].append(t)
    print(f"ResNet-50-IBN-b pos='residual' bs 256 bf16 step: single launch {spread(times[True])} ms, "
          f"un-fused {spread(times[False])} ms", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["once"]:
        F_._BN_BLOCK = args[3] == "on"
        call = site(args[1], SITES[int(args[2])])
        for _ in range(6):
            call()
    elif "model" in args:
        model()
    else:
        sites()
