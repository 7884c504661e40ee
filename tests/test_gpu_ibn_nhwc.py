"""The single-launch channels-last IBN layer (functional.IBNorm, cnsn_forward_ibn / cnsn_backward_ibn) against torch's own
nn.InstanceNorm2d / nn.BatchNorm2d in float64 — what the reference's IBN backbones instantiate
(models/imagenet/resnet_ibn_cnsn.py:24-44, :63-65) — through the modules of callers/ibn.py: y, dx, d-addend, every parameter
gradient, the running buffers, num_batches_tracked and momentum=None; toy shapes over the whole matrix (training / eval,
ReLU on / off, with / without the addend, affine=False, a constant plane) and every ResNet-50-IBN site at N = 256 in the
variant the backbone runs; the calls the launch does not take give today's results.  Every shape that RUNS the launch here has a
power-of-two channel count: C = 48 is only asked for its plan (test_fallbacks_give_todays_results), never run — the launch at
channel counts that are no power of two is test_gpu_nhwc_geometry.py's."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from cnsn_amd import functional  # noqa: E402
from cnsn_amd.callers import IBN, InstanceNorm2d  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last


def make_module(c, half, affine=True, momentum=0.1, seed=0):
    g = torch.Generator().manual_seed(seed + 11)
    if half == c:
        mod = InstanceNorm2d(c, affine=affine)
    else:
        mod = IBN(c, ratio=half / c)
        assert mod.half == half
        mod.BN.momentum = momentum
    with torch.no_grad():
        ins = mod if half == c else mod.IN
        if affine:
            ins.weight.copy_(torch.rand(half, generator=g) + 0.5)
            ins.bias.copy_(torch.randn(half, generator=g))
        if half < c:
            mod.BN.weight.copy_(torch.rand(c - half, generator=g) + 0.5)
            mod.BN.bias.copy_(torch.randn(c - half, generator=g))
            mod.BN.running_mean.copy_(torch.randn(c - half, generator=g) * 0.1)
            mod.BN.running_var.copy_(torch.rand(c - half, generator=g) + 0.5)
            mod.BN.num_batches_tracked.fill_(3)
    return mod


def torch_twin(mod, c, half, dtype, dev):
    """the reference's layer with the module's parameters and buffers: nn.InstanceNorm2d (+ nn.BatchNorm2d) in `dtype`"""
    ins = mod if half == c else mod.IN
    tin = nn.InstanceNorm2d(half, affine=ins.affine)
    tbn = None
    if half < c:
        tbn = nn.BatchNorm2d(c - half, momentum=mod.BN.momentum)
        tbn.load_state_dict(mod.BN.state_dict())
        tbn.train(mod.BN.training)
    if ins.affine:
        with torch.no_grad():
            tin.weight.copy_(ins.weight)
            tin.bias.copy_(ins.bias)
    tin, tbn = tin.to(dev, dtype), (tbn.to(dev, dtype) if tbn is not None else None)
    if tbn is not None:
        tbn.num_batches_tracked = tbn.num_batches_tracked.to(torch.int64)
    return tin, tbn


def reference(mod, c, half, x, a, gy, mask, dtype, dev):
    """(y, dX, parameter gradients, BatchNorm2d state) of torch's layer on X = x [+ a] (the sum rounded in the activations' dtype,
    as the reference's in-place `out += identity`), its backward run through the device's ReLU mask"""
    tin, tbn = torch_twin(mod, c, half, dtype, dev)
    X = (x if a is None else x + a).to(dev, dtype).detach().requires_grad_()
    parts = [tin(X[:, :half].contiguous())]
    if tbn is not None:
        parts.append(tbn(X[:, half:].contiguous()))
    pre = torch.cat(parts, 1)
    pre.backward(gy.to(dev, dtype) * (mask.to(dev, dtype) if mask is not None else 1))
    grads = {}
    if tin.affine:
        grads["in_w"], grads["in_b"] = tin.weight.grad, tin.bias.grad
    if tbn is not None:
        grads["bn_w"], grads["bn_b"] = tbn.weight.grad, tbn.bias.grad
    state = {k: v for k, v in tbn.state_dict().items()} if tbn is not None else {}
    return pre.detach(), X.grad, grads, state


def compare(name, got, t64, t32, dtype, param=False):
    got, t64, t32 = got.detach().double().cpu(), t64.detach().double().cpu(), t32.detach().double().cpu()
    if dtype == torch.float32:
        scale = max(1.0, float(t64.abs().max()))
        noise = float((t32 - t64).abs().max())
        err = float((got - t64).abs().max())
        bound = max(1e-5 * scale, 2 * noise)
        print(f"    {name}: err {err:.3e} bound {bound:.3e} (oracle32 noise {noise:.3e}, scale {scale:.3g})")
        assert err <= bound, f"{name}: err {err:.3e}, oracle32 noise {noise:.3e}, scale {scale:.3g}"
    else:
        err = float((got - t32).abs().max())
        ref = max(float(t32.abs().max()), 1e-6)
        bound = 1e-2 * ref if not param else 1e-2 * ref + 1e-5
        print(f"    {name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{name}: err {err:.3e} vs max {ref:.3e}"


def run_case(shape, dtype, half, relu=True, addend=False, training=True, affine=True, momentum=0.1, const_plane=False, seed=0,
             expect_fused=True, ref_dev=torch.device("cpu"), edit=None):
    """edit(x64, a64): changes the drawn float64 inputs in place before anything reads them (test_gpu_shift_sample.py)"""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    x64 = torch.randn(shape, generator=gen, dtype=torch.float64) * 1.5 + torch.randn(n, c, 1, 1, generator=gen, dtype=torch.float64)
    a64 = torch.randn(shape, generator=gen, dtype=torch.float64) if addend else None
    gy64 = torch.randn(shape, generator=gen, dtype=torch.float64)
    if const_plane:
        x64[0, 0] = 3.0
        if a64 is not None:
            a64[0, 0] = 0.0
        gy64[0, 0] = 0.0        # (kept out of the parameter gradients, as test_gpu_ibn.py does)
    if edit is not None:
        edit(x64, a64)
    mod = make_module(c, half, affine, momentum, seed)
    mod.train(training)
    twin64 = make_module(c, half, affine, momentum, seed).train(training)     # (state before the call, for the references)
    dmod = mod.to(DEV)
    xg = x64.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    ag = a64.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_() if addend else None
    assert functional.ibn_plan(xg, half, relu, addend, training) == expect_fused
    y = dmod.forward_act(xg, ag, relu=relu)
    assert y.dtype == dtype and y.is_contiguous(memory_format=CL) and y.shape == xg.shape
    y.backward(gy64.to(dtype).to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    mask = (y.detach() > 0).cpu() if relu else None
    xs, as_ = x64.to(dtype), (a64.to(dtype) if addend else None)
    X = xs if as_ is None else (xs + as_)        # (rounded to the dtype: the device's sum)
    r64 = reference(twin64, c, half, X.double(), None, gy64, mask, torch.float64, ref_dev)
    r32 = reference(make_module(c, half, affine, momentum, seed).train(training), c, half, X.float(), None, gy64, mask, torch.float32,
                    ref_dev)
    pre64, pre32 = r64[0], r32[0]
    if relu:
        pre64, pre32 = pre64.clamp_min(0), pre32.clamp_min(0)
    compare("y", y, pre64, pre32, dtype)
    compare("dx", xg.grad, r64[1], r32[1], dtype)
    if addend:
        assert torch.equal(ag.grad, xg.grad), "d-addend is the gradient of the sum"
    ins = dmod if half == c else dmod.IN
    got = {}
    if affine:
        got["in_w"], got["in_b"] = ins.weight.grad, ins.bias.grad
    if half < c:
        got["bn_w"], got["bn_b"] = dmod.BN.weight.grad, dmod.BN.bias.grad
    assert set(got) == set(r64[2])
    for k in got:
        compare(k, got[k], r64[2][k], r32[2][k], dtype, param=True)
    if half < c:
        st = dmod.BN.state_dict()
        assert int(st["num_batches_tracked"]) == int(r64[3]["num_batches_tracked"]) == (4 if training else 3)
        for k in ("running_mean", "running_var"):
            t64 = r64[3][k].double().cpu()
            err = float((st[k].double().cpu() - t64).abs().max())
            bound = (1e-5 if dtype == torch.float32 else 1e-2) * max(1.0, float(t64.abs().max()))
            print(f"    {k}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, f"{k}: err {err:.3e}"
    return y


TOY = [((8, 16, 6, 7), 8), ((12, 32, 9, 9), 16), ((2, 16, 64, 64), 8), ((8, 64, 16, 16), 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,half", TOY, ids=[f"{s}-h{h}" for s, h in TOY])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "id"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_toy_matrix(shape, half, dtype, training, relu, addend):
    run_case(shape, dtype, half, relu=relu, addend=addend, training=training, seed=hash((shape, half)) % 1000)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "f16"])
def test_instance_norm_affine_false_and_constant_plane(dtype):
    run_case((8, 32, 10, 10), dtype, 32, relu=True, addend=True, affine=False, const_plane=True, seed=5)
    run_case((8, 32, 10, 10), dtype, 16, relu=True, const_plane=True, seed=6)


def test_momentum_none_cumulative_average():
    run_case((8, 32, 12, 12), torch.float32, 16, momentum=None, seed=7)


# every site of ResNet-50-IBN-a / -b at N = 256 (224x224 input), in the variant the backbone runs: training, ReLU, the addend at
# IBN-b's block ends
SITES = [("a", (256, 64, 56, 56), 32, False), ("a", (256, 128, 56, 56), 64, False), ("a", (256, 128, 28, 28), 64, False),
         ("a", (256, 256, 28, 28), 128, False), ("a", (256, 256, 14, 14), 128, False),
         ("b-stem", (256, 64, 112, 112), 64, False), ("b-end", (256, 256, 56, 56), 256, True), ("b-end", (256, 512, 28, 28), 512, True)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,shape,half,addend", SITES, ids=[f"{k}-{s[1]}x{s[2]}" for k, s, _, _ in SITES])
def test_full_size_sites(kind, shape, half, addend, dtype):
    run_case(shape, dtype, half, relu=True, addend=addend, training=True, seed=shape[1] + shape[2], ref_dev=DEV)
    torch.cuda.empty_cache()


def today(mod, x):
    """callers/ibn.py's code before the single launch: the split, InstanceNorm2d's plane-statistics kernels, nn.BatchNorm2d, cat"""
    if isinstance(mod, InstanceNorm2d):
        return functional.InstanceNorm.apply(x, mod.weight, mod.bias, mod.eps)
    rest = x.size(1) - mod.half
    y_in = functional.InstanceNorm.apply(x.narrow(1, 0, mod.half).contiguous(), mod.IN.weight, mod.IN.bias, mod.IN.eps)
    return torch.cat([y_in, mod.BN(x.narrow(1, mod.half, rest).contiguous())], dim=1)


@pytest.mark.parametrize("case", ["nchw", "c_not_8", "half_not_8", "n_over_256"])
def test_fallbacks_give_todays_results(case):
    # (half_not_8: C = 48 is eligible, only half = 12 is not)
    shape, halves, fmt = {"nchw": ((8, 32, 8, 8), (16, 32), torch.contiguous_format), "c_not_8": ((8, 20, 8, 8), (10, 20), CL),
                          "half_not_8": ((8, 48, 8, 8), (12,), CL), "n_over_256": ((260, 16, 4, 4), (8, 16), CL)}[case]
    torch.manual_seed(3)
    x = torch.randn(shape, device=DEV).contiguous(memory_format=fmt)
    if case == "half_not_8":
        assert functional.ibn_plan(x, 16, False) and functional.ibn_plan(x, 48, False)
    for half in halves:
        mod = make_module(shape[1], half).to(DEV).train()
        twin = make_module(shape[1], half).to(DEV).train()
        assert not functional.ibn_plan(x, half, False)
        y = mod(x)
        assert torch.equal(y, today(twin, x)), f"{case} half={half}: not today's result"
        yr = mod.forward_act(x, relu=True)
        assert torch.equal(yr, torch.relu(today(twin, x))), f"{case} half={half}: forward_act is not relu(today's result)"


@pytest.mark.parametrize("half", [16, 32], ids=["ibn", "in"])
def test_no_launch_under_graph_capture(half):
    """under stream capture the layer runs today's code (the persistent launch is not captured: its barrier bases would be
    replayed): the replayed output equals today's result"""
    torch.manual_seed(4)
    x = torch.randn(8, 32, 8, 8, device=DEV).contiguous(memory_format=CL)
    assert functional.ibn_plan(x, half, True)
    mod = make_module(32, half).to(DEV).train()
    twin = make_module(32, half).to(DEV).train()
    with torch.no_grad():
        want = torch.relu(today(twin, x))                 # (also loads today's kernels before the capture)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph):
                inside = functional.ibn_plan(x, half, True)
                y = mod.forward_act(x, relu=True)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
    assert not inside
    assert torch.equal(y, want), "captured layer: not today's result"


def test_fused_forward_backward_after_the_switch_moves():
    """a forward that took the launch, then the co-resident kernels switched off before its backward (cnsn_resident_enable(0)):
    a forward would now be declined, the backward of this one still runs (no other backward reads its record) and the gradients
    match"""
    was = functional.resident_allowed()
    try:
        shape, dtype, half = (8, 32, 12, 12), torch.float32, 16
        gen = torch.Generator().manual_seed(9)
        x64 = torch.randn(shape, generator=gen, dtype=torch.float64)
        gy64 = torch.randn(shape, generator=gen, dtype=torch.float64)
        mod, twin = make_module(32, half).to(DEV).train(), make_module(32, half).train()
        xg = x64.float().to(DEV).contiguous(memory_format=CL).requires_grad_()
        y = mod.forward_act(xg, relu=True)
        assert y.grad_fn is not None and type(y.grad_fn).__name__ == "IBNormBackward"
        functional.set_resident(False)
        assert not functional.ibn_plan(xg, half, True)           # (the forward is declined now ...)
        assert type(mod.forward_act(xg.detach(), relu=True).grad_fn).__name__ != "IBNormBackward"
        y.backward(gy64.float().to(DEV).contiguous(memory_format=CL))   # (... the backward of the launch that ran is not)
        torch.cuda.synchronize()
        mask = (y.detach() > 0).cpu()
        r64 = reference(twin, 32, half, x64.float().double(), None, gy64, mask, torch.float64, torch.device("cpu"))
        r32 = reference(make_module(32, half).train(), 32, half, x64.float(), None, gy64, mask, torch.float32, torch.device("cpu"))
        compare("dx", xg.grad, r64[1], r32[1], dtype)
        compare("bn_w", mod.BN.weight.grad, r64[2]["bn_w"], r32[2]["bn_w"], dtype, param=True)
        compare("in_w", mod.IN.weight.grad, r64[2]["in_w"], r32[2]["in_w"], dtype, param=True)
    finally:
        functional.set_resident(was)


@pytest.mark.parametrize("shape,half", [((16, 64, 28, 28), 32), ((16, 256, 14, 14), 256)], ids=["ibn", "in+addend"])
def test_bf16_autocast_fused_against_unfused(shape, half):
    """a bf16-autocast channels-last step of conv -> IBN layer + ReLU (the backbones' pattern): the single launch against the same
    step with CNSN_NHWC_FUSED=0 (today's layers, switched through cnsn_reload_env), by direction"""
    import os
    from cnsn_amd import _ffi
    torch.manual_seed(21)
    c = shape[1]
    x = torch.randn(shape[0], c, shape[2], shape[3], device=DEV).contiguous(memory_format=CL)
    skip = torch.randn(shape, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL) if half == c else None
    conv = nn.Conv2d(c, c, 1, bias=False).to(DEV).to(memory_format=CL)
    gy = torch.randn(shape, device=DEV).contiguous(memory_format=CL)

    def step():
        mod = make_module(c, half).to(DEV).train()
        conv.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = conv(x)
            y = mod.forward_act(h, skip, relu=True)
        (y.float() * gy).sum().backward()
        ins = mod if half == c else mod.IN
        grads = [conv.weight.grad, ins.weight.grad, ins.bias.grad] + ([mod.BN.weight.grad] if half < c else [])
        return type(y.grad_fn).__name__, y.detach().float(), [g.detach().clone() for g in grads]

    route_f, y_f, g_f = step()
    old = os.environ.get("CNSN_NHWC_FUSED")
    try:
        os.environ["CNSN_NHWC_FUSED"] = "0"
        _ffi.reload_env()
        route_p, y_p, g_p = step()
    finally:
        if old is None:
            os.environ.pop("CNSN_NHWC_FUSED", None)
        else:
            os.environ["CNSN_NHWC_FUSED"] = old
        _ffi.reload_env()
    assert route_f == "IBNormBackward" and route_p != "IBNormBackward"

    def cosd(u, v):
        return 1 - float(torch.nn.functional.cosine_similarity(u.double().flatten(), v.double().flatten(), dim=0))
    assert cosd(y_f, y_p) <= 1e-4
    for i, (a, b) in enumerate(zip(g_f, g_p)):
        assert cosd(a, b) <= 1e-3, f"gradient {i}: cosine distance {cosd(a, b):.2e}"


def test_running_buffers_in_bf16_and_a_host_counter_go_through_the_marshal():
    """functional.IBNorm called directly (no callers._fusable in front) with the BatchNorm2d's running buffers held in bf16 and
    its counter on the host: the one BatchNorm2d marshal (functional._Bn2dBuffers) hands the kernel float32 copies, writes the
    update back rounded, and counts on the host — y, dx and the four parameter gradients are bit-identical to the run with float32
    buffers and a device counter, the bf16 buffers are that run's rounded to bf16, both counters read 1."""
    n, c, h, w, half = 8, 32, 6, 6, 16
    gen = torch.Generator().manual_seed(21)
    x0 = (torch.randn(n, c, h, w, generator=gen) * 1.5).to(DEV, torch.bfloat16).contiguous(memory_format=CL)
    gy = torch.randn(n, c, h, w, generator=gen).to(DEV, torch.bfloat16).contiguous(memory_format=CL)
    assert functional.ibn_plan(x0, half, relu=True, has_addend=False, bn_training=True)
    start = [torch.rand(half, generator=gen) + 0.5, torch.randn(half, generator=gen),          # in_w, in_b
             torch.rand(c - half, generator=gen) + 0.5, torch.randn(c - half, generator=gen),  # bn_w, bn_b
             torch.randn(c - half, generator=gen) * 0.1, torch.rand(c - half, generator=gen) + 0.5]   # running mean / var
    start[4], start[5] = start[4].bfloat16().float(), start[5].bfloat16().float()             # (equal values in either dtype)

    def run(buf_dtype, counter_dev):
        params = [t.clone().to(DEV).requires_grad_() for t in start[:4]]
        rm, rv = start[4].to(DEV, buf_dtype), start[5].to(DEV, buf_dtype)
        nbt = torch.zeros((), dtype=torch.int64, device=counter_dev)
        x = x0.clone().requires_grad_()
        y = functional.IBNorm.apply(x, None, *params, rm, rv, half, True, 1e-5, True, 1e-5, 0.1, nbt)
        y.backward(gy)
        torch.cuda.synchronize()
        return [y.detach(), x.grad, *(p.grad for p in params)], rm, rv, nbt

    want, rm32, rv32, nbt32 = run(torch.float32, DEV)
    got, rm16, rv16, nbt16 = run(torch.bfloat16, "cpu")
    for name, u, v in zip(("y", "dx", "d_in_w", "d_in_b", "d_bn_w", "d_bn_b"), got, want):
        assert u.dtype == v.dtype and torch.equal(u, v), name
    assert rm16.dtype == rv16.dtype == torch.bfloat16
    assert torch.equal(rm16, rm32.bfloat16()) and torch.equal(rv16, rv32.bfloat16())
    assert not torch.equal(rm32, start[4].to(DEV)) and not torch.equal(rv32, start[5].to(DEV))   # (the launch did update them)
    assert int(nbt32) == 1 and int(nbt16) == 1 and not nbt16.is_cuda
