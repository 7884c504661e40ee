"""`callers.bn_act` — BatchNorm2d (+ add) + ReLU in one channels-last launch (functional.BatchNormAct, cnsn_forward_bn_act /
cnsn_backward_bn_act) — against torch's own nn.BatchNorm2d in float64, what the reference's backbones instantiate
(models/imagenet/resnet_cnsn.py:104-110, :257-259), the backward run through the DEVICE's ReLU mask.  Method and tolerances are
those of tests/test_gpu_ibn_nhwc.py::compare: fp32 `err <= max(1e-5*scale, 2*noise)` with `noise` = torch fp32 against torch
fp64 on the same values; 16-bit `err <= 1e-2 * max|ref|` against the fp32 reference (+ 1e-5 absolute on parameter gradients).
Compared: y, dx, d_addend, d_weight, d_bias, running_mean, running_var, num_batches_tracked, output dtype and strides.  Every
case asserts what `functional.bn_act_plan` answers, so a silent fall-back cannot pass for the kernel; every figure is printed
before it is asserted (`pytest -s` keeps the margins)."""
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import _ffi, functional  # noqa: E402
from cnsn_amd.callers import _sites, bn_act  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last


@pytest.fixture(autouse=True)
def wherever_the_kernels_apply():
    """CNSN_NHWC_FUSED=2: a class the AUTO rule leaves to torch stays under test (the plan then says yes wherever the kernels
    apply); the AUTO rule itself is test_auto_rule_declines_only_by_size's"""
    old = os.environ.get("CNSN_NHWC_FUSED")
    os.environ["CNSN_NHWC_FUSED"] = "2"
    _ffi.reload_env()
    yield
    if old is None:
        os.environ.pop("CNSN_NHWC_FUSED", None)
    else:
        os.environ["CNSN_NHWC_FUSED"] = old
    _ffi.reload_env()


def make_bn(c, momentum=0.1, seed=0, cls=nn.BatchNorm2d):
    g = torch.Generator().manual_seed(seed + 11)
    bn = cls(c, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(3)
    return bn


def reference(state, momentum, training, x, a, gy, mask, dtype, dev):
    """(pre-activation, dx, d-addend, d-weight, d-bias, state) of torch's nn.BatchNorm2d (+ the add) in `dtype` on `dev`, the
    backward run through `mask`"""
    c = x.shape[1]
    tbn = nn.BatchNorm2d(c, momentum=momentum)
    tbn.load_state_dict(state)
    tbn = tbn.to(dev, dtype).train(training)
    tbn.num_batches_tracked = tbn.num_batches_tracked.to(torch.int64)
    X = x.to(dev, dtype).detach().requires_grad_(gy is not None)
    A = a.to(dev, dtype).detach().requires_grad_(gy is not None) if a is not None else None
    pre = tbn(X)
    if A is not None:
        pre = pre + A
    if gy is None:
        return pre.detach(), None, None, None, None, tbn.state_dict()
    pre.backward(gy.to(dev, dtype) * (mask.to(dev, dtype) if mask is not None else 1))
    return pre.detach(), X.grad, (A.grad if A is not None else None), tbn.weight.grad, tbn.bias.grad, tbn.state_dict()


def compare(name, got, t64, t32, dtype, param=False):
    got, t64, t32 = got.detach().double(), t64.detach().double().to(got.device), t32.detach().double().to(got.device)
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
    return err, bound


def run_case(shape, dtype, relu=True, addend=False, training=True, momentum=0.1, special=False, seed=0, expect_fused=True,
             gen_dev="cpu", edit=None, out=None):
    """special: channel 0 is constant (variance 0), channel 1 has a mean 1 000 x its standard deviation.  gen_dev: where the
    inputs are drawn and the float64 reference runs (the full-size cases: the GPU, one case at a time).  edit(bn, x64, a64):
    changes the module's parameters and the drawn inputs in place before anything reads them (test_gpu_bn_act_geometry.py:
    channels with weight 0).  out: a dict that receives the device's tensors, the gradient it was given and the two references.
    Returns {tensor: (err, bound)} of everything compared."""
    n, c, h, w = shape
    gen = torch.Generator(device=gen_dev).manual_seed(seed)

    def draw(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64, device=gen_dev)
    x64 = draw(*shape) * 1.5 + draw(1, c, 1, 1)
    if special:
        x64[:, 0] = 3.0
        x64[:, 1] = 1000.0 + draw(n, h, w)
    a64 = draw(*shape) if addend else None
    gy64 = draw(*shape) if training else None
    bn = make_bn(c, momentum, seed).train(training)
    if edit is not None:
        with torch.no_grad():
            edit(bn, x64, a64)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    dbn = bn.to(DEV)
    xs, as_ = x64.to(dtype), (a64.to(dtype) if addend else None)                  # (the values the device sees)
    xg = xs.to(DEV).contiguous(memory_format=CL).requires_grad_(training)
    ag = as_.to(DEV).contiguous(memory_format=CL).requires_grad_(training) if addend else None
    print(f"\n  {shape} {dtype} relu={relu} addend={addend} training={training} plan={expect_fused}")
    assert functional.bn_act_plan(xg, relu, addend, training) == expect_fused
    with torch.set_grad_enabled(training):
        y = bn_act(dbn, xg, ag, relu=relu)
    assert y.dtype == dtype and y.is_contiguous(memory_format=CL) and y.shape == xg.shape
    if training:
        assert (type(y.grad_fn).__name__ == "BatchNormActBackward") == expect_fused
        y.backward(gy64.to(dtype).to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    mask = (y.detach() > 0) if relu else None
    ref_dev = DEV if gen_dev != "cpu" else torch.device("cpu")
    r64 = reference(state, momentum, training, xs.double(), as_.double() if addend else None, gy64, mask, torch.float64, ref_dev)
    r32 = reference(state, momentum, training, xs.float(), as_.float() if addend else None, gy64, mask, torch.float32, ref_dev)
    pre64, pre32 = r64[0], r32[0]
    if relu:
        pre64, pre32 = pre64.clamp_min(0), pre32.clamp_min(0)
    margins = {"y": compare("y", y, pre64, pre32, dtype)}
    if training:
        margins["dx"] = compare("dx", xg.grad, r64[1], r32[1], dtype)
        assert xg.grad.is_contiguous(memory_format=CL) and xg.grad.dtype == dtype
        if addend:
            margins["d_addend"] = compare("d_addend", ag.grad, r64[2], r32[2], dtype)
        margins["d_weight"] = compare("d_weight", dbn.weight.grad, r64[3], r32[3], dtype, param=True)
        margins["d_bias"] = compare("d_bias", dbn.bias.grad, r64[4], r32[4], dtype, param=True)
    st = dbn.state_dict()
    if out is not None:
        out.update(y=y.detach(), dx=xg.grad, d_addend=ag.grad if addend else None, d_weight=dbn.weight.grad, d_bias=dbn.bias.grad,
                   running_mean=st["running_mean"], running_var=st["running_var"], gy=gy64.to(dtype) if training else None,
                   ref64=r64, ref32=r32)
    assert int(st["num_batches_tracked"]) == int(r64[5]["num_batches_tracked"]) == (4 if training else 3)
    for k in ("running_mean", "running_var"):
        t64 = r64[5][k].double().cpu()
        err = float((st[k].double().cpu() - t64).abs().max())
        bound = (1e-5 if dtype == torch.float32 else 1e-2) * max(1.0, float(t64.abs().max()))
        print(f"    {k}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{k}: err {err:.3e}"
        margins[k] = (err, bound)
    return margins


# a row tail, several column blocks, N above 256 (which no other single launch takes).  The launch takes a training call with at
# least 8 tiles of 64 rows: (4,8,8,8) has 256 rows — four tiles — and stays with torch; the eval launch has no such floor
TOY = [(4, 8, 8, 8), (6, 16, 9, 11), (3, 520, 6, 5), (9, 2048, 7, 7), (300, 64, 5, 5)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "f16"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", TOY, ids=[str(s) for s in TOY])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "id"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_toy_matrix(shape, dtype, training, relu, addend):
    expect = not (training and shape == (4, 8, 8, 8))
    run_case(shape, dtype, relu=relu, addend=addend, training=training, seed=sum(shape) % 1000, expect_fused=expect)


def test_four_of_the_five_toy_shapes_are_taken():
    for dtype in DTYPES:
        taken = [functional.bn_act_plan(torch.empty(s, dtype=dtype, device=DEV).contiguous(memory_format=CL), True, False, True)
                 for s in TOY]
        assert taken == [False, True, True, True, True]


def test_momentum_none_cumulative_average():
    run_case((6, 16, 9, 11), torch.float32, momentum=None, seed=7)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_constant_channel_and_mean_1000_sigma(dtype, addend):
    """channel 0 constant (variance 0: rstd = 1/sqrt(eps)), channel 1 with mean = 1 000 sigma: the sums are taken about a
    shift k read from the tensor (the median of three of its rows), so sum (x - k)^2 - (sum (x - k))^2 / R does not cancel.
    Observed on the MI355X with k = the first row, fp32, y:
    err 9.0e-06 against a bound of 6.3e-05 (twice the 2.1e-05 of torch's own fp32 BatchNorm2d against float64)."""
    m = run_case((32, 16, 12, 12), dtype, relu=True, addend=addend, special=True, seed=5)
    print(f"  margin of y: err {m['y'][0]:.3e} against {m['y'][1]:.3e}")


# the shapes the backbone runs at bs 256, config 4's batch at two of them, the plain tail with its addend
SITES = [(256, 64, 112, 112), (256, 64, 56, 56), (256, 128, 56, 56), (256, 128, 28, 28), (256, 256, 28, 28), (256, 256, 14, 14),
         (256, 512, 14, 14), (256, 512, 7, 7), (96, 64, 56, 56), (96, 512, 7, 7)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SITES, ids=[str(s) for s in SITES])
def test_full_size_sites(shape, dtype):
    run_case(shape, dtype, relu=True, training=True, seed=shape[1] + shape[2], gen_dev="cuda")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(256, 256, 56, 56), (256, 2048, 7, 7)], ids=str)
def test_full_size_plain_tail(shape):
    run_case(shape, torch.bfloat16, relu=True, addend=True, training=True, seed=shape[1], gen_dev="cuda")
    torch.cuda.empty_cache()


def test_auto_rule_declines_only_by_size():
    """the AUTO rule (CNSN_NHWC_FUSED unset or 1) is a pure function of the call — a size bound; whatever it declines, mode 2
    takes (the fixture), and the backward of a forward that ran is never declined"""
    import ctypes as C
    lib = cnsn_amd.lib()
    os.environ["CNSN_NHWC_FUSED"] = "1"
    _ffi.reload_env()
    answers = []
    for shape in SITES:
        x = torch.empty(shape, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=CL)
        d = functional._bn_act_desc(x, True, False)
        answers.append((x.numel() * 2, lib.cnsn_bn_act_plan(C.byref(d), 0, 0)))
        assert lib.cnsn_bn_act_plan(C.byref(d), 0, 1) == 1
    answers.sort()
    took = [t for _, t in answers]
    assert took == sorted(took), f"not a size bound: {answers}"
    assert took[-1] == 1, "the largest site is declined"


class SubBn(nn.BatchNorm2d):
    pass


def plain(bn, x, a, relu):
    y = bn(x) if a is None else bn(x) + a
    return torch.relu(y) if relu else y


def step_pair(make, x, a, relu=True, training=True):
    """forward + backward through bn_act and through the plain statements, from equal modules"""
    out = []
    for fn in (bn_act, plain):
        bn = make().to(DEV).train(training)
        xg = x.clone().requires_grad_()
        ag = a.clone().requires_grad_() if a is not None else None
        y = fn(bn, xg, ag, relu)
        y.backward(torch.ones_like(y) * 0.5)
        out.append((type(y.grad_fn).__name__, [y.detach(), xg.grad, bn.weight.grad, bn.bias.grad] + ([ag.grad] if a is not None else [])
                    + [v.clone() for v in bn.state_dict().values()]))
    return out


@pytest.mark.parametrize("case", ["switch", "degraded", "resident_off", "nhwc_fused_0", "subclass", "sync_bn", "nchw", "no_affine",
                                  "no_running_stats", "eval_with_grad", "c_not_vec"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_fallbacks_are_the_plain_statements(case, addend, monkeypatch):
    torch.manual_seed(3)
    c = 10 if case == "c_not_vec" else 32                                         # (10 floats: no whole number of 16-byte vectors)
    fmt = torch.contiguous_format if case == "nchw" else CL
    x = torch.randn(16, c, 10, 10, device=DEV).contiguous(memory_format=fmt)
    a = torch.randn(16, c, 10, 10, device=DEV).contiguous(memory_format=fmt) if addend else None
    make, training = (lambda: make_bn(c)), case != "eval_with_grad"
    assert functional.bn_act_plan(x, True, addend, training) == (case not in ("nchw", "c_not_vec"))
    was = functional.resident_allowed()
    try:
        if case == "switch":
            monkeypatch.setattr(_sites, "FUSE_BN_ACT", False)
        elif case == "degraded":
            monkeypatch.setattr(_ffi.lib(), "cnsn_resident_degraded", lambda: 1)
            assert not functional.bn_act_plan(x, True, addend, True)
        elif case == "resident_off":
            functional.set_resident(False)
            assert not functional.bn_act_plan(x, True, addend, True)
        elif case == "nhwc_fused_0":
            os.environ["CNSN_NHWC_FUSED"] = "0"
            _ffi.reload_env()
            assert not functional.bn_act_plan(x, True, addend, True)
        elif case == "subclass":
            make = lambda: make_bn(c, cls=SubBn)                                   # noqa: E731
        elif case == "sync_bn":
            make = lambda: make_bn(c, cls=nn.SyncBatchNorm)                        # noqa: E731  (one process: BatchNorm2d's arithmetic)
        elif case == "no_affine":
            make = lambda: nn.BatchNorm2d(c, affine=False)                         # noqa: E731
        elif case == "no_running_stats":
            make = lambda: nn.BatchNorm2d(c, track_running_stats=False)            # noqa: E731
        (name_f, got), (_, want) = step_pair(make, x, a, training=training) if case not in ("no_affine",) else (
            step_pair_no_affine(make, x, a))
        assert name_f != "BatchNormActBackward"
        for u, v in zip(got, want):
            assert (u is None and v is None) or torch.equal(u, v)
    finally:
        functional.set_resident(was)


def step_pair_no_affine(make, x, a):
    out = []
    for fn in (bn_act, plain):
        bn = make().to(DEV).train()
        xg = x.clone().requires_grad_()
        y = fn(bn, xg, a, True)
        y.backward(torch.ones_like(y) * 0.5)
        out.append((type(y.grad_fn).__name__, [y.detach(), xg.grad] + [v.clone() for v in bn.state_dict().values()]))
    return out


def test_the_healthy_call_is_taken_and_differs_from_nothing_else():
    """the counterpart of the fall-back cases: the same tensors with everything healthy DO take the launch"""
    torch.manual_seed(3)
    x = torch.randn(16, 32, 10, 10, device=DEV).contiguous(memory_format=CL)
    (name_f, got), (name_p, want) = step_pair(lambda: make_bn(32), x, None)
    assert name_f == "BatchNormActBackward" and name_p != name_f
    assert float((got[0] - want[0]).abs().max()) <= 1e-5 * max(1.0, float(want[0].abs().max()))


def test_parameters_in_another_dtype_and_autocast():
    """a module kept in bf16 (`.to(torch.bfloat16)`): float32 copies go in, the buffers are written back, the gradients come back
    in the parameters' dtype; under autocast the activations are bf16 and the parameters fp32"""
    torch.manual_seed(8)
    x = torch.randn(16, 32, 10, 10, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    bn, twin = make_bn(32).to(DEV).to(torch.bfloat16).train(), make_bn(32).to(DEV).to(torch.bfloat16).train()
    xg, xw = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, want = bn_act(bn, xg), torch.relu(twin(xw))
    assert type(y.grad_fn).__name__ == "BatchNormActBackward" and y.dtype == torch.bfloat16
    y.float().sum().backward()
    want.float().sum().backward()
    assert bn.weight.grad.dtype == torch.bfloat16 and bn.running_mean.dtype == torch.bfloat16
    assert float((y.float() - want.float()).abs().max()) <= 1e-2 * float(want.float().abs().max())
    assert float((bn.running_var.float() - twin.running_var.float()).abs().max()) <= 1e-2 * float(twin.running_var.float().abs().max())
    assert float((bn.bias.grad.float() - twin.bias.grad.float()).abs().max()) <= 1e-2 * float(twin.bias.grad.float().abs().max()) + 1e-5
    conv = nn.Conv2d(32, 32, 1, bias=False).to(DEV).to(memory_format=CL)
    bn32 = make_bn(32).to(DEV).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = bn_act(bn32, conv(x.float()))
    assert out.dtype == torch.bfloat16 and type(out.grad_fn).__name__ == "BatchNormActBackward"
    out.float().sum().backward()
    assert bn32.weight.grad.dtype == torch.float32 and conv.weight.grad is not None


def test_resnet50_step_with_the_switch_on_and_off():
    """ResNet50CNSN in channels-last, fp32, one training step with the switch on against the same weights with the switch off
    (torch's nn.BatchNorm2d + ReLU) — two arithmetically equivalent paths, bounds those of
    tests/test_gpu_nhwc.py::test_resnet50_in_channels_last_matches_the_nchw_model"""
    from cnsn_amd.callers import ResNet50CNSN
    torch.manual_seed(0)
    net_on = ResNet50CNSN(num_classes=10).to(DEV).to(memory_format=CL).train()
    net_off = ResNet50CNSN(num_classes=10).to(DEV).to(memory_format=CL).train()
    net_off.load_state_dict(net_on.state_dict())
    x = torch.randn(8, 3, 64, 64, device=DEV).contiguous(memory_format=CL)
    was = _sites.FUSE_BN_ACT
    try:
        _sites.FUSE_BN_ACT = True
        assert functional.bn_act_plan(torch.empty(8, 64, 32, 32, device=DEV).contiguous(memory_format=CL))
        y_on = net_on(x)
        y_on.square().mean().backward()
        _sites.FUSE_BN_ACT = False
        y_off = net_off(x)
        y_off.square().mean().backward()
    finally:
        _sites.FUSE_BN_ACT = was
    torch.cuda.synchronize()
    scale = max(1.0, float(y_off.abs().max()))
    err = float((y_on - y_off).abs().max())
    print(f"\n  logits: err {err:.3e} bound {3e-3 * scale:.3e}")
    assert err <= 3e-3 * scale

    def cos(u, v):
        return float(torch.nn.functional.cosine_similarity(u.double().flatten(), v.double().flatten(), dim=0))
    for name in ("conv1.weight", "fc.weight", "layer2.1.cnsn.selfnorm.g_fc.weight"):
        u, v = net_on.get_parameter(name).grad, net_off.get_parameter(name).grad
        print(f"  {name}: cosine {cos(u, v):.6f}")
        assert cos(u, v) >= 0.99, name
    for name in ("bn1", "layer3.2.bn2"):
        a, b = net_on.get_submodule(name), net_off.get_submodule(name)
        assert type(a) is nn.BatchNorm2d
        err_m = float((a.running_mean - b.running_mean).abs().max())
        err_v = float((a.running_var - b.running_var).abs().max())
        print(f"  {name}: running_mean err {err_m:.3e} running_var err {err_v:.3e}")
        assert err_m <= 1e-3 and err_v <= 1e-3 * max(1.0, float(b.running_var.abs().max()))
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1


def test_graph_capture_replays_the_eager_result():
    """one captured and replayed forward + backward of bn_act gives the eager result (under capture the barrier block lies in the
    call's workspace, the persistent context is not used)"""
    torch.manual_seed(4)
    x = torch.randn(16, 32, 12, 12, device=DEV).contiguous(memory_format=CL)
    a = torch.randn(16, 32, 12, 12, device=DEV).contiguous(memory_format=CL)
    gy = torch.randn(16, 32, 12, 12, device=DEV).contiguous(memory_format=CL)
    eager_bn, graph_bn = make_bn(32).to(DEV).train(), make_bn(32).to(DEV).train()
    xe, ae = x.clone().requires_grad_(), a.clone().requires_grad_()
    ye = bn_act(eager_bn, xe, ae)
    ye.backward(gy)
    torch.cuda.synchronize()
    xs, as_ = x.clone().requires_grad_(), a.clone().requires_grad_()
    state = {k: v.clone() for k, v in graph_bn.state_dict().items()}
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            inside = functional.bn_act_plan(xs, True, True, True)
            yg = bn_act(graph_bn, xs, as_)
            name = type(yg.grad_fn).__name__
            gx, ga, gw, gb = torch.autograd.grad(yg, (xs, as_, graph_bn.weight, graph_bn.bias), gy)
    torch.cuda.current_stream().wait_stream(side)
    graph_bn.load_state_dict(state)                # (whatever the capture itself did to the buffers)
    graph.replay()
    torch.cuda.synchronize()
    assert inside and name == "BatchNormActBackward"
    assert torch.equal(yg, ye.detach()) and torch.equal(gx, xe.grad) and torch.equal(ga, ae.grad)
    assert torch.equal(gw, eager_bn.weight.grad) and torch.equal(gb, eager_bn.bias.grad)
    assert torch.equal(graph_bn.running_mean, eager_bn.running_mean) and torch.equal(graph_bn.running_var, eager_bn.running_var)
    assert int(graph_bn.num_batches_tracked) == int(eager_bn.num_batches_tracked) == 4
