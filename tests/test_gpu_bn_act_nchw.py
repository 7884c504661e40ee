"""`callers.bn_act` on dense NCHW tensors — BatchNorm2d (+ add) + ReLU in two plain launches per direction
(functional.BatchNormActNCHW, cnsn_forward_bn_act_nchw / cnsn_backward_bn_act_nchw) — against torch's own nn.BatchNorm2d in
float64, the backward run through the DEVICE's ReLU mask.  Method and tolerances are those of tests/test_gpu_bn_act.py
(`compare`, `reference`, `make_bn`, imported): fp32 `err <= max(1e-5*scale, 2*noise)` with `noise` = torch fp32 against torch
fp64 on the same values; 16-bit `err <= 1e-2 * max|ref|` against the fp32 reference (+ 1e-5 absolute on parameter gradients);
running buffers and num_batches_tracked as there.  The references see the values the device sees: x, the addend and grad_y
rounded to the tensor's type.  Every case switches `_sites.FUSE_BN_ACT_NCHW` on through a fixture that
restores it, asserts the plan's answer, the grad_fn's name and the geometry class the shape landed in
(cnsn_bn_act_nchw_geometry), and prints every figure before it asserts (`pytest -s` keeps the margins)."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import functional  # noqa: E402
from cnsn_amd.callers import _sites, bn_act  # noqa: E402
from tests.test_gpu_bn_act import compare, make_bn, reference  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last
NAME = "BatchNormActNCHWBackward"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


@pytest.fixture(autouse=True)
def nchw_route_on():
    was = _sites.FUSE_BN_ACT_NCHW
    _sites.FUSE_BN_ACT_NCHW = True
    yield
    _sites.FUSE_BN_ACT_NCHW = was


def geometry_class(x, training=True):
    """(class, tiles per channel): `instances` — several instances per tile, the plane whole; `ranges` — several tiles per
    plane; `plane` — a tile is one whole plane.  `+ragged`: the last instance group is shorter; `+wide`: more tiles per channel
    than the 256 threads of a workgroup add in one step"""
    tiles, ipt, epr, threads = functional.bn_act_nchw_geometry(x, training)
    n, _, h, w = x.shape
    assert threads == 256 and tiles == -(-n // ipt) * -(-(h * w) // epr)
    name = "ranges" if epr < h * w else ("instances" if ipt > 1 else "plane")
    if ipt > 1 and n % ipt:
        name += "+ragged"
    if tiles > threads:
        name += "+wide"
    return name, tiles


def run_case(shape, dtype, cls, relu=True, addend=False, training=True, momentum=0.1, special=False, seed=0, edit=None, out=None):
    """special: channel 0 is constant, channel 1 has a mean of 1 000 standard deviations.  edit(bn, x64): changes the module and
    the inputs before anything reads them.  Both references run on the CPU, once per case: torch's fp32 BatchNorm2d backward on
    the GPU is itself 1 % off at planes of odd size — observed on the MI355X at (3, 4, 225, 223), d_weight against float64:
    torch fp32 on the GPU 4.3e+00 of 4.3e+02, torch fp32 on the CPU 4.4e-04, these launches 1.4e-05 — and the 16-bit bound is
    taken against the fp32 reference."""
    n, c, h, w = shape
    ref_dev = torch.device("cpu")
    gen = torch.Generator().manual_seed(seed)

    def draw(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)
    x64 = draw(*shape) * 1.5 + draw(1, c, 1, 1)
    if special:
        x64[:, 0] = 3.0
        x64[:, 1] = 1000.0 + draw(n, h, w)
    a64 = draw(*shape) if addend else None
    gy64 = draw(*shape).to(dtype).double() if training else None                  # (x, addend, grad_y: the values the device sees)
    bn = make_bn(c, momentum, seed).train(training)
    if edit is not None:
        with torch.no_grad():
            edit(bn, x64)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    dbn = bn.to(DEV)
    xs, as_ = x64.to(dtype), (a64.to(dtype) if addend else None)                  # (the values the device sees)
    xg = xs.to(DEV).requires_grad_(training)
    ag = as_.to(DEV).requires_grad_(training) if addend else None
    got_cls, tiles = geometry_class(xg, training)
    print(f"\n  {shape} {dtype} relu={relu} addend={addend} training={training}: {got_cls}, {tiles} tiles per channel")
    assert got_cls == cls
    assert functional.bn_act_nchw_plan(xg, relu, addend, training) and not functional.bn_act_plan(xg, relu, addend, training)
    with torch.set_grad_enabled(training):
        y = bn_act(dbn, xg, ag, relu=relu)
    assert y.dtype == dtype and y.is_contiguous() and y.shape == xg.shape
    if training:
        assert type(y.grad_fn).__name__ == NAME
        y.backward(gy64.to(dtype).to(DEV))
    else:
        assert y.grad_fn is None
    torch.cuda.synchronize()
    mask = (y.detach() > 0) if relu else None
    r64 = reference(state, momentum, training, xs.double(), as_.double() if addend else None, gy64, mask, torch.float64, ref_dev)
    r32 = reference(state, momentum, training, xs.float(), as_.float() if addend else None, gy64, mask, torch.float32, ref_dev)
    pre64, pre32 = r64[0], r32[0]
    if relu:
        pre64, pre32 = pre64.clamp_min(0), pre32.clamp_min(0)
    compare("y", y, pre64, pre32, dtype)
    if training:
        compare("dx", xg.grad, r64[1], r32[1], dtype)
        assert xg.grad.is_contiguous() and xg.grad.dtype == dtype
        if addend:
            compare("d_addend", ag.grad, r64[2], r32[2], dtype)
        compare("d_weight", dbn.weight.grad, r64[3], r32[3], dtype, param=True)
        compare("d_bias", dbn.bias.grad, r64[4], r32[4], dtype, param=True)
    st = dbn.state_dict()
    if out is not None:
        out.update(y=y.detach(), dx=xg.grad, d_addend=ag.grad if addend else None, d_weight=dbn.weight.grad, d_bias=dbn.bias.grad,
                   gy=gy64.to(dtype).to(DEV) if training else None)
    assert int(st["num_batches_tracked"]) == int(r64[5]["num_batches_tracked"]) == (4 if training else 3)
    for k in ("running_mean", "running_var"):
        t64 = r64[5][k].double().cpu()
        err = float((st[k].double().cpu() - t64).abs().max())
        bound = (1e-5 if dtype == torch.float32 else 1e-2) * max(1.0, float(t64.abs().max()))
        print(f"    {k}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{k}: err {err:.3e}"


# the smallest shapes of every geometry class (tests/test_bn_act_nchw_layout.py checks the same classes without a GPU):
#   odd everything, planes that start off a 16-byte boundary    a plane of 49 16-bit values: 98 bytes, one tile / a ragged last tile
#   many instances per tile, several tiles                      a tile is one whole plane of 33 x 37 (4 884 bytes)
#   one element per plane                                       several tiles per plane, in 16 and in 32 bits
SMALL = [((5, 3, 9, 11), F32, "instances"), ((37, 6, 7, 7), BF16, "instances"), ((137, 6, 7, 7), BF16, "instances+ragged"),
         ((128, 8, 8, 8), F32, "instances"), ((4, 3, 33, 37), F32, "plane"), ((2, 16, 1, 1), F32, "instances"),
         ((16, 8, 64, 64), F16, "ranges"), ((137, 6, 7, 7), F16, "instances+ragged"), ((5, 3, 9, 11), BF16, "instances"),
         ((3, 2, 50, 53), F32, "ranges"), ((3, 2, 75, 77), BF16, "ranges")]


def ids(cases):
    return [f"{s}-{str(d)[6:]}" for s, d, _ in cases]


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "id"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_small_matrix(case, training, relu, addend):
    shape, dtype, cls = case
    run_case(shape, dtype, cls, relu=relu, addend=addend, training=training, seed=sum(shape) % 1000)


# several tiles per plane at full plane sizes; (8, 2, 256, 256): 512 tiles per channel, two per thread of the reducing workgroup
LARGE = [((3, 4, 224, 224), F32, "ranges"), ((8, 4, 256, 256), BF16, "ranges"), ((8, 2, 256, 256), F32, "ranges+wide"),
         ((3, 4, 225, 223), F16, "ranges")]


@pytest.mark.parametrize("case", LARGE, ids=ids(LARGE))
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_large_planes(case, addend):
    shape, dtype, cls = case
    run_case(shape, dtype, cls, relu=True, addend=addend, seed=shape[2])


def test_momentum_none_cumulative_average():
    run_case((5, 3, 9, 11), F32, "instances", momentum=None, seed=7)
    run_case((128, 8, 8, 8), F32, "instances", momentum=None, seed=8)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
def test_constant_channel_and_mean_1000_sigma(dtype, addend):
    """channel 0 constant (variance 0: rstd = 1/sqrt(eps)), channel 1 with mean = 1 000 sigma: the sums are taken about the
    channel's first element, so sum (x - s)^2 - (sum (x - s))^2 / R does not cancel"""
    run_case((32, 16, 12, 12), dtype, "instances+ragged", relu=True, addend=addend, special=True, seed=5)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_channel_with_weight_zero(dtype):
    """a channel whose weight is 0: its output is the bias, dx is 0, and the ReLU mask is the sign of the bias (+ addend)"""
    def edit(bn, x64):
        bn.weight[1] = 0.0
        bn.weight[2] = 0.0
        bn.bias[2] = -0.25
    run_case((16, 4, 10, 10), dtype, "instances", relu=True, addend=False, seed=9, edit=edit)
    run_case((16, 4, 10, 10), dtype, "instances", relu=True, addend=True, seed=9, edit=edit)


@pytest.mark.parametrize("case", [((137, 6, 7, 7), BF16, "instances+ragged"), ((3, 2, 50, 53), F32, "ranges")], ids=["small", "ranges"])
def test_d_addend_is_the_masked_gradient_exactly_and_two_calls_are_bit_identical(case):
    shape, dtype, cls = case
    a, b = {}, {}
    run_case(shape, dtype, cls, relu=True, addend=True, seed=3, out=a)
    run_case(shape, dtype, cls, relu=True, addend=True, seed=3, out=b)
    assert torch.equal(a["d_addend"], a["gy"] * (a["y"] > 0))
    for k in ("y", "dx", "d_addend", "d_weight", "d_bias"):
        assert torch.equal(a[k], b[k]), k


def route(x, a=None, c=None):
    bn = make_bn(c or x.shape[1]).to(DEV).train()
    y = bn_act(bn, x.requires_grad_(), a)
    return y


def test_other_layouts_are_not_taken_by_the_nchw_route():
    torch.manual_seed(2)
    x = torch.randn(16, 32, 10, 10, device=DEV)
    assert type(route(x.clone()).grad_fn).__name__ == NAME
    cl = x.clone().contiguous(memory_format=CL)
    assert not functional.bn_act_nchw_plan(cl)
    assert type(route(cl).grad_fn).__name__ != NAME                               # (the channels-last route or torch)
    wide = torch.randn(16, 32, 10, 20, device=DEV)[:, :, :, ::2]
    assert not wide.is_contiguous() and not functional.bn_act_nchw_plan(wide)
    y = route(wide.detach())
    assert type(y.grad_fn).__name__ not in (NAME, "BatchNormActBackward")
    part = torch.randn(16, 64, 10, 10, device=DEV)[:, 8:40]                       # a channel slice: dense planes, wrong strides
    assert type(route(part.detach()).grad_fn).__name__ not in (NAME, "BatchNormActBackward")
    # a float64 tensor and a module the route leaves alone
    assert type(bn_act(nn.BatchNorm2d(32).to(DEV).double(), x.double().requires_grad_()).grad_fn).__name__ != NAME
    assert type(bn_act(nn.BatchNorm2d(32, affine=False).to(DEV), x.clone().requires_grad_()).grad_fn).__name__ != NAME


def test_switch_off_keeps_torch_nodes():
    _sites.FUSE_BN_ACT_NCHW = False                                               # (the fixture restores it)
    torch.manual_seed(2)
    x = torch.randn(16, 32, 10, 10, device=DEV)
    y = route(x)
    names = [type(y.grad_fn).__name__, type(y.grad_fn.next_functions[0][0]).__name__]
    print(f"\n  switch off: {names}")
    assert names[0].startswith("ReluBackward") and "BatchNormBackward" in names[1]
    twin = make_bn(32).to(DEV).train()
    assert torch.equal(y, torch.relu(twin(x.detach())))


def test_eval_with_a_gradient_keeps_torch():
    x = torch.randn(4, 8, 6, 6, device=DEV, requires_grad=True)
    bn = make_bn(8).to(DEV).eval()
    assert type(bn_act(bn, x).grad_fn).__name__ != NAME
    with torch.no_grad():
        twin = torch.relu(make_bn(8).to(DEV).eval()(x))
        y = bn_act(bn, x)
    err = float((y - twin).abs().max())
    print(f"\n  eval launch against torch: err {err:.3e}")
    assert err <= 1e-5 * max(1.0, float(twin.abs().max()))


def test_unaligned_base_pointer_is_copied_not_refused():
    """a dense view that starts off a 16-byte boundary: the Function copies it once (functional._dense), the entry point itself
    answers CNSN_E_UNSUPPORTED for such a pointer"""
    flat = torch.randn(4 * 6 * 5 * 5 + 1, device=DEV)
    x = flat[1:].view(4, 6, 5, 5)
    assert x.data_ptr() % 16 and x.is_contiguous()
    lib = cnsn_amd.lib()
    d = functional._bn_act_desc(x, True, False)
    bn = make_bn(6).to(DEV)
    d.bn.weight, d.bn.bias, d.bn.running_mean, d.bn.running_var = (t.data_ptr() for t in (bn.weight, bn.bias, bn.running_mean,
                                                                                          bn.running_var))
    ws = torch.empty(1 << 16, device=DEV)
    y = torch.empty(4, 6, 5, 5, device=DEV)
    st = lib.cnsn_forward_bn_act_nchw(C.byref(d), x.data_ptr(), None, y.data_ptr(), None, ws.data_ptr(), ws.numel() * 4, None)
    assert st == -9
    out = bn_act(bn.train(), x.detach().requires_grad_())
    assert type(out.grad_fn).__name__ == NAME
    want = torch.relu(make_bn(6).to(DEV).train()(x))
    assert float((out - want).detach().abs().max()) <= 1e-5 * max(1.0, float(want.detach().abs().max()))


def test_graph_capture_replays_on_fresh_values():
    """forward + backward of one layer recorded with torch.cuda.graph on one stream — a linear chain of four plain launches —
    and replayed on fresh input values: the eager call's results"""
    torch.manual_seed(4)
    shape = (16, 32, 12, 12)
    first = [torch.randn(shape, device=DEV) for _ in range(3)]
    fresh = [torch.randn(shape, device=DEV) * 2 + 1 for _ in range(3)]
    warm = make_bn(32).to(DEV).train()                                            # (the library's first launches: not under capture)
    bn_act(warm, first[0].clone().requires_grad_(), first[1]).backward(first[2])
    torch.cuda.synchronize()
    graph_bn = make_bn(32).to(DEV).train()
    state = {k: v.clone() for k, v in graph_bn.state_dict().items()}
    xs, as_, gs = first[0].clone().requires_grad_(), first[1].clone().requires_grad_(), first[2].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inside = functional.bn_act_nchw_plan(xs, True, True, True)
        yg = bn_act(graph_bn, xs, as_)
        name = type(yg.grad_fn).__name__
        gx, ga, gw, gb = torch.autograd.grad(yg, (xs, as_, graph_bn.weight, graph_bn.bias), gs)
    assert inside and name == NAME
    graph_bn.load_state_dict(state)                # (whatever the capture itself did to the buffers)
    with torch.no_grad():
        xs.copy_(fresh[0]), as_.copy_(fresh[1]), gs.copy_(fresh[2])
    graph.replay()
    torch.cuda.synchronize()
    eager_bn = make_bn(32).to(DEV).train()
    xe, ae = fresh[0].clone().requires_grad_(), fresh[1].clone().requires_grad_()
    ye = bn_act(eager_bn, xe, ae)
    ye.backward(fresh[2])
    torch.cuda.synchronize()
    for nm, got, want in (("y", yg, ye), ("dx", gx, xe.grad), ("d_addend", ga, ae.grad), ("d_weight", gw, eager_bn.weight.grad),
                          ("d_bias", gb, eager_bn.bias.grad), ("running_mean", graph_bn.running_mean, eager_bn.running_mean),
                          ("running_var", graph_bn.running_var, eager_bn.running_var)):
        compare(nm, got, want, want, F32)
    assert int(graph_bn.num_batches_tracked) == int(eager_bn.num_batches_tracked) == 4


def test_small_wideresnet_switch_on_against_off():
    """WideResNet-10-1 with SelfNorm units, bs 8, 32x32, fp32: one training step with the switch on against the same weights with
    the switch off — the reference — within max(1e-5*scale, 2*noise), `noise` = the switch-off run against a float64 copy of the
    model (torch's own units, oracle/): logits and every parameter gradient"""
    from cnsn_amd.callers import WideResNetCNSN
    from oracle import cnsn_oracle as orc
    torch.manual_seed(0)
    kw = dict(depth=10, num_classes=10, widen_factor=1, cnsn_type="sn")
    net_on = WideResNetCNSN(**kw).to(DEV).train()
    with torch.no_grad():
        for m in net_on.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2)
    net_off = copy.deepcopy(net_on)
    net_64 = WideResNetCNSN(impl=orc, **kw)
    net_64.load_state_dict(net_on.state_dict())
    net_64 = net_64.to(DEV).double().train()
    x = torch.randn(8, 3, 32, 32, device=DEV)

    def step(net, xin):
        out = net(xin)
        seen, todo, ours = set(), [out.grad_fn], 0
        while todo:                                                               # the autograd nodes of this library's NCHW launches
            fn = todo.pop()
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            ours += type(fn).__name__ == NAME
            todo.extend(f for f, _ in fn.next_functions)
        out.square().mean().backward()
        return out.detach(), ours
    y_on, nodes_on = step(net_on, x)
    _sites.FUSE_BN_ACT_NCHW = False                                               # (the fixture restores it)
    y_off, nodes_off = step(net_off, x)
    y_64, _ = step(net_64, x.double())
    torch.cuda.synchronize()
    print(f"\n  {NAME} nodes: {nodes_on} with the switch on, {nodes_off} with it off")
    assert nodes_on >= 3 and nodes_off == 0                                       # (bn2 of each of the three blocks at least)
    worst = 0.0
    for m_on, m_off in zip(net_on.modules(), net_off.modules()):
        if isinstance(m_on, nn.BatchNorm2d):
            assert int(m_on.num_batches_tracked) == int(m_off.num_batches_tracked) == 1
            worst = max(worst, float(((m_on.running_var - m_off.running_var).abs() / m_off.running_var.abs().clamp_min(1.0)).max()))
    print(f"  running_var of the BatchNorm2d modules: worst difference {worst:.3e} (relative above 1)")
    assert worst <= 1e-5

    def check(name, got, ref32, ref64):
        scale = max(1.0, float(ref32.abs().max()))
        noise = float((ref32.double() - ref64).abs().max())
        err = float((got - ref32).abs().max())
        bound = max(1e-5 * scale, 2 * noise)
        print(f"    {name}: err {err:.3e} bound {bound:.3e} (noise {noise:.3e}, scale {scale:.3g})")
        return err <= bound, name
    results = [check("logits", y_on, y_off, y_64)]
    p64 = dict(net_64.named_parameters())
    for (name, p_on), (_, p_off) in zip(net_on.named_parameters(), net_off.named_parameters()):
        results.append(check(name, p_on.grad, p_off.grad, p64[name].grad))
    assert all(ok for ok, _ in results), [n for ok, n in results if not ok]
