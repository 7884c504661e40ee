"""The block's last BatchNorm2d inside the SelfNorm launch with the identity BEHIND the op, or without one:
`CNSN.forward_bn_block(conv_out, bn, identity, relu, add_mode="post")` =
    out = self.bn3(out); out = self.cnsn(out); out += identity; out = self.relu(out)     (models/imagenet/resnet_cnsn.py:108-122,
pos='residual') and `add_mode="none"` = `self.cnsn(self.bn3(out))` in front of the IBN-b block's InstanceNorm2d
(resnet_ibn_cnsn.py:109-127), ONE launch per direction on channels-last tensors (cnsn_forward_bn_block / cnsn_backward_bn_block
with a POST / NONE epilogue, csrc/cnsn_nhwc_bnhead_kernels.h).

Truth: torch's BatchNorm2d + the oracle's SelfNorm composed on the CPU in float64 (fp32 for its noise), bn3's output rounded to
the activation dtype where the block stores it, the backward through the device's ReLU mask.  Bars, helpers and inputs are
those of tests/test_gpu_bn_block.py (`compare`, `make_bn`), tests/test_gpu_parity.py (`cond_input`) and
tests/golden/gen_golden_fill.py (`fill_sn`).  The seeds follow test_gpu_bn_block.py's rule; at every one of them, for every
shape and dtype below, the fp32 oracle's mask of the POST pre-activation is the float64 one's at every element (checked on the
CPU before they were fixed: 0 differences), inside compare()'s 1e-4 / 5e-3."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import functional as F_  # noqa: E402
from oracle import cnsn_oracle as orc  # noqa: E402
from tests.golden.gen_golden_fill import fill_sn  # noqa: E402
from tests.test_gpu_bn_block import compare, make_bn  # noqa: E402
from tests.test_gpu_nhwc_full_size import healthy, knobs, launches  # noqa: E402
from tests.test_gpu_nhwc_geometry import BIT16, FP32, check_geometry  # noqa: E402
from tests.test_gpu_parity import DEV, cond_input  # noqa: E402

CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SHAPES = [(12, 16, 9, 7), (37, 8, 14, 14), (5, 2048, 7, 7), (256, 8, 12, 12)]
TOO_FEW_TILES = [(6, 64, 7, 7), (3, 520, 6, 5)]
MODES = [("post", True), ("post", False), ("none", False)]
MODE_IDS = ["post+relu", "post", "none"]


def seed_of(shape, dtype):
    return (31 if dtype == F32 else 7) + shape[1]


@functools.lru_cache(maxsize=None)
def inputs(shape, dtype, seed):
    """conv_out, identity, grad_y on the CPU, quantised to `dtype` (shared by every test of a shape; never written to)"""
    conv = (cond_input(shape, seed) * 0.7).to(dtype)
    idt = (cond_input(shape, seed + 1) * 0.5).to(dtype)
    gy = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64).to(dtype)
    return conv, idt, gy


def oracle(conv, idt, gy, c, seed, mode, relu, mask, dtype):
    """{'t64', 'o32' (, 'o32u': 16-bit, the composition without the rounding of bn3's output)}: the pre-activation
    `sn(rnd(bn(c))) [+ identity]`, the gradients through `mask` and the layers' state, in the keys compare() reads"""
    out = {}
    models = [("t64", torch.float64, True), ("o32", F32, True)] + ([("o32u", F32, False)] if dtype != F32 else [])
    for tag, odt, rounded in models:
        def rnd(t):
            return t if not rounded or dtype == F32 else t + (t.detach().to(dtype).to(t.dtype) - t.detach())
        bn_t = make_bn(c, seed, odt, "cpu")
        sn_t = fill_sn(orc.SelfNorm(c), seed, F32).to(odt).train()
        ct, it = conv.to(odt, copy=True).requires_grad_(), idt.to(odt, copy=True).requires_grad_()     # (the shared inputs stay as they are)
        pre = sn_t(rnd(bn_t(ct)))
        if mode == "post":
            pre = pre + it
        (pre * mask.to(odt) if relu else pre).backward(gy.to(odt))
        out[tag] = dict(pre=pre.detach(), dc=ct.grad, di=it.grad if mode == "post" else torch.zeros_like(ct),
                        bn=[p.grad for p in bn_t.parameters()], sn=[p.grad for p in sn_t.parameters()],
                        bn_rm=bn_t.running_mean.clone(), bn_rv=bn_t.running_var.clone(), sn_rm=sn_t.g_bn.running_mean.clone(),
                        sn_rv=sn_t.g_bn.running_var.clone(), nbt=int(bn_t.num_batches_tracked),
                        sn_nbt=int(sn_t.g_bn.num_batches_tracked))
    return out


def call(m, bn, cg, ig, mode, relu, identity_bn=None):
    return m.forward_bn_block(cg, bn, ig if mode != "none" else None, relu=relu, identity_bn=identity_bn, add_mode=mode)


def device_forward(shape, dtype, mode, relu, fused, expect_plan=True):
    """the library's forward on the shared inputs; `fused` False: its un-fused sequence (`F_._BN_BLOCK = False`)"""
    c = shape[1]
    seed = seed_of(shape, dtype)
    conv, idt, _ = inputs(shape, dtype, seed)
    bn = make_bn(c, seed, F32, DEV)
    m = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(c), seed, F32)).to(DEV).train()
    cg = conv.to(DEV).contiguous(memory_format=CL).requires_grad_()
    ig = idt.to(DEV).contiguous(memory_format=CL).requires_grad_()
    old = F_._BN_BLOCK
    F_._BN_BLOCK = fused
    try:
        if fused:
            fused = F_.bn_block_plan(cg, cnsn_amd.FusedConfig(sn_active=True, add_mode=mode, relu=relu))
            assert fused == expect_plan, (shape, mode)
        y = call(m, bn, cg, ig, mode, relu)
        assert (type(y.grad_fn).__name__ == "FusedBnBlockBackward") == fused
    finally:
        F_._BN_BLOCK = old
    return y, cg, ig, bn, m


def device_backward(state, gy, shape, mode):
    """... its backward for `gy` (CPU, the activation dtype): every output in the keys compare() reads"""
    y, cg, ig, bn, m = state
    y.backward(gy.to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    assert y.is_contiguous(memory_format=CL) and cg.grad.is_contiguous(memory_format=CL)
    if mode == "post":
        assert ig.grad.is_contiguous(memory_format=CL)
    else:
        assert ig.grad is None
    g_bn = m.selfnorm.g_bn
    return dict(y=y.detach().cpu().double(), dc=cg.grad.cpu().double(),
                di=ig.grad.cpu().double() if mode == "post" else torch.zeros(shape, dtype=torch.float64),
                bn=[p.grad.cpu().double() for p in bn.parameters()], sn=[p.grad.cpu().double() for p in m.selfnorm.parameters()],
                bn_rm=bn.running_mean.cpu().double(), bn_rv=bn.running_var.cpu().double(), sn_rm=g_bn.running_mean.cpu().double(),
                sn_rv=g_bn.running_var.cpu().double(), nbt=int(bn.num_batches_tracked), sn_nbt=int(g_bn.num_batches_tracked))


def run(shape, dtype, mode, relu, fused=True, expect_plan=True):
    """(the oracle through the device's mask, what the library returns); `fused` False: the library's un-fused sequence"""
    seed = seed_of(shape, dtype)
    conv, idt, gy = inputs(shape, dtype, seed)
    got = device_backward(device_forward(shape, dtype, mode, relu, fused, expect_plan), gy, shape, mode)
    return oracle(conv, idt, gy, shape[1], seed, mode, relu, got["y"] > 0, dtype), got


def check(ref, got, dtype, relu, what, fused=True, shape=None):
    """compare()'s bars for y, d_conv, d_identity, the five parameter gradients, BatchNorm2d's two running buffers and the
    gate's running variance; once more with the gate's running MEAN in the running variance's place (the fourth buffer, same
    bar); both counters"""
    assert len(got["bn"]) == 2 and len(got["sn"]) == 3
    compare(ref, got, dtype, relu, what, fused=fused, shape=shape)
    compare({k: dict(v, sn_rv=v["sn_rm"]) for k, v in ref.items()}, dict(got, sn_rv=got["sn_rm"]), dtype, relu, (what, "sn_rm"),
            fused=fused, shape=shape)
    assert got["nbt"] == got["sn_nbt"] == ref["t64"]["sn_nbt"] == 1


def ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode,relu", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_against_torch_in_float64(shape, mode, relu, dtype):
    ref, got = run(shape, dtype, mode, relu)
    check(ref, got, dtype, relu, (shape, mode, relu, dtype))


@pytest.mark.parametrize("mode,relu", MODES, ids=MODE_IDS)
def test_fused_f16(mode, relu):
    shape = (8, 64, 7, 7)
    ref, got = run(shape, F16, mode, relu)
    check(ref, got, F16, relu, (shape, mode, relu, F16))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode,relu", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_against_the_unfused_sequence(shape, mode, relu, dtype):
    """The fused launch against the library's own un-fused sequence (`F_._BN_BLOCK = False`: bn3, then the op's launches) on the
    same inputs, with compare()'s bars: the un-fused results stand where compare() takes the fp32 composition — 16-bit:
    |fused - un-fused| <= 1e-2 of the scale for y, d_conv, d_identity and the parameter bar with its un-rounded-composition clause
    (the oracle's un-rounded composition stays in its place); fp32: |fused - truth64| <= max(1e-5 * scale, 2 * |un-fused -
    truth64|).  Both backwards run through ONE shared mask, as tests/test_gpu_bn_block.py::
    test_full_size_against_the_unfused_sequence does it: the upstream gradient is zeroed where the two paths' ReLU masks differ
    (at most compare()'s 1e-4 / 5e-3 of the elements), so the gradients compare the two paths' arithmetic and not their flips.

    (The un-fused sequence on its own does NOT meet the 16-bit parameter bar against the float64 truth — bn3 weight up to 3.6e-3,
    the gate's fc weight 1.85e-2 of the scale where the fused launch has 5.1e-4 / 4.3e-3, profiles/r09_bn_block_post.md section 5;
    that is a property of the path this launch replaces and is not asserted here.)"""
    seed = seed_of(shape, dtype)
    conv, idt, gy = inputs(shape, dtype, seed)
    states = {fused: device_forward(shape, dtype, mode, relu, fused) for fused in (True, False)}
    if relu:
        same = ((states[True][0] > 0) == (states[False][0] > 0)).cpu()
        assert 1.0 - float(same.double().mean()) < (1e-4 if dtype == F32 else 5e-3), (shape, mode, dtype)
        gy = gy * same.to(gy.dtype)
    got, unfused = (device_backward(states[fused], gy, shape, mode) for fused in (True, False))
    ref = oracle(conv, idt, gy, shape[1], seed, mode, relu, got["y"] > 0, dtype)
    ref["o32"] = dict(unfused, pre=unfused["y"])        # (behind a ReLU y is the pre-activation wherever compare() looks at it)
    check(ref, got, dtype, relu, (shape, mode, relu, dtype, "against the un-fused sequence"))


@pytest.mark.parametrize("shape,half,dtype", [(s, h, F32) for s, h in FP32] + [(s, h, BF16) for s, h in BIT16],
                         ids=[ids(s) + "-fp32" for s, _ in FP32] + [ids(s) + "-bf16" for s, _ in BIT16])
def test_geometry_post_relu(shape, half, dtype, capfd, monkeypatch):
    """channel counts that are no power of two (tests/test_gpu_nhwc_geometry.py's lists): each direction ran ONE bn-block launch
    with status 0 and the tile rule's tiles, S, rows and tcb; values against the float64 truth"""
    with knobs(monkeypatch, CNSN_DEBUG="1"), healthy():
        capfd.readouterr()
        ref, got = run(shape, dtype, "post", True)
        err = capfd.readouterr().err
    check_geometry(launches(err), "bn-block", shape, dtype, 4, 4)
    assert err.count("mode=post") == 2, err
    check(ref, got, dtype, True, (shape, dtype, "geometry"))


def test_plan_answers_for_a_post_and_a_none_epilogue():
    """what the parent commit lacks: cnsn_bn_block_plan answers 1 for a POST (and a NONE) epilogue, and the call is ONE autograd
    node of the fused launch"""
    shape = (12, 16, 9, 7)
    x = torch.randn(shape, device=DEV).contiguous(memory_format=CL)
    for mode, relu in MODES:
        assert F_.bn_block_plan(x, cnsn_amd.FusedConfig(sn_active=True, add_mode=mode, relu=relu)), (mode, relu)
    assert not F_.bn_block_plan(x, cnsn_amd.FusedConfig(sn_active=True, add_mode="none", relu=True))     # (no add: no ReLU either)
    bn = make_bn(16, 1, F32, DEV)
    m = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(16), 1, F32)).to(DEV).train()
    y = m.forward_bn_block(x.clone(memory_format=CL).requires_grad_(), bn, x, relu=True, add_mode="post")
    assert type(y.grad_fn).__name__ == "FusedBnBlockBackward"
    with pytest.raises(AssertionError):
        m.forward_bn_block(x, bn, None, relu=True, add_mode="post")      # no identity: 'none' only


def _state(y, cg, ig, bn, bn2, m):
    out = [y.detach(), cg.grad] + ([ig.grad] if ig.grad is not None else [])
    for mod in (bn, bn2, m):
        if mod is not None:
            out += [p.grad for p in mod.parameters()] + list(mod.state_dict().values())
    return out


def _fallback(shape, mode, relu, how, channels_last=True, eval_mode=False, armed=False, two=False):
    """forward_bn_block where no fused launch applies against today's statements on identical modules: bit-equal"""
    c = shape[1]
    conv, idt, gy = inputs(shape, F32, seed_of(shape, F32))
    fmt = CL if channels_last else torch.contiguous_format
    runs = []
    for literal in (False, True):
        bn = make_bn(c, 3, F32, DEV)
        bn2 = make_bn(c, 53, F32, DEV) if two else None
        cn = cnsn_amd.CrossNorm("neither", 1) if armed else None
        m = cnsn_amd.CNSN(cn, fill_sn(cnsn_amd.SelfNorm(c), 3, F32)).to(DEV).train()
        if eval_mode:
            m.eval()
            bn.eval()
        if armed:
            m.crossnorm.active = True
        np.random.seed(0)
        torch.manual_seed(0)
        cg = conv.to(DEV).contiguous(memory_format=fmt).requires_grad_()
        ig = idt.to(DEV).contiguous(memory_format=fmt).requires_grad_()
        if not literal:
            assert not (F_.bn_block_plan(cg, cnsn_amd.FusedConfig(sn_active=True, add_mode=mode, relu=relu))
                        and not (eval_mode or armed or two)), how
            y = call(m, bn, cg, ig, mode, relu, identity_bn=bn2)
            assert type(y.grad_fn).__name__ != "FusedBnBlockBackward", how
        elif mode == "none":
            y = m(bn(cg))
        else:
            y = m.forward_block(bn(cg), ig if bn2 is None else bn2(ig), add_mode=mode, relu=relu)
        y.backward(gy.to(DEV).contiguous(memory_format=fmt))
        torch.cuda.synchronize()
        runs.append(_state(y, cg, ig, bn, bn2, m))
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(u, v) for u, v in zip(*runs)), how


@pytest.mark.parametrize("mode,relu", [("post", True), ("none", False)], ids=["post+relu", "none"])
def test_fall_backs_are_todays_statements(mode, relu):
    for shape in TOO_FEW_TILES:
        _fallback(shape, mode, relu, ("fewer than 8 tiles", shape))
    _fallback((12, 16, 9, 7), mode, relu, "NCHW", channels_last=False)
    _fallback((12, 16, 9, 7), mode, relu, "eval", eval_mode=True)
    _fallback((12, 16, 9, 7), mode, relu, "armed CrossNorm", armed=True)


def test_identity_bn_with_post_is_not_fused():
    _fallback((12, 16, 9, 7), "post", True, "identity_bn", two=True)
