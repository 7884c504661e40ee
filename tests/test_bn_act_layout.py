"""BatchNorm2d (+ add) + ReLU in one channels-last launch (callers.bn_act, functional.BatchNormAct, cnsn_*_bn_act, ABI 9 — added in
round 8) without a GPU: the new names are declared, bound and exported; the entry points answer argument errors with the
documented status codes before anything reaches the device; the plan is a pure function of the call (any N) and follows the
switches in the forward only; every call the launch does not take — all of them on a CPU — gives exactly the plain statements'
results; the backbones' modules and `state_dict` keys are what they were."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import cnsn_amd
from cnsn_amd import _ffi
from oracle import cnsn_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cnsn_bn_act_plan", "cnsn_bn_act_saved_floats", "cnsn_bn_act_workspace_bytes", "cnsn_forward_bn_act", "cnsn_backward_bn_act")


def test_new_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "cnsn_hip.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in _ffi.SIGNATURES
        assert hasattr(C.CDLL(_ffi.LIB_PATH), n), f"libcnsn_hip.so lacks {n}"
    assert "typedef struct cnsn_bn_act" in src and re.search(r"#define CNSN_ABI_VERSION 9\b", src)
    assert _ffi.ABI_VERSION == 9 == cnsn_amd.lib().cnsn_abi_version()          # (purely additive: the number stays)
    assert C.sizeof(_ffi.BnAct) == 104
    import cnsn_amd.callers as callers
    from cnsn_amd import functional
    assert "bn_act" in callers.__all__ and callable(callers.bn_act)
    assert hasattr(functional, "BatchNormAct") and callable(functional.bn_act_plan)
    from cnsn_amd.callers import _sites
    assert isinstance(_sites.FUSE_BN_ACT, bool)


def make_desc(**kw):
    d = _ffi.BnAct()
    d.struct_bytes = C.sizeof(_ffi.BnAct)
    d.dtype, d.N, d.C, d.H, d.W, d.relu, d.add = _ffi.CNSN_BF16, 8, 64, 8, 8, 1, 0
    d.bn.struct_bytes = C.sizeof(_ffi.BnTail)
    d.bn.training, d.bn.eps, d.bn.momentum = 1, 1e-5, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fwd(lib, d, x=16, addend=None, y=32, saved=None, ws=48, ws_bytes=1 << 24):
    return lib.cnsn_forward_bn_act(C.byref(d), x, addend, y, saved, ws, ws_bytes, None)


def bwd(lib, d, gy=16, x=16, addend=None, saved=16, dx=32, da=None, ws=48, ws_bytes=1 << 24):
    return lib.cnsn_backward_bn_act(C.byref(d), gy, x, addend, saved, dx, da, None, None, ws, ws_bytes, None)


def test_bn_act_argument_validation_without_gpu():
    lib = cnsn_amd.lib()
    d = make_desc()
    assert lib.cnsn_bn_act_saved_floats(C.byref(d)) == 2 * 64                     # O(C): mean, rstd
    assert lib.cnsn_bn_act_saved_floats(C.byref(make_desc(N=1024, C=2048))) == 2 * 2048
    assert lib.cnsn_bn_act_plan(None, 0, 0) == -1                                 # CNSN_E_NULL
    assert lib.cnsn_forward_bn_act(None, 16, None, 32, None, 48, 1 << 20, None) == -1
    assert lib.cnsn_backward_bn_act(None, 16, 16, None, 16, 32, None, None, None, 48, 1 << 20, None) == -1
    bad = make_desc(struct_bytes=8)
    assert lib.cnsn_bn_act_plan(C.byref(bad), 0, 0) == -8                         # CNSN_E_STRUCT
    assert lib.cnsn_bn_act_saved_floats(C.byref(bad)) == 0 and lib.cnsn_bn_act_workspace_bytes(C.byref(bad)) == 0
    assert fwd(lib, bad) == -8 and bwd(lib, bad) == -8
    bn_bad = make_desc()
    bn_bad.bn.struct_bytes = 4
    assert lib.cnsn_bn_act_plan(C.byref(bn_bad), 0, 0) == -8 and fwd(lib, bn_bad) == -8 and bwd(lib, bn_bad) == -8
    assert lib.cnsn_bn_act_plan(C.byref(make_desc(dtype=7)), 0, 0) == -3          # CNSN_E_DTYPE
    for shape in (dict(N=0), dict(C=0), dict(H=-1), dict(W=0)):                   # CNSN_E_SHAPE
        assert lib.cnsn_bn_act_plan(C.byref(make_desc(**shape)), 0, 0) == -2, shape
        assert fwd(lib, make_desc(**shape)) == -2 and bwd(lib, make_desc(**shape)) == -2, shape
    # ineligible calls: plan 0, entry points CNSN_E_UNSUPPORTED (nothing launched) — C no whole number of 16-byte vectors, one
    # row, fewer than 8 tiles of 64 rows
    for inel in (dict(C=60), dict(C=4), dict(dtype=_ffi.CNSN_F32, C=6), dict(N=1, H=1, W=1), dict(N=4)):
        for back in (0, 1):
            assert lib.cnsn_bn_act_plan(C.byref(make_desc(**inel)), 0, back) == 0, inel
        assert fwd(lib, make_desc(**inel)) == -9 and bwd(lib, make_desc(**inel)) == -9, inel
    # no limit on N: nothing here is per instance
    for n in (257, 1024):
        big = make_desc(N=n)
        assert lib.cnsn_bn_act_plan(C.byref(big), 0, 0) == 1 and lib.cnsn_bn_act_plan(C.byref(big), 1, 1) == 1, n
        assert lib.cnsn_bn_act_workspace_bytes(C.byref(big)) > 0
    assert lib.cnsn_bn_act_plan(C.byref(make_desc(dtype=_ffi.CNSN_F32, C=4, N=300, H=5, W=5)), 0, 0) == 1
    # eval mode: the plain forward launch, no backward
    ev = make_desc()
    ev.bn.training = 0
    assert lib.cnsn_bn_act_plan(C.byref(ev), 0, 0) == 1 and lib.cnsn_bn_act_plan(C.byref(ev), 0, 1) == 0
    assert bwd(lib, ev) == -9
    # eligible shape; missing / misaligned pointers and a short workspace are refused before any launch
    assert lib.cnsn_bn_act_plan(C.byref(d), 1, 0) == 1 and lib.cnsn_bn_act_plan(C.byref(d), 0, 1) == 1
    assert fwd(lib, d, x=None) == -1
    assert fwd(lib, d) == -1                                                      # the BatchNorm2d's arrays are NULL
    d.bn.weight, d.bn.bias, d.bn.running_mean, d.bn.running_var = 256, 512, 768, 1024
    assert fwd(lib, d, x=24) == -4                                                # CNSN_E_ALIGN
    assert fwd(lib, d, addend=40) == -4 and fwd(lib, d, saved=20) == -4
    assert fwd(lib, d, ws_bytes=16) == -6                                         # CNSN_E_WORKSPACE
    assert bwd(lib, d, saved=None) == -1
    assert bwd(lib, d, addend=64) == -1                                           # ReLU behind an addend: grad_addend is owed
    assert bwd(lib, d, addend=64, da=72) == -4 and bwd(lib, d, gy=8) == -4
    assert bwd(lib, d, ws_bytes=16) == -6
    assert lib.cnsn_bn_act_workspace_bytes(C.byref(d)) <= 1 << 20


def test_bn_act_plan_follows_the_switches_forward_only():
    """the forward asks what the other single launches ask — the co-resident kernels allowed (cnsn_resident_enable /
    CNSN_RESIDENT), CNSN_NHWC_FUSED not 0 and, above 2, the tensor within that many MiB; the backward of a launch that ran asks
    none of it"""
    from cnsn_amd import functional
    lib = cnsn_amd.lib()
    small, big = make_desc(N=64, H=16, W=16), make_desc(N=256, H=112, W=112)   # 2 MiB / 392 MiB in bf16
    was = functional.resident_allowed()
    old = os.environ.get("CNSN_NHWC_FUSED")

    def plans(d):
        return lib.cnsn_bn_act_plan(C.byref(d), 0, 0), lib.cnsn_bn_act_plan(C.byref(d), 0, 1)
    try:
        os.environ["CNSN_NHWC_FUSED"] = "2"
        _ffi.reload_env()
        assert plans(small) == (1, 1) and plans(big) == (1, 1)
        functional.set_resident(False)
        assert plans(small) == (0, 1) and plans(big) == (0, 1)
        functional.set_resident(True)
        for knob, want_small, want_big in (("0", (0, 1), (0, 1)), ("3", (1, 1), (0, 1)), ("2", (1, 1), (1, 1))):
            os.environ["CNSN_NHWC_FUSED"] = knob
            _ffi.reload_env()
            assert plans(small) == want_small and plans(big) == want_big, knob
    finally:
        if old is None:
            os.environ.pop("CNSN_NHWC_FUSED", None)
        else:
            os.environ["CNSN_NHWC_FUSED"] = old
        _ffi.reload_env()
        functional.set_resident(was)


class MyBatchNorm(nn.BatchNorm2d):
    pass


def make_bn(cls, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    bn = cls(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


@pytest.mark.parametrize("cls", [nn.BatchNorm2d, MyBatchNorm], ids=["plain", "subclass"])
@pytest.mark.parametrize("fmt", [torch.contiguous_format, torch.channels_last], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "id"])
def test_bn_act_on_cpu_is_the_plain_statements(cls, fmt, training, addend, relu):
    from cnsn_amd.callers import bn_act
    torch.manual_seed(5)
    x = torch.randn(6, 16, 5, 7).contiguous(memory_format=fmt)
    a = torch.randn(6, 16, 5, 7).contiguous(memory_format=fmt) if addend else None
    gy = torch.randn(6, 16, 5, 7)
    got_bn, want_bn = make_bn(cls, 16).train(training), make_bn(cls, 16).train(training)
    xg, xw = x.clone().requires_grad_(), x.clone().requires_grad_()
    got = bn_act(got_bn, xg, a, relu=relu)
    want = want_bn(xw) if a is None else want_bn(xw) + a
    want = torch.relu(want) if relu else want
    assert torch.equal(got, want)
    got.backward(gy)
    want.backward(gy)
    assert torch.equal(xg.grad, xw.grad) and torch.equal(got_bn.weight.grad, want_bn.weight.grad)
    for (k, u), (_, v) in zip(got_bn.state_dict().items(), want_bn.state_dict().items()):
        assert torch.equal(u, v), k
    assert type(got_bn) is cls


def keys_of(m):
    return [f"{k}|{tuple(v.shape)}" for k, v in m.state_dict().items()]


class Cfg:
    active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"


@pytest.mark.parametrize("which", ["resnet50", "ibn_a", "ibn_b", "seg", "fcn_head"])
def test_state_dict_keys_do_not_depend_on_the_switch(which):
    from cnsn_amd.callers import FCNHead, ResNet50CNSN, SegResNet50CNSN, _sites, resnet50_ibn_a, resnet50_ibn_b
    build = {"resnet50": lambda: ResNet50CNSN(impl=orc), "ibn_a": lambda: resnet50_ibn_a(Cfg, impl=orc),
             "ibn_b": lambda: resnet50_ibn_b(Cfg, impl=orc), "seg": lambda: SegResNet50CNSN(impl=orc),
             "fcn_head": lambda: FCNHead(64, 5)}[which]
    was = _sites.FUSE_BN_ACT
    try:
        _sites.FUSE_BN_ACT = True
        on = build()
        _sites.FUSE_BN_ACT = False
        off = build()
    finally:
        _sites.FUSE_BN_ACT = was
    assert keys_of(on) == keys_of(off)
    assert [type(m) for m in on.modules()] == [type(m) for m in off.modules()]
    if which == "resnet50":
        assert type(on.bn1) is nn.BatchNorm2d and type(on.layer3[2].bn2) is nn.BatchNorm2d
    if which == "fcn_head":
        assert list(on.state_dict()) == ["0.weight", "1.weight", "1.bias", "1.running_mean", "1.running_var", "1.num_batches_tracked",
                                         "4.weight", "4.bias"]


def test_backbones_on_cpu_give_the_same_result_with_the_switch_on_and_off():
    """on a CPU no call is taken, so the switch must not change a single bit of a forward + backward (the oracle's units)"""
    from cnsn_amd.callers import FCNHead, ResNet50CNSN, SegResNet50CNSN, _sites
    was = _sites.FUSE_BN_ACT
    results = []
    try:
        for on in (True, False):
            _sites.FUSE_BN_ACT = on
            torch.manual_seed(11)
            net = ResNet50CNSN(num_classes=7, layers=(1, 1, 1, 1), cnsn_type=None, impl=orc).train()
            seg = SegResNet50CNSN(layers=(1, 1, 1, 1), cnsn_type="sn", cn_pos=None, block_idxs="1_2", pos="post", impl=orc).train()
            head = FCNHead(2048, 3).train()
            x = torch.randn(2, 3, 32, 32)
            out = net(x)
            torch.manual_seed(12)
            so = head(seg(x)["out"])
            (out.sum() + so.sum()).backward()
            results.append((out.detach(), so.detach(), net.conv1.weight.grad.clone(), seg.conv1.weight.grad.clone(),
                            net.bn1.running_mean.clone(), seg.layer1[0].bn3.running_var.clone()))
    finally:
        _sites.FUSE_BN_ACT = was
    for u, v in zip(*results):
        assert torch.equal(u, v)
