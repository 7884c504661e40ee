"""BatchNorm2d (+ add) + ReLU on NCHW tensors in two plain launches per direction (cnsn_*_bn_act_nchw, functional.BatchNormActNCHW,
ABI 9 — added in round 12) without a GPU: the names are declared, bound and exported; the plan answers eligible and ineligible
descriptors as include/cnsn_hip.h says; the tile geometry — walked here in Python exactly as the header describes it — cuts
every channel's N*H*W elements into tiles that partition them, is the same on every query, and fits the workspace; the entry
points refuse argument errors before anything reaches the device; the new translation unit compiled without scratch; with the
switch off (the default) nothing in `callers` changes."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import cnsn_amd
from cnsn_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cnsn_bn_act_nchw_plan", "cnsn_bn_act_nchw_workspace_bytes", "cnsn_bn_act_nchw_geometry", "cnsn_forward_bn_act_nchw",
         "cnsn_backward_bn_act_nchw")
F32, BF16, F16 = _ffi.CNSN_F32, _ffi.CNSN_BF16, _ffi.CNSN_F16


def make_desc(shape=(8, 64, 8, 8), dtype=BF16, training=1, **kw):
    d = _ffi.BnAct()
    d.struct_bytes = C.sizeof(_ffi.BnAct)
    d.dtype, (d.N, d.C, d.H, d.W), d.relu, d.add = dtype, shape, 1, 0
    d.bn.struct_bytes = C.sizeof(_ffi.BnTail)
    d.bn.training, d.bn.eps, d.bn.momentum = training, 1e-5, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def geometry(lib, d, backward=0):
    out = (C.c_int32 * 4)()
    st = lib.cnsn_bn_act_nchw_geometry(C.byref(d), backward, out)
    return st, tuple(out)


def test_new_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "cnsn_hip.h")).read()
    handle = C.CDLL(_ffi.LIB_PATH)
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in _ffi.SIGNATURES
        assert hasattr(handle, n), f"libcnsn_hip.so lacks {n}"
    assert re.search(r"#define CNSN_ABI_VERSION 9\b", src) and cnsn_amd.lib().cnsn_abi_version() == 9   # (additive: the number stays)
    assert C.sizeof(_ffi.BnAct) == 104                                            # the descriptor is unchanged
    from cnsn_amd import functional
    from cnsn_amd.callers import _sites
    assert hasattr(functional, "BatchNormActNCHW") and callable(functional.bn_act_nchw_plan)
    assert _sites.FUSE_BN_ACT_NCHW is (os.environ.get("CNSN_BN_ACT_NCHW", "0") == "1")


def test_plan_answers():
    lib = cnsn_amd.lib()

    def plan(d, back):
        return lib.cnsn_bn_act_nchw_plan(C.byref(d), 0, back)
    # eligible: any C >= 1, any H, W, any N with N*H*W >= 2, the three dtypes, both directions; the addend does not bear on it
    for shape in ((5, 3, 9, 11), (37, 6, 7, 7), (128, 8, 8, 8), (3, 4, 224, 224), (2, 16, 1, 1), (1, 1, 1, 2), (1024, 1, 3, 1),
                  (16, 2048, 64, 64), (1, 1, 46340, 46340)):
        for dtype in (F32, BF16, F16):
            d = make_desc(shape, dtype)
            assert plan(d, 0) == 1 and plan(d, 1) == 1, (shape, dtype)
            assert lib.cnsn_bn_act_nchw_plan(C.byref(d), 1, 0) == 1
    # one value per channel has no batch statistics
    one = make_desc((1, 16, 1, 1))
    assert plan(one, 0) == 0 and plan(one, 1) == 0 and geometry(lib, one)[0] == -9
    # eval: forward only, and one value per channel is fine there
    ev = make_desc(training=0)
    assert plan(ev, 0) == 1 and plan(ev, 1) == 0 and geometry(lib, ev, 1)[0] == -9 and geometry(lib, ev, 0)[0] == 0
    assert plan(make_desc((1, 16, 1, 1), training=0), 0) == 1
    # the index range the header states: fewer than 2^31 elements
    for shape in ((2, 1, 32768, 32768), (256, 2048, 64, 64), (1, 2 ** 30, 1, 2), (2 ** 30, 2, 2 ** 30, 2 ** 30)):
        big = make_desc(shape)
        assert plan(big, 0) == 0 and plan(big, 1) == 0, shape
        assert lib.cnsn_bn_act_nchw_workspace_bytes(C.byref(big)) == 0
    # argument errors
    assert lib.cnsn_bn_act_nchw_plan(None, 0, 0) == -1
    bad = make_desc(struct_bytes=8)
    assert plan(bad, 0) == -8 and lib.cnsn_bn_act_nchw_workspace_bytes(C.byref(bad)) == 0 and geometry(lib, bad)[0] == -8
    bn_bad = make_desc()
    bn_bad.bn.struct_bytes = 4
    assert plan(bn_bad, 0) == -8
    assert plan(make_desc(dtype=7), 0) == -3
    for shape in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, -1, 4), (4, 4, 4, 0)):
        assert plan(make_desc(shape), 0) == -2, shape
    assert lib.cnsn_bn_act_nchw_geometry(C.byref(make_desc()), 0, None) == -1


SHAPES = [(5, 3, 9, 11), (37, 6, 7, 7), (137, 6, 7, 7), (128, 8, 8, 8), (3, 4, 224, 224), (8, 4, 256, 256), (8, 1, 256, 256),
          (2, 16, 1, 1), (16, 8, 64, 64), (128, 16, 32, 32), (128, 128, 8, 8), (16, 64, 256, 256), (16, 2048, 64, 64),
          (256, 64, 112, 112), (1, 1, 1, 2), (7, 5, 225, 225), (1, 3, 1, 100003), (100003, 1, 1, 1), (2, 2, 1025, 1023),
          (5, 1, 4096, 4096)]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tiles_partition_every_channel(shape, dtype):
    """the walk of include/cnsn_hip.h: tile t takes instances [ig*ipt, ..) and plane elements [s*epr, ..), ig = t / S, s = t % S,
    S = ceil(P / epr), cut at N and P — every (instance, element) of a channel exactly once, no tile empty"""
    lib = cnsn_amd.lib()
    n, c, h, w = shape
    p = h * w
    d = make_desc(shape, dtype)
    st, (tiles, ipt, epr, threads) = geometry(lib, d)
    assert st == 0 and threads == 256 and tiles >= 1 and ipt >= 1 and epr >= 1
    for back in (0, 1):                                                           # identical on every query, either direction
        assert geometry(lib, d, back) == (0, (tiles, ipt, epr, threads))
    assert geometry(lib, make_desc(shape, dtype, training=0)) == (0, (tiles, ipt, epr, threads))
    s_per_plane = -(-p // epr)
    groups = -(-n // ipt)
    assert tiles == groups * s_per_plane
    assert ipt == 1 or s_per_plane == 1                  # several instances per tile OR several tiles per plane
    if s_per_plane > 1:
        assert epr % (16 // (4 if dtype == F32 else 2)) == 0                      # ranges inside a plane start on whole vectors
    inst = torch.zeros(n, dtype=torch.int64)
    elem = torch.zeros(p, dtype=torch.int64)
    covered = 0
    for t in range(tiles):
        ig, s = divmod(t, s_per_plane)
        n0, n1 = ig * ipt, min(n, (ig + 1) * ipt)
        e0, e1 = s * epr, min(p, (s + 1) * epr)
        assert n0 < n1 and e0 < e1, f"tile {t} is empty"
        covered += (n1 - n0) * (e1 - e0)
        if s == 0:
            inst[n0:n1] += 1
        if ig == 0:
            elem[e0:e1] += 1
    # rectangles of a grid whose rows cover the instances once and whose columns cover the plane once
    assert covered == n * p and bool((inst == 1).all()) and bool((elem == 1).all())
    ws = lib.cnsn_bn_act_nchw_workspace_bytes(C.byref(d))
    assert ws >= c * tiles * 2 * 4
    assert ws == lib.cnsn_bn_act_nchw_workspace_bytes(C.byref(d)) and ws <= c * tiles * 8 + 1024
    assert c * tiles < 2 ** 31


def test_geometry_classes_exist():
    """the classes the GPU tests name: many instances per tile, a ragged last instance group, several tiles per plane, and more
    tiles per channel than the 256 threads of a workgroup add in one step"""
    lib = cnsn_amd.lib()
    tiles, ipt, epr, _ = geometry(lib, make_desc((128, 8, 8, 8), F32))[1]
    assert ipt > 1 and epr == 64 and tiles > 1
    tiles, ipt, epr, _ = geometry(lib, make_desc((137, 6, 7, 7), BF16))[1]
    assert ipt > 1 and tiles > 1 and 137 % ipt != 0
    tiles, ipt, epr, _ = geometry(lib, make_desc((3, 4, 224, 224), F32))[1]
    assert ipt == 1 and epr < 224 * 224 and tiles > 3
    tiles, ipt, epr, _ = geometry(lib, make_desc((8, 1, 256, 256), F32))[1]
    assert ipt == 1 and tiles > 256


def fwd(lib, d, x=16, addend=None, y=32, saved=None, ws=48, ws_bytes=1 << 24):
    return lib.cnsn_forward_bn_act_nchw(C.byref(d), x, addend, y, saved, ws, ws_bytes, None)


def bwd(lib, d, gy=16, x=16, addend=None, saved=16, dx=32, da=None, ws=48, ws_bytes=1 << 24):
    return lib.cnsn_backward_bn_act_nchw(C.byref(d), gy, x, addend, saved, dx, da, None, None, ws, ws_bytes, None)


def test_entry_points_refuse_before_any_launch():
    lib = cnsn_amd.lib()
    assert lib.cnsn_forward_bn_act_nchw(None, 16, None, 32, None, 48, 1 << 20, None) == -1
    assert lib.cnsn_backward_bn_act_nchw(None, 16, 16, None, 16, 32, None, None, None, 48, 1 << 20, None) == -1
    bad = make_desc(struct_bytes=8)
    assert fwd(lib, bad) == -8 and bwd(lib, bad) == -8
    assert fwd(lib, make_desc(dtype=7)) == -3 and fwd(lib, make_desc((4, 0, 4, 4))) == -2
    # ineligible: CNSN_E_UNSUPPORTED — one value per channel in training, beyond the index range, eval backward
    assert fwd(lib, make_desc((1, 16, 1, 1))) == -9 and bwd(lib, make_desc((1, 16, 1, 1))) == -9
    assert fwd(lib, make_desc((256, 2048, 64, 64))) == -9 and bwd(lib, make_desc((256, 2048, 64, 64))) == -9
    assert bwd(lib, make_desc(training=0)) == -9
    d = make_desc()
    assert fwd(lib, d, x=None) == -1
    assert fwd(lib, d) == -1                                                      # the BatchNorm2d's arrays are NULL
    d.bn.weight, d.bn.bias, d.bn.running_mean, d.bn.running_var = 256, 512, 768, 1024
    # ... and a base pointer that is not 16-byte aligned
    assert fwd(lib, d, x=24) == -9 and fwd(lib, d, y=40) == -9 and fwd(lib, d, addend=40) == -9
    assert bwd(lib, d, gy=8) == -9 and bwd(lib, d, dx=36) == -9 and bwd(lib, d, addend=64, da=72) == -9
    assert fwd(lib, d, ws_bytes=16) == -6 and bwd(lib, d, ws_bytes=16) == -6      # CNSN_E_WORKSPACE
    assert bwd(lib, d, saved=None) == -1
    assert bwd(lib, d, addend=64) == -1                                           # ReLU behind an addend: grad_addend is owed


def test_the_new_unit_compiled_without_scratch():
    with open(os.path.join(ROOT, "crossnorm-selfnorm_amd", "build_report.json")) as fh:
        report = json.load(fh)
    unit = report["cnsn_nchw_bn"]
    # fwd stats x3 dtypes, fwd apply / eval / bwd stats / bwd apply x3 dtypes x {addend, none}
    assert unit["kernels"] >= 27 and unit["with_scratch"] == 0 and unit["max_scratch_bytes_per_lane"] == 0


class Cfg:
    pass


def test_switch_off_is_the_default_and_cpu_calls_are_the_plain_statements(monkeypatch):
    """on a CPU neither route takes a call, so the switch must not change a bit; WideResNet keeps its modules and keys"""
    import torch.nn as nn
    from cnsn_amd.callers import WideResNetCNSN, _sites, bn_act
    from oracle import cnsn_oracle as orc
    results, keys = [], []
    for on in (False, True):
        monkeypatch.setattr(_sites, "FUSE_BN_ACT_NCHW", on)
        torch.manual_seed(3)
        net = WideResNetCNSN(depth=10, num_classes=5, widen_factor=1, cnsn_type="sn", impl=orc).train()
        x = torch.randn(2, 3, 32, 32)
        out = net(x)
        out.sum().backward()
        bn = nn.BatchNorm2d(4).train()
        xb = torch.randn(3, 4, 5, 5, requires_grad=True)
        y = bn_act(bn, xb)
        assert "BatchNormAct" not in type(y.grad_fn).__name__
        results.append((out.detach(), net.conv1.weight.grad.clone(), net.bn1.running_var.clone(),
                        net.block1.layer[0].bn2.running_mean.clone(), y.detach()))
        keys.append([f"{k}|{tuple(v.shape)}" for k, v in net.state_dict().items()])
        assert type(net.bn1) is nn.BatchNorm2d and type(net.block2.layer[0].relu2) is nn.ReLU
    assert keys[0] == keys[1]
    for u, v in zip(*results):
        assert torch.equal(u, v)
