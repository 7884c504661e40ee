"""ResNet-50-IBN-a / -b (callers/resnet_ibn.py) without a GPU: both backbones expose the reference's state_dict keys, shapes and
key order (G9, generated from the imported reference by tests/golden/gen_golden_ibn.py), the new names are declared and
exported, and the IBN entry points of the C ABI (cnsn_ibn_*, ABI 9) answer argument errors with the documented status codes
before anything reaches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cnsn_amd
from cnsn_amd import _ffi
from oracle import cnsn_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(os.path.join(golden_dir, "g9_ibn.npz"))


class Cfg:
    active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"


def keys_of(m):
    return [f"{k}|{tuple(v.shape)}" for k, v in m.state_dict().items()]


@pytest.mark.parametrize("variant", ["a", "b"])
def test_state_dict_keys_and_order_match_reference(g9, variant):
    from cnsn_amd.callers import resnet50_ibn_a, resnet50_ibn_b
    build = {"a": resnet50_ibn_a, "b": resnet50_ibn_b}[variant]
    assert keys_of(build(Cfg, impl=orc)) == [str(k) for k in g9[f"{variant}_keys"]]
    assert keys_of(build(Cfg)) == [str(k) for k in g9[f"{variant}_keys"]]      # (this library's CNSN modules)


def test_ibn_sites_and_quirks():
    from cnsn_amd.callers import IBN, InstanceNorm2d, ResNet50IBNCNSN
    a = ResNet50IBNCNSN(ibn_cfg=("a", "a", "a", None), impl=orc)
    ibn = [n for n, m in a.named_modules() if isinstance(m, IBN)]
    assert len(ibn) == 13 and all(n.endswith(".bn1") for n in ibn) and not any(n.startswith("layer4") for n in ibn)
    assert [a.get_submodule(n).half for n in ("layer1.0.bn1", "layer2.0.bn1", "layer3.0.bn1")] == [32, 64, 128]
    b = ResNet50IBNCNSN(ibn_cfg=("b", "b", None, None), impl=orc)
    ins = [n for n, m in b.named_modules() if isinstance(m, InstanceNorm2d)]
    assert ins == ["bn1", "layer1.2.IN", "layer2.3.IN"]
    assert getattr(b.layer1[2], "cnsn", None) is None and getattr(b.layer2[3], "cnsn", None) is None   # IN + pos='post': no unit
    assert b.layer1[1].cnsn is not None and b.layer3[5].cnsn is not None
    assert isinstance(b.avgpool, torch.nn.AvgPool2d) and b.avgpool.kernel_size == 7
    # the init loop covers InstanceNorm2d; CrossNorm sites are collected for aug=True
    assert float(b.layer1[2].IN.weight.detach().min()) == 1.0 and float(b.layer1[2].IN.bias.detach().abs().max()) == 0.0
    cn = ResNet50IBNCNSN(ibn_cfg=("b", "b", None, None), cnsn_type="cnsn", active_num=2, impl=orc)
    assert cn.cn_num == 16 - 2 and cn.active_num == 2


def test_resnet50_cnsn_modules_unchanged():
    from cnsn_amd.callers import ResNet50CNSN
    m = ResNet50CNSN(impl=orc)
    assert all(type(getattr(m.get_submodule(f"layer{i}")[0], "bn1")) is torch.nn.BatchNorm2d for i in range(1, 5))
    assert not any(n.endswith(".IN") for n, _ in m.named_modules())
    assert isinstance(m.avgpool, torch.nn.AdaptiveAvgPool2d)


def test_new_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "cnsn_hip.h")).read()
    names = ("cnsn_ibn_plan", "cnsn_ibn_saved_floats", "cnsn_ibn_workspace_bytes", "cnsn_forward_ibn", "cnsn_backward_ibn")
    for n in names:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in _ffi.SIGNATURES
        assert hasattr(C.CDLL(_ffi.LIB_PATH), n), f"libcnsn_hip.so lacks {n}"
    assert "typedef struct cnsn_ibn" in src and re.search(r"#define CNSN_ABI_VERSION 9\b", src)
    assert _ffi.ABI_VERSION == 9 == cnsn_amd.lib().cnsn_abi_version()
    assert C.sizeof(_ffi.Ibn) == 128
    import cnsn_amd.callers as callers
    from cnsn_amd import functional
    for n in ("ResNet50IBNCNSN", "resnet50_ibn_a", "resnet50_ibn_b"):
        assert n in callers.__all__ and hasattr(callers, n)
    assert hasattr(functional, "IBNorm") and hasattr(functional, "ibn_plan")
    assert hasattr(callers.IBN, "forward_act") and hasattr(callers.InstanceNorm2d, "forward_act")


def make_desc(**kw):
    d = _ffi.Ibn()
    d.struct_bytes = C.sizeof(_ffi.Ibn)
    d.dtype, d.N, d.C, d.H, d.W, d.half, d.relu, d.eps_in = _ffi.CNSN_BF16, 8, 64, 8, 8, 32, 1, 1e-5
    d.bn.struct_bytes = C.sizeof(_ffi.BnTail)
    d.bn.training, d.bn.eps, d.bn.momentum = 1, 1e-5, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_ibn_argument_validation_without_gpu():
    lib = cnsn_amd.lib()
    d = make_desc()
    assert lib.cnsn_ibn_saved_floats(C.byref(d)) == 5 * 8 * 64
    assert lib.cnsn_ibn_plan(None, 0, 0) == -1                                   # CNSN_E_NULL
    assert lib.cnsn_forward_ibn(None, 16, None, 32, None, 48, 1 << 20, None) == -1
    bad = make_desc(struct_bytes=8)
    assert lib.cnsn_ibn_plan(C.byref(bad), 0, 0) == -8                           # CNSN_E_STRUCT
    assert lib.cnsn_ibn_saved_floats(C.byref(bad)) == 0 and lib.cnsn_ibn_workspace_bytes(C.byref(bad)) == 0
    assert lib.cnsn_forward_ibn(C.byref(bad), 16, None, 32, None, 48, 1 << 20, None) == -8
    assert lib.cnsn_backward_ibn(C.byref(bad), 16, 16, None, 16, 32, None, None, None, None, 48, 1 << 20, None) == -8
    bn_bad = make_desc()
    bn_bad.bn.struct_bytes = 4                                                   # the BatchNorm2d half's struct is checked ...
    assert lib.cnsn_ibn_plan(C.byref(bn_bad), 0, 0) == -8
    in_only = make_desc(half=64)
    in_only.bn.struct_bytes = 4                                                  # ... and ignored when half == C
    assert lib.cnsn_ibn_plan(C.byref(in_only), 0, 0) >= 0
    assert lib.cnsn_ibn_plan(C.byref(make_desc(dtype=7)), 0, 0) == -3            # CNSN_E_DTYPE
    for shape in (dict(N=0), dict(W=0), dict(half=-8), dict(half=72)):           # CNSN_E_SHAPE
        assert lib.cnsn_ibn_plan(C.byref(make_desc(**shape)), 0, 0) == -2, shape
        assert lib.cnsn_forward_ibn(C.byref(make_desc(**shape)), 16, None, 32, None, 48, 1 << 20, None) == -2, shape
    # ineligible calls: plan 0, entry points CNSN_E_UNSUPPORTED (nothing launched)
    for inel in (dict(half=0), dict(half=12), dict(C=60, half=32), dict(N=1), dict(N=257), dict(H=1, W=1)):
        assert lib.cnsn_ibn_plan(C.byref(make_desc(**inel)), 0, 0) == 0, inel
        assert lib.cnsn_forward_ibn(C.byref(make_desc(**inel)), 16, None, 32, None, 48, 1 << 20, None) == -9, inel
        assert lib.cnsn_backward_ibn(C.byref(make_desc(**inel)), 16, 16, None, 16, 32, None, None, None, None, 48, 1 << 20,
                                     None) == -9, inel
    # eligible shape, missing / misaligned pointers and a short workspace are refused before any launch
    assert lib.cnsn_ibn_plan(C.byref(d), 1, 0) == 1 and lib.cnsn_ibn_plan(C.byref(d), 0, 1) == 1
    assert lib.cnsn_forward_ibn(C.byref(d), None, None, 32, None, 48, 1 << 20, None) == -1
    assert lib.cnsn_forward_ibn(C.byref(d), 16, None, 32, None, 48, 1 << 20, None) == -1      # BatchNorm2d arrays NULL
    d.bn.weight, d.bn.bias, d.bn.running_mean, d.bn.running_var = 256, 512, 768, 1024
    assert lib.cnsn_forward_ibn(C.byref(d), 24, None, 32, None, 48, 1 << 20, None) == -4      # CNSN_E_ALIGN
    assert lib.cnsn_forward_ibn(C.byref(d), 16, 40, 32, None, 48, 1 << 20, None) == -4
    assert lib.cnsn_forward_ibn(C.byref(d), 16, None, 32, None, 48, 16, None) == -6           # CNSN_E_WORKSPACE
    assert lib.cnsn_backward_ibn(C.byref(d), 16, 16, None, None, 32, None, None, None, None, 48, 1 << 20, None) == -1
    assert lib.cnsn_backward_ibn(C.byref(d), 16, 16, None, 16, 32, None, None, None, None, 48, 16, None) == -6


def test_ibn_plan_follows_the_switches_forward_only():
    """the forward asks what the other single launches ask — the co-resident kernels allowed (cnsn_resident_enable /
    CNSN_RESIDENT), CNSN_NHWC_FUSED not 0 and, above 2, the tensor within that many MiB; the backward of a launch that ran
    asks none of it"""
    from cnsn_amd import functional
    lib = cnsn_amd.lib()
    small, big = make_desc(), make_desc(N=256, H=112, W=112, half=64, C=64)    # 64 KiB / 392 MiB in bf16
    was = functional.resident_allowed()
    old = os.environ.get("CNSN_NHWC_FUSED")

    def plans(d):
        return lib.cnsn_ibn_plan(C.byref(d), 0, 0), lib.cnsn_ibn_plan(C.byref(d), 0, 1)
    try:
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
