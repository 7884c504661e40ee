"""cnsn_bn_block_plan for the POST / NONE epilogues (pos='residual' block tails, csrc/cnsn_nhwc_bnhead_kernels.h) and the argument
errors of the three entry points — on the CPU: like the size queries the plan is a pure function of the descriptors (256 compute
units assumed without a device), and every error below is returned before anything is launched."""
import ctypes as C

import pytest
import torch

import cnsn_amd
from cnsn_amd import _ffi
from tests.test_nhwc_workspace_layout import DTYPES, problem

E_STRUCT, E_NULL = -8, -1      # CNSN_E_STRUCT, CNSN_E_NULL (include/cnsn_hip.h)


def epilogue(mode, relu, addend=None):
    e = _ffi.Epilogue()
    e.struct_bytes = C.sizeof(_ffi.Epilogue)
    e.add_mode, e.relu, e.addend = mode, relu, addend
    return e


def plan(shape, dtype, mode, relu, **kw):
    kw = dict(dict(sn_active=1, sn_training=1), **kw)
    return cnsn_amd.lib().cnsn_bn_block_plan(C.byref(problem(shape, dtype, **kw)), C.byref(epilogue(mode, relu)))


MODES = [(_ffi.ADD_PRE, 1), (_ffi.ADD_PRE, 0), (_ffi.ADD_POST, 1), (_ffi.ADD_POST, 0), (_ffi.ADD_NONE, 0)]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(12, 16, 9, 7), (37, 8, 14, 14), (5, 2048, 7, 7), (256, 8, 12, 12), (256, 256, 56, 56),
                                   (256, 2048, 7, 7)], ids=lambda s: "x".join(map(str, s)))
def test_every_add_mode_is_planned(shape, dtype):
    assert [plan(shape, DTYPES[dtype], m, r) for m, r in MODES] == [1] * len(MODES)
    assert plan(shape, DTYPES[dtype], _ffi.ADD_NONE, 1) == 0        # without an add there is no ReLU either


@pytest.mark.parametrize("mode,relu", MODES)
def test_what_stays_declined(mode, relu):
    f32 = DTYPES["fp32"]
    assert plan((6, 64, 7, 7), f32, mode, relu) == 0 and plan((3, 520, 6, 5), f32, mode, relu) == 0      # fewer than 8 tiles
    assert plan((257, 64, 14, 14), f32, mode, relu) == 0                                               # N > 256
    assert plan((12, 16, 9, 7), f32, mode, relu, layout=_ffi.LAYOUT_NCHW) == 0
    assert plan((12, 16, 9, 7), f32, mode, relu, sn_training=0) == 0                                   # eval mode
    assert plan((12, 16, 9, 7), f32, mode, relu, cn_active=1) == 0                                     # CrossNorm
    assert plan((12, 16, 9, 7), f32, mode, relu, sn_two=1) == 0                                        # two gates


def test_argument_errors():
    lib = cnsn_amd.lib()
    p = problem((12, 16, 9, 7), DTYPES["fp32"], sn_active=1, sn_training=1)
    bad = epilogue(_ffi.ADD_POST, 1)
    bad.struct_bytes -= 4
    assert lib.cnsn_bn_block_plan(C.byref(p), C.byref(bad)) == E_STRUCT
    assert lib.cnsn_bn_block_plan(C.byref(p), C.byref(epilogue(7, 1))) == 0          # no such add mode: nothing to launch
    bn = _ffi.BnTail()
    bn.struct_bytes = C.sizeof(_ffi.BnTail)
    bn.training, bn.eps, bn.momentum = 1, 1e-5, 0.1
    skip = _ffi.BnTail()                                                             # (its pointers are never followed here)
    skip.struct_bytes = C.sizeof(_ffi.BnTail)
    skip.training, skip.eps, skip.momentum = 1, 1e-5, 0.1
    skip.weight = skip.bias = skip.running_mean = skip.running_var = 4096
    fwd = lambda e, skip: lib.cnsn_forward_bn_block(C.byref(p), C.byref(e), C.byref(bn), skip, None, None, None, None, None,  # noqa: E731
                                                    None, 0, None)
    # (grad_y .. d_bn_bias: ten missing pointers; the skip path's two gradient arrays are "there")
    bwd = lambda e, skip: lib.cnsn_backward_bn_block(C.byref(p), C.byref(e), C.byref(bn), skip, *([None] * 10), 4096, 4096,  # noqa: E731
                                                     None, 0, None)
    for call in (fwd, bwd):
        assert call(epilogue(_ffi.ADD_POST, 1), None) == E_NULL                      # a POST add without its addend
        assert call(epilogue(_ffi.ADD_NONE, 0), None) == E_NULL                      # (planned; the tensors are missing)
        assert call(epilogue(_ffi.ADD_NONE, 1), None) == _ffi.E_UNSUPPORTED
        # a BatchNorm2d on the skip path goes with the PRE add only — said before any pointer is looked at
        assert call(epilogue(_ffi.ADD_POST, 1, 4096), C.byref(skip)) == _ffi.E_UNSUPPORTED
        assert call(epilogue(_ffi.ADD_PRE, 1, 4096), C.byref(skip)) == E_NULL


def test_python_argument_errors():
    m = cnsn_amd.CNSN(None, cnsn_amd.SelfNorm(16)).train()
    bn = torch.nn.BatchNorm2d(16)
    x = torch.randn(4, 16, 5, 5)
    for kw in (dict(identity=None, add_mode="post"), dict(identity=None, add_mode="pre"), dict(identity=x, add_mode="none"),
               dict(identity=x, add_mode="sideways")):
        with pytest.raises(AssertionError):
            m.forward_bn_block(x, bn, kw["identity"], relu=False, add_mode=kw["add_mode"])
