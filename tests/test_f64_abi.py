"""The float64 entry points of the C ABI (cnsn_*_f64, CNSN_F64 = 3; additive, the ABI number stays) without a GPU: declared,
bound and exported; every argument error is answered with its documented status code before anything reaches the device
(fake aligned pointers: a call that got past validation would fault here); the old entry points still refuse dtype 3; the
CNSN_F64_NATIVE knob switches the Python route."""
import ctypes as C
import os
import re

import pytest
import torch

import cnsn_amd
from cnsn_amd import _ffi
from cnsn_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN, E_BOX, E_WORKSPACE, E_BATCH, E_STRUCT, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7, -8, -9
BIG = 1 << 30


def test_f64_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "cnsn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(cnsn_[a-z_0-9]+_f64)\s*\(", src)))
    assert names == sorted(_ffi.SIGNATURES_F64) and len(names) == 7
    handle = C.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f"libcnsn_hip.so lacks {n}"
    assert re.search(r"CNSN_F64 = 3\b", src) and re.search(r"#define CNSN_ABI_VERSION 9\b", src)
    assert _ffi.CNSN_F64 == 3 and _ffi.ABI_VERSION == 9 == cnsn_amd.lib().cnsn_abi_version()
    for struct in ("cnsn_f64_scalars", "cnsn_gate_f64", "cnsn_gate_grad_f64"):
        assert f"typedef struct {struct} " in src
    assert (C.sizeof(_ffi.F64Scalars), C.sizeof(_ffi.GateF64), C.sizeof(_ffi.GateGradF64)) == (48, 56, 32)
    for n in ("FusedCNSNF64", "PlaneStatsF64", "PlaneAffineF64", "f64_native"):
        assert hasattr(F, n)


def problem(**kw):
    p = _ffi.Problem()
    p.struct_bytes = C.sizeof(_ffi.Problem)
    p.dtype, p.N, p.C, p.H, p.W = _ffi.CNSN_F64, 8, 4, 16, 16
    p.content_box = _ffi.box4(None)
    p.style_box = _ffi.box4(None)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def scalars(**kw):
    s = _ffi.F64Scalars(C.sizeof(_ffi.F64Scalars), 0, 0.0, 1e-5, 1e-12, 1e-5, 0.1)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def gate(**kw):
    g = _ffi.GateF64(C.sizeof(_ffi.GateF64), 0, 16, 16, 16, 16, 16, None)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def gate_grad(**kw):
    g = _ffi.GateGradF64(C.sizeof(_ffi.GateGradF64), 0, 16, 16, 16)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def fwd(p, sc="default", x=16, perm=None, chan=None, g=None, f=None, y=32, saved=None, ws=48, ws_bytes=BIG):
    sc = scalars() if sc == "default" else sc
    ref = lambda s: C.byref(s) if s is not None else None    # noqa: E731
    return cnsn_amd.lib().cnsn_forward_f64(ref(p), ref(sc), x, perm, chan, ref(g), ref(f), y, saved, ws, ws_bytes, None)


def bwd(p, sc="default", gy=16, x=16, perm=None, chan=None, g=None, f=None, saved=16, dx=32, dg=None, df=None, ws=48,
        ws_bytes=BIG):
    sc = scalars() if sc == "default" else sc
    ref = lambda s: C.byref(s) if s is not None else None    # noqa: E731
    return cnsn_amd.lib().cnsn_backward_f64(ref(p), ref(sc), gy, x, perm, chan, ref(g), ref(f), saved, dx, ref(dg), ref(df), ws,
                                            ws_bytes, None)


def test_forward_backward_status_codes_without_gpu():
    lib = cnsn_amd.lib()
    p = problem(sn_active=1, sn_training=1)
    need = lib.cnsn_workspace_bytes_f64(C.byref(p))
    assert need > 0
    # all side arrays are doubles: 8*(6P + saved + 5P) forward, 8*(8 + 4 + 11)P backward
    assert need >= 8 * 23 * 32
    twin = problem(sn_active=1, sn_training=1, dtype=_ffi.CNSN_F32)
    assert lib.cnsn_saved_floats(C.byref(twin)) == 2 * (20 * 32 + 2 * 4)     # the common record: doubles, counted in floats
    assert lib.cnsn_saved_floats(C.byref(p)) == 0                            # (an old entry point: CNSN_F64 is refused)
    # NULL: problem, scalars, tensors, a gate the call needs, one of its arrays, the permutation of a CrossNorm call
    assert fwd(None) == E_NULL and bwd(None) == E_NULL
    assert fwd(p, sc=None, g=gate()) == E_NULL and bwd(p, sc=None, g=gate(), dg=gate_grad()) == E_NULL
    assert fwd(p, x=None, g=gate()) == E_NULL and fwd(p, y=None, g=gate()) == E_NULL and fwd(p, ws=None, g=gate()) == E_NULL
    assert fwd(p, g=None) == E_NULL and fwd(p, g=gate(bn_bias=None)) == E_NULL
    assert fwd(problem(sn_active=1, sn_two=1, sn_training=1), g=gate(), f=None) == E_NULL
    assert fwd(problem(cn_active=1), perm=None) == E_NULL
    assert bwd(p, g=gate(), dg=None) == E_NULL and bwd(p, g=gate(), dg=gate_grad(d_bn_weight=None)) == E_NULL
    assert bwd(p, g=gate(), dg=gate_grad(), saved=None) == E_NULL and bwd(p, g=gate(), dg=gate_grad(), gy=None) == E_NULL
    assert bwd(p, g=gate(), dg=gate_grad(), dx=None) == E_NULL
    # shape
    for shape in (dict(N=0), dict(C=0), dict(H=-1), dict(W=0)):
        assert fwd(problem(**shape)) == E_SHAPE and bwd(problem(**shape)) == E_SHAPE, shape
        assert lib.cnsn_workspace_bytes_f64(C.byref(problem(**shape))) == 0
    # dtype: only CNSN_F64
    for dt in (_ffi.CNSN_F32, _ffi.CNSN_BF16, _ffi.CNSN_F16, 7):
        assert fwd(problem(dtype=dt)) == E_DTYPE and bwd(problem(dtype=dt)) == E_DTYPE
        assert lib.cnsn_workspace_bytes_f64(C.byref(problem(dtype=dt))) == 0
    # 16-byte alignment of every activation pointer and the workspace
    q = problem()
    for k in ("x", "y", "ws"):
        assert fwd(q, **{k: 24}) == E_ALIGN, k
    for k in ("gy", "x", "dx", "ws"):
        assert bwd(q, **{k: 24}) == E_ALIGN, k
    # boxes: outside the plane, empty
    for box in ((0, 0, 17, 4), (3, 3, 3, 8), (0, 5, 4, 2)):
        assert fwd(problem(cn_active=1, content_box=_ffi.box4(box)), perm=16) == E_BOX, box
        assert bwd(problem(cn_active=1, style_box=_ffi.box4(box)), perm=16) == E_BOX, box
    # workspace one byte short
    assert fwd(p, g=gate(), ws_bytes=need - 1) == E_WORKSPACE
    assert bwd(p, g=gate(), dg=gate_grad(), ws_bytes=need - 1) == E_WORKSPACE
    # BatchNorm1d in training mode needs N > 1; eval mode takes N = 1 (validated up to the workspace)
    one = problem(N=1, sn_active=1, sn_training=1)
    assert fwd(one, g=gate()) == E_BATCH and bwd(one, g=gate(), dg=gate_grad()) == E_BATCH
    assert fwd(problem(N=1, sn_active=1, sn_training=0), g=gate(), ws_bytes=0) == E_WORKSPACE
    # struct sizes: the problem, the scalars, a gate, a gate gradient
    assert fwd(problem(struct_bytes=8)) == E_STRUCT and bwd(problem(struct_bytes=8)) == E_STRUCT
    assert lib.cnsn_workspace_bytes_f64(C.byref(problem(struct_bytes=8))) == 0
    assert fwd(q, sc=scalars(struct_bytes=40)) == E_STRUCT and bwd(q, sc=scalars(struct_bytes=40)) == E_STRUCT
    assert fwd(p, g=gate(struct_bytes=48)) == E_STRUCT
    assert bwd(p, g=gate(), dg=gate_grad(struct_bytes=24)) == E_STRUCT
    # channels-last is the caller's to convert
    cl = problem(layout=_ffi.LAYOUT_NHWC)
    assert fwd(cl) == E_UNSUPPORTED and bwd(cl) == E_UNSUPPORTED and lib.cnsn_workspace_bytes_f64(C.byref(cl)) == 0


def test_plane_primitives_status_codes_without_gpu():
    lib = cnsn_amd.lib()
    bad_box = _ffi.box4((0, 0, 5, 2))
    assert lib.cnsn_plane_stats_f64(None, 2, 2, 4, 4, None, 1e-5, 64, None) == E_NULL
    assert lib.cnsn_plane_stats_f64(16, 2, 2, 4, 4, None, 1e-5, None, None) == E_NULL
    assert lib.cnsn_plane_stats_f64(8, 2, 2, 4, 4, None, 1e-5, 64, None) == E_ALIGN
    assert lib.cnsn_plane_stats_f64(16, 0, 2, 4, 4, None, 1e-5, 64, None) == E_SHAPE
    assert lib.cnsn_plane_stats_f64(16, 2, 2, 4, 4, bad_box, 1e-5, 64, None) == E_BOX
    assert lib.cnsn_plane_stats_backward_f64(16, 2, 2, 4, 4, None, 16, 16, 16, None, 32, None) == E_NULL
    assert lib.cnsn_plane_stats_backward_f64(16, 2, 2, 4, 4, None, 16, 16, 16, 16, 40, None) == E_ALIGN
    assert lib.cnsn_plane_stats_backward_f64(16, 2, 2, 4, 4, bad_box, 16, 16, 16, 16, 32, None) == E_BOX
    assert lib.cnsn_plane_stats_backward_f64(16, 2, 2, 4, 0, None, 16, 16, 16, 16, 32, None) == E_SHAPE
    assert lib.cnsn_plane_affine_f64(16, 2, 2, 4, 4, None, 16, 32, None) == E_NULL
    assert lib.cnsn_plane_affine_f64(16, 2, 2, 4, 4, 16, 16, 24, None) == E_ALIGN
    assert lib.cnsn_plane_affine_f64(16, 2, -2, 4, 4, 16, 16, 32, None) == E_SHAPE
    assert lib.cnsn_plane_dot_f64(None, 16, 2, 2, 4, 4, 64, None) == E_NULL
    assert lib.cnsn_plane_dot_f64(16, 16, 2, 2, 4, 4, None, None) == E_NULL
    assert lib.cnsn_plane_dot_f64(24, 16, 2, 2, 4, 4, 64, None) == E_ALIGN
    assert lib.cnsn_plane_dot_f64(16, 16, 2, 2, 0, 4, 64, None) == E_SHAPE


def test_old_entry_points_still_refuse_dtype_3():
    lib = cnsn_amd.lib()
    p = problem()                                                            # dtype = CNSN_F64
    assert lib.cnsn_workspace_bytes(C.byref(p)) == 0 and lib.cnsn_saved_floats(C.byref(p)) == 0
    assert lib.cnsn_forward(C.byref(p), 16, None, None, None, None, 32, None, 48, BIG, None) == E_DTYPE
    assert lib.cnsn_backward(C.byref(p), 16, 16, None, None, None, None, 16, 32, None, None, 48, BIG, None) == E_DTYPE
    assert lib.cnsn_forward_fused(C.byref(p), None, 16, None, None, None, None, 32, None, 48, BIG, None) == E_DTYPE
    assert lib.cnsn_which_path(C.byref(p), None, 0, 0) == E_DTYPE
    assert lib.cnsn_plane_stats(16, 3, 2, 2, 4, 4, None, 1e-5, 64, None) == E_DTYPE
    assert lib.cnsn_plane_stats_backward(16, 3, 2, 2, 4, 4, None, 16, 16, 16, 16, 32, None) == E_DTYPE
    assert lib.cnsn_plane_affine(16, 3, 2, 2, 4, 4, 16, 16, 32, None) == E_DTYPE
    assert lib.cnsn_plane_dot(16, 16, 3, 2, 2, 4, 4, 64, None) == E_DTYPE


def test_knob_switches_the_route(monkeypatch):
    monkeypatch.delenv("CNSN_F64_NATIVE", raising=False)
    assert F.f64_native_enabled()
    x = torch.zeros(2, 2, 4, 4, dtype=torch.float64)
    assert not F.f64_native(x)                       # a CPU tensor is nobody's to compute ...
    with pytest.raises(cnsn_amd.CnsnError):          # ... and still raises
        cnsn_amd.calc_ins_mean_std(x)
    with pytest.raises(cnsn_amd.CnsnError):
        cnsn_amd.SelfNorm(2).double()(x)
    assert not F.f64_native(x.float()) and not F.f64_native(None)
    monkeypatch.setenv("CNSN_F64_NATIVE", "0")
    assert not F.f64_native_enabled() and not F.f64_native(x)
    monkeypatch.setenv("CNSN_F64_NATIVE", "1")
    assert F.f64_native_enabled()
