"""torch.autograd glue over the float64 entry points of the C ABI (cnsn_*_f64): siblings of `functional.FusedCNSN`,
`PlaneStats` and `PlaneAffine` for `double` tensors.  Elements, plane statistics, gate parameters, running statistics and
parameter gradients are float64 from the tensor to the result — nothing is rounded to float32 on the way.  Always the plain
streaming launches (no persistent grid, no context): what a `.double()` model, `torch.autograd.gradcheck` and a 1e-10 check
of the backward algebra need, not a training hot path."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _ffi
from . import functional as _F


def f64_native_enabled() -> bool:
    """CNSN_F64_NATIVE=0 restores the float-copy route (float64 in, float32 kernels, float64 out) for A/B runs; read at
    every call, so a test may flip it inside one process"""
    return os.environ.get("CNSN_F64_NATIVE", "1") != "0"


def f64_native(x) -> bool:
    """True when `x` is computed by the float64 kernels: a float64 tensor on the device, and the knob not 0"""
    return isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.is_cuda and f64_native_enabled()


def float_copy_is_channels_last(x: torch.Tensor, cfg, chan_perm) -> bool:
    """whether the float-copy route would compute this call where a channels-last `x` lies and return a channels-last
    result (`functional._nhwc_call` asked about `x.float()`): the native route computes on an NCHW copy, as the reference
    does, and hands the result back in that same memory format"""
    twin = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device="meta")   # shape, strides and element size decide
    return _F._nhwc_call(twin, cfg, chan_perm)


_F64 = (torch.float64,)


def _scalars(cfg) -> _ffi.F64Scalars:
    return _ffi.F64Scalars(C.sizeof(_ffi.F64Scalars), 0, 0.0 if cfg.lam is None else float(cfg.lam), float(cfg.eps_cn),
                           float(cfg.eps_sn), float(cfg.eps_bn), float(cfg.momentum))


def _problem(x, cfg) -> _ffi.Problem:
    """cnsn_problem_t of a float64 call (its float scalar fields are not read: `_scalars`)"""
    p = _F._problem_shape(x, cfg, _ffi.CNSN_F64)
    p.layout = _ffi.LAYOUT_NCHW
    return p


def _sizes(prob):
    """(floats of `saved`, bytes of workspace).  `saved` is the common record (doubles): its size is a function of N and C
    alone, asked with the float32 twin of the problem."""
    lib = _ffi.lib()
    twin = _ffi.Problem.from_buffer_copy(prob)
    twin.dtype = _ffi.CNSN_F32
    return lib.cnsn_saved_floats(C.byref(twin)), lib.cnsn_workspace_bytes_f64(C.byref(prob))


def _gate(w, gamma, beta, rm, rv, nbt, training):
    """a gate's tensors as the float64 kernels take them.  A float64 module (`SelfNorm.double()`) passes its parameters and
    buffers as they are; a float32 module passes double copies, and its running statistics are copied back — rounded to
    float32 — after a training-mode launch."""
    return _F._GateBuffers(w, gamma, beta, rm, rv, nbt, training, torch.float64, _ffi.GateF64)


def _gate_grad_views(c: int, dev):
    return _F._gate_grad_views(c, dev, 0, torch.float64, _ffi.GateGradF64)


class FusedCNSNF64(torch.autograd.Function):
    """y = SelfNorm(CrossNorm(x)) with either half optional, in float64 — cnsn_forward_f64 / cnsn_backward_f64."""

    @staticmethod
    @_F._on_device_of
    def forward(ctx, x, cfg, perm, chan_perm, g_w, g_gamma, g_beta, g_rm, g_rv, f_w, f_gamma, f_beta, f_rm, f_rv,
                g_nbt=None, f_nbt=None):
        _F._require_device(x, "cnsn_forward_f64", _F64)
        assert not cfg.has_epilogue, "the float64 path has no epilogue (CNSN.forward_block composes it)"
        lib = _ffi.lib()
        x = _F._dense(x)                         # NCHW copy of anything else, as the reference's .contiguous() (cnsn.py:14)
        dev = x.device
        prob, sc = _problem(x, cfg), _scalars(cfg)
        if cfg.cn_active:
            perm = _F._h2d.to_device(perm, dev)
            chan_perm = _F._h2d.to_device(chan_perm, dev) if chan_perm is not None else None
        else:
            perm = chan_perm = None
        gate_g = _gate(g_w, g_gamma, g_beta, g_rm, g_rv, g_nbt, cfg.sn_training) if cfg.sn_active else None
        gate_f = _gate(f_w, f_gamma, f_beta, f_rm, f_rv, f_nbt, cfg.sn_training) \
            if (cfg.sn_active and cfg.sn_two) else None
        y = torch.empty_like(x)
        need_bwd = any(ctx.needs_input_grad)
        saved_floats, ws_bytes = _sizes(prob)
        saved = torch.empty(saved_floats, dtype=torch.float32, device=dev) if need_bwd else None
        ws = _F._workspace(ws_bytes, dev)
        st = lib.cnsn_forward_f64(C.byref(prob), C.byref(sc), _F._ptr(x), _F._ptr(perm), _F._ptr(chan_perm),
                                  C.byref(gate_g.c) if gate_g else None, C.byref(gate_f.c) if gate_f else None, _F._ptr(y),
                                  _F._ptr(saved), _F._ptr(ws), ws_bytes, _F._stream(x))
        _ffi.check(st, "cnsn_forward_f64")
        if cfg.sn_active and cfg.sn_training:
            gate_g.write_back()
            if gate_f:
                gate_f.write_back()
        if need_bwd:
            ctx.cfg, ctx.prob, ctx.sc, ctx.ws_bytes = cfg, prob, sc, ws_bytes
            ctx.gates = (gate_g, gate_f)
            ctx.param_dtypes = tuple(t.dtype if t is not None else None for t in (g_w, g_gamma, g_beta, f_w, f_gamma, f_beta))
            ctx.save_for_backward(x, saved, perm, chan_perm)
        return y

    @staticmethod
    @_F._on_device_of
    def backward(ctx, gy):
        lib = _ffi.lib()
        x, saved, perm, chan_perm = ctx.saved_tensors
        cfg, prob, sc = ctx.cfg, ctx.prob, ctx.sc
        gate_g, gate_f = ctx.gates
        gy = _F._grad_like(gy, x, False)
        dev = x.device
        dx = torch.empty_like(x)
        ws = _F._workspace(ctx.ws_bytes, dev)
        gg = gf = gg_c = gf_c = None
        if cfg.sn_active:
            gg, gg_c = _gate_grad_views(x.shape[1], dev)
            if cfg.sn_two:
                gf, gf_c = _gate_grad_views(x.shape[1], dev)
        st = lib.cnsn_backward_f64(C.byref(prob), C.byref(sc), _F._ptr(gy), _F._ptr(x), _F._ptr(perm), _F._ptr(chan_perm),
                                   C.byref(gate_g.c) if gate_g else None, C.byref(gate_f.c) if gate_f else None,
                                   _F._ptr(saved), _F._ptr(dx), C.byref(gg_c) if gg_c else None,
                                   C.byref(gf_c) if gf_c else None, _F._ptr(ws), ctx.ws_bytes, _F._stream(x))
        _ffi.check(st, "cnsn_backward_f64")
        pd = ctx.param_dtypes
        out_g = [None] * 3 if gg is None else _F._cast_grads(gg, pd[:3])
        out_f = [None] * 3 if gf is None else _F._cast_grads(gf, pd[3:])
        #      x   cfg  perm  chan  g_w..g_beta   g_rm g_rv   f_w..f_beta  f_rm f_rv  g_nbt f_nbt
        return (dx, None, None, None, *out_g, None, None, *out_f, None, None, None, None)


def fused_cnsn_f64(x, cfg, perm=None, chan_perm=None, g=None, f=None):
    """`functional.fused_cnsn` for a float64 tensor; the result has the memory format the float-copy route gives it"""
    ga = (g.fc_weight, g.bn_weight, g.bn_bias, g.running_mean, g.running_var) if g else (None,) * 5
    fa = (f.fc_weight, f.bn_weight, f.bn_bias, f.running_mean, f.running_var) if f else (None,) * 5
    g_nbt = g.num_batches_tracked if (g and cfg.sn_training) else None
    f_nbt = f.num_batches_tracked if (f and cfg.sn_training) else None
    cl = x.is_cuda and float_copy_is_channels_last(x, cfg, chan_perm if cfg.cn_active else None)
    y = FusedCNSNF64.apply(x, cfg, perm, chan_perm, *ga, *fa, g_nbt, f_nbt)
    return y.contiguous(memory_format=torch.channels_last) if cl else y


class PlaneStatsF64(torch.autograd.Function):
    """(mean, std) of every plane in float64 — cnsn_plane_stats_f64 / cnsn_plane_stats_backward_f64."""

    @staticmethod
    @_F._on_device_of
    def forward(ctx, x, eps, box):
        return _F._plane_stats_forward(ctx, x, eps, box, True)

    @staticmethod
    @_F._on_device_of
    def backward(ctx, gmean, gstd):
        return _F._plane_stats_backward(ctx, gmean, gstd, True), None, None


class PlaneAffineF64(torch.autograd.Function):
    """y = scale[n,c]*x + shift[n,c] in float64 — cnsn_plane_affine_f64 (+ cnsn_plane_dot_f64 for the backward)."""

    @staticmethod
    @_F._on_device_of
    def forward(ctx, x, scale, shift):
        return _F._plane_affine_forward(ctx, x, scale, shift, True)

    @staticmethod
    @_F._on_device_of
    def backward(ctx, gy):
        return _F._plane_affine_backward(ctx, gy, True)
