"""The float64 path on the device (cnsn_*_f64 -> functional.FusedCNSNF64 / PlaneStatsF64 / PlaneAffineF64 -> cnsn.py) against autograd
through the op-for-op oracle in float64 on the CPU.

Bar: rtol = 1e-10, atol = 1e-11 — that of tests/test_closed_form.py, the project's statement of what two float64 evaluations of
this op agree to (over that file's matrix the closed form and autograd differ by at most 0.09 of it, so the oracle's own noise
leaves a factor above ten).  Every comparison prints its largest err / (atol + rtol*|ref|) before it asserts; the module's
summary of those ratios (and, with CNSN_F64_REPORT=<file>, a JSON copy) is what profiles/r11_f64.md quotes.

Every case asserts `f64_native(x)` first: a silent fall-back to the float-copy route cannot pass."""
import itertools
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, executed only with -m gpu on the box
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import functional as F  # noqa: E402
from oracle import cnsn_oracle as orc  # noqa: E402

DEV = torch.device("cuda:0")
RTOL, ATOL = 1e-10, 1e-11
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    for k in sorted(RATIOS):
        print(f"[f64 ratio] {k[0]:<10} {k[1]:<14} {RATIOS[k]:.3e}")
    path = os.environ.get("CNSN_F64_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{a}/{b}": v for (a, b), v in RATIOS.items()}, fh, indent=1, sort_keys=True)


def ratio(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def close(got, ref, group, name, what=""):
    r = ratio(got, ref)
    print(f"{group} {name} {what}: err / (atol + rtol*|ref|) = {r:.3e}")
    RATIOS[(group, name)] = max(RATIOS.get((group, name), 0.0), r)
    assert r <= 1.0, f"{name} {what}: {r:.3e} of the bar rtol={RTOL}, atol={ATOL}"


# ---- inputs: those of tests/test_closed_form.py
def seed_of(*a):
    return zlib.crc32(repr(a).encode()) % 100000


def cond_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, c = shape[:2]
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    s = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) * 1.5 + 0.5
    m = torch.randn(n, c, 1, 1, generator=g, dtype=torch.float64)
    return x * s + m


def make_sn(C, is_two, seed):
    g = torch.Generator().manual_seed(seed)

    def branch():
        return dict(w=(torch.rand(C, 2, generator=g, dtype=torch.float64) * 1.4 - 0.7).requires_grad_(),
                    gamma=(torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(),
                    beta=(torch.rand(C, generator=g, dtype=torch.float64) - 0.5).requires_grad_(),
                    run_mean=torch.rand(C, generator=g, dtype=torch.float64) - 0.5,
                    run_var=torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    sn = branch()
    sn["f"] = branch() if is_two else None
    return sn


MODES = list(itertools.product(orc.CROPS, (False, True), (None, 0.3), ("cn", "sn", "cnsn"), (False, True), (True, False)))


def truth(x, G, d, sn, kind, crop, lam, chan, is_two, training):
    """autograd through the oracle, float64, CPU: y, dx, the gates' gradients, their running statistics after the call"""
    x = x.clone().requires_grad_()
    u = x
    if kind != "sn":
        u = orc.cn_op_2ins_space_chan(u, crop=crop, lam=lam, chan=chan, draws=d)
    y = u
    out, params = {}, []
    if sn is not None:
        rm, rv = sn["run_mean"].clone(), sn["run_var"].clone()
        fp = None
        if is_two:
            f = sn["f"]
            frm, frv = f["run_mean"].clone(), f["run_var"].clone()
            fp = (f["w"].view(-1, 1, 2), f["gamma"], f["beta"], frm, frv)
            out.update(f_rm=frm, f_rv=frv)
        y = orc.selfnorm_forward(u, sn["w"].view(-1, 1, 2), sn["gamma"], sn["beta"], rm, rv, training=training, f_params=fp)
        out.update(g_rm=rm, g_rv=rv)
        params = [sn["w"], sn["gamma"], sn["beta"]] + ([sn["f"]["w"], sn["f"]["gamma"], sn["f"]["beta"]] if is_two else [])
    grads = torch.autograd.grad(y, [x] + params, G)
    out.update(y=y.detach(), dx=grads[0])
    for k, g in zip(("g_dw", "g_dgamma", "g_dbeta", "f_dw", "f_dgamma", "f_dbeta"), grads[1:]):
        out[k] = g
    return out


def device_gate(b):
    leaf = lambda t: t.detach().clone().to(DEV).requires_grad_()    # noqa: E731
    return F.GateParams(leaf(b["w"].view(-1, 1, 2)), leaf(b["gamma"]), leaf(b["beta"]), b["run_mean"].clone().to(DEV),
                        b["run_var"].clone().to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))


def native(x, G, d, sn, kind, lam, is_two, training):
    """the same call through functional.fused_cnsn on the device"""
    xg = x.clone().to(DEV).requires_grad_()
    assert F.f64_native(xg)
    cfg = F.FusedConfig(cn_active=kind != "sn", content_box=d.content_box if kind != "sn" else None,
                        style_box=d.style_box if kind != "sn" else None, lam=lam if kind != "sn" else None,
                        sn_active=sn is not None, sn_two=bool(sn is not None and is_two), sn_training=training)
    g = device_gate(sn) if sn is not None else None
    f = device_gate(sn["f"]) if (sn is not None and is_two) else None
    y = F.fused_cnsn(xg, cfg, perm=d.perm if kind != "sn" else None, chan_perm=d.chan_perm if kind != "sn" else None, g=g, f=f)
    assert y.dtype == torch.float64 and y.grad_fn is not None and type(y.grad_fn).__name__.startswith("FusedCNSNF64")
    y.backward(G.to(DEV))
    torch.cuda.synchronize()
    out = dict(y=y.detach(), dx=xg.grad)
    for tag, gate in (("g", g), ("f", f)):
        if gate is not None:
            out.update({f"{tag}_dw": gate.fc_weight.grad.view(-1, 2), f"{tag}_dgamma": gate.bn_weight.grad,
                        f"{tag}_dbeta": gate.bn_bias.grad, f"{tag}_rm": gate.running_mean, f"{tag}_rv": gate.running_var,
                        f"{tag}_nbt": int(gate.num_batches_tracked)})
    return out


def check_case(group, x, G, d, sn, kind, crop, lam, chan, is_two, training, what=""):
    want = truth(x, G, d, sn, kind, crop, lam, chan, is_two, training)
    got = native(x, G, d, sn, kind, lam, is_two, training)
    for k in sorted(want):
        close(got[k], want[k], group, k, what)
        assert got[k].dtype == torch.float64
    for tag in (("g", "f") if (sn is not None and is_two) else ("g",) if sn is not None else ()):
        assert got[f"{tag}_nbt"] == (1 if training else 0), (tag, got[f"{tag}_nbt"])     # counted in the launch, training only
        if not training:                                                                 # eval writes nothing back
            src = sn if tag == "g" else sn["f"]
            assert torch.equal(got[f"{tag}_rm"].cpu(), src["run_mean"]) and torch.equal(got[f"{tag}_rv"].cpu(), src["run_var"])


# ---- 1. every mode against autograd
@pytest.mark.parametrize("crop,chan,lam,kind,is_two,training", MODES)
def test_every_mode_matches_autograd(crop, chan, lam, kind, is_two, training):
    if kind == "sn" and (crop != "neither" or chan or lam is not None):
        pytest.skip("CN options irrelevant for SN only")
    if kind == "cn" and (is_two or not training):
        pytest.skip("SN options irrelevant for CN only")
    shape = (6, 5, 9, 11)
    seed = seed_of(crop, chan, lam, kind, is_two, training)
    torch.manual_seed(seed)
    np.random.seed(seed)
    x = cond_input(shape, seed)
    G = torch.randn(shape, dtype=torch.float64)
    d = orc.draw_cn(shape, crop, beta=1, chan=chan)
    sn = make_sn(shape[1], is_two, seed + 1) if kind != "cn" else None
    check_case("modes:" + kind, x, G, d, sn, kind, crop, lam, chan, is_two, training, f"{crop} chan={chan} lam={lam}")


# ---- 2. the bar discriminates: the float-copy route (CNSN_F64_NATIVE=0) misses it, the native route through the same modules holds it
def module_case(kind, is_two):
    shape, crop = (6, 5, 9, 11), ("both" if kind == "cnsn" else "neither")
    seed = seed_of(crop, False, None, kind, is_two, True)
    torch.manual_seed(seed)
    np.random.seed(seed)
    x = cond_input(shape, seed)
    d = orc.draw_cn(shape, crop, beta=1)
    sn = make_sn(shape[1], is_two, seed + 1)
    want = truth(x, torch.ones(shape, dtype=torch.float64), d, sn, kind, crop, None, False, is_two, True)["y"]

    def run():
        mod = cnsn_amd.SelfNorm(shape[1], is_two=is_two).double()
        with torch.no_grad():
            for fc, bn, b in ((mod.g_fc, mod.g_bn, sn),) + (((mod.f_fc, mod.f_bn, sn["f"]),) if is_two else ()):
                fc.weight.copy_(b["w"].view(-1, 1, 2))
                bn.weight.copy_(b["gamma"])
                bn.bias.copy_(b["beta"])
                bn.running_mean.copy_(b["run_mean"])
                bn.running_var.copy_(b["run_var"])
        top = cnsn_amd.CNSN(cnsn_amd.CrossNorm("both", 1) if kind == "cnsn" else None, mod).to(DEV).train()
        if kind == "cnsn":
            top.crossnorm.active = True
            top.crossnorm.next_draws = cnsn_amd.CNDraws(d.perm, d.style_box, None, d.content_box)
        with torch.no_grad():
            y = top(x.to(DEV))
        torch.cuda.synchronize()
        return y
    return run, want


@pytest.mark.parametrize("kind,is_two", [("sn", False), ("cnsn", True)])
def test_float_copy_route_misses_the_bar(kind, is_two, monkeypatch):
    run, want = module_case(kind, is_two)
    monkeypatch.delenv("CNSN_F64_NATIVE", raising=False)
    assert F.f64_native(torch.empty(1, dtype=torch.float64, device=DEV))
    close(run(), want, "modules", "y", f"{kind} native")
    monkeypatch.setenv("CNSN_F64_NATIVE", "0")
    assert not F.f64_native(torch.empty(1, dtype=torch.float64, device=DEV))
    y32 = run()
    r = ratio(y32, want)
    print(f"float-copy route, {kind}: y at {r:.3e} of the bar")
    assert y32.dtype == torch.float64 and r > 1.0, "the float32 kernels cannot hold a float64 bar: is the knob read?"


# ---- 3. geometry: every instantiation and tail of the tensor passes.  Lanes per plane by the number of 16-byte vectors
# (csrc/cnsn_host_plan.h::pick_shape): <= 32 -> 16, <= 4096 -> 64, above -> the whole block; VEC = 2 on even planes (rows, with boxes)
def geometry_case(shape, kind, is_two, training, cbox=None, sbox=None, lam=None, chan=False):
    seed = seed_of(shape, kind, is_two, training, cbox, sbox, lam, chan)
    gen = torch.Generator().manual_seed(seed)
    x = cond_input(shape, seed)
    G = torch.randn(shape, generator=gen, dtype=torch.float64)
    d = orc.CNDraws(perm=torch.randperm(shape[0], generator=gen), style_box=sbox,
                    chan_perm=torch.randperm(shape[1], generator=gen) if chan else None, content_box=cbox)
    crop = {(False, False): "neither", (False, True): "style", (True, False): "content", (True, True): "both"}[
        (cbox is not None, sbox is not None)]
    sn = make_sn(shape[1], is_two, seed + 1) if kind != "cn" else None
    check_case("geometry", x, G, d, sn, kind, crop, lam, chan, is_two, training, f"{shape} c={cbox} s={sbox}")


@pytest.mark.parametrize("shape", [(3, 2, 7, 7),        # odd plane: VEC = 1, 49 vectors on 64 lanes
                                   (2, 3, 5, 6),        # 15 vectors on 16 lanes
                                   (2, 2, 33, 34),      # 561 vectors on 64 lanes: the unrolled loop and its tail
                                   (2, 1, 64, 66),      # 2112 vectors: 33 per lane of a wave
                                   (2, 1, 96, 98),      # 4704 vectors: the whole block per plane, sums through LDS
                                   (2, 1, 95, 99),      # the same with VEC = 1 (9405 vectors)
                                   (5, 3, 4, 4)],       # 15 planes of 16 lanes: the last block is one plane short
                         ids=str)
def test_unboxed_geometry(shape):
    geometry_case(shape, "cnsn", True, True, chan=shape[1] > 1)
    geometry_case(shape, "sn", False, False)


def test_batch_beyond_one_workgroup_step():
    """N = 257: the smallest batch at which a thread of the double mid kernels (one workgroup of 256 threads per channel)
    takes a second step through its instances"""
    geometry_case((257, 2, 2, 3), "cnsn", True, True, chan=True)
    geometry_case((257, 2, 2, 3), "sn", False, True)


def test_single_instance():
    geometry_case((1, 3, 6, 8), "sn", True, False)      # N = 1: eval mode only (BatchNorm1d needs two values per channel)
    geometry_case((1, 3, 6, 8), "cn", False, True, lam=0.3)
    x = torch.zeros(1, 3, 6, 8, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):                     # CNSN_E_BATCH, as nn.BatchNorm1d raises
        cnsn_amd.SelfNorm(3).double().to(DEV).train()(x)


def boxes_of(H, W):
    return dict(top_left=(0, 0, 3, 4), bottom_right=(H - 3, W - 4, H, W), row=(2, 1, 3, W - 1), column=(1, 3, H - 1, 4),
                whole=(0, 0, H, W), inner=(1, 1, H - 2, W - 2))


@pytest.mark.parametrize("hw", [(7, 9), (8, 10)], ids=["odd-W", "even-W"])
@pytest.mark.parametrize("cb,sb", [("top_left", "bottom_right"), ("bottom_right", "top_left"), ("row", "column"),
                                   ("column", "row"), ("whole", "inner"), ("inner", "whole"), ("row", None), (None, "column")])
def test_boxed_geometry(hw, cb, sb):
    b = boxes_of(*hw)
    geometry_case((3, 2) + hw, "cnsn", cb == "row", True, cbox=b.get(cb), sbox=b.get(sb), lam=0.3 if sb == "row" else None)


def test_boxed_geometry_on_larger_planes():
    geometry_case((2, 2, 33, 34), "cnsn", False, True, cbox=(5, 3, 30, 31), sbox=(0, 0, 10, 34), chan=True)   # 64 lanes, VEC 2
    geometry_case((2, 1, 95, 99), "cn", False, True, cbox=(0, 1, 95, 98), sbox=(94, 0, 95, 99))              # whole block, VEC 1


# ---- 4. torch.autograd.gradcheck with torch's defaults for double (eps 1e-6, atol 1e-5, rtol 1e-3)
GC_SHAPE = (4, 3, 6, 8)
GC_BOXES = dict(neither=(None, None), style=(None, (1, 2, 5, 7)), content=((0, 1, 4, 6), None), both=((2, 0, 6, 5), (1, 2, 5, 7)))


def gc_input(seed, shape=GC_SHAPE):
    x = cond_input(shape, seed).to(DEV).requires_grad_()
    assert F.f64_native(x)
    return x


def gc_draws(crop, chan=False):
    gen = torch.Generator().manual_seed(7)
    cb, sb = GC_BOXES[crop]
    return cnsn_amd.CNDraws(torch.randperm(GC_SHAPE[0], generator=gen), sb, torch.randperm(GC_SHAPE[1], generator=gen) if chan else None,
                            cb)


@pytest.mark.parametrize("crop,lam,chan", [("neither", None, False), ("style", None, False), ("content", None, False),
                                           ("both", None, False), ("both", 0.3, False), ("style", None, True)])
def test_gradcheck_crossnorm(crop, lam, chan):
    d = gc_draws(crop, chan)
    assert torch.autograd.gradcheck(lambda t: cnsn_amd.cn_op_2ins_space_chan(t, crop=crop, lam=lam, chan=chan, draws=d),
                                    (gc_input(1),))


def test_gradcheck_plane_functions():
    assert torch.autograd.gradcheck(cnsn_amd.calc_ins_mean_std, (gc_input(2),))
    assert torch.autograd.gradcheck(cnsn_amd.instance_norm_mix, (gc_input(3), gc_input(4, (4, 3, 5, 7))))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("is_two", [False, True], ids=["one-gate", "two-gates"])
def test_gradcheck_selfnorm(training, is_two):
    from tests.golden.gen_golden_fill import fill_sn
    sn = fill_sn(cnsn_amd.SelfNorm(GC_SHAPE[1], is_two=is_two), 5, torch.float64).to(DEV).train(training)
    # (the running statistics drift during the check; training-mode outputs do not read them)
    assert torch.autograd.gradcheck(sn, (gc_input(5),))


def test_gradcheck_cnsn_functional():
    from tests.golden.gen_golden_fill import fill_sn
    sn = fill_sn(cnsn_amd.SelfNorm(GC_SHAPE[1]), 6, torch.float64).to(DEV).train()
    d = gc_draws("both")
    cfg = F.FusedConfig(cn_active=True, content_box=d.content_box, style_box=d.style_box, sn_active=True, sn_training=True)
    leaf = lambda t: t.detach().clone().requires_grad_()    # noqa: E731
    w, gamma, beta = leaf(sn.g_fc.weight), leaf(sn.g_bn.weight), leaf(sn.g_bn.bias)

    def fn(t, w, gamma, beta):
        g = F.GateParams(w, gamma, beta, sn.g_bn.running_mean, sn.g_bn.running_var, None)
        return F.fused_cnsn(t, cfg, perm=d.perm, g=g)
    assert torch.autograd.gradcheck(fn, (gc_input(6), w, gamma, beta))     # the gate's parameters too


# ---- 5. module surface
def test_double_module_keeps_float64_everywhere():
    from tests.golden.gen_golden_fill import fill_sn
    sn = fill_sn(cnsn_amd.SelfNorm(5, is_two=True), 3, torch.float64).to(DEV).train()
    x = cond_input((4, 5, 6, 7), 11).to(DEV).requires_grad_()
    assert F.f64_native(x)
    y = sn(x)
    y.sum().backward()
    for k, v in sn.state_dict().items():
        assert v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float64), k
    assert all(p.dtype == torch.float64 and p.grad is not None and p.grad.dtype == torch.float64 for p in sn.parameters())
    assert int(sn.g_bn.num_batches_tracked) == 1 == int(sn.f_bn.num_batches_tracked)
    assert y.dtype == x.grad.dtype == torch.float64


def test_float32_module_on_float64_input():
    """parameters travel as double copies: y and dx at the bar against the oracle given the same fp32-valued parameters in double;
    parameter gradients come back as float32, one rounding from the truth; the running statistics are copied back rounded"""
    from tests.golden.gen_golden_fill import fill_sn
    shape = (6, 5, 9, 11)
    sn = fill_sn(cnsn_amd.SelfNorm(shape[1], is_two=True), 4, torch.float32).to(DEV).train()
    ref = fill_sn(orc.SelfNorm(shape[1], is_two=True), 4, torch.float32).double().train()      # fp32 VALUES, held in double
    x64, G = cond_input(shape, 12), torch.randn(shape, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    xr = x64.clone().requires_grad_()
    yr = ref(xr)
    yr.backward(G)
    xg = x64.to(DEV).requires_grad_()
    assert F.f64_native(xg)
    y = sn(xg)
    y.backward(G.to(DEV))
    close(y, yr, "modules", "y", "fp32 module")
    close(xg.grad, xr.grad, "modules", "dx", "fp32 module")
    for (n, p), q in zip(sn.named_parameters(), ref.parameters()):
        assert p.grad.dtype == torch.float32 == p.dtype, n
        err = (p.grad.cpu().double() - q.grad).abs()
        print(f"fp32 module {n}.grad: err / (2^-23*|ref| + 1e-11) = {float((err / (2.0 ** -23 * q.grad.abs() + 1e-11)).max()):.3e}")
        assert bool((err <= 2.0 ** -23 * q.grad.abs() + 1e-11).all()), (n, float(err.max()))
    for bn, bo in ((sn.g_bn, ref.g_bn), (sn.f_bn, ref.f_bn)):
        assert int(bn.num_batches_tracked) == 1
        for name in ("running_mean", "running_var"):
            got, want = getattr(bn, name), getattr(bo, name)
            assert got.dtype == torch.float32
            assert bool(((got.cpu().double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-11).all()), name


@pytest.mark.parametrize("add_mode", ["pre", "post"])
def test_forward_block_in_float64(add_mode):
    from tests.golden.gen_golden_fill import fill_sn
    shape = (6, 5, 9, 11)
    top = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(shape[1]), 8, torch.float64)).to(DEV).train()
    ref = fill_sn(orc.SelfNorm(shape[1]), 8, torch.float64).train()
    x64, a64 = cond_input(shape, 14), cond_input(shape, 15)
    G = torch.randn(shape, generator=torch.Generator().manual_seed(16), dtype=torch.float64)
    xr, ar = x64.clone().requires_grad_(), a64.clone().requires_grad_()
    yr = torch.relu(ref(xr + ar)) if add_mode == "pre" else torch.relu(ref(xr) + ar)
    yr.backward(G)
    xg, ag = x64.to(DEV).requires_grad_(), a64.to(DEV).requires_grad_()
    assert F.f64_native(xg)
    y = top.forward_block(xg, ag, add_mode=add_mode, relu=True)
    y.backward(G.to(DEV))
    close(y, yr, "modules", "y", f"forward_block {add_mode}")
    close(xg.grad, xr.grad, "modules", "dx", f"forward_block {add_mode}")
    close(ag.grad, ar.grad, "modules", "dx", f"forward_block {add_mode} addend")
    for p, q in zip(top.selfnorm.parameters(), ref.parameters()):
        close(p.grad, q.grad, "modules", "g_dw", f"forward_block {add_mode} parameters")


def test_channels_last_input_and_repeatability():
    from tests.golden.gen_golden_fill import fill_sn
    shape = (4, 8, 6, 7)                                   # C a multiple of 4: the float-copy route answers in channels-last
    sn = fill_sn(cnsn_amd.SelfNorm(shape[1]), 9, torch.float64).to(DEV).eval()
    x = cond_input(shape, 17).to(DEV)
    xcl = x.contiguous(memory_format=torch.channels_last)
    assert F.f64_native(xcl) and not xcl.is_contiguous()
    with torch.no_grad():
        y, ycl, again = sn(x), sn(xcl), sn(x)
    assert torch.equal(y, ycl) and torch.equal(y, again)   # bit for bit: computed on the NCHW copy; no state between launches
    assert ycl.is_contiguous(memory_format=torch.channels_last) and y.is_contiguous()
    d = cnsn_amd.CNDraws(torch.tensor([2, 0, 3, 1]), (1, 1, 5, 6), None, (0, 2, 4, 7))
    z = [cnsn_amd.cn_op_2ins_space_chan(t, crop="both", draws=d) for t in (x, xcl, x)]
    assert torch.equal(z[0], z[1]) and torch.equal(z[0], z[2]) and z[1].is_contiguous()     # (boxes: NCHW out, as the float-copy route)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    sn.train()
    for t in (xa, xb):
        sn(t).square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
