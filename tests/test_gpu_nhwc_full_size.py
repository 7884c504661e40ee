"""Full-size oracle parity of the channels-last single-launch kernels (csrc/cnsn_nhwc_fused_kernels.h) and of the fused
bottleneck tail (csrc/cnsn_nhwc_bnhead_kernels.h) at every ResNet-50 site of BASELINE.json's configs 3 and 4.

The small-shape files (test_gpu_nhwc.py, test_gpu_bn_block.py) cannot reach what only full-size inputs reach: the
non-temporal (`keep = 0`) instantiations, picked when the tensors a launch streams do not fit in 320 MiB; the kept-sum
forward with those policies; the tile loop with several tiles per workgroup and phase B with all 256 threads live (N = 256);
and the edge of the single-launch path itself (N = 256 takes it, N = 257 does not).

Discipline of test_gpu_full_size.check_case: the truth is the oracle's eager ops in float64 ON THE GPU on the same quantised
inputs, and the fp32 oracle prices the oracle's own noise.  With a ReLU the forward is compared against the oracle's own
ReLU (the masks may differ only inside the rounding band around zero, at a rate below 1e-2) and the gradients against the
oracle differentiated through the device's mask (test_gpu_fused_block.check).  Bars are north_star's for every output:
  fp32  |hip - truth64| <= max(1e-5 * scale, 2 * |oracle32 - truth64|)
  bf16  |hip - oracle32| <= 1e-2 * max|oracle32| (tensors), 1e-3 * max|oracle32| + 1e-5 (parameter gradients, running
        statistics)
Every case also asserts which kernels ran (`which_path` / `bn_block_plan` / the grad_fn, and the CNSN_DEBUG=1 line of each
single launch with its `keep` flag and status 0), that no cluster launch timed out and that nothing is degraded.  Every
comparison appends a row to the parity margins file of test_gpu_full_size._record (profiles/parity_table.py ->
profiles/r07_nhwc_parity_margins.md)."""
import contextlib
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import _ffi  # noqa: E402
from cnsn_amd import functional as F_  # noqa: E402
from oracle import cnsn_oracle as orc  # noqa: E402
from tests.golden.gen_golden_fill import fill_sn  # noqa: E402
from tests.test_gpu_bn_block import make_bn  # noqa: E402
from tests.test_gpu_full_size import R50, R50_96, _record, ids  # noqa: E402

DEV = torch.device("cuda:0")
CL = torch.channels_last
SHAPES = R50 + R50_96
DTYPES = [torch.bfloat16, torch.float32]
SN_SEED = 4

# ---- the host's cache-policy rule, re-stated (csrc/cnsn_nhwc_fused.hip): `keep` = 1 when the tensors a launch streams fit
# in 320 MiB.  The CNSN_DEBUG line of every launch is checked against it.
KEEP_BYTES = 320 << 20
# (a PRE add in front of a channels-last call keeps X = x + identity: its backward is the op's backward on X, add "none")
STREAMS = {"fused_fwd": lambda add, relu: 2 if add == "pre" else 1,
           "fused_bwd": lambda add, relu: 3 if (add == "pre" or (relu and add != "none")) else 2,
           "bn_fwd": lambda add, relu: 2,
           "bn_bwd": lambda add, relu: 3}


def keep_of(launch, shape, dtype, add="pre", relu=True):
    return int(STREAMS[launch](add, relu) * math.prod(shape) * torch.finfo(dtype).bits // 8 <= KEEP_BYTES)


# the matrix below reaches both instantiations of every launch whose policy depends on the shape
for _launch in ("bn_fwd", "bn_bwd"):
    assert {keep_of(_launch, s, d) for s in SHAPES for d in DTYPES} == {0, 1}, _launch
assert {keep_of("fused_bwd", s, d, "none", True) for s in SHAPES for d in DTYPES} == {0, 1}
assert {keep_of("fused_fwd", s, torch.float32, "none", False) for s in SHAPES} == {0, 1}

_LINE = re.compile(r"\[cnsn\] nhwc (single-launch|bn-block) (fwd|bwd): tiles=(\d+) \(S=(\d+) rows=(\d+) tcb=(\d+)\) groups=(\d+) "
                   r"keep=(\d) -> status (-?\d+)")


def launches(err):
    """the single-launch kernels' CNSN_DEBUG lines: {(family, direction): dict(keep, status, geometry)}"""
    out = {}
    for m in _LINE.finditer(err):
        key = (m.group(1), m.group(2))
        assert key not in out, f"two {key} launches in one case"
        out[key] = dict(tiles=int(m.group(3)), S=int(m.group(4)), rows=int(m.group(5)), tcb=int(m.group(6)),
                        groups=int(m.group(7)), keep=int(m.group(8)), status=int(m.group(9)))
    return out


@contextlib.contextmanager
def knobs(monkeypatch, **kv):
    """CNSN_* knobs for one case, re-read by the library and restored afterwards (test_kept_sum_gives_the_same_bits)"""
    for k, v in kv.items():
        monkeypatch.setenv(k, v)
    cnsn_amd.reload_env()
    try:
        yield
    finally:
        for k in kv:
            monkeypatch.delenv(k, raising=False)
        cnsn_amd.reload_env()


@contextlib.contextmanager
def healthy():
    """no cluster launch gives up inside the block, and nothing is degraded after it"""
    t0 = _ffi._timeout_count()
    yield
    torch.cuda.synchronize()
    assert _ffi._timeout_count() == t0, "a single-launch kernel timed out"
    assert cnsn_amd.lib().cnsn_resident_degraded() == 0


def rnd(t, dtype):
    """round to the activation dtype in the forward, identity in the backward (what storing a 16-bit tensor does)"""
    if dtype == torch.float32:
        return t
    return t + (t.detach().to(dtype).to(t.dtype) - t.detach())


def make_inputs(shape, dtype, seed, scale_b=0.7, edit=None):
    """edit(x, b): changes the drawn inputs in place before they are rounded to `dtype` (test_gpu_shift_sample.py)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n, c = shape[:2]
    x = torch.randn(shape, generator=g, device=DEV)
    x.mul_(torch.rand(n, c, 1, 1, generator=g, device=DEV) * 1.5 + 0.5).add_(torch.randn(n, c, 1, 1, generator=g, device=DEV))
    b = torch.randn(shape, generator=g, device=DEV).mul_(scale_b)
    gy = torch.randn(shape, generator=g, device=DEV)
    if edit is not None:
        edit(x, b)
    return x.to(dtype), b.to(dtype), gy.to(dtype)


class Checker:
    """north_star's bars; every comparison recorded next to its bound"""

    def __init__(self, shape, dtype, row):
        self.shape, self.dtype, self.row = shape, dtype, row

    def __call__(self, name, got, truth, ref32, param=False, keep=None, ref32u=None):
        """`ref32u` (16-bit fused bottleneck tail): the composition without the intermediate roundings — see bn_oracle"""
        got, truth, ref32 = got.double(), truth.double(), ref32.double()
        spread = float((ref32u.double() - ref32).abs().max()) if ref32u is not None else 0.0
        if self.dtype == torch.float32:
            scale = max(1.0, float(truth.abs().max()))
            err, noise = float((got - truth).abs().max()), float((ref32 - truth).abs().max())
            rel, bound = 1e-5, max(1e-5 * scale, 2 * noise)
        else:
            scale = max(float(ref32.abs().max()), 1e-6)
            err, noise = float((got - ref32).abs().max()), float((ref32 - truth).abs().max())
            if ref32u is not None:      # (the fused launch may sit nearer the un-rounded composition: bn_oracle)
                err = min(err, float((got - ref32u.double()).abs().max()))
            rel = 1e-3 if param else 1e-2
            bound = rel * scale + (1e-5 if param else 0.0)
            if param:                   # the two compositions' own spread, never above north_star's 1e-2
                bound = min(1e-2 * scale, max(bound, 2 * spread))
            if param and self.row["path"] == "unfused":
                # the N = 257 fall-back runs MIOpen's 16-bit BatchNorm2d, not this library's arithmetic: what is downstream of it
                # is held to north_star's 1e-2 (measured: bn.weight 5.2e-3, SelfNorm running mean 2.8e-3 of the scale)
                bound = 1e-2 * scale + 1e-5
        _record(dict(self.row, shape=list(self.shape), dtype=str(self.dtype).replace("torch.", "").replace("float32", "fp32"), out=name,
                     err=err, scale=scale, oracle32_noise=noise, bound=bound, rel_tol=rel, keep=keep, oracle32_on="gpu",
                     rounding_spread=spread))
        print(f"    {name}: err {err:.3e} bound {bound:.3e} (oracle32 noise {noise:.3e}, scale {scale:.3g})")
        assert err <= bound, f"{self.row} {self.shape} {self.dtype} {name}: err {err:.3e} > bound {bound:.3e} (oracle32 noise {noise:.3e}, scale {scale:.3g})"


def check_masks(hip_y, pre64, dtype, ctx):
    band = (1e-4 if dtype == torch.float32 else 3e-2) * max(1.0, float(pre64.abs().max()))
    differ = (hip_y > 0) != (pre64 > 0)
    assert not bool((differ & (pre64.abs() > band)).any()), f"{ctx}: ReLU mask differs away from zero"
    assert float(differ.double().mean()) < 1e-2, ctx


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# (a) CNSN.forward_block on channels-last tensors: SelfNorm alone, y = act(SelfNorm(x [+ identity]))
# ------------------------------------------------------------------------------------------------------------------------
def block_oracle(x, b, gy, dtype, mode, relu, mask):
    """float64 truth and fp32 oracle, ON THE GPU: pre-activation (the forward compared against the oracle's own ReLU) and the
    backward through `mask` (the device's)"""
    c = x.shape[1]
    out = {}
    for tag, odt in (("t64", torch.float64), ("o32", torch.float32)):
        sn = fill_sn(orc.SelfNorm(c), SN_SEED, torch.float32).to(odt).to(DEV).train()   # (the device's fp32 values)
        xr = x.detach().to(odt, copy=True).requires_grad_()
        br = b.detach().to(odt, copy=True).requires_grad_() if mode == "pre" else None
        h = rnd(xr + br, dtype) if mode == "pre" else xr          # (`out += identity` leaves a tensor of the activations' dtype)
        pre = sn(h)
        y = pre * mask.to(odt) if relu else pre
        y.backward(gy.to(odt))
        out[tag] = dict(pre=pre.detach(), dx=xr.grad, db=br.grad if br is not None else None,
                        pg={k: v.grad for k, v in sn.named_parameters()}, st=dict(sn.state_dict()))
        del xr, br, h, pre, y, sn
    return out


_case_cache = {}      # one case: its inputs and oracle results, shared by the strategies of that case when the masks agree


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _case_cache.clear()
    free()


def run_block(shape, dtype, mode, relu, fused, capfd, monkeypatch, edit=None):
    """edit(x, b): make_inputs' hook (the cached inputs and oracle results are the edit's own)"""
    seed = 1000 + shape[1] + shape[0] + (7 if mode == "pre" else 0)
    key = (tuple(shape), str(dtype), mode, relu, edit)
    if key not in _case_cache.get("key", ()):
        _case_cache.clear()
        free()
        _case_cache.update(key=(key,), inputs=make_inputs(shape, dtype, seed, edit=edit))
    x, b, gy = _case_cache["inputs"]
    n, c = shape[:2]
    with knobs(monkeypatch, CNSN_NHWC_FUSED=fused, CNSN_DEBUG="1"), healthy():
        mod = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(c), SN_SEED, torch.float32)).to(DEV).train()
        xg = x.clone(memory_format=CL).requires_grad_()
        bg = b.clone(memory_format=CL).requires_grad_() if mode == "pre" else None
        cfg = cnsn_amd.FusedConfig(add_mode=mode, relu=relu, **mod.selfnorm._fused_args_peek()[0])
        want = "resident" if (fused == "2" and n <= 256) else "streaming"
        path = "single-launch" if want == "resident" else "two-pass"
        assert cnsn_amd.which_path(xg, cfg) == want and cnsn_amd.which_path(xg, cfg, backward=True) == want, (shape, fused)
        capfd.readouterr()
        y = mod.forward_block(xg, bg, add_mode=mode, relu=relu)
        y.backward(gy.contiguous(memory_format=CL))
        torch.cuda.synchronize()
        seen = launches(capfd.readouterr().err)
    assert y.is_contiguous(memory_format=CL) and xg.grad.is_contiguous(memory_format=CL)
    if want == "resident":
        assert set(seen) == {("single-launch", "fwd"), ("single-launch", "bwd")}, seen
        assert all(v["status"] == 0 for v in seen.values()), seen
        assert seen["single-launch", "fwd"]["keep"] == keep_of("fused_fwd", shape, dtype, mode, relu)
        assert seen["single-launch", "bwd"]["keep"] == keep_of("fused_bwd", shape, dtype, "none", relu)     # (kept sum)
        kf = "sum" if mode == "pre" else seen["single-launch", "fwd"]["keep"]       # (the kept-sum forward has no cache-policy variants)
        kb = seen["single-launch", "bwd"]["keep"]
        geom = {k: seen["single-launch", "bwd"][k] for k in ("tiles", "S", "rows", "tcb")}
    else:
        assert not seen, seen
        kf = kb = geom = None
    hip = dict(y=y.detach(), dx=xg.grad, db=bg.grad if bg is not None else None,
               pg={k.split(".", 1)[1]: v.grad for k, v in mod.named_parameters()},
               st={k.split(".", 1)[1]: v for k, v in mod.state_dict().items()})
    del xg, bg, y
    mask = (hip["y"] > 0) if relu else None
    hit = "ref" in _case_cache and (mask is None or torch.equal(mask, _case_cache["mask"]))
    if not hit:
        _case_cache.pop("ref", None)
        free()
        _case_cache["ref"] = block_oracle(x, b, gy, dtype, mode, relu, mask)
        _case_cache["mask"] = mask
    ref = _case_cache["ref"]
    t64, o32 = ref["t64"], ref["o32"]
    ctx = (shape, str(dtype), mode, relu, path)
    one = Checker(shape, dtype, dict(kind="sn-block", crop=f"{mode}{'+relu' if relu else ''}", layout="nhwc", path=path,
                                     strategy=cnsn_amd.functional._strategy, geom=geom))
    act = torch.relu if relu else (lambda t: t)
    one("y", hip["y"], act(t64["pre"]), act(o32["pre"]), keep=kf)
    if relu:
        check_masks(hip["y"], t64["pre"], dtype, ctx)
    one("dx", hip["dx"], t64["dx"], o32["dx"], keep=kb)
    if mode == "pre":
        one("d_identity", hip["db"], t64["db"], o32["db"], keep=kb)
    for k in t64["pg"]:
        one(f"grad {k}", hip["pg"][k], t64["pg"][k], o32["pg"][k], param=True, keep=kb)
    for k in t64["st"]:
        if "num_batches" in k:
            assert int(hip["st"][k]) == int(t64["st"][k]) == 1, (ctx, k)
        else:
            one(f"state {k}", hip["st"][k], t64["st"][k], o32["st"][k], param=True, keep=kf)
    del hip, mask
    return seen     # (the launches' debug lines: test_gpu_nhwc_geometry.py checks their geometry)


@pytest.mark.parametrize("strategy", ["2", "0"], ids=["single-launch", "two-pass"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_block_full_size(shape, dtype, strategy, capfd, monkeypatch):
    """relu(SelfNorm(out + identity)) — what callers/resnet.py runs at a bottleneck when the tail is not fused — under both
    channels-last strategies (CNSN_NHWC_FUSED=2: the single launch, its kept-sum forward; =0: the two-pass kernels)"""
    run_block(shape, dtype, "pre", True, strategy, capfd, monkeypatch)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_block_full_size_no_epilogue(shape, capfd, monkeypatch):
    """SelfNorm alone without add or ReLU: the single launch's non-SUM forward with both cache policies, fp32"""
    run_block(shape, torch.float32, "none", False, "2", capfd, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------
# (b) CNSN.forward_bn_block: relu(SelfNorm(BatchNorm2d(conv_out) + identity | BatchNorm2d(skip conv)))
# ------------------------------------------------------------------------------------------------------------------------
class _Store(torch.autograd.Function):
    """a tensor stored in the activation dtype and its gradient stored the same way (the un-fused sequence hands both on)"""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def bn_oracle(conv, idt, gy, dtype, two, mask, seed, unfused=False):
    """torch.nn.BatchNorm2d + the oracle's SelfNorm in float64 and fp32 on the GPU.

    16-bit activations are rounded where the reference's block stores them (bn3's output, the in-place add, the downsample's
    output).  The fused launch rounds the element-wise X = T(T(bn3(c)) + b) the same way but takes every statistic from the
    un-rounded sums (cnsn_nhwc_bnhead_kernels.h, "Numerics"): it lies between the composition with those roundings ("o32",
    the truth) and the one without them ("o32u"), and the parameter gradients — sums whose terms cancel — move by up to a few
    1e-3 of their scale between the two (measured: 2.1e-3 of the scale for bn.weight at (256,2048,7,7) downsample, 3.3e-3
    at (9,64,7,7)).  `unfused`: the sequence's 16-bit gradient of the BatchNorm2d outputs as well (MIOpen reads it)."""
    c = conv.shape[1]
    out = {}
    lo = dtype != torch.float32
    for tag, odt, rounded in (("t64", torch.float64, True), ("o32", torch.float32, True), ("o32u", torch.float32, False)):
        if tag == "o32u" and not lo:
            continue
        bn = make_bn(c, seed, odt, DEV)
        bn2 = make_bn(c, seed + 50, odt, DEV) if two else None
        sn = fill_sn(orc.SelfNorm(c), seed, torch.float32).to(odt).to(DEV).train()
        ct, it = conv.detach().to(odt, copy=True).requires_grad_(), idt.detach().to(odt, copy=True).requires_grad_()
        if not (rounded and lo):
            r = rs = (lambda t: t)
        else:
            r = (lambda t: rnd(t, dtype))
            rs = (lambda t: _Store.apply(t, dtype)) if unfused else r
        pre = sn(r(rs(bn(ct)) + (rs(bn2(it)) if two else it)))
        y = pre * mask.to(odt)
        y.backward(gy.to(odt))
        mods = dict(bn=bn, sn=sn, **({"bn2": bn2} if two else {}))
        out[tag] = dict(pre=pre.detach(), dc=ct.grad, di=it.grad,
                        pg={f"{m}.{k}": v.grad for m, mod in mods.items() for k, v in mod.named_parameters()},
                        st={f"{m}.{k}": v for m, mod in mods.items() for k, v in mod.state_dict().items()})
        del ct, it, pre, y, mods, bn, bn2, sn
    return out


def run_bn_block(shape, dtype, two, capfd, monkeypatch, expect_fused=True, edit=None):
    """edit(conv, idt): make_inputs' hook"""
    seed = 2000 + shape[1] + shape[0] + (3 if two else 0)
    free()
    conv, idt, gy = make_inputs(shape, dtype, seed, scale_b=0.5, edit=edit)
    c = shape[1]
    path = "bn-block" if expect_fused else "unfused"
    with knobs(monkeypatch, CNSN_DEBUG="1"), healthy():
        bn = make_bn(c, seed, torch.float32, DEV)
        bn2 = make_bn(c, seed + 50, torch.float32, DEV) if two else None
        m = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(c), seed, torch.float32)).to(DEV).train()
        cg = conv.clone(memory_format=CL).requires_grad_()
        ig = idt.clone(memory_format=CL).requires_grad_()
        cfg = cnsn_amd.FusedConfig(add_mode="pre", relu=True, **m.selfnorm._fused_args_peek()[0])
        assert F_.bn_block_plan(cg, cfg) == expect_fused, (shape, dtype)
        capfd.readouterr()
        y = m.forward_bn_block(cg, bn, ig, relu=True, identity_bn=bn2)
        assert (type(y.grad_fn).__name__ == "FusedBnBlockBackward") == expect_fused, type(y.grad_fn).__name__
        y.backward(gy.contiguous(memory_format=CL))
        torch.cuda.synchronize()
        seen = launches(capfd.readouterr().err)
    assert y.is_contiguous(memory_format=CL) and cg.grad.is_contiguous(memory_format=CL)
    if expect_fused:
        assert set(seen) == {("bn-block", "fwd"), ("bn-block", "bwd")}, seen
        assert all(v["status"] == 0 for v in seen.values()), seen
        kf, kb = seen["bn-block", "fwd"]["keep"], seen["bn-block", "bwd"]["keep"]
        assert kf == keep_of("bn_fwd", shape, dtype) and kb == keep_of("bn_bwd", shape, dtype), (kf, kb)
        geom = {k: seen["bn-block", "bwd"][k] for k in ("tiles", "S", "rows", "tcb")}
    else:
        assert not any(f == "bn-block" for f, _ in seen), seen
        kf = kb = geom = None
    mods = dict(bn=bn, sn=m.selfnorm, **({"bn2": bn2} if two else {}))
    hip = dict(y=y.detach(), dc=cg.grad, di=ig.grad,
               pg={f"{k}.{n}": v.grad for k, mod in mods.items() for n, v in mod.named_parameters()},
               st={f"{k}.{n}": v for k, mod in mods.items() for n, v in mod.state_dict().items()})
    mask = hip["y"] > 0
    del cg, ig, y
    ref = bn_oracle(conv, idt, gy, dtype, two, mask, seed, unfused=not expect_fused)
    t64, o32, o32u = ref["t64"], ref["o32"], ref.get("o32u")
    ctx = (shape, str(dtype), two, path)
    one = Checker(shape, dtype, dict(kind="bn-block", crop="downsample" if two else "identity", layout="nhwc", path=path,
                                     strategy=cnsn_amd.functional._strategy, geom=geom))
    one("y", hip["y"], torch.relu(t64["pre"]), torch.relu(o32["pre"]), keep=kf,
        ref32u=None if o32u is None else torch.relu(o32u["pre"]))
    check_masks(hip["y"], t64["pre"], dtype, ctx)
    one("d_conv", hip["dc"], t64["dc"], o32["dc"], keep=kb, ref32u=None if o32u is None else o32u["dc"])
    one("d_identity", hip["di"], t64["di"], o32["di"], keep=kb, ref32u=None if o32u is None else o32u["di"])
    assert set(hip["pg"]) == set(t64["pg"]) and set(hip["st"]) == set(t64["st"])
    for k in t64["pg"]:
        one(f"grad {k}", hip["pg"][k], t64["pg"][k], o32["pg"][k], param=True, keep=kb,
            ref32u=None if o32u is None else o32u["pg"][k])
    for k in t64["st"]:
        if "num_batches" in k:
            assert int(hip["st"][k]) == int(t64["st"][k]) == 1, (ctx, k)
        else:
            one(f"state {k}", hip["st"][k], t64["st"][k], o32["st"][k], param=True, keep=kf,
                ref32u=None if o32u is None else o32u["st"][k])
    del ref, t64, o32, o32u, hip, mask, conv, idt, gy
    free()
    return seen


@pytest.mark.parametrize("two", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bn_block_full_size(shape, dtype, two, capfd, monkeypatch):
    run_bn_block(shape, dtype, two, capfd, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------
# (d) the edge of the single-launch path: N = 256 takes it (phase B: a thread per instance), N = 257 does not
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [256, 257])
def test_batch_edge_of_the_single_launch(n, dtype, capfd, monkeypatch):
    shape = (n, 256, 14, 14)
    x = torch.empty(shape, device=DEV, dtype=dtype).contiguous(memory_format=CL)
    cfg = cnsn_amd.FusedConfig(sn_active=True, add_mode="pre", relu=True)
    with knobs(monkeypatch, CNSN_NHWC_FUSED="2"):
        assert (cnsn_amd.which_path(x, cfg) == "resident") == (n <= 256)
    del x
    run_block(shape, dtype, "pre", True, "2", capfd, monkeypatch)             # (asserts the path: resident at 256, streaming at 257)
    run_bn_block(shape, dtype, True, capfd, monkeypatch, expect_fused=n <= 256)
    _case_cache.clear()
    free()
