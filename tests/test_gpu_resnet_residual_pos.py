"""The ResNet-50 callers at pos='residual' — the position the reference's best published model trains at
(imagenet-scripts/run-cnsn-augmix.sh: resnet50_ibn_b, cnsn_type=sn, pos=residual): every bottleneck's bn3 runs inside the
SelfNorm launch (`CNSN.forward_bn_block(.., add_mode="post")`; `add_mode="none"` in front of the IBN-b blocks' InstanceNorm2d),
16 `bn-block` launches per direction and step, none with the switch off (`functional._BN_BLOCK`, what CNSN_BN_BLOCK=0 sets);
against the same weights with the switch off by the method and bars of
tests/test_gpu_bn_block.py::test_resnet50_with_and_without_the_fused_tail: logits by value, gradients by direction.

The IBN model's head is `AvgPool2d(7)` (the reference's, for 224x224 inputs); on the 96x96 input of this file the last feature
map is 3x3, so the test swaps in an adaptive pool (no parameters: the `state_dict` is untouched)."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from cnsn_amd import functional as F_  # noqa: E402
from cnsn_amd.callers import ResNet50CNSN, ResNet50IBNCNSN  # noqa: E402
from tests.test_gpu_nhwc_full_size import healthy, knobs  # noqa: E402
from tests.test_gpu_parity import DEV  # noqa: E402

CL = torch.channels_last
_BN_BLOCK_LINE = re.compile(r"\[cnsn\] nhwc bn-block (fwd|bwd): .* -> status (-?\d+) mode=(pre|post|none)")


def plain():
    return ResNet50CNSN(num_classes=10, cnsn_type="sn", pos="residual")


def ibn_b():
    m = ResNet50IBNCNSN(ibn_cfg=("b", "b", None, None), num_classes=10, cnsn_type="sn", pos="residual")
    m.avgpool = torch.nn.AdaptiveAvgPool2d((1, 1))
    return m


def cos(u, v):
    return float(torch.nn.functional.cosine_similarity(u.flatten().double(), v.flatten().double(), dim=0))


@pytest.mark.parametrize("make,modes", [(plain, {"post": 16}), (ibn_b, {"post": 14, "none": 2})], ids=["resnet50", "resnet50_ibn_b"])
def test_residual_pos_with_and_without_the_fused_tail(make, modes, capfd, monkeypatch):
    torch.manual_seed(4)
    np.random.seed(4)
    a = make()
    keys = list(a.state_dict().keys())
    a = a.to(DEV).to(memory_format=CL).train()
    b = make().to(DEV)
    b.load_state_dict(a.state_dict())
    b = b.to(memory_format=CL).train()
    assert list(b.state_dict().keys()) == keys == list(a.state_dict().keys())
    x = torch.randn(6, 3, 96, 96, device=DEV).contiguous(memory_format=CL)
    yl = torch.randint(0, 10, (6,), device=DEV)
    old = F_._BN_BLOCK
    seen = {}
    try:
        with knobs(monkeypatch, CNSN_DEBUG="1"), healthy():
            for fused, model in ((True, a), (False, b)):
                F_._BN_BLOCK = fused
                capfd.readouterr()
                out = model(x)
                torch.nn.functional.cross_entropy(out, yl).backward()
                torch.cuda.synchronize()
                seen[fused] = (out.detach(), _BN_BLOCK_LINE.findall(capfd.readouterr().err))
    finally:
        F_._BN_BLOCK = old
    (la, lines), (lb, lines_off) = seen[True], seen[False]
    assert lines_off == [], lines_off
    assert all(st == "0" for _, st, _ in lines), lines
    for d in ("fwd", "bwd"):
        assert {m: sum(1 for dd, _, mm in lines if dd == d and mm == m) for m in modes} == modes, (d, lines)
    assert len(lines) == 32
    assert list(a.state_dict().keys()) == keys

    assert float((la - lb).abs().max()) <= 2e-3 * max(1.0, float(lb.abs().max()))
    assert cos(a.conv1.weight.grad, b.conv1.weight.grad) >= 0.995
    # (six images through 50 layers: rounding-sized differences of the statistics move a few ReLU masks — directions, not values)
    assert cos(a.layer3[2].bn3.weight.grad, b.layer3[2].bn3.weight.grad) >= 0.995
    assert cos(a.layer2[0].downsample[1].weight.grad, b.layer2[0].downsample[1].weight.grad) >= 0.995
    assert cos(a.layer2[0].downsample[0].weight.grad, b.layer2[0].downsample[0].weight.grad) >= 0.995
    assert cos(a.layer2[3].bn3.weight.grad, b.layer2[3].bn3.weight.grad) >= 0.995          # (IBN-b: the block with add_mode 'none')
    assert float((a.layer3[0].downsample[1].running_mean - b.layer3[0].downsample[1].running_mean).abs().max()) <= 1e-4
    assert cos(a.layer1[0].cnsn.selfnorm.g_fc.weight.grad, b.layer1[0].cnsn.selfnorm.g_fc.weight.grad) >= 0.99
    assert float((a.layer2[1].bn3.running_var - b.layer2[1].bn3.running_var).abs().max()) <= 1e-4
    assert int(a.layer4[2].bn3.num_batches_tracked) == int(b.layer4[2].bn3.num_batches_tracked) == 1
