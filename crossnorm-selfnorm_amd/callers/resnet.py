"""ResNet-50 (v1.5 bottlenecks: stride on the 3x3) with one CNSN unit per bottleneck — counterpart of
the reference's `models/imagenet/resnet_cnsn.py` (BottleneckCustom :37-124, ResNet :127-270,
resnet50 :309-323), same sub-module names / `state_dict` keys.

SelfNorm sites per forward at batch B, pos='post' (SURVEY.md §3.2): (B,256,56,56) x3, (B,512,28,28) x4,
(B,1024,14,14) x6, (B,2048,7,7) x3."""
import torch
import torch.nn as nn

from .. import functional as _F
from . import _sites
from ._sites import CrossNormSites, make_cnsn, residual_sum
from .bn_act import bn_act
from .ibn import IBN, InstanceNorm2d


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, impl, c_in, planes, stride, downsample, pos, beta, crop, cnsn_type, ibn=None):
        super().__init__()
        c_out = planes * self.expansion
        self.ibn = ibn                                 # the IBN-Net variant of callers/resnet_ibn.py (resnet_ibn_cnsn.py:49-87)
        self.conv1 = nn.Conv2d(c_in, planes, 1, bias=False)
        self.bn1 = IBN(planes) if ibn == "a" else nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, c_out, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(c_out)
        if ibn == "b":                                 # :63 — registered where the reference registers it (state_dict order)
            self.IN = InstanceNorm2d(c_out, affine=True)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        if ibn == "b" and pos == "post":               # the InstanceNorm2d takes the unit's place (:66-67)
            cnsn_type = None
        if cnsn_type is not None:                      # None: CrossNorm only in image space (:62)
            assert pos in ("residual", "pre", "post", "identity")
            self.cnsn = make_cnsn(impl, cnsn_type, crop, beta, c_in if pos == "pre" else c_out)   # :73-80
        self.pos = pos if cnsn_type is not None else None

    def forward(self, x):
        h = self.cnsn(x) if self.pos == "pre" else x
        h = self.conv1(h)
        # BatchNorm2d (IBN) + ReLU: one launch on channels-last tensors (callers/bn_act.py, IBN.forward_act)
        h = self.bn1.forward_act(h) if self.ibn == "a" else bn_act(self.bn1, h)
        h = bn_act(self.bn2, self.conv2(h))
        h = self.conv3(h)
        # :99-122.  pos='post': bn3 (and the downsample's BatchNorm2d), the add, the CNSN unit and the ReLU are ONE call when the
        # unit offers it (this library's `CNSN.forward_bn_block`: one launch per direction on channels-last tensors, the
        # un-fused sequence otherwise).  pos='residual': bn3, the unit, the add behind it and the ReLU (add_mode 'post'; IBN-b:
        # bn3 and the unit, add_mode 'none', in front of the InstanceNorm2d's own launch); the downsample's BatchNorm2d is a
        # `bn_act` launch of its own there (CNSN_BN_BLOCK=0: nn.BatchNorm2d as it is, like bn3).
        fb = None
        if _sites.FUSE_BLOCK and self.pos in ("post", "residual") and h.is_cuda:
            fb = getattr(getattr(self, "cnsn", None), "forward_bn_block", None)
        if self.ibn == "b":                            # resnet_ibn_cnsn.py:108-122: relu(IN(bn3(h) + identity))
            skip = x if self.downsample is None else self._skip(x, fb is not None and _F._BN_BLOCK)
            if fb is not None:                         # (pos='residual': at 'post' an IBN-b block has no unit)
                h = fb(h, self.bn3, None, relu=False, add_mode="none")
            else:
                h = self.bn3(h)
                if self.pos == "residual":
                    h = self.cnsn(h)
                elif self.pos == "identity":
                    skip = self.cnsn(skip)
            return self.IN.forward_act(h, skip, relu=True)
        if fb is not None and self.pos == "residual":
            return fb(h, self.bn3, x if self.downsample is None else self._skip(x, _F._BN_BLOCK), relu=True, add_mode="post")
        if fb is not None:
            if self.downsample is None:
                return fb(h, self.bn3, x, relu=True)
            if len(self.downsample) == 2 and isinstance(self.downsample[1], nn.BatchNorm2d):
                return fb(h, self.bn3, self.downsample[0](x), relu=True, identity_bn=self.downsample[1])
            return fb(h, self.bn3, self.downsample(x), relu=True)
        skip = x if self.downsample is None else self.downsample(x)
        if getattr(self, "cnsn", None) is None:        # no unit here: the plain end relu(bn3(h) + skip)
            return bn_act(self.bn3, h, skip)
        return residual_sum(self.cnsn, self.pos, self.bn3(h), skip, relu=True)

    def _skip(self, x, own_launch):
        """the downsample path; `own_launch`: a `Sequential(conv, BatchNorm2d)` runs its BatchNorm2d through `bn_act`"""
        down = self.downsample
        if own_launch and len(down) == 2 and isinstance(down[1], nn.BatchNorm2d):
            return bn_act(down[1], down[0](x), relu=False)
        return down(x)


class ResNet50CNSN(nn.Module, CrossNormSites):
    def __init__(self, num_classes=1000, layers=(3, 4, 6, 3), active_num=1, pos="post", beta=None, crop=None,
                 cnsn_type="sn", impl=None):
        super().__init__()
        if impl is None:
            from .. import cnsn as impl
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        kw = dict(pos=pos, beta=beta, crop=crop, cnsn_type=cnsn_type)
        c_in = 64
        for i, (planes, blocks) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            units = []
            for b in range(blocks):
                down = None
                if b == 0 and (stride != 1 or c_in != planes * 4):
                    down = nn.Sequential(nn.Conv2d(c_in, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
                units.append(_Bottleneck(impl, c_in, planes, stride if b == 0 else 1, down, **kw))
                c_in = planes * 4
            setattr(self, f"layer{i + 1}", nn.Sequential(*units))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(c_in, num_classes)
        for m in self.modules():                                   # initialisation as :182-187
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._collect_sites(impl, cnsn_type, active_num)

    def forward(self, x, aug=False):
        if aug:
            self._enable_cross_norm()
        x = self.maxpool(bn_act(self.bn1, self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))
