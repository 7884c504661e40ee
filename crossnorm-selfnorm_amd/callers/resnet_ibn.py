"""ResNet-50-IBN-a / -b with one CNSN unit per bottleneck — counterpart of the reference's
`models/imagenet/resnet_ibn_cnsn.py` (ResNet :127-240, resnet50_ibn_a :243-258, resnet50_ibn_b :291-306), the backbone of
its best published model (README: ResNet-50 + CNSN + IBN + AugMix), selected by `imagenet.py --model resnet50_ibn_a |
resnet50_ibn_b` (:509-512).  Same sub-module names, `state_dict` keys and key order; the bottleneck is resnet.py's with
its `ibn` argument.

IBN sites at batch N (224x224): IBN-a `layerK.i.bn1 = IBN(planes)` in every block of layers 1-3 (13 sites, IN on the first
planes/2 channels), IBN-b the stem `bn1 = InstanceNorm2d(64)` on (N,64,112,112) and `layer1.2.IN`, `layer2.3.IN` on
(N,256,56,56), (N,512,28,28) — each with the ReLU behind it in one launch per direction on channels-last tensors
(callers/ibn.py).  Quirks kept: 'b' only on the last block of layers 1-2, an IBN-b block with `IN` and pos='post' has no
CNSN unit, `AvgPool2d(7)`, the init loop covers InstanceNorm2d."""
import torch
import torch.nn as nn

from ._sites import CrossNormSites
from .bn_act import bn_act
from .ibn import InstanceNorm2d
from .resnet import _Bottleneck


class ResNet50IBNCNSN(nn.Module, CrossNormSites):
    def __init__(self, ibn_cfg=("a", "a", "a", None), layers=(3, 4, 6, 3), num_classes=1000, active_num=1, pos="post", beta=None,
                 crop=None, cnsn_type="sn", impl=None):
        super().__init__()
        if impl is None:
            from .. import cnsn as impl
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = InstanceNorm2d(64, affine=True) if ibn_cfg[0] == "b" else nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        kw = dict(pos=pos, beta=beta, crop=crop, cnsn_type=cnsn_type)
        c_in = 64
        for i, (planes, blocks, ibn) in enumerate(zip((64, 128, 256, 512), layers, ibn_cfg)):
            stride = 1 if i == 0 else 2
            units = []
            for b in range(blocks):
                down = None
                if b == 0 and (stride != 1 or c_in != planes * 4):
                    down = nn.Sequential(nn.Conv2d(c_in, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
                # (:216-226) 'b' only on the last block of the stage; 'a' on every block
                unit_ibn = None if (ibn == "b" and b < blocks - 1) else ibn
                units.append(_Bottleneck(impl, c_in, planes, stride if b == 0 else 1, down, ibn=unit_ibn, **kw))
                c_in = planes * 4
            setattr(self, f"layer{i + 1}", nn.Sequential(*units))
        self.avgpool = nn.AvgPool2d(7)
        self.fc = nn.Linear(c_in, num_classes)
        for m in self.modules():                                   # initialisation as :182-189
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, InstanceNorm2d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._collect_sites(impl, cnsn_type, active_num)

    def forward(self, x, aug=False):
        if aug:
            self._enable_cross_norm()
        x = self.conv1(x)
        x = self.bn1.forward_act(x) if isinstance(self.bn1, InstanceNorm2d) else bn_act(self.bn1, x)
        x = self.maxpool(x)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet50_ibn_a(config, impl=None):
    """ResNet-50-IBN-a from the reference's config object (`active_num, pos, beta, crop, cnsn_type`, :243-258)."""
    return ResNet50IBNCNSN(ibn_cfg=("a", "a", "a", None), active_num=config.active_num, pos=config.pos, beta=config.beta,
                           crop=config.crop, cnsn_type=config.cnsn_type, impl=impl)


def resnet50_ibn_b(config, impl=None):
    """ResNet-50-IBN-b from the reference's config object (:291-306)."""
    return ResNet50IBNCNSN(ibn_cfg=("b", "b", None, None), active_num=config.active_num, pos=config.pos, beta=config.beta,
                           crop=config.crop, cnsn_type=config.cnsn_type, impl=impl)
