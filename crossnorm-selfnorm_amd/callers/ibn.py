"""Instance / Instance-Batch normalisation of the reference's IBN backbones on the plane-statistics
kernels of this library: `nn.InstanceNorm2d(C, affine=True)` and `IBN` (models/imagenet/resnet_ibn_cnsn.py:24-44,
:63) with the same attribute names and `state_dict` keys (`IN.weight`, `IN.bias`, `BN.*`).

InstanceNorm2d here = one plane-statistics launch (cnsn_plane_stats) + one per-plane affine launch
(cnsn_plane_affine) forward, and a dedicated backward (functional.InstanceNorm): per-plane sums of G and G*(x - mean)
(cnsn_plane_dot_shifted) + ONE apply launch (cnsn_plane_combine) — 3 + 5 tensor passes; (N, C)-sized torch ops in
between.  HIP device tensors only.

On channels-last tensors (what every model workload runs) both modules take ONE launch per direction instead
(functional.IBNorm, cnsn_forward_ibn: the split, both normalisations, the cat and — through `forward_act` — the add in
front and the ReLU behind, 3 + 5 tensor passes in all) whenever `functional.ibn_plan` says so; otherwise the code above,
unchanged."""
import torch
import torch.nn as nn

from .. import functional as _F


class InstanceNorm2d(nn.Module):
    """nn.InstanceNorm2d(num_features, eps, affine=True, track_running_stats=False): per-(n,c) plane
    `(x - mean) / sqrt(biased var + eps) * weight[c] + bias[c]`."""

    def __init__(self, num_features, eps=1e-5, affine=True):
        super().__init__()
        self.num_features, self.eps, self.affine = num_features, eps, affine
        if affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def forward(self, x):
        assert x.dim() == 4 and x.size(1) == self.num_features
        if _F.ibn_plan(x, self.num_features, relu=False):
            return self._launch(x, None, False)
        return _F.InstanceNorm.apply(x, self.weight if self.affine else None, self.bias if self.affine else None, self.eps)

    def forward_act(self, x, addend=None, relu=True):
        """`relu(self(x [+ addend]))` — the IBN-b stem (`relu(bn1(conv1(x)))`) and block end (`relu(IN(out + identity))`,
        resnet_ibn_cnsn.py:117-122, :138-139) in the single launch when it takes the call, the separate ops otherwise."""
        if _fusable_addend(x, addend) and _F.ibn_plan(x, self.num_features, relu, addend is not None):
            return self._launch(x, addend, relu)
        return _act(self(x if addend is None else x + addend), relu)

    def _launch(self, x, addend, relu):
        w, b = (self.weight, self.bias) if self.affine else (None, None)
        return _F.IBNorm.apply(x, addend, w, b, None, None, None, None, self.num_features, bool(relu), float(self.eps), False, 0.0,
                               0.0, None)


class IBN(nn.Module):
    """Half the channels through InstanceNorm2d, the rest through BatchNorm2d (resnet_ibn_cnsn.py:24-44)."""

    def __init__(self, planes, ratio=0.5):
        super().__init__()
        self.half = int(planes * ratio)
        self.IN = InstanceNorm2d(self.half, affine=True)
        self.BN = nn.BatchNorm2d(planes - self.half)

    def forward(self, x):
        if self._fusable(x, None, False):
            return self._launch(x, None, False)
        # the first `half` channels are instance-normalised, the others batch-normalised, order kept
        # (`.narrow` views are strided: both normalisations want dense tensors, as the reference's split does)
        rest = x.size(1) - self.half
        y_in = self.IN(x.narrow(1, 0, self.half).contiguous())
        y_bn = self.BN(x.narrow(1, self.half, rest).contiguous())
        return torch.cat([y_in, y_bn], dim=1)

    def forward_act(self, x, addend=None, relu=True):
        """`relu(self(x [+ addend]))` — IBN-a's `relu(bn1(conv1(x)))` (resnet_ibn_cnsn.py:97-99) in the single launch when it
        takes the call, the separate ops otherwise."""
        if self._fusable(x, addend, relu):
            return self._launch(x, addend, relu)
        return _act(self(x if addend is None else x + addend), relu)

    def _fusable(self, x, addend, relu):
        bn, inn = self.BN, self.IN
        if not (type(bn) is nn.BatchNorm2d and bn.affine and bn.track_running_stats and type(inn) is InstanceNorm2d
                and inn.num_features == self.half and _fusable_addend(x, addend)):
            return False
        if not all(t.dtype == torch.float32 and t.is_contiguous() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            return False
        return _F.ibn_plan(x, self.half, relu, addend is not None, bn.training)

    def _launch(self, x, addend, relu):
        from ..cnsn import SelfNorm
        bn, inn = self.BN, self.IN
        _, eps, momentum, counter = SelfNorm._bn_call_state(bn, in_kernel=True)   # nn.BatchNorm2d's per-call book-keeping
        w, b = (inn.weight, inn.bias) if inn.affine else (None, None)
        return _F.IBNorm.apply(x, addend, w, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.half, bool(relu),
                               float(inn.eps), bn.training, eps, momentum, counter)


def _fusable_addend(x, addend):
    return addend is None or (isinstance(addend, torch.Tensor) and addend.shape == x.shape and addend.dtype == x.dtype
                              and addend.device == x.device)


def _act(y, relu):
    return torch.relu(y) if relu else y
