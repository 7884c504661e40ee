"""`act(bn(x) [+ addend])` around an `nn.BatchNorm2d` module AS IT IS — the plainest pattern of the backbones,
`relu(bn(conv(x)))` (models/imagenet/resnet_cnsn.py:104-110, :257-259) and the plain block end `relu(bn3(h) + identity)`.

On channels-last HIP tensors the module's parameters and buffers go to this library's own launch (functional.BatchNormAct,
cnsn_forward_bn_act: batch statistics, the running-buffer update, the add and the ReLU in ONE launch per direction, 3 + 5
tensor passes where BatchNorm2d and an in-place ReLU as separate kernels move 5 + 8) whenever `functional.bn_act_plan` says
so; otherwise exactly the statements the backbones had before.  The module is not replaced: its type, its `state_dict`
keys and its buffers stay what they are."""
import torch
import torch.nn as nn

from .. import functional as _F
from . import _sites


def bn_act(bn, x, addend=None, relu=True):
    """`relu(bn(x))`, `relu(bn(x) + addend)` (relu=False: without the ReLU).  One launch of this library when `type(bn) is
    nn.BatchNorm2d` (no subclass, not SyncBatchNorm) with affine parameters and running statistics, `x` is a HIP tensor in
    strict channels-last order, `functional.bn_act_plan` takes the call and — in eval mode — no gradient is needed;
    `_sites.FUSE_BN_ACT = False` (CNSN_BN_ACT=0) switches it off.  With `_sites.FUSE_BN_ACT_NCHW` (CNSN_BN_ACT_NCHW=1, off by
    default) a dense NCHW tensor under the same module conditions goes to the library's two plain launches per direction
    (functional.BatchNormActNCHW) when `functional.bn_act_nchw_plan` takes it.  Everything else runs the plain statements."""
    if _sites.FUSE_BN_ACT and _fusable(bn, x, addend, relu):
        from ..cnsn import SelfNorm
        _, eps, momentum, counter = SelfNorm._bn_call_state(bn, in_kernel=True)   # nn.BatchNorm2d's per-call book-keeping
        return _F.BatchNormAct.apply(x, addend, bn.weight, bn.bias, bn.running_mean, bn.running_var, bool(relu), bn.training, eps,
                                     momentum, counter)
    if _sites.FUSE_BN_ACT_NCHW and _module_ok(bn, x, addend) and x.is_contiguous() \
            and _F.bn_act_nchw_plan(x, relu, addend is not None, bn.training):   # (a dense NCHW tensor: two plain launches)
        from ..cnsn import SelfNorm
        _, eps, momentum, counter = SelfNorm._bn_call_state(bn, in_kernel=True)
        return _F.BatchNormActNCHW.apply(x, addend, bn.weight, bn.bias, bn.running_mean, bn.running_var, bool(relu), bn.training,
                                         eps, momentum, counter)
    if addend is None:
        return torch.relu_(bn(x)) if relu else bn(x)       # (nn.ReLU(inplace=True) on BatchNorm2d's fresh output)
    y = bn(x) + addend
    return torch.relu(y) if relu else y


def _fusable(bn, x, addend, relu):
    return _module_ok(bn, x, addend) and _F.bn_act_plan(x, relu, addend is not None, bn.training)


def _module_ok(bn, x, addend):
    """what either route asks of the module and the call, before its plan"""
    if not (type(bn) is nn.BatchNorm2d and bn.affine and bn.track_running_stats and bn.running_mean is not None):
        return False
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.shape[1] == bn.num_features):
        return False
    if addend is not None and not (isinstance(addend, torch.Tensor) and addend.shape == x.shape and addend.dtype == x.dtype
                                   and addend.device == x.device):
        return False
    if bn.weight.device != x.device or bn.running_mean.device != x.device:
        return False
    if not bn.training and torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad
                                                        or (addend is not None and addend.requires_grad)):
        return False                                       # (eval mode with a gradient: frozen-BatchNorm2d fine-tuning keeps torch's path)
    return True
