"""ResNet-50-IBN-a / -b (callers/resnet_ibn.py) through the HIP modules against G9 — the imported reference backbones
(models/imagenet/resnet_ibn_cnsn.py) run by tests/golden/gen_golden_ibn.py: logits in NCHW and channels-last, one
channels-last training step (every IBN layer in its single launch) by value and by direction, and a bf16-autocast step of the
single launches against the same step with CNSN_NHWC_FUSED=0, each measured against G9's fp64 step (at G9's fill the bf16 logits
of EITHER path are ~0.17 in cosine distance from the fp64 ones; the layer-level comparison of the two, where bf16 rounding is
all that separates them: tests/test_gpu_ibn_nhwc.py::test_bf16_autocast_fused_against_unfused)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import _ffi  # noqa: E402
from cnsn_amd.callers import resnet50_ibn_a, resnet50_ibn_b  # noqa: E402
from tests.golden.gen_golden_fill import fill_by_name  # noqa: E402

BUILD = {"a": resnet50_ibn_a, "b": resnet50_ibn_b}
LAUNCHES = {"a": 13, "b": 3}     # IBN layers of IBN-a (layers 1-3, every block); InstanceNorm2d layers of IBN-b (stem, two block ends)


class Cfg:
    active_num, pos, beta, crop, cnsn_type = 1, "post", None, None, "sn"


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(os.path.join(golden_dir, "g9_ibn.npz"))


@pytest.fixture(scope="module")
def x_in(golden_dir):
    return torch.from_numpy(np.load(os.path.join(golden_dir, "g6_models.npz"))["r50_x"])


def make(v, g9, channels_last):
    m = fill_by_name(BUILD[v](Cfg, impl=cnsn_amd.cnsn), int(g9["seed"])).cuda()
    return m.to(memory_format=torch.channels_last) if channels_last else m


def launches(out):
    seen, todo, n = set(), [out.grad_fn], 0
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        n += type(fn).__name__ == "IBNormBackward"
        todo.extend(nxt for nxt, _ in fn.next_functions)
    return n


def bar(name, got, t64, t32, tol=1e-3):
    t64, t32 = torch.from_numpy(t64), torch.from_numpy(t32).double()
    got = got.detach().cpu().double().reshape(t64.shape)
    err, ref_err, scale = float((got - t64).abs().max()), float((t32 - t64).abs().max()), float(t64.abs().max())
    assert err <= max(tol * scale, 3 * ref_err), f"{name}: err {err:.3e}, reference fp32 err {ref_err:.3e}, scale {scale:.3g}"


def cos_dist(u, v):
    return 1 - float(torch.nn.functional.cosine_similarity(u.detach().double().cpu().flatten(), v.detach().double().cpu().flatten(), dim=0))


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_logits_match_reference(g9, x_in, variant, channels_last):
    m = make(variant, g9, channels_last)
    x = x_in.cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    m.train()
    with torch.no_grad():
        out = {"train": m(x)}
        m.eval()
        out["eval"] = m(x)
    for k, v in out.items():
        bar(f"IBN-{variant} {k} logits", v, g9[f"{variant}_f64_{k}"], g9[f"{variant}_f32_{k}"])


@pytest.mark.parametrize("variant", ["a", "b"])
def test_train_step_channels_last_matches_reference(g9, x_in, variant):
    """one training step in channels-last, every IBN layer in the single launch: logits and running statistics by value, fc rows by
    value, the IBN / InstanceNorm parameters and conv1 by direction (the G6b construction: many MIOpen convolutions and ReLUs lie
    between them and the loss, and the reference's own fp32 step is off its fp64 step by about 1e-3 in cosine there)"""
    m = make(variant, g9, True).train()
    x = x_in.cuda().contiguous(memory_format=torch.channels_last)
    logits = m(x)
    assert launches(logits) == LAUNCHES[variant]
    (logits * torch.from_numpy(g9["w"]).float().cuda()).sum().backward()
    torch.cuda.synchronize()
    bar("logits", logits, g9[f"{variant}_f64_step_logits"], g9[f"{variant}_f32_step_logits"])
    params, state = dict(m.named_parameters()), m.state_dict()
    for k in [str(v) for v in g9[f"{variant}_running_names"]]:
        bar(k, state[k], g9[f"{variant}_f64_{k}"], g9[f"{variant}_f32_{k}"])
    rows = int(g9["fc_rows"])
    for k in [str(v) for v in g9[f"{variant}_grad_names"]]:
        t64, t32 = g9[f"{variant}_f64_grad_{k}"], g9[f"{variant}_f32_grad_{k}"]
        if k == "fc.weight":
            bar(f"grad {k}", params[k].grad[:rows], t64, t32)
            continue
        d = cos_dist(params[k].grad, torch.from_numpy(t64))
        ref = cos_dist(torch.from_numpy(t32), torch.from_numpy(t64))
        assert d <= max(1e-3, 3 * ref), f"grad {k}: cosine distance {d:.2e}, reference fp32 {ref:.2e}"


def bf16_step(m, x, w):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = m(x)
    n = launches(logits)
    (logits.float() * w).sum().backward()
    torch.cuda.synchronize()
    return n, logits.detach().float(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("variant", ["a", "b"])
def test_bf16_autocast_step_fused_against_unfused(g9, x_in, variant):
    """a bf16-autocast channels-last training step with the single launches against the same step with CNSN_NHWC_FUSED=0
    (switched through cnsn_reload_env), by direction.  Both are ~0.18 (cosine distance of the logits) from G9's fp64 step at this
    fill, so they are not compared with each other: the single launches may be no farther from the fp64 step than the un-fused
    layers are.  Asserted on the logits and the fc rows; the gradients deeper in the network (IBN / InstanceNorm parameters,
    conv1) are 0.58-1.13 from the fp64 ones on EITHER path (measured: no correlation left in bf16 at this fill) and are printed
    only — the layer-level test in test_gpu_ibn_nhwc.py compares them where bf16 rounding is all that separates the paths"""
    x = x_in.cuda().contiguous(memory_format=torch.channels_last)
    w = torch.from_numpy(g9["w"]).float().cuda()
    n_f, lf, gf = bf16_step(make(variant, g9, True).train(), x, w)
    old = os.environ.get("CNSN_NHWC_FUSED")
    try:
        os.environ["CNSN_NHWC_FUSED"] = "0"
        _ffi.reload_env()
        n_p, lp, gp = bf16_step(make(variant, g9, True).train(), x, w)
    finally:
        if old is None:
            os.environ.pop("CNSN_NHWC_FUSED", None)
        else:
            os.environ["CNSN_NHWC_FUSED"] = old
        _ffi.reload_env()
    assert (n_f, n_p) == (LAUNCHES[variant], 0)
    rows = int(g9["fc_rows"])
    pairs = [("logits", lf, lp, g9[f"{variant}_f64_step_logits"])]
    for k in [str(v) for v in g9[f"{variant}_grad_names"]]:
        cut = (lambda t: t[:rows]) if k == "fc.weight" else (lambda t: t)
        pairs.append((f"grad {k}", cut(gf[k]), cut(gp[k]), g9[f"{variant}_f64_grad_{k}"]))
    for name, got_f, got_p, t64 in pairs:
        t = torch.from_numpy(t64)
        d_f, d_p = cos_dist(got_f, t), cos_dist(got_p, t)
        print(f"IBN-{variant} bf16 {name}: cosine distance to the fp64 step {d_f:.3e} (single launch) / {d_p:.3e} (CNSN_NHWC_FUSED=0)")
        if name in ("logits", "grad fc.weight"):
            assert d_f <= 2 * d_p + 1e-2, f"{name}: cosine distance to the fp64 step {d_f:.3e} (single launch) vs {d_p:.3e} (un-fused)"
