"""Outliers at the sample the one-pass statistics take their sums about.

Every channels-last family and the NCHW two-pass kernels sum d = X - K and d^2 in float32 (in lane and in the LDS row merge; only
the merge over tiles is double) about a shift K read from the tensor itself.  The rest of the suite tests one side of that design:
planes whose mean dwarfs their spread.  This file tests the other side: a K that is itself atypical.  If K lies D sigma off its
plane every d is about D sigma, and the float32 sums lose about D^2 * 2^-24 of the variance — invisible to a reference that takes
its statistics in two passes.

The inputs are drawn by the helpers of the files that own each family (their seeds, their bars, unchanged); a hook then moves
  first        pixel (0, 0) of every plane to the plane's mean + D * its standard deviation (both taken before the edit)
  corners      the four corner pixels of every plane likewise (what a zero-padded convolution does to a flat plane)
  first_image  image 0 as a whole by D * the channel's standard deviation, N = 64 (the families with BatchNorm2d statistics)
  control      D = 0 through the same hook: the plumbing of this file alone
with D in {8, 64, 1024}.  Where the statistics are those of a SUM (a PRE add, the IBN layer's addend) the sum is moved: x is edited
and the addend zeroed there.  The bottleneck tail is edited on both convolution outputs in one case and on the identity alone in
another (the cross sum c*b sees both).  The BatchNorm2d + ReLU launch's addend is added behind the normalisation and is left alone.

Everything the helpers compare is compared (y, dx, d-addend, parameter gradients, running statistics) at their own bars: fp32
`|hip - truth64| <= max(1e-5 * scale, 2 * |oracle32 - truth64|)`.  On top of that every fp32 case asserts that the noise arm of
that bound is asleep for y — `2 * |oracle32 - truth64| < 1e-5 * scale` — so that an input on which the reference itself is
noisy cannot quietly admit the kernel; a case that fails THAT is a bad case, not a bad kernel.  The 49 combinations that do are
listed in NOISY below and left out, level by level — nearly all of them SelfNorm at (2,16,64,64), whose BatchNorm1d over a batch
of two is close to singular; (8,16,64,64) runs the same pixel chunks there at every level.  Every case also asserts the launch
it meant to run: `bn_act_plan` / `ibn_plan` / `which_path` / the grad_fn inside the helpers and the CNSN_DEBUG line of each single
launch with status 0 and the re-stated geometry.  The register-resident NCHW strategies (resident, mono, local) take exact
two-pass statistics: they are the controls of the NCHW cases.  One bf16 case per family (D = 64, first) checks the plumbing; the
16-bit bars (1e-2 of the maximum) say nothing about the precision.

Every figure is printed before it is asserted, and once more as a `shift-sample` line per tensor (profiles/r09_shift_sample.md
is made from those lines)."""
import functools
import re
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LEVELS = [8, 64, 1024]          # powers of two
PIXELS = {"control": ((0, 0),), "first": ((0, 0),), "corners": ((0, 0), (0, -1), (-1, 0), (-1, -1))}


def move(t, pattern, d, addend=None):
    """moves the pattern's pixels of every plane of X = t (+ addend) to the plane's mean + d * its standard deviation, both taken
    before the edit: t is set there and the addend zeroed.  first_image: image 0 of X moves by d * the channel's standard
    deviation over (N, H, W).  In place; any floating dtype, any device."""
    total = t if addend is None else t + addend
    if pattern == "first_image":
        t[0] += d * total.std(dim=(0, 2, 3), keepdim=True)[0]
        return
    value = total.mean(dim=(2, 3)) + d * total.std(dim=(2, 3))
    for h, w in PIXELS[pattern]:
        t[:, :, h, w] = value
        if addend is not None:
            addend[:, :, h, w] = 0


@functools.lru_cache(maxsize=None)
def editor(family, pattern, d, target="x"):
    """the hook of one (family, pattern, D): one object per combination, so that the helpers' caches can key on it"""
    if family == "bn_act":              # edit(bn, x64, a64): the addend is added behind the normalisation
        return lambda bn, x, a: move(x, pattern, d)
    if family == "tail":                # edit(conv, identity)
        def tail(conv, idt):
            if target == "both":
                move(conv, pattern, d)
            move(idt, pattern, d)
        return tail
    if family == "nchw":                # edit(x64)
        return lambda x: move(x, pattern, d)
    if target == "sum":                 # IBN with its addend, the SelfNorm block's PRE add: edit(x, addend)
        return lambda x, a: move(x, pattern, d, a)
    return lambda x, a: move(x, pattern, d)


def levels(patterns):
    """(pattern, D) of one shape: the control and every level of every pattern"""
    return [("control", 0)] + [(p, d) for p in patterns for d in LEVELS]


def ids_of(cases):
    return [f"{p}-D{d}" for p, d in cases]


SPATIAL, IMAGE = levels(("first", "corners")), levels(("first_image",))
PLANES = [(8, 16, 14, 14), (2, 16, 64, 64)]      # M = 196: one chunk; M = 4096: eight pixel chunks of 512
SN_PLANES = PLANES + [(8, 16, 64, 64)]           # SelfNorm's BatchNorm1d over a batch of two is nearly singular: see NOISY
BATCH = (64, 16, 4, 4)                           # first_image

# The combinations on which the REFERENCE is too noisy to judge anybody: 2 * |oracle32 - truth64| of y reaches 1e-5 * scale, so
# the noise arm of the bar would widen it (measured on the MI355X with the float64 / float32 references of the helpers; the
# kernels play no part in it).  They are left out, level by level; every other case asserts that the arm is asleep.  Nearly all
# of them are SelfNorm at N = 2, whose BatchNorm1d normalises two numbers per channel — (8,16,64,64) runs the same eight pixel
# chunks of 512 with a batch the reference can take.  The others are planes with a 1024-sigma pixel on the tail's identity path,
# which reaches SelfNorm un-normalised.  Listed from 0.8 of the threshold on: ("block", shape, add mode, pattern, D),
# ("tail", shape, downsample, edited, pattern, D), ("nchw", shape, pattern, D), ("ibn", shape, half, addend, pattern, D).
NOISY = {
    ('ibn', (64, 16, 4, 4), 8, False, 'first_image', 1024), ('block', (2, 16, 64, 64), 'pre', 'control', 0),
    ('block', (2, 16, 64, 64), 'pre', 'first', 8), ('block', (2, 16, 64, 64), 'pre', 'first', 64),
    ('block', (2, 16, 64, 64), 'pre', 'first', 1024), ('block', (2, 16, 64, 64), 'pre', 'corners', 8),
    ('block', (2, 16, 64, 64), 'pre', 'corners', 64), ('block', (2, 16, 64, 64), 'pre', 'corners', 1024),
    ('block', (2, 16, 64, 64), 'none', 'control', 0), ('block', (2, 16, 64, 64), 'none', 'first', 8),
    ('block', (2, 16, 64, 64), 'none', 'corners', 8), ('tail', (8, 16, 14, 14), False, 'both', 'first', 1024),
    ('tail', (8, 16, 14, 14), False, 'both', 'corners', 64), ('tail', (8, 16, 14, 14), False, 'both', 'corners', 1024),
    ('tail', (8, 16, 14, 14), False, 'identity', 'first', 1024), ('tail', (8, 16, 14, 14), False, 'identity', 'corners', 64),
    ('tail', (8, 16, 14, 14), False, 'identity', 'corners', 1024), ('tail', (2, 16, 64, 64), False, 'both', 'control', 0),
    ('tail', (2, 16, 64, 64), False, 'both', 'first', 8), ('tail', (2, 16, 64, 64), False, 'both', 'first', 64),
    ('tail', (2, 16, 64, 64), False, 'both', 'first', 1024), ('tail', (2, 16, 64, 64), False, 'both', 'corners', 8),
    ('tail', (2, 16, 64, 64), False, 'both', 'corners', 64), ('tail', (2, 16, 64, 64), False, 'both', 'corners', 1024),
    ('tail', (2, 16, 64, 64), False, 'identity', 'control', 0), ('tail', (2, 16, 64, 64), False, 'identity', 'first', 64),
    ('tail', (2, 16, 64, 64), False, 'identity', 'first', 1024), ('tail', (2, 16, 64, 64), False, 'identity', 'corners', 8),
    ('tail', (2, 16, 64, 64), False, 'identity', 'corners', 64), ('tail', (2, 16, 64, 64), False, 'identity', 'corners', 1024),
    ('tail', (2, 16, 64, 64), True, 'both', 'control', 0), ('tail', (2, 16, 64, 64), True, 'both', 'first', 8),
    ('tail', (2, 16, 64, 64), True, 'both', 'first', 64), ('tail', (2, 16, 64, 64), True, 'both', 'first', 1024),
    ('tail', (2, 16, 64, 64), True, 'both', 'corners', 8), ('tail', (2, 16, 64, 64), True, 'both', 'corners', 64),
    ('tail', (2, 16, 64, 64), True, 'both', 'corners', 1024), ('tail', (2, 16, 64, 64), True, 'identity', 'control', 0),
    ('tail', (2, 16, 64, 64), True, 'identity', 'first', 8), ('tail', (2, 16, 64, 64), True, 'identity', 'first', 64),
    ('tail', (2, 16, 64, 64), True, 'identity', 'first', 1024), ('tail', (2, 16, 64, 64), True, 'identity', 'corners', 8),
    ('tail', (2, 16, 64, 64), True, 'identity', 'corners', 64), ('tail', (2, 16, 64, 64), True, 'identity', 'corners', 1024),
    ('tail', (8, 16, 64, 64), False, 'both', 'first', 1024), ('tail', (8, 16, 64, 64), False, 'both', 'corners', 1024),
    ('tail', (8, 16, 64, 64), False, 'identity', 'first', 1024), ('tail', (8, 16, 64, 64), False, 'identity', 'corners', 1024),
    ('nchw', (2, 16, 64, 64), 'first', 64)}


def quiet(*key):
    return key not in NOISY


def case_id(*parts):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in parts)


if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from tests import test_gpu_bn_act_geometry as bn_geometry  # noqa: E402
from tests import test_gpu_ibn_nhwc as ibn  # noqa: E402
from tests import test_gpu_nhwc_geometry as geometry  # noqa: E402
from tests import test_gpu_parity as parity  # noqa: E402
from tests.test_gpu_nhwc_full_size import healthy, knobs, run_block, run_bn_block  # noqa: E402

_FIGURE = re.compile(r"^ +(.+?): err (\S+) bound (\S+)(?: \(oracle32 noise (\S+), scale (\S+)\))?$", re.M)


class Figures:
    """what the helper of a case printed: shown again (`pytest -s`), one `shift-sample` line per tensor, and the noise arm of
    y's bound asserted asleep when the case passed"""

    def __init__(self, capfd, label, dtype):
        self.capfd, self.label, self.dtype = capfd, label, dtype

    def __enter__(self):
        self.capfd.readouterr()
        return self

    def __exit__(self, kind, exc, tb):
        cap = self.capfd.readouterr()
        sys.stdout.write(cap.out)
        sys.stderr.write(cap.err)
        rows = [(m.group(1), float(m.group(2)), float(m.group(3)), m.group(4), m.group(5)) for m in _FIGURE.finditer(cap.out)]
        for name, err, bound, noise, scale in rows:
            print(f"shift-sample | {self.label} | {name} | err {err:.3e} | bound {bound:.3e} | err/bound {err / bound:.3f}"
                  + (f" | noise {noise} scale {scale}" if noise else ""))
        if kind is None:
            ys = [r for r in rows if r[0] == "y"]
            assert len(ys) == 1, f"{self.label}: {len(ys)} figures of y"
            if self.dtype == F32:
                noise, scale = float(ys[0][3]), float(ys[0][4])
                assert 2 * noise < 1e-5 * scale, f"{self.label}: the reference's own noise ({noise:.3e}) widens y's bound"
        return False


def label(family, shape, dtype, pattern, d, *more):
    return " ".join([family, "x".join(map(str, shape)), "fp32" if dtype == F32 else "bf16", *map(str, more), pattern, f"D={d}"])


# ------------------------------------------------------------------------------------------------------------------------
# BatchNorm2d (+ add) + ReLU: one shift per channel for all N*H*W rows
# ------------------------------------------------------------------------------------------------------------------------
def bn_act_case(shape, dtype, pattern, d, capfd, monkeypatch, **kw):
    with Figures(capfd, label("bn_act", shape, dtype, pattern, d), dtype):
        bn_geometry.run(shape, dtype, capfd, monkeypatch, edit=editor("bn_act", pattern, d), **kw)


assert bn_geometry.geom((8, 16, 8, 8), F32) == dict(R=512, C=16, tc=4, tcb=4, rows=64, ncb=1, wpc=8, chunk=64, tiles=8)
assert bn_geometry.geom((64, 8, 3, 3), F32)["tiles"] >= 8 and bn_geometry.geom((300, 64, 5, 5), F32)["chunk"] == 65
assert bn_geometry.geom((32, 64, 56, 56), F32)["chunk"] > 4 * bn_geometry.geom((32, 64, 56, 56), F32)["rows"]


# (8,16,8,8): exactly 8 tiles of 64 rows on 64 rows of threads — one element per lane, the LDS merge alone
@pytest.mark.parametrize("pattern,d", SPATIAL, ids=ids_of(SPATIAL))
@pytest.mark.parametrize("shape", [(8, 16, 8, 8), (300, 64, 5, 5)], ids=str)
def test_bn_act(shape, pattern, d, capfd, monkeypatch):
    bn_act_case(shape, F32, pattern, d, capfd, monkeypatch)


@pytest.mark.parametrize("pattern,d", IMAGE, ids=ids_of(IMAGE))
def test_bn_act_first_image(pattern, d, capfd, monkeypatch):
    bn_act_case((64, 8, 3, 3), F32, pattern, d, capfd, monkeypatch)


@pytest.mark.parametrize("pattern,d", SPATIAL, ids=ids_of(SPATIAL))
def test_bn_act_several_elements_per_lane(pattern, d, capfd, monkeypatch):
    """25 MB, drawn and referenced on the GPU: chunks of 98 rows on 16 rows of threads"""
    try:
        bn_act_case((32, 64, 56, 56), F32, pattern, d, capfd, monkeypatch, gen_dev="cuda")
    finally:
        bn_geometry.free()


# ------------------------------------------------------------------------------------------------------------------------
# the IBN layer: per-plane shifts, InstanceNorm2d per plane and BatchNorm2d over the planes of a channel
# ------------------------------------------------------------------------------------------------------------------------
def ibn_case(shape, dtype, half, addend, pattern, d, capfd, monkeypatch):
    with Figures(capfd, label("ibn", shape, dtype, pattern, d, f"half={half}", "x+a" if addend else "x"), dtype):
        with knobs(monkeypatch, CNSN_DEBUG="1"), healthy():
            ibn.run_case(shape, dtype, half, addend=addend, seed=shape[1] + shape[2],
                         edit=editor("ibn", pattern, d, "sum" if addend else "x"))
            torch.cuda.synchronize()
            cap = capfd.readouterr()
            sys.stdout.write(cap.out)      # (Figures reads it again)
        seen = {}
        for m in geometry._IBN_LINE.finditer(cap.err):
            assert ("ibn", m.group(1)) not in seen, cap.err
            seen["ibn", m.group(1)] = dict(tiles=int(m.group(2)), S=int(m.group(3)), rows=int(m.group(4)), tcb=int(m.group(5)),
                                           groups=int(m.group(6)), half=int(m.group(7)), status=int(m.group(9)))
        geometry.check_geometry(seen, "ibn", shape, dtype, 8, 4)
        assert all(v["half"] == half for v in seen.values()), seen


IBN = [(s, h, a, p, d) for s in PLANES for h in (8, 16) for a in (False, True) for p, d in SPATIAL if quiet("ibn", s, h, a, p, d)]


@pytest.mark.parametrize("shape,half,addend,pattern,d", IBN, ids=[case_id(s, f"half{h}", "x+a" if a else "x", p, f"D{d}")
                                                                  for s, h, a, p, d in IBN])
def test_ibn(shape, half, addend, pattern, d, capfd, monkeypatch):
    ibn_case(shape, F32, half, addend, pattern, d, capfd, monkeypatch)


IBN_IMAGE = [(p, d) for p, d in IMAGE if quiet("ibn", BATCH, 8, False, p, d)]


@pytest.mark.parametrize("pattern,d", IBN_IMAGE, ids=ids_of(IBN_IMAGE))
def test_ibn_first_image(pattern, d, capfd, monkeypatch):
    ibn_case(BATCH, F32, 8, False, pattern, d, capfd, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------
# the SelfNorm block: the single launch (CNSN_NHWC_FUSED=2) and the a-launch-per-pass kernels (=0)
# ------------------------------------------------------------------------------------------------------------------------
def block_case(shape, dtype, mode, relu, fused, pattern, d, capfd, monkeypatch):
    with Figures(capfd, label("sn-block", shape, dtype, pattern, d, f"fused={fused}", mode), dtype):
        seen = run_block(shape, dtype, mode, relu, fused, capfd, monkeypatch,
                         edit=editor("block", pattern, d, "sum" if mode == "pre" else "x"))
        if fused == "2":
            geometry.check_geometry(seen, "single-launch", shape, dtype, 8, 4)
        else:
            assert not seen, seen           # (run_block asserted which_path == "streaming")


BLOCK = [(s, m, r, f, p, d) for s in SN_PLANES for m, r in (("pre", True), ("none", False)) for f in ("2", "0") for p, d in SPATIAL
         if quiet("block", s, m, p, d)]


@pytest.mark.parametrize("shape,mode,relu,fused,pattern,d", BLOCK,
                         ids=[case_id(s, m, "single-launch" if f == "2" else "per-pass", p, f"D{d}") for s, m, r, f, p, d in BLOCK])
def test_selfnorm_block(shape, mode, relu, fused, pattern, d, capfd, monkeypatch):
    block_case(shape, F32, mode, relu, fused, pattern, d, capfd, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------
# the bottleneck tail: five sums c, c^2, b, b^2, c*b about the shifts of both tensors
# ------------------------------------------------------------------------------------------------------------------------
def tail_case(shape, dtype, two, target, pattern, d, capfd, monkeypatch):
    with Figures(capfd, label("tail", shape, dtype, pattern, d, "downsample" if two else "identity", f"edit={target}"), dtype):
        seen = run_bn_block(shape, dtype, two, capfd, monkeypatch, edit=editor("tail", pattern, d, target))
        geometry.check_geometry(seen, "bn-block", shape, dtype, 4, 4)


def tail_cases(shapes, cases):
    return [(s, two, t, p, d) for s in shapes for two in (False, True) for t in ("both", "identity") for p, d in cases
            if quiet("tail", s, two, t, p, d)]


def tail_ids(cases):
    return [case_id(s, "downsample" if two else "identity", f"edit-{t}", p, f"D{d}") for s, two, t, p, d in cases]


TAIL, TAIL_IMAGE = tail_cases(SN_PLANES, SPATIAL), tail_cases([BATCH], IMAGE)


@pytest.mark.parametrize("shape,two,target,pattern,d", TAIL, ids=tail_ids(TAIL))
def test_tail(shape, two, target, pattern, d, capfd, monkeypatch):
    tail_case(shape, F32, two, target, pattern, d, capfd, monkeypatch)


@pytest.mark.parametrize("shape,two,target,pattern,d", TAIL_IMAGE, ids=tail_ids(TAIL_IMAGE))
def test_tail_first_image(shape, two, target, pattern, d, capfd, monkeypatch):
    tail_case(shape, F32, two, target, pattern, d, capfd, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------
# NCHW: the forced two-pass strategy (one-pass sums about a shift) and the register-resident controls
# ------------------------------------------------------------------------------------------------------------------------
# what `which_path` answers under each forced strategy.  mono and local take the 14x14 and 7x7 planes and leave the 64x64 ones to
# the two-pass kernels, so those shapes' control is `resident` alone; fp32 7x7 planes under two_pass run the packed kernels (and
# under `resident` too: their controls are mono and local)
NCHW_PATHS = [((8, 16, 14, 14), "two_pass", "streaming"), ((8, 16, 14, 14), "resident", "resident"), ((8, 16, 14, 14), "local", "local"),
              ((8, 16, 14, 14), "mono", "mono"), ((2, 16, 64, 64), "two_pass", "streaming"), ((2, 16, 64, 64), "resident", "resident"),
              ((8, 16, 64, 64), "two_pass", "streaming"), ((8, 16, 64, 64), "resident", "resident"),
              ((8, 16, 7, 7), "two_pass", "packed"), ((8, 16, 7, 7), "local", "local"), ((8, 16, 7, 7), "mono", "mono")]
NCHW = [(s, st, path, p, d) for s, st, path in NCHW_PATHS for p, d in SPATIAL if quiet("nchw", s, p, d)]


def nchw_case(shape, dtype, strategy, path, pattern, d, capfd):
    cnsn_amd.set_strategy(strategy)
    try:
        with Figures(capfd, label("nchw", shape, dtype, pattern, d, strategy), dtype):
            probe, cfg = torch.empty(shape, dtype=dtype, device="cuda"), cnsn_amd.FusedConfig(sn_active=True)
            assert cnsn_amd.which_path(probe, cfg) == path and cnsn_amd.which_path(probe, cfg, backward=True) == path
            seed = parity.seed_of(shape, "shift-sample")
            out = parity.run_pair(shape, "neither", "sn", dtype, seed, edit=editor("nchw", pattern, d))
            parity.assert_parity(out, dtype, (shape, strategy, pattern, d))
    finally:
        cnsn_amd.set_strategy("auto")


@pytest.mark.parametrize("shape,strategy,path,pattern,d", NCHW, ids=[case_id(s, st, p, f"D{d}") for s, st, _, p, d in NCHW])
def test_nchw(shape, strategy, path, pattern, d, capfd):
    nchw_case(shape, F32, strategy, path, pattern, d, capfd)


# ------------------------------------------------------------------------------------------------------------------------
# 16 bits: the plumbing of every family (the bars are 1e-2 of the maximum)
# ------------------------------------------------------------------------------------------------------------------------
def test_bf16_bn_act(capfd, monkeypatch):
    bn_act_case((8, 32, 8, 8), BF16, "first", 64, capfd, monkeypatch)


@pytest.mark.parametrize("half", [8, 16], ids=["ibn", "in"])
def test_bf16_ibn(half, capfd, monkeypatch):
    ibn_case(PLANES[0], BF16, half, half == 16, "first", 64, capfd, monkeypatch)


@pytest.mark.parametrize("fused", ["2", "0"], ids=["single-launch", "per-pass"])
def test_bf16_selfnorm_block(fused, capfd, monkeypatch):
    block_case(PLANES[0], BF16, "pre", True, fused, "first", 64, capfd, monkeypatch)


def test_bf16_tail(capfd, monkeypatch):
    tail_case(PLANES[0], BF16, True, "both", "first", 64, capfd, monkeypatch)


def test_bf16_nchw_two_pass(capfd):
    """16-bit 14x14 planes under the forced two-pass strategy run the packed kernels"""
    nchw_case(PLANES[0], BF16, "two_pass", "packed", "first", 64, capfd)
