"""The tile walker of the channels-last single-launch kernels (NhwcThread / nhwc_rows_sum in csrc/cnsn_nhwc_kernels.h, tiled by
nhwc_fused_geom in csrc/cnsn_nhwc_fused.hip) at channel counts that are no power of two, INSIDE the persistent launches of all
three families that share it: the SelfNorm block (cnsn_nhwc_fused_kernels.h), the fused bottleneck tail
(cnsn_nhwc_bnhead_kernels.h) and the IBN layer (cnsn_nhwc_ibn_kernels.h).

The other files run these launches at C = 8 .. 2048 in powers of two only ((3,520,6,5) has fewer than eight tiles and runs the
two-pass kernels), so the branches below never ran inside a single launch:
  idle      rows * tcb < 256: the threads with r >= rows stay inert in every phase and still add up rows in nhwc_rows_sum
  no_pixel  M < rows: threads of a live row without a pixel (the `cnt` arithmetic of the reverse walks, K from pixel 0, zero sums)
  chunks    idle threads with S > 1 and a shorter last pixel chunk
  odd_wide  tcb odd and above 64 with two column blocks; phase B's slots loop (more groups than workgroups) with the identity
            phase_b_group mapping (groups % 8 != 0)
  rows_1    tcb odd above 128: one row, 127 idle threads
  partial   tc % tcb != 0: the last column block lies partly outside the tensor (`vc < g.tc`, `first + off >= g.C`)
  odd_small tcb odd below 64 (after one halving in fp32)
Every case goes through the helpers of the files that own the families — run_block / run_bn_block of test_gpu_nhwc_full_size.py,
run_case of test_gpu_ibn_nhwc.py, run_case / check of test_gpu_fused_block.py for the POST add — with their bars unchanged, and
asserts that each direction ran ONE single launch with status 0 whose tiles, S, rows and tcb are what the rule re-stated below
gives for the device's compute-unit count."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
WG_PER_CU = 4        # CNSN_NHWC_WG_PER_CU


def geom(shape, dtype, cus=256):
    """nhwc_fused_geom re-stated (csrc/cnsn_nhwc_fused.hip): two tiles per workgroup of a grid of WG_PER_CU x `cus`"""
    n, c, h, w = shape
    m, tc, target = h * w, c // (16 // (torch.finfo(dtype).bits // 8)), 2 * WG_PER_CU * cus
    tcb = min(tc, 256)
    while tcb > 64 and tcb % 2 == 0 and n * -(-tc // tcb) < target:
        tcb //= 2
    rows, ncb = 256 // tcb, -(-tc // tcb)
    s = max(1, min(-(-target // (n * ncb)), max(m // (8 * rows), 1)))
    mchunk = -(-m // s)
    s = -(-m // mchunk)
    return dict(tc=tc, tcb=tcb, rows=rows, ncb=ncb, S=s, mchunk=mchunk, M=m, tiles=n * s * ncb)


def classes(shape, dtype, cus=256):
    g = geom(shape, dtype, cus)
    idle, groups = g["rows"] * g["tcb"] < 256, shape[1] // 8       # (groups: phase B of the SelfNorm / IBN forward)
    out = set()
    if idle and g["tcb"] < 8 and g["M"] >= g["rows"]:
        out.add("idle")
    if g["M"] < g["rows"]:
        out.add("no_pixel")
    if idle and g["S"] > 1 and g["M"] % g["mchunk"] != 0:
        out.add("chunks")
    if g["tcb"] % 2 and g["tcb"] > 64 and g["rows"] > 1 and groups % 8 != 0 and groups > g["tiles"]:     # (grid <= tiles)
        out.add("odd_wide")
    if g["tcb"] % 2 and g["ncb"] == 2:
        out.add("two_blocks")
    if g["rows"] == 1:
        out.add("rows_1")
    if g["tc"] % g["tcb"]:
        out.add("partial")
    if g["tcb"] % 2 and 8 < g["tcb"] < 64:
        out.add("odd_small")
    return out


# (shape, IBN `half`) by activation width.  N * ncb >= 8 everywhere: the launch applies whatever the compute-unit count.
FP32 = [((8, 24, 6, 7), 8),         # tcb 6, rows 42: 4 idle threads, every live thread has a pixel
        ((8, 24, 4, 4), 16),        # M 16 < rows 42
        ((8, 24, 29, 31), 8),       # S 2, chunks of 450 and 449 pixels
        ((8, 520, 6, 5), 264),      # tcb 65, rows 3, ncb 2; 65 / 130 groups on a grid of 16
        ((4, 1032, 3, 3), 512),     # tcb 64, ncb 5: the last block holds 2 of its 64 columns
        ((8, 264, 5, 5), 128)]      # tcb 66 -> 33, rows 7
BIT16 = [((8, 24, 10, 9), 8),       # tcb 3, rows 85: 1 idle thread, M 90
         ((8, 24, 6, 7), 8),        # M 42 < rows 85
         ((8, 24, 4, 4), 16),       # M 16 < rows 85
         ((8, 520, 6, 5), 264),     # tcb 65, rows 3, ncb 1: 8 tiles, 65 / 130 groups on a grid of 8
         ((8, 1032, 3, 3), 512),    # tcb 129: one row
         ((4, 2056, 3, 3), 1024),   # tcb 64, ncb 5: the last block holds 1 column
         ((8, 264, 5, 5), 128)]     # tcb 33, rows 7
# the shape lists reach every class at 256 compute units.  Not both widths reach all of them at these sizes: one row in fp32
# needs an odd number of four-channel columns, which the IBN layer's C % 8 == 0 rules out; in 16 bits two pixel chunks of a
# three-column tensor need 2 * 8 * 85 pixels and two odd column blocks C >= 1040.
assert set().union(*(classes(s, F32) for s, _ in FP32)) == {"idle", "no_pixel", "chunks", "odd_wide", "two_blocks", "partial",
                                                            "odd_small"}
assert set().union(*(classes(s, BF16) for s, _ in BIT16)) == {"idle", "no_pixel", "odd_wide", "rows_1", "partial", "odd_small"}
assert all(classes(s, F32) for s, _ in FP32) and all(classes(s, BF16) for s, _ in BIT16)
assert all(geom(s, d, cus)["tiles"] >= 8 for cus in (64, 256, 304) for lst, d in ((FP32, F32), (BIT16, BF16)) for s, _ in lst)
assert all(h % 8 == 0 and s[1] % 8 == 0 for s, h in FP32 + BIT16)
assert geom((3, 520, 6, 5), F32)["tiles"] == 6 and geom((3, 520, 6, 5), BF16)["tiles"] == 3       # (two-pass: fewer than 8 tiles)

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import cnsn_amd  # noqa: E402
from cnsn_amd import _ffi  # noqa: E402
from cnsn_amd import functional as F_  # noqa: E402
from tests import test_gpu_ibn_nhwc as ibn  # noqa: E402
from tests.golden.gen_golden_fill import fill_sn  # noqa: E402
from tests.test_gpu_fused_block import check as block_check, run_case as block_case  # noqa: E402
from tests.test_gpu_nhwc_full_size import (CL, DEV, SN_SEED, healthy, knobs, launches, make_inputs, run_block,  # noqa: E402
                                           run_bn_block)
from tests.test_gpu_parity import seed_of  # noqa: E402

CUS = torch.cuda.get_device_properties(0).multi_processor_count      # (reshost::cu_count: hipDeviceAttributeMultiprocessorCount)
CASES = [(s, h, d) for s, h in FP32 for d in (F32,)] + [(s, h, d) for s, h in BIT16 for d in (BF16,)]
CASE_IDS = ["x".join(map(str, s)) + ("-fp32" if d == F32 else "-bf16") for s, _, d in CASES]
_IBN_LINE = re.compile(r"\[cnsn\] nhwc ibn (fwd|bwd): tiles=(\d+) \(S=(\d+) rows=(\d+) tcb=(\d+)\) groups=(\d+) half=(\d+) "
                       r"keep=(\d) -> status (-?\d+)")


def check_geometry(seen, family, shape, dtype, gc_fwd, gc_bwd):
    """one forward and one backward single launch, both with status 0 and the re-stated rule's tiles"""
    assert set(seen) == {(family, "fwd"), (family, "bwd")}, seen
    want = geom(shape, dtype, CUS)
    for (_, direction), v in seen.items():
        assert v["status"] == 0, seen
        assert {k: v[k] for k in ("tiles", "S", "rows", "tcb")} == {k: want[k] for k in ("tiles", "S", "rows", "tcb")}, (v, want)
        assert v["groups"] == shape[1] // (gc_fwd if direction == "fwd" else gc_bwd), v


@pytest.mark.parametrize("mode,relu", [("pre", True), ("none", False)], ids=["pre+relu", "none"])
@pytest.mark.parametrize("shape,half,dtype", CASES, ids=CASE_IDS)
def test_selfnorm_block(shape, half, dtype, mode, relu, capfd, monkeypatch):
    """the kept-sum forward (PRE add + ReLU) and SelfNorm alone, CNSN_NHWC_FUSED=2"""
    check_geometry(run_block(shape, dtype, mode, relu, "2", capfd, monkeypatch), "single-launch", shape, dtype, 8, 4)


@pytest.mark.parametrize("shape,half,dtype", CASES, ids=CASE_IDS)
def test_selfnorm_block_post_add(shape, half, dtype, capfd, monkeypatch):
    """y = relu(SelfNorm(x) + addend): the launch that reads a second tensor in its apply phase and writes the masked gradient"""
    seed = seed_of(shape, "sn", "neither", "post", True, str(dtype))
    with knobs(monkeypatch, CNSN_NHWC_FUSED="2", CNSN_DEBUG="1"), healthy():
        capfd.readouterr()
        out = block_case(shape, "sn", "neither", "post", True, dtype, seed, channels_last=True)
        seen = launches(capfd.readouterr().err)
    check_geometry(seen, "single-launch", shape, dtype, 8, 4)
    block_check(out, dtype, True, (shape, "sn", "post", True, dtype, "single-launch"))


@pytest.mark.parametrize("two", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape,half,dtype", CASES, ids=CASE_IDS)
def test_bn_block(shape, half, dtype, two, capfd, monkeypatch):
    check_geometry(run_bn_block(shape, dtype, two, capfd, monkeypatch), "bn-block", shape, dtype, 4, 4)


def run_ibn(shape, dtype, half, capfd, monkeypatch, **kw):
    with knobs(monkeypatch, CNSN_DEBUG="1"), healthy():
        capfd.readouterr()
        ibn.run_case(shape, dtype, half, seed=shape[1] + shape[2], **kw)
        err = capfd.readouterr().err
    seen = {}
    for m in _IBN_LINE.finditer(err):
        assert ("ibn", m.group(1)) not in seen, err
        seen["ibn", m.group(1)] = dict(tiles=int(m.group(2)), S=int(m.group(3)), rows=int(m.group(4)), tcb=int(m.group(5)),
                                       groups=int(m.group(6)), half=int(m.group(7)), status=int(m.group(9)))
    check_geometry(seen, "ibn", shape, dtype, 8, 4)
    assert all(v["half"] == half for v in seen.values()), seen


@pytest.mark.parametrize("shape,half,dtype", CASES, ids=CASE_IDS)
def test_ibn(shape, half, dtype, capfd, monkeypatch):
    run_ibn(shape, dtype, half, capfd, monkeypatch)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_ibn_workgroup_crosses_from_instance_to_batch_norm(dtype, capfd, monkeypatch):
    """half = 72 of 256 channels on a grid of 8: four forward / eight backward slots per workgroup, and the workgroup that owns
    channels 64..95 handles InstanceNorm groups (no block sum) and then BatchNorm groups (block sums) in the same launch"""
    shape, half = (8, 256, 4, 4), 72
    assert geom(shape, dtype, CUS)["tiles"] == 8 and (64 // 8) * 8 < half < 96 and (shape[1] // 8) % 8 == 0
    run_ibn(shape, dtype, half, capfd, monkeypatch)


@pytest.mark.parametrize("kw", [dict(half=24, addend=True), dict(half=8, training=False), dict(half=24, affine=False),
                                dict(half=8, relu=False)], ids=["in-only+addend", "eval", "affine-false", "no-relu"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_ibn_variants_with_idle_threads(dtype, kw, capfd, monkeypatch):
    kw = dict(kw)
    run_ibn((8, 24, 6, 7), dtype, kw.pop("half"), capfd, monkeypatch, **kw)


@pytest.mark.parametrize("kw", [dict(half=520, addend=True), dict(half=264, training=False), dict(half=264, addend=True)],
                         ids=["in-only+addend", "eval", "addend"])
def test_ibn_variants_two_column_blocks(kw, capfd, monkeypatch):
    kw = dict(kw)
    run_ibn((8, 520, 6, 5), F32, kw.pop("half"), capfd, monkeypatch, **kw)


def test_f16(capfd, monkeypatch):
    """one float16 case per family: one row, the partial last column block, the slot loop"""
    check_geometry(run_block((8, 1032, 3, 3), F16, "pre", True, "2", capfd, monkeypatch), "single-launch", (8, 1032, 3, 3), F16, 8, 4)
    check_geometry(run_bn_block((4, 2056, 3, 3), F16, True, capfd, monkeypatch), "bn-block", (4, 2056, 3, 3), F16, 4, 4)
    run_ibn((8, 520, 6, 5), F16, 264, capfd, monkeypatch, addend=True)


def test_which_path_reports_what_runs(capfd, monkeypatch):
    """(3,520,6,5) fp32 has six tiles: no single launch (a grid needs one workgroup per barrier group).  which_path says so, the
    launch is not attempted, the workspace is the same and the values are the two-pass kernels' own, bit for bit."""
    import ctypes as C
    shape, dtype = (3, 520, 6, 5), F32
    x, b, gy = make_inputs(shape, dtype, 77)

    def run(fused):
        with knobs(monkeypatch, CNSN_NHWC_FUSED=fused, CNSN_DEBUG="1"), healthy():
            mod = cnsn_amd.CNSN(None, fill_sn(cnsn_amd.SelfNorm(shape[1]), SN_SEED, torch.float32)).to(DEV).train()
            xg, bg = x.clone(memory_format=CL).requires_grad_(), b.clone(memory_format=CL).requires_grad_()
            cfg = cnsn_amd.FusedConfig(add_mode="pre", relu=True, **mod.selfnorm._fused_args_peek()[0])
            paths = {"fwd": cnsn_amd.which_path(xg, cfg), "bwd": cnsn_amd.which_path(xg, cfg, backward=True)}
            prob = F_._problem(xg, cfg)
            prob.layout = _ffi.LAYOUT_NHWC
            ws = cnsn_amd.lib().cnsn_workspace_bytes(C.byref(prob))
            capfd.readouterr()
            y = mod.forward_block(xg, bg, add_mode="pre", relu=True)
            y.backward(gy.contiguous(memory_format=CL))
            torch.cuda.synchronize()
            seen = launches(capfd.readouterr().err)
        vals = [y.detach(), xg.grad, bg.grad] + [p.grad for p in mod.parameters()] + [v for v in mod.state_dict().values()]
        return paths, seen, ws, vals

    paths, seen, ws, vals = run("2")
    ran = {d for (fam, d), v in seen.items() if fam == "single-launch" and v["status"] == 0}
    for d in ("fwd", "bwd"):
        assert (paths[d] == "resident") == (d in ran), (paths, seen)
    assert paths == {"fwd": "streaming", "bwd": "streaming"} and not seen, (paths, seen)
    paths0, seen0, ws0, vals0 = run("0")
    assert paths0 == paths and not seen0 and ws0 == ws and ws > 0
    assert len(vals) == len(vals0) and all(torch.equal(u, v) for u, v in zip(vals, vals0))
