"""The tile rule of the BatchNorm2d (+ add) + ReLU single launch (bn_act_geom in csrc/cnsn_nhwc_bn.hip, walked by BnActTile /
bn_act_rows_sum in csrc/cnsn_nhwc_bn_kernels.h) across its OWN geometry.  This family does not use the tile walker the other
three channels-last families share (tests/test_gpu_nhwc_geometry.py): it cuts the R x C matrix (R = N*H*W) into row chunks and
balanced column blocks and aims at 1024 tiles of at least 64 rows.

Over every shape tests/test_gpu_bn_act.py gives the training launch, tcb (vector columns per block) is 2 .. 64 in powers of
two, rows * tcb == 256, rows >= 4, and a workgroup walks at most two tiles.  The classes below never ran there:
  idle        rows * tcb < 256: threads with r >= rows (the `t.r < g.rows` guard of bn_act_rows_sum, `active` of BnActTile)
  odd         tcb odd and above 1
  wide        tcb > 64: a matrix row spans two to four wavefronts
  full256     tcb == 256: the widest block the rule knows
  rows_1      one row per workgroup: the LDS merge adds a single row
  rows_few    two or three rows
  partial     tc % tcb != 0: the last column block lies partly outside the matrix (`vc < g.tc`, `first + off >= g.C`)
  ncb_odd     8 is no multiple of ncb, several chunks per block: a workgroup's successive tiles change column block
  short_last  the last row chunk is shorter than the others
  no_row      chunk < rows: threads of a live row index without a row (the `cnt` arithmetic of the reverse walks, zero sums)
  tail_tiles  tiles % 8 != 0: the grid (a multiple of 8) is smaller than the tile count whatever the device
The rule only leaves the narrowest block (8 vector columns a pass, balanced) once ncb * (R // 64) >= 1024 holds for a wider
one, so a block above 64 columns needs R // 64 >= 1024 / ncb rows of 64: the WIDE lists are the smallest tensors that reach
each class (45 .. 256 MB); they are drawn and checked on the GPU one at a time, like the full-size cases of test_gpu_bn_act.py.

Every case goes through run_case of tests/test_gpu_bn_act.py — the float64 torch oracle and the fp32 / 16-bit bars of that
file's `compare`, unchanged — under CNSN_NHWC_FUSED=2 and CNSN_DEBUG=1, and asserts that each direction printed ONE launch
with status 0 whose R, C, tiles, ncb, tcb, rows, chunk and keep are what the rule re-stated below gives.

test_results_do_not_depend_on_the_grid holds the kernel header's claim ("every result does not depend on how many workgroups
the grid got"): with CNSN_HEADROOM_CUS = compute units - 8 reshost::grid_for sizes the grid for 8 compute units — at most 8
workgroups of 256 threads each, so at most 64 — and every output is bit-identical to the full grid's.

test_relu_mask_where_the_pre_activation_is_zero: channels with weight 0, where v = fmaf(0, x - mean, bias) is the bias exactly.
The oracle is differentiated through the device's own `y > 0`, so a wrong mask at an exact zero is invisible to it; here the
values and the mask are asserted exactly."""
import re
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TILES, MIN_ROWS, BLOCK, EVAL_ITERS = 1024, 64, 256, 8       # kBnActTiles, kBnActMinRows, kBlock, kBnActEvalIters
KEEP_BYTES = 320 << 20                                      # keep_first_read (csrc/cnsn_nhwc.h)


def geom(shape, dtype, eval_mode=False):
    """bn_act_geom re-stated (csrc/cnsn_nhwc_bn.hip)"""
    n, c, h, w = shape
    r, tc = n * h * w, c // (16 // (torch.finfo(dtype).bits // 8))
    slots = max(r // MIN_ROWS, 1)
    for t in (256, 128, 64, 32, 16, 8):
        ncb = -(-tc // t)
        tcb = -(-tc // ncb)
        if eval_mode or ncb * slots >= TILES:
            break
    ncb = -(-tc // tcb)
    rows = BLOCK // tcb
    chunk = rows * EVAL_ITERS if eval_mode else -(-r // min(-(-TILES // ncb), slots))
    wpc = -(-r // chunk)
    return dict(R=r, C=c, tc=tc, tcb=tcb, rows=rows, ncb=ncb, wpc=wpc, chunk=chunk, tiles=ncb * wpc)


def keep_of(direction, shape, dtype, relu, addend):
    """keep_first_read re-stated: the forward streams x once before it is read again, the backward gy and x (and the addend
    behind a ReLU)"""
    n, c, h, w = shape
    tensors = 1 if direction == "fwd" else (3 if (relu and addend) else 2)
    return int(tensors * n * c * h * w * (torch.finfo(dtype).bits // 8) <= KEEP_BYTES)


def classes(shape, dtype):
    g = geom(shape, dtype)
    out = set()
    if g["rows"] * g["tcb"] < BLOCK:
        out.add("idle")
    if g["tcb"] % 2 and g["tcb"] > 1:
        out.add("odd")
    if g["tcb"] > 64:
        out.add("wide")
    if g["tcb"] == 256:
        out.add("full256")
    if g["rows"] == 1:
        out.add("rows_1")
    if g["rows"] in (2, 3):
        out.add("rows_few")
    if g["tc"] % g["tcb"]:
        out.add("partial")
    if 8 % g["ncb"] and g["wpc"] > 1:
        out.add("ncb_odd")
    if g["R"] % g["chunk"]:
        out.add("short_last")
    if g["chunk"] < g["rows"]:
        out.add("no_row")
    if g["tiles"] % 8:
        out.add("tail_tiles")
    return out


ALL = {"idle", "odd", "wide", "full256", "rows_1", "rows_few", "partial", "ncb_odd", "short_last", "no_row", "tail_tiles"}

SMALL32 = [(8, 24, 8, 9),          # tcb 6, rows 42: 4 idle threads, 9 tiles
           (8, 72, 8, 9),          # tcb 6, ncb 3: 27 tiles
           (10, 4, 8, 8)]          # tcb 1, rows 256, chunk 64: 192 threads without a row
SMALL16 = [(8, 40, 8, 9),          # tcb 5, rows 51: 1 idle thread
           (8, 72, 9, 9),          # tcb 5, ncb 2: the last block holds 4 of 5 columns, the last chunk 63 of 65 rows
           (8, 136, 9, 9),         # tcb 6, ncb 3: the last block holds 5 of 6 columns
           (10, 8, 8, 8)]          # tcb 1, rows 256
WIDE32 = [(22, 520, 32, 32),       # 45 MB: tcb 44, ncb 3, rows 5, last block 42 columns, last chunk 22 rows, 1026 tiles
          (32, 520, 32, 32),       # 65 MB: tcb 65, ncb 2, rows 3, 61 idle threads
          (64, 520, 32, 32),       # 130 MB: tcb 130, rows 1, 126 idle threads
          (16, 2056, 32, 32),      # 128 MB: tcb 103, ncb 5, rows 2, last block 102 columns, 1025 tiles
          (64, 1024, 32, 32)]      # 256 MB: tcb 256, rows 1
WIDE16 = [(32, 1040, 32, 32),      # 65 MB: tcb 65, rows 3
          (64, 1032, 32, 32),      # 129 MB: tcb 129, rows 1
          (33, 2056, 32, 32),      # 133 MB: tcb 129, ncb 2, last block 128 columns, chunk 66
          (64, 2048, 32, 32)]      # 256 MB: tcb 256
# the cases that also run with an addend (the ADD instantiations: two rows in flight in phase C, a second output of the
# backward) and without the ReLU
VARIANT32, VARIANT16 = SMALL32 + [(22, 520, 32, 32)], SMALL16 + [(33, 2056, 32, 32)]
# one float16 case each for rows_1, partial and idle
F16_CASES = [((64, 1032, 32, 32), "rows_1"), ((8, 72, 9, 9), "partial"), ((8, 40, 8, 9), "idle")]
# tests/test_gpu_bn_act.py::TOY (asserted equal to it below, once that module may be imported)
TOY = [(4, 8, 8, 8), (6, 16, 9, 11), (3, 520, 6, 5), (9, 2048, 7, 7), (300, 64, 5, 5)]
# results against the grid: more tiles than the 64 workgroups a grid sized for 8 compute units can have
GRID = [((9, 2048, 7, 7), F32), ((9, 2048, 7, 7), BF16), ((300, 64, 5, 5), F32), ((300, 64, 5, 5), BF16),
        ((80, 72, 8, 9), F32),             # tcb 6, ncb 3: 270 tiles
        ((80, 136, 9, 9), BF16),           # tcb 6, ncb 3, partial: 300 tiles
        ((22, 520, 32, 32), F32), ((16, 2056, 32, 32), F32), ((33, 2056, 32, 32), BF16)]   # ~1024 tiles of changing column block


def taken(shape, dtype):
    """bn_act_ok's shape conditions of the training launch: whole 16-byte vectors, at least 8 tiles"""
    return (shape[1] * (torch.finfo(dtype).bits // 8)) % 16 == 0 and geom(shape, dtype)["tiles"] >= 8


assert set().union(*(classes(s, F32) for s in SMALL32 + WIDE32)) == ALL
assert set().union(*(classes(s, BF16) for s in SMALL16 + WIDE16)) == ALL
assert all(classes(s, F32) for s in SMALL32 + WIDE32) and all(classes(s, BF16) for s in SMALL16 + WIDE16)
assert all(taken(s, F32) for s in SMALL32 + WIDE32) and all(taken(s, d) for s in SMALL16 + WIDE16 for d in (BF16, F16))
assert all(geom(s, F16) == geom(s, BF16) and k in classes(s, F16) for s, k in F16_CASES)
assert not any(classes(s, d) & {"idle", "odd", "wide", "rows_1", "rows_few"} for s in TOY for d in (F32, BF16, F16))   # the gap
assert all(taken(s, d) and geom(s, d)["tiles"] > 64 for s, d in GRID)
# the figures quoted next to the lists
assert geom((22, 520, 32, 32), F32) == dict(R=22528, C=520, tc=130, tcb=44, rows=5, ncb=3, wpc=342, chunk=66, tiles=1026)
assert geom((16, 2056, 32, 32), F32) == dict(R=16384, C=2056, tc=514, tcb=103, rows=2, ncb=5, wpc=205, chunk=80, tiles=1025)
assert {k: geom((64, 520, 32, 32), F32)[k] for k in ("tcb", "rows", "ncb")} == dict(tcb=130, rows=1, ncb=1)
assert {k: geom((33, 2056, 32, 32), BF16)[k] for k in ("tcb", "rows", "ncb", "chunk")} == dict(tcb=129, rows=1, ncb=2, chunk=66)
assert geom((64, 1024, 32, 32), F32)["tcb"] == geom((64, 2048, 32, 32), BF16)["tcb"] == 256
assert geom((3, 520, 6, 5), F32, True)["tcb"] == 130 and geom((3, 520, 6, 5), F32, True)["rows"] == 1     # (eval: TOY reaches it)
# both cache policies of the backward are reached (the forward's tensors all fit)
assert {keep_of("bwd", s, F32, True, False) for s in WIDE32} == {keep_of("bwd", s, BF16, True, False) for s in WIDE16} == {0, 1}

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from tests import test_gpu_bn_act as bn  # noqa: E402
from tests.test_gpu_nhwc_full_size import healthy, knobs  # noqa: E402

assert TOY == bn.TOY
CUS = torch.cuda.get_device_properties(0).multi_processor_count      # (reshost::cu_count: hipDeviceAttributeMultiprocessorCount)
NAME = {F32: "fp32", BF16: "bf16", F16: "f16"}
_LINE = re.compile(r"\[cnsn\] nhwc bn_act (fwd|bwd): R=(\d+) C=(\d+) tiles=(\d+) \(ncb=(\d+) tcb=(\d+) rows=(\d+) chunk=(\d+)\) "
                   r"keep=(\d) -> status (-?\d+) grid=(\d+)")
_ANY = re.compile(r"\[cnsn\] nhwc bn_act (fwd|bwd):")


def ids(cases):
    return ["x".join(map(str, s)) + "-" + NAME[d] for s, d in cases]


def launches(err):
    """the two CNSN_DEBUG lines of a training step: {direction: the printed numbers}; every bn_act line must parse"""
    out = {}
    for m in _LINE.finditer(err):
        assert m.group(1) not in out, f"two {m.group(1)} launches in one case:\n{err}"
        keys = ("R", "C", "tiles", "ncb", "tcb", "rows", "chunk", "keep", "status", "grid")
        out[m.group(1)] = dict(zip(keys, (int(v) for v in m.groups()[1:])))
    assert len(_ANY.findall(err)) == len(out), err
    return out


def run(shape, dtype, capfd, monkeypatch, relu=True, addend=False, env=None, **kw):
    """run_case under CNSN_NHWC_FUSED=2 and CNSN_DEBUG=1; one forward and one backward launch, status 0, the re-stated geometry.
    Returns (the device's tensors, run_case's margins, the launches)"""
    out = {}
    with knobs(monkeypatch, CNSN_NHWC_FUSED="2", CNSN_DEBUG="1", **(env or {})), healthy():
        capfd.readouterr()
        try:
            margins = bn.run_case(shape, dtype, relu=relu, addend=addend, seed=sum(shape) % 1000, out=out, **kw)
        finally:
            cap = capfd.readouterr()
            sys.stdout.write(cap.out)           # (run_case's figures: `pytest -s` shows them)
    seen = launches(cap.err)
    want = geom(shape, dtype)
    print(f"    geometry {want} classes {sorted(classes(shape, dtype))}\n    launches {seen}")
    assert set(seen) == {"fwd", "bwd"}, cap.err
    for direction, v in seen.items():
        assert v["status"] == 0, seen
        assert {k: v[k] for k in ("R", "C", "tiles", "ncb", "tcb", "rows", "chunk")} == {
            k: want[k] for k in ("R", "C", "tiles", "ncb", "tcb", "rows", "chunk")}, (v, want)
        assert v["keep"] == keep_of(direction, shape, dtype, relu, addend), (direction, v)
        assert 8 <= v["grid"] <= (v["tiles"] & ~7) and v["grid"] % 8 == 0, v
    return out, margins, seen


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


VARIANTS = [(True, False), (True, True), (False, False)]
VARIANT_IDS = ["relu", "relu+addend", "id"]
SMALL = [(s, F32) for s in SMALL32] + [(s, BF16) for s in SMALL16]
WIDE = [(s, F32) for s in WIDE32] + [(s, BF16) for s in WIDE16]


@pytest.mark.parametrize("relu,addend", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("shape,dtype", SMALL, ids=ids(SMALL))
def test_small_shapes(shape, dtype, relu, addend, capfd, monkeypatch):
    run(shape, dtype, capfd, monkeypatch, relu=relu, addend=addend)


@pytest.mark.parametrize("shape,dtype", WIDE, ids=ids(WIDE))
def test_wide_shapes(shape, dtype, capfd, monkeypatch):
    try:
        _, margins, _ = run(shape, dtype, capfd, monkeypatch, gen_dev="cuda")
        print("    err / bound: " + " ".join(f"{k} {e / b:.3f}" for k, (e, b) in margins.items()))
    finally:
        free()


WIDE_VARIANTS = [((22, 520, 32, 32), F32), ((33, 2056, 32, 32), BF16)]


@pytest.mark.parametrize("relu,addend", VARIANTS[1:], ids=VARIANT_IDS[1:])
@pytest.mark.parametrize("shape,dtype", WIDE_VARIANTS, ids=ids(WIDE_VARIANTS))
def test_wide_shapes_with_an_addend_and_without_relu(shape, dtype, relu, addend, capfd, monkeypatch):
    try:
        _, margins, _ = run(shape, dtype, capfd, monkeypatch, relu=relu, addend=addend, gen_dev="cuda")
        print("    err / bound: " + " ".join(f"{k} {e / b:.3f}" for k, (e, b) in margins.items()))
    finally:
        free()


@pytest.mark.parametrize("shape,kind", F16_CASES, ids=[k for _, k in F16_CASES])
def test_f16(shape, kind, capfd, monkeypatch):
    try:
        run(shape, F16, capfd, monkeypatch, relu=True, addend=kind != "rows_1", gen_dev="cuda" if kind == "rows_1" else "cpu")
    finally:
        free()


COMPARED = ("y", "dx", "d_addend", "d_weight", "d_bias", "running_mean", "running_var")


@pytest.mark.parametrize("shape,dtype", GRID, ids=ids(GRID))
def test_results_do_not_depend_on_the_grid(shape, dtype, capfd, monkeypatch):
    """y = relu(bn(x) + addend), forward and backward, on the grid the device gives and on one of at most 64 workgroups (fewer
    than the tiles: every workgroup walks several tiles, of changing column block where ncb does not divide the grid)"""
    big = shape[0] * shape[1] * shape[2] * shape[3] > (1 << 22)
    kw = dict(relu=True, addend=True, gen_dev="cuda" if big else "cpu")
    try:
        full, _, seen_full = run(shape, dtype, capfd, monkeypatch, **kw)
        for k in ("ref64", "ref32", "gy"):
            full.pop(k)
        small, _, seen_small = run(shape, dtype, capfd, monkeypatch, env=dict(CNSN_HEADROOM_CUS=str(CUS - 8)), **kw)
        for direction in ("fwd", "bwd"):
            tiles, grid = seen_small[direction]["tiles"], seen_small[direction]["grid"]
            assert grid <= 64 < tiles, seen_small
            assert seen_full[direction]["grid"] > grid, (seen_full, seen_small)
        print(f"    grids: {seen_full['fwd']['grid']} and {seen_small['fwd']['grid']} workgroups for {seen_small['fwd']['tiles']} tiles")
        for k in COMPARED:
            assert torch.equal(full[k], small[k]), f"{k} depends on the grid"
    finally:
        full = small = None
        free()


# ---- the ReLU mask where the pre-activation is exactly zero
Z_BIAS0, Z_TINY, Z_HALF, Z_ROUND = 0, 1, 2, 3           # the channels with weight 0
TINY = 2.0 ** -26                                        # a float and a bfloat16; rounds to zero as a float16 (half its least subnormal)
ROUND = 1.0 + 2.0 ** -10                                 # a float and a float16; 1 as a bfloat16


def zero_weight_channels(addend):
    def edit(mod, x64, a64):
        n, c, h, w = x64.shape
        chans = (Z_BIAS0, Z_TINY, Z_HALF, Z_ROUND) if addend else (Z_BIAS0, Z_TINY)
        for ch in chans:
            mod.weight[ch] = 0.0
        mod.bias[Z_BIAS0] = 0.0
        mod.bias[Z_TINY] = TINY
        if addend:
            odd = (torch.arange(n * h * w, device=a64.device).view(n, h, w) % 2).to(a64.dtype)     # the row of the R x C matrix
            a64[:, Z_BIAS0] = 0.0
            a64[:, Z_TINY] = 0.0
            mod.bias[Z_HALF] = 0.5
            a64[:, Z_HALF] = odd - 0.5                   # -0.5 on even rows, +0.5 on odd rows: the sum is 0 or 1
            mod.bias[Z_ROUND] = ROUND
            a64[:, Z_ROUND] = -1.0
    return edit


@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+a"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "f16"])
def test_relu_mask_where_the_pre_activation_is_zero(dtype, addend, capfd, monkeypatch):
    """weight 0: v is the bias exactly in any dtype.  bias 0 -> y = 0, mask closed; bias 2^-26 -> stored as 0 in float16 (mask
    closed), as itself in bfloat16 and float (open); with an addend bias 0.5 -+ 0.5 -> 0 / 1 by row; bias 1 + 2^-10 and addend -1
    -> BatchNorm2d's output is rounded to the tensor's type before the sum, as the un-fused sequence does: 1 - 1 = 0 in bfloat16
    (closed; a kernel that sums in float would open it), 2^-10 in float16 and float."""
    shape = (8, 24, 8, 9) if dtype == F32 else (8, 40, 8, 9)
    out, _, _ = run(shape, dtype, capfd, monkeypatch, relu=True, addend=addend, edit=zero_weight_channels(addend))
    y, gy = out["y"], out["gy"].to(out["y"].device)
    n, c, h, w = shape
    odd = (torch.arange(n * h * w, device=y.device).view(n, h, w) % 2).to(dtype)
    want = {Z_BIAS0: torch.zeros(n, h, w, device=y.device, dtype=dtype),
            Z_TINY: torch.full((n, h, w), 0.0 if dtype == F16 else TINY, device=y.device, dtype=dtype)}
    if addend:
        want[Z_HALF] = odd
        want[Z_ROUND] = torch.full((n, h, w), 0.0 if dtype == BF16 else 2.0 ** -10, device=y.device, dtype=dtype)
    assert float(want[Z_TINY].max()) == (0.0 if dtype == F16 else TINY)                      # (what the dtype holds)
    for ch, v in want.items():
        assert torch.equal(y[:, ch], v), f"y of channel {ch}: {y[:, ch].unique()}"
        assert not bool(out["dx"][:, ch].count_nonzero()), f"dx of channel {ch} (weight 0)"
    if addend:
        assert torch.equal(out["d_addend"], gy * (y > 0)), "d_addend is not gy under the mask of y"
        for ch, v in want.items():
            assert torch.equal(out["d_addend"][:, ch], gy[:, ch] * (v > 0)), f"d_addend of channel {ch}"
    # d_bias of each channel: the sum of gy under the EXPECTED mask (float64; float32 for the oracle's own noise), the
    # parameter bar of test_gpu_bn_act.py::compare
    for ch, v in want.items():
        masked = gy[:, ch] * (v > 0)
        bn.compare(f"d_bias[{ch}]", out["d_bias"][ch:ch + 1], masked.double().sum().view(1), masked.float().sum().view(1), dtype,
                   param=True)
        if not bool((v > 0).any()):
            assert float(out["d_bias"][ch]) == 0.0
