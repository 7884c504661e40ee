"""The channels-last launches' caller-owned buffers keep their sizes: cnsn_workspace_bytes (layout = NHWC), cnsn_ibn_workspace_bytes,
cnsn_bn_act_workspace_bytes and the three *_saved_floats against integers recorded from the build before the single-launch
families' workspace layouts moved onto one carver (nhwc_host::Carver, csrc/cnsn_nhwc.h).  Without a device the library assumes 256
compute units, so every call here answers on a CPU, and the answer is a pure function of the descriptor.  Equality, no margin.

The size functions take the problem alone: an epilogue's PRE add changes no field of it, so "with and without a PRE add" is one
call and one column (`sn`); SelfNorm in eval mode (`sn_eval`) is recorded next to it because the BatchNorm2d-in-front launches'
region only counts in training mode.

`python tests/test_nhwc_workspace_layout.py` prints the table of the library it finds."""
import ctypes as C

import pytest

import cnsn_amd
from cnsn_amd import _ffi

# the shapes a ResNet-50 runs at batch 256 (BatchNorm2d + ReLU sites, then the four block outputs), then the odd ones: one tile row,
# the smallest tensor, N above a workgroup's 256 threads, channels no power of two, N = 257
SHAPES = [(256, 64, 112, 112), (256, 64, 56, 56), (256, 128, 56, 56), (256, 128, 28, 28), (256, 256, 28, 28), (256, 256, 14, 14),
          (256, 512, 14, 14), (256, 512, 7, 7), (256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7),
          (8, 32, 6, 6), (2, 8, 2, 1), (300, 64, 5, 5), (256, 24, 7, 7), (257, 64, 14, 14)]
DTYPES = {"bf16": _ffi.CNSN_BF16, "fp32": _ffi.CNSN_F32}
PROBLEMS = {"sn": dict(sn_active=1, sn_training=1), "sn_eval": dict(sn_active=1), "sn_two": dict(sn_active=1, sn_two=1, sn_training=1),
            "cnsn": dict(cn_active=1, sn_active=1, sn_training=1)}
COLUMNS = ("ws sn", "ws sn_eval", "ws sn_two", "ws cnsn", "saved sn", "saved sn_eval", "saved sn_two", "saved cnsn",
           "ibn ws half=C/2", "ibn ws half=C", "ibn saved half=C/2", "ibn saved half=C", "bn_act ws train", "bn_act ws eval",
           "bn_act saved train", "bn_act saved eval")


def problem(shape, dtype, **kw):
    p = _ffi.Problem()
    p.struct_bytes = C.sizeof(_ffi.Problem)
    p.dtype = dtype
    p.N, p.C, p.H, p.W = shape
    p.content_box = p.style_box = _ffi.box4(None)
    p.eps_cn, p.eps_sn, p.eps_bn, p.momentum = 1e-5, 1e-12, 1e-5, 0.1
    p.strategy, p.layout = _ffi.STRATEGY_AUTO, _ffi.LAYOUT_NHWC
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def ibn(shape, dtype, half):
    d = _ffi.Ibn()
    d.struct_bytes = C.sizeof(_ffi.Ibn)
    d.dtype = dtype
    d.N, d.C, d.H, d.W = shape
    d.half, d.relu, d.eps_in = half, 1, 1e-5
    d.bn.struct_bytes = C.sizeof(_ffi.BnTail)
    d.bn.training, d.bn.eps, d.bn.momentum = 1, 1e-5, 0.1
    return d


def bn_act(shape, dtype, training):
    d = _ffi.BnAct()
    d.struct_bytes = C.sizeof(_ffi.BnAct)
    d.dtype = dtype
    d.N, d.C, d.H, d.W = shape
    d.relu = 1
    d.bn.struct_bytes = C.sizeof(_ffi.BnTail)
    d.bn.training, d.bn.eps, d.bn.momentum = int(training), 1e-5, 0.1
    return d


def row(lib, shape, dtype):
    probs = [problem(shape, dtype, **kw) for kw in PROBLEMS.values()]
    ibns = [ibn(shape, dtype, shape[1] // 2), ibn(shape, dtype, shape[1])]
    bns = [bn_act(shape, dtype, True), bn_act(shape, dtype, False)]
    return (*(lib.cnsn_workspace_bytes(C.byref(p)) for p in probs), *(lib.cnsn_saved_floats(C.byref(p)) for p in probs),
            *(lib.cnsn_ibn_workspace_bytes(C.byref(d)) for d in ibns), *(lib.cnsn_ibn_saved_floats(C.byref(d)) for d in ibns),
            *(lib.cnsn_bn_act_workspace_bytes(C.byref(d)) for d in bns), *(lib.cnsn_bn_act_saved_floats(C.byref(d)) for d in bns))


# (shape, dtype) -> COLUMNS, recorded from the parent build
EXPECTED = {
    ((256, 64, 112, 112), 'bf16'): (7670272, 7670272, 5047808, 5047808, 655616, 655616, 655616, 655616, 1315072, 1315072, 81920, 81920, 529152, 256, 128, 128),
    ((256, 64, 112, 112), 'fp32'): (7670272, 7670272, 5047808, 5047808, 655616, 655616, 655616, 655616, 1315072, 1315072, 81920, 81920, 529152, 256, 128, 128),
    ((256, 64, 56, 56), 'bf16'): (7670272, 7670272, 5047808, 5047808, 655616, 655616, 655616, 655616, 1315072, 1315072, 81920, 81920, 529152, 256, 128, 128),
    ((256, 64, 56, 56), 'fp32'): (7670272, 7670272, 5047808, 5047808, 655616, 655616, 655616, 655616, 1315072, 1315072, 81920, 81920, 529152, 256, 128, 128),
    ((256, 128, 56, 56), 'bf16'): (15340032, 15340032, 10095104, 10095104, 1311232, 1311232, 1311232, 1311232, 2625792, 2625792, 163840, 163840, 1053952, 256, 256, 256),
    ((256, 128, 56, 56), 'fp32'): (15340032, 15340032, 10095104, 10095104, 1311232, 1311232, 1311232, 1311232, 2625792, 2625792, 163840, 163840, 1053952, 256, 256, 256),
    ((256, 128, 28, 28), 'bf16'): (14815744, 14815744, 9570816, 9570816, 1311232, 1311232, 1311232, 1311232, 2101504, 2101504, 163840, 163840, 1053952, 256, 256, 256),
    ((256, 128, 28, 28), 'fp32'): (15340032, 15340032, 10095104, 10095104, 1311232, 1311232, 1311232, 1311232, 2625792, 2625792, 163840, 163840, 1053952, 256, 256, 256),
    ((256, 256, 28, 28), 'bf16'): (30679552, 30679552, 20189696, 20189696, 2622464, 2622464, 2622464, 2622464, 5247232, 5247232, 327680, 327680, 2103552, 256, 512, 512),
    ((256, 256, 28, 28), 'fp32'): (30679552, 30679552, 20189696, 20189696, 2622464, 2622464, 2622464, 2622464, 5247232, 5247232, 327680, 327680, 2103552, 256, 512, 512),
    ((256, 256, 14, 14), 'bf16'): (28058112, 28058112, 17568256, 17568256, 2622464, 2622464, 2622464, 2622464, 2625792, 2625792, 327680, 327680, 1054976, 256, 512, 512),
    ((256, 256, 14, 14), 'fp32'): (29630976, 29630976, 19141120, 19141120, 2622464, 2622464, 2622464, 2622464, 4198656, 4198656, 327680, 327680, 1054976, 256, 512, 512),
    ((256, 512, 14, 14), 'bf16'): (59261440, 59261440, 38281728, 38281728, 5244928, 5244928, 5244928, 5244928, 8392960, 8392960, 655360, 655360, 2105600, 256, 1024, 1024),
    ((256, 512, 14, 14), 'fp32'): (61358592, 61358592, 40378880, 40378880, 5244928, 5244928, 5244928, 5244928, 6295808, 6295808, 655360, 655360, 2105600, 256, 1024, 1024),
    ((256, 512, 7, 7), 'bf16'): (54018560, 54018560, 33038848, 33038848, 5244928, 5244928, 5244928, 5244928, 3150080, 3150080, 655360, 655360, 532736, 256, 1024, 1024),
    ((256, 512, 7, 7), 'fp32'): (56115712, 56115712, 35136000, 35136000, 5244928, 5244928, 5244928, 5244928, 3150080, 3150080, 655360, 655360, 532736, 256, 1024, 1024),
    ((256, 256, 56, 56), 'bf16'): (30679552, 30679552, 20189696, 20189696, 2622464, 2622464, 2622464, 2622464, 5247232, 5247232, 327680, 327680, 2103552, 256, 512, 512),
    ((256, 256, 56, 56), 'fp32'): (30679552, 30679552, 20189696, 20189696, 2622464, 2622464, 2622464, 2622464, 5247232, 5247232, 327680, 327680, 2103552, 256, 512, 512),
    ((256, 512, 28, 28), 'bf16'): (61358592, 61358592, 40378880, 40378880, 5244928, 5244928, 5244928, 5244928, 10490112, 10490112, 655360, 655360, 4202752, 256, 1024, 1024),
    ((256, 512, 28, 28), 'fp32'): (61358592, 61358592, 40378880, 40378880, 5244928, 5244928, 5244928, 5244928, 6295808, 6295808, 655360, 655360, 4202752, 256, 1024, 1024),
    ((256, 1024, 14, 14), 'bf16'): (122716672, 122716672, 80757248, 80757248, 10489856, 10489856, 10489856, 10489856, 12587264, 12587264, 1310720, 1310720, 4206848, 256, 2048, 2048),
    ((256, 1024, 14, 14), 'fp32'): (122716672, 122716672, 80757248, 80757248, 10489856, 10489856, 10489856, 10489856, 8392960, 8392960, 1310720, 1310720, 4206848, 256, 2048, 2048),
    ((256, 2048, 7, 7), 'bf16'): (237044224, 237044224, 153125376, 153125376, 20979712, 20979712, 20979712, 20979712, 12587264, 12587264, 2621440, 2621440, 2117888, 256, 4096, 4096),
    ((256, 2048, 7, 7), 'fp32'): (228655616, 228655616, 144736768, 144736768, 20979712, 20979712, 20979712, 20979712, 12587264, 12587264, 2621440, 2621440, 2117888, 256, 4096, 4096),
    ((8, 32, 6, 6), 'bf16'): (107008, 107008, 65536, 65536, 10368, 10368, 10368, 10368, 10496, 10496, 1280, 1280, 5632, 256, 64, 64),
    ((8, 32, 6, 6), 'fp32'): (107008, 107008, 65536, 65536, 10368, 10368, 10368, 10368, 10496, 10496, 1280, 1280, 5632, 256, 64, 64),
    ((2, 8, 2, 1), 'bf16'): (7680, 7680, 4864, 4864, 672, 672, 672, 672, 5120, 5120, 80, 80, 4864, 256, 16, 16),
    ((2, 8, 2, 1), 'fp32'): (7680, 7680, 4864, 4864, 672, 672, 672, 672, 5120, 5120, 80, 80, 4864, 256, 16, 16),
    ((300, 64, 5, 5), 'bf16'): (7912960, 7912960, 4839936, 4839936, 768256, 768256, 768256, 768256, 465152, 465152, 96000, 96000, 64256, 256, 128, 128),
    ((300, 64, 5, 5), 'fp32'): (7912960, 7912960, 4839936, 4839936, 768256, 768256, 768256, 768256, 465152, 465152, 96000, 96000, 64256, 256, 128, 128),
    ((256, 24, 7, 7), 'bf16'): (2532864, 2532864, 1549312, 1549312, 245856, 245856, 245856, 245856, 151808, 151808, 30720, 30720, 42240, 256, 48, 48),
    ((256, 24, 7, 7), 'fp32'): (2532864, 2532864, 1549312, 1549312, 245856, 245856, 245856, 245856, 151808, 151808, 30720, 30720, 42240, 256, 48, 48),
    ((257, 64, 14, 14), 'bf16'): (6779136, 6779136, 4146432, 4146432, 658176, 658176, 658176, 658176, 399104, 399104, 82240, 82240, 401664, 256, 128, 128),
    ((257, 64, 14, 14), 'fp32'): (6779136, 6779136, 4146432, 4146432, 658176, 658176, 658176, 658176, 399104, 399104, 82240, 82240, 265472, 256, 128, 128),
}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sizes_are_the_recorded_ones(shape, dtype):
    got = row(cnsn_amd.lib(), shape, DTYPES[dtype])
    want = EXPECTED[(shape, dtype)]
    assert len(got) == len(want) == len(COLUMNS)
    for name, g, w in zip(COLUMNS, got, want):
        assert g == w, f"{name}: {g} bytes / floats, recorded {w}"


def test_the_table_is_not_trivial():
    """every shape and dtype has a row, and every column but the eval launch's (no workspace: the 256 spare bytes) varies"""
    assert set(EXPECTED) == {(s, d) for s in SHAPES for d in DTYPES}
    for i, name in enumerate(COLUMNS):
        col = {v[i] for v in EXPECTED.values()}
        assert min(col) > 0 and (len(col) > 1 or name == "bn_act ws eval"), name


if __name__ == "__main__":
    for s in SHAPES:
        for d in DTYPES:
            print(f"    ({s}, {d!r}): {row(cnsn_amd.lib(), s, DTYPES[d])},")
