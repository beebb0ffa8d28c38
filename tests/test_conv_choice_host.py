"""launch_conv's kernel choice (csrc/conv_igemm.hip: conv_validate, conv_choose, the instance tables) through the host-only hook irsde_debug_conv_choice.
No device is touched: the hook takes the compute-unit count as an argument and uses the default tuning knobs unless it is handed others.

tests/golden/conv_choice_pins.txt holds what the dispatch chose BEFORE conv_choose existed (the nested branches of launch_conv, recorded from a copy of
that code whose launch sites printed their template parameters, grid and LDS size) for the literal case list pin_cases() — recorded values, never
produced by the function under test.  (Four lines, the fused-LayerNorm layers on 16-bit operands, were re-recorded when that choice turned out to be a bug:
tests/golden/README.md.)"""
import ctypes
import itertools
import os
import re

import pytest

from image_restoration_sde_amd import _lib

# the hook's arguments, in order
FIELDS = ("B", "H", "W", "C0", "C1", "Cout", "K", "stride", "pad", "up", "op", "st", "pair", "feat", "splits", "nz", "tune", "cu")
BIAS, FILM, SILU, RES, IN_SCALE, CH_SCALE, GATE, SHUFFLE, LN_G = (1 << i for i in range(9))
F32, BF16, FP16, BF16_ACT, FP16_ACT, PAIR_BF16, PAIR_FP16 = (0, 0, 0), (1, 0, 0), (2, 0, 0), (1, 1, 0), (2, 2, 0), (1, 0, 1), (2, 0, 1)   # (op, st, pair)
TUNE_CODES = (0, 3, 5, 6, 7, 50, 60, 61, 64, 65, 70, 71, 72, 73)
KNOB_NAMES = ("small_bn", "small_bn_f32", "pair_tile256", "pair_inscale256", "no_bufa", "zloop", "zloop_1x1", "zloop_maxnk", "zloop_minblk", "zloop_deep", "zloop_ragged64")
KNOB_DEFAULTS = (2, 0, 1, 0, 0, -1, -1, 32, 1024, 1, 2048)


def case(B, H, W, C0, C1, Cout, K, stride=1, pad=None, up=0, mode=F32, feat=0, splits=1, nz=1, tune=0, cu=256):
    return (B, H, W, C0, C1, Cout, K, stride, K // 2 if pad is None else pad, up) + mode + (feat, splits, nz, tune, cu)


_buf = ctypes.create_string_buffer(512)


def choose(c, knobs=None):
    """The hook's line as a dict, or the refusal's message as a str"""
    L = _lib.lib()
    kn = (ctypes.c_int * 11)(*knobs) if knobs else None
    if L.irsde_debug_conv_choice(*c, kn, _buf, len(_buf)) != 0:
        return L.irsde_last_error().decode()
    return dict(kv.split("=") for kv in _buf.value.decode().replace(" of ", "/").split())


def short(d):
    """(name, op, act, inscale, zbatch, zrows, grid, threads, lds) — PINNED's form"""
    assert d["tile"] == "0x0" if d["name"] in ("narrow3", "halo") else re.fullmatch(r"(igemm|pair|zloop|zloop1x1_)" + d["tile"], d["name"]), d
    return (d["name"], int(d["op"]), int(d["act"]), int(d["inscale"]), int(d["zbatch"]), int(d["zrows"]), d["grid"], int(d["threads"]), int(d["lds"]))


# tests/test_gpu_parity.py CONV_CASES: (B, C0, C1, H, W, Cout, K, stride, pad, in_shift, bias, film, silu, res)
CONV_CASES = [
    (2, 64, 0, 24, 20, 64, 3, 1, 1, 0, False, True, True, False),
    (2, 64, 0, 24, 20, 64, 3, 1, 1, 0, False, False, True, True),
    (1, 128, 64, 16, 16, 128, 3, 1, 1, 0, False, True, True, False),
    (1, 128, 64, 16, 16, 128, 1, 1, 0, 0, False, False, False, False),
    (2, 64, 0, 12, 12, 384, 1, 1, 0, 0, False, False, False, False),
    (2, 128, 0, 12, 12, 256, 1, 1, 0, 0, True, False, False, False),
    (2, 128, 0, 12, 12, 64, 1, 1, 0, 0, True, False, False, False),
    (2, 64, 0, 16, 24, 128, 4, 2, 1, 0, True, False, False, False),
    (2, 128, 0, 8, 12, 64, 3, 1, 1, 1, True, False, False, False),
    (2, 64, 0, 24, 20, 3, 3, 1, 1, 0, True, False, False, False),
    (1, 64, 0, 256, 256, 3, 3, 1, 1, 0, True, False, False, False),
    (1, 32, 0, 7, 9, 96, 3, 1, 1, 0, False, False, True, False),
    (1, 1024, 512, 4, 4, 256, 3, 1, 1, 0, False, True, True, False),
    (2, 256, 0, 12, 20, 256, 3, 1, 1, 0, True, False, True, True),
    (1, 256, 0, 6, 10, 256, 3, 1, 1, 1, True, False, False, False),
    (2, 64, 32, 20, 70, 160, 3, 1, 1, 0, True, True, True, True),
    (1, 64, 0, 17, 33, 128, 3, 1, 1, 1, True, False, False, False),
]


def pin_cases():
    out = []
    for B, C0, C1, H, W, Cout, K, stride, pad, up, bias, film, silu, res in CONV_CASES:
        for mode in (F32, BF16, FP16, BF16_ACT, FP16_ACT, PAIR_BF16):
            out.append(case(B, H, W, C0, C1, Cout, K, stride, pad, up, mode, BIAS * bias | FILM * film | SILU * silu | RES * res))
    # the 16 x 256^2 U-Net (nf = 64, depth 4): direct 3x3 layers of the four levels, a concat layer, the 4x4 stride-2 and upsampling convs, the attention
    # 1x1 layers, the final conv; the component GEMMs of its three-launch Winograd layers (16 and 36 components)
    unet = [(16, 256, 256, 64, 0, 64, 3), (16, 128, 128, 128, 0, 128, 3), (16, 64, 64, 256, 0, 256, 3), (16, 32, 32, 512, 0, 512, 3),
            (16, 64, 64, 256, 256, 256, 3), (16, 32, 32, 512, 512, 512, 3), (16, 256, 256, 64, 0, 3, 3), (16, 256, 256, 64, 0, 384, 1), (16, 256, 256, 128, 0, 64, 1),
            (16, 32, 32, 512, 0, 1536, 1), (16, 32, 32, 128, 0, 512, 1)]
    for g in unet:
        for mode in (F32, BF16, FP16, BF16_ACT, PAIR_FP16):
            out.append(case(*g, mode=mode, feat=BIAS))
    out += [case(16, 256, 256, 64, 0, 128, 4, 2, 1, mode=m, feat=BIAS) for m in (F32, BF16, PAIR_BF16)]
    out += [case(16, 32, 32, 512, 0, 256, 3, up=1, mode=m, feat=BIAS) for m in (F32, BF16, BF16_ACT)]
    for T, Cin, Cout, nz in [(65536, 64, 64, 36), (16384, 128, 128, 36), (4096, 256, 256, 36), (1024, 512, 512, 36), (1024, 1024, 512, 36), (256, 1024, 1024, 36),
                             (65536, 128, 128, 16), (512, 512, 512, 36), (8192, 128, 256, 16), (4096, 1056, 256, 36), (2048, 640, 256, 36)]:
        out += [case(1, 1, T, Cin, 0, Cout, 1, nz=nz, cu=cu, tune=t) for cu in (256, 64) for t in (0, 70, 71, 72)]
    # B = 2 NAFNet (width 64, 256^2) 1x1 layers on 16-bit operands: IRSDE_SMALL_BN narrows the column tile by M and the CU count
    for H, c in [(256, 64), (128, 128), (64, 256), (32, 512), (16, 1024)]:
        for Cout, feat in [(c, IN_SCALE | CH_SCALE | RES | BIAS), (2 * c, GATE | BIAS), (c, CH_SCALE | RES | BIAS)]:
            for mode in (BF16, FP16, FP16_ACT, F32):
                out += [case(2, H, H, c, 0, Cout, 1, mode=mode, feat=feat, cu=cu, tune=t) for cu in (256, 64) for t in (0, 7)]
    # the tuning codes on the small shapes of the hook tests, and the quirks
    small = [(1, 8, 8, 32, 32, 64, 3), (2, 8, 12, 64, 0, 128, 3), (1, 8, 8, 64, 0, 256, 3), (1, 8, 8, 64, 0, 64, 1), (2, 12, 12, 64, 0, 384, 1), (16, 64, 64, 256, 0, 256, 1)]
    for g in small:
        for mode in (F32, BF16, FP16, BF16_ACT, FP16_ACT, PAIR_BF16, PAIR_FP16):
            out += [case(*g, mode=mode, feat=BIAS | SILU | RES, tune=t) for t in (3, 5, 6, 50, 60, 61, 64, 65, 70, 71, 72, 73)]
    for mode in (F32, BF16, FP16, FP16_ACT, PAIR_BF16, PAIR_FP16):   # SCA-scaled layers: no halo kernel, no 256 tile (PAIR: 256 x 128)
        out += [case(16, 64, 64, 256, 0, 256, K, mode=mode, feat=IN_SCALE | BIAS, tune=t) for K in (1, 3) for t in (0, 50, 60, 61)]
    out += [case(16, 64, 64, 256, 0, 256, 3, mode=m, feat=BIAS, splits=3, tune=t) for m in (F32, BF16, PAIR_BF16) for t in (0, 60)]   # split-K: no halo, no 256 tile
    out.append(case(16, 1024, 1024, 32, 0, 32, 3))                 # a 2 GiB input: generic pointers
    out.append(case(16, 1024, 1023, 32, 0, 32, 3))                 # just below: buffer descriptors
    out.append(case(1, 256, 256, 64, 0, 3, 3, mode=PAIR_BF16))     # PAIR comes before the 3-channel kernel
    out.append(case(1, 256, 256, 64, 0, 3, 3, tune=7))             # rules_off: no 3-channel kernel
    out += [case(16, 256, 256, 64, 0, Cout, 1, feat=f) for Cout in (64, 128, 256) for f in (0, BIAS)]   # tile-loop 1x1 form: the bias columns in LDS
    out += [case(2, 16, 16, 64, 0, Cout, 1, feat=LN_G | BIAS | RES, mode=m) for Cout in (64, 128) for m in (F32, BF16, FP16)]
    return out


def pinned():
    """case -> short() form, or the refusal's message"""
    out = {}
    for line in open(os.path.join(os.path.dirname(__file__), "golden", "conv_choice_pins.txt")):
        c, want = line.rstrip("\n").split(" | ")
        w = want.split()
        out[tuple(int(v) for v in c.split())] = want[4:] if w[0] == "ERR" else (w[0],) + tuple(int(v) for v in w[1:6]) + (w[6], int(w[7]), int(w[8]))
    return out


def sweep_cases():
    """(b): Cout x geometry x Cin x K x operand / storage / pair x features x splits x nz x tuning code"""
    geoms = [(16, 128, 128), (1, 1, 600), (1, 1, 8192)]   # M = 262144 (every automatic rule fires), 600 (under-filled grids), 8192 (one row: the component GEMMs)
    cins = [(64, 0), (32, 32), (640, 0)]
    ks = [(1, 1, 0), (3, 1, 1), (4, 2, 1)]
    modes = [F32, BF16, FP16, BF16_ACT, FP16_ACT, PAIR_BF16, PAIR_FP16]
    feats = [0, IN_SCALE]
    for Cout, (B, H, W), (C0, C1), (K, stride, pad), mode, feat, splits, nz, tune in itertools.product(
            (3, 32, 64, 96, 128, 256, 512), geoms, cins, ks, modes, feats, (1, 3), (1, 16, 36), TUNE_CODES):
        yield (B, H, W, C0, C1, Cout, K, stride, pad, 0) + mode + (feat, splits, nz, tune, 256)


def extra_cases():
    """(c): what the product above cannot reach — a knob (the PAIR kernels' SCA-scaled 256 x 256 instances), tensors of 2 GiB"""
    inscale256 = tuple(1 if n == "pair_inscale256" else d for n, d in zip(KNOB_NAMES, KNOB_DEFAULTS))
    for mode in (PAIR_BF16, PAIR_FP16):
        yield case(16, 64, 64, 256, 0, 256, 3, mode=mode, feat=IN_SCALE), inscale256
    for tune in (3, 50):   # f32 256-row tiles on generic pointers
        yield case(16, 1024, 1024, 32, 0, 256, 3, tune=tune), None


def test_pinned_choices():
    cases, PINNED = pin_cases(), pinned()
    assert len(set(cases)) == len(cases) and set(cases) == set(PINNED)
    bad = []
    for c in cases:
        got = choose(c)
        got = got if isinstance(got, str) else short(got)
        if got != PINNED[c]:
            bad.append((dict(zip(FIELDS, c)), got, PINNED[c]))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(cases), bad[:3])


def test_mixed_operand_and_storage_modes_are_refused():
    """f32 operands on 16-bit tensors, bf16 operands on fp16 tensors and the reverse: refused before any kernel is chosen, whatever the layer"""
    mixed = [(0, 1, 0), (0, 2, 0), (1, 2, 0), (2, 1, 0)]
    for (B, H, W), (C0, C1), Cout, (K, stride, pad), mode, nz, tune in itertools.product(
            [(2, 8, 12), (16, 128, 128), (1, 1, 8192)], [(64, 0), (32, 32)], (3, 64, 256), [(1, 1, 0), (3, 1, 1)], mixed, (1, 36), TUNE_CODES):
        d = choose((B, H, W, C0, C1, Cout, K, stride, pad, 0) + mode + (0, 1, nz, tune, 256))
        assert isinstance(d, str) and re.match(r"launch_conv: (bf16 activation storage needs|fp16 operands go|fp16 activation storage needs)", d), d


def test_default_knobs_are_the_documented_defaults():
    c = case(2, 32, 32, 512, 0, 512, 1, mode=FP16, feat=IN_SCALE)
    assert choose(c) == choose(c, KNOB_DEFAULTS)
    off = (0,) + KNOB_DEFAULTS[1:]
    assert choose(c)["name"] == "igemm128x32" and choose(c, off)["name"] == "igemm128x128"   # IRSDE_SMALL_BN = 0: the base rule


def test_sweep_resolves_every_case_and_reaches_every_instance():
    """Every case is refused by conv_validate (one of launch_conv's messages) or resolves to a kernel: a table row, the 3-channel kernel or the halo path.
    The hook fails with "no kernel instance" where the choice has no row, so a str that is no validation message fails here.  Together the cases reach
    every row of the instance tables."""
    refusals = re.compile(r"launch_conv: (channel counts must|split-K needs|split-K has no gate|fused LayerNorm needs|split-operand pairs go|in_scale needs|the fused LayerNorm epilogue|"
                          r"bf16 activation storage needs|fp16 operands go|fp16 activation storage needs|NAFNet fusions are)")
    rows, nrows, n, families = set(), None, 0, set()
    for c, knobs in itertools.chain(((c, None) for c in sweep_cases()), extra_cases(), ((c, None) for c in pin_cases())):
        d = choose(c, knobs)
        n += 1
        if isinstance(d, str):
            assert refusals.match(d), (dict(zip(FIELDS, c)), d)
            continue
        row, nrows = (int(v) for v in d["row"].split("/"))
        families.add(int(d["family"]))
        assert (row >= 0) == (int(d["family"]) not in (1, 4)) and row < nrows, d
        if row >= 0:
            rows.add(row)
            assert int(d["threads"]) in (256, 512) and 0 < int(d["lds"]) <= 160 * 1024, d
    assert families == {0, 1, 2, 3, 4, 5}
    assert nrows == 56 and rows == set(range(nrows)), sorted(set(range(nrows)) - rows)
