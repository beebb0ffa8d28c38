"""Float64 restatement of the whole ConvParams contract of launch_conv (csrc/conv_igemm.hip) and the case table that reaches every row of its instance
tables (test infrastructure: numpy only).

Epilogue order, as the kernel documents it: bias -> FiLM (one shared row, or one row per image) -> SiLU -> ch_scale -> then one of
    gate     product of channels j and j + Cout / 2, then gate_film: (.)(s + 1) + t, per image
    shuffle  PixelShuffle(2), then + res (res has the shuffled shape)
    ln_g     straight after the bias: (v - mean) rsqrt(var + 1e-5) g over the channels, then + res
    else     + res
in_scale multiplies input element (b, k) before the product.

Modes, restated the way tests/test_gpu_parity.py and tests/naf_f16act_oracle.py do:
    16-bit operands  the weights and the staged input are rounded to bf16 / fp16 (`O.bf16_convs` / `O.f16_convs`); with in_scale the staged input is
                     round16(fl32(x * in_scale)): the fp32 product of the staging code, then ONE rounding (`O.round_f16` goes through float32, and the float64
                     product of two float32 values is exact, so conv2d's operand rounding of x * s is that value — naf_f16act_oracle.naf_block's conv3)
    16-bit storage   inputs and residual rounded to the storage type first (naf_f16act_oracle._st), one final rounding of the stored result
    PAIR             the plain float64 product

A case is a dict made by `case()`; `tensors(c)` makes its inputs from the case's name alone; `reference(c, t, operands=, storage=)` is the oracle.  Layouts
are the reference's (NCHW / OIHW); a batched case (nz > 1) is a stack of 1x1 GEMMs: x [nz][W][C0], w [nz][Cout][C0], out [nz][W][Cout]."""
import zlib

import numpy as np

import naf_f16act_oracle as F
from oracle import irsde_oracle as O

BIAS, FILM, SILU, RES, IN_SCALE, CH_SCALE, GATE, SHUFFLE, LN_G = (1 << i for i in range(9))
GATE_FILM, FILM_PER_IMAGE = 1 << 16, 1 << 17   # the oracle's own bits (the choice hook sees neither: they do not change the choice)
F32, BF16, FP16, BF16_ACT, FP16_ACT, PAIR_BF16, PAIR_FP16 = (0, 0, 0), (1, 0, 0), (2, 0, 0), (1, 1, 0), (2, 2, 0), (1, 0, 1), (2, 0, 1)   # (operand, storage, pair)
MODE_NAMES = {F32: "f32", BF16: "bf16", FP16: "fp16", BF16_ACT: "bf16act", FP16_ACT: "fp16act", PAIR_BF16: "pairbf16", PAIR_FP16: "pairfp16"}
KNOB_NAMES = ("small_bn", "small_bn_f32", "pair_tile256", "pair_inscale256", "no_bufa", "zloop", "zloop_1x1", "zloop_maxnk", "zloop_minblk", "zloop_deep", "zloop_ragged64")
KNOB_DEFAULTS = (2, 0, 1, 0, 0, -1, -1, 32, 1024, 1, 2048)

# The instance tables of csrc/conv_igemm.hip, row by row: (tile, op, act, inscale) — op: 0 f32, 1 f32 with buffer descriptors, 2 bf16, 3 fp16; act: 0 f32, 1 bf16, 2 fp16
_T5 = ("128x128", "128x64", "128x32", "256x128", "256x256")
_T4 = ("128x128", "128x64", "128x32", "256x256")
_T3 = ("128x128", "128x64", "128x32")
_TP = ("256x256", "256x128", "128x64")
ROWS = ([(t, 0, 0, 0) for t in _T5] + [(t, 1, 0, 0) for t in _T5] + [(t, 0, 0, 1) for t in _T3] + [(t, 1, 0, 1) for t in _T3] +
        [(t, 2, 0, 0) for t in _T4] + [(t, 3, 0, 0) for t in _T4] + [(t, 3, 2, 0) for t in _T4] + [(t, 2, 1, 0) for t in _T4] +
        [(t, 2, 0, 1) for t in _T3] + [(t, 3, 0, 1) for t in _T3] + [(t, 3, 2, 1) for t in _T3] +
        [(t, 2, 0, 0) for t in _TP] + [(t, 3, 0, 0) for t in _TP] + [(t, 2, 0, 1) for t in _TP] + [(t, 3, 0, 1) for t in _TP] +
        [("128x128", 0, 0, 0), ("128x64", 0, 0, 0), ("64x128", 0, 0, 0)])
assert len(ROWS) == 56


def case(name, row, kernel, B, H, W, C0, C1, Cout, K=1, stride=1, pad=None, up=0, mode=F32, feat=0, splits=1, nz=1, tune=0, knobs=None):
    """row: the instance-table row the launch must reach (None: conv_validate must refuse the layer); kernel: the choice's name.  knobs: {knob name: value}
    over the defaults, or None = the hook's NULL."""
    return dict(name=name, row=row, kernel=kernel, B=B, H=H, W=W, C0=C0, C1=C1, Cout=Cout, K=K, stride=stride, pad=K // 2 if pad is None else pad, up=up,
                mode=mode, feat=feat, splits=splits, nz=nz, tune=tune, knobs=knobs)


def knob_array(c):
    if c["knobs"] is None:
        return None
    assert set(c["knobs"]) <= set(KNOB_NAMES)
    return tuple(c["knobs"].get(n, d) for n, d in zip(KNOB_NAMES, KNOB_DEFAULTS))


def out_hw(c):
    return (((c["H"] << c["up"]) + 2 * c["pad"] - c["K"]) // c["stride"] + 1, ((c["W"] << c["up"]) + 2 * c["pad"] - c["K"]) // c["stride"] + 1)


def device_bytes(c):
    """fp32 bytes of out + in0 + in1 + res + partial, as the hook's caller and the hook allocate them"""
    Ho, Wo = out_hw(c)
    M = c["B"] * Ho * Wo * c["nz"]
    nout = M * (c["Cout"] // 2 if c["feat"] & GATE else c["Cout"])
    nin = c["B"] * c["H"] * c["W"] * c["nz"] * (c["C0"] + c["C1"])
    return 4 * (nout + nin + (nout if c["feat"] & RES else 0) + (c["splits"] * M * c["Cout"] if c["splits"] > 1 else 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# (a) one case per instance-table row at least: the smallest shape that reaches the row and can still go wrong.  No case depends on the device's CU count:
# a non-zero tuning code switches the grid-filling rules off, tune 0 is used only where no rule reads the CU count (f32 without IRSDE_SMALL_BN_F32, PAIR), the
# fused-LayerNorm cases of (b) carry explicit knobs.  Geometries: 2 x 9 x 11 (M = 198: two 128-row tiles, the second ragged, the image boundary at row 99 inside
# the first), 2 x 13 x 11 (M = 286: two 256-row tiles), 3 x 13 x 11 (M = 429: four 128-row tiles).  Cout 160 / 96 / 20 / 288: the last column tile of the
# 128 / 64 / 32 / 256 wide tiles is masked.  C0 + C1 >= 64: more than one K-step.
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
G198, G286, G429 = (2, 9, 11), (2, 13, 11), (3, 13, 11)
CONV3, CONV5 = IN_SCALE | CH_SCALE | RES | BIAS, CH_SCALE | RES | BIAS
NO_BUFA = {"no_bufa": 1}
ROW_CASES = [
    # f32, generic pointers (tune 6; the 256-row tiles: IRSDE_NO_BUFA with tune 3 / 50)
    case("row00", 0, "igemm128x128", *G198, 64, 32, 160, 3, feat=BIAS | FILM | SILU | RES, tune=6),
    case("row01", 1, "igemm128x64", *G198, 64, 0, 96, 3, feat=BIAS | FILM | FILM_PER_IMAGE | SILU, tune=6),
    case("row02", 2, "igemm128x32", *G198, 64, 0, 20, 3, up=1, feat=BIAS | RES, tune=6),
    case("row03", 3, "igemm256x128", *G286, 64, 32, 160, 1, feat=BIAS | SILU | RES, tune=3, knobs=NO_BUFA),
    case("row04", 4, "igemm256x256", *G286, 96, 0, 288, 1, feat=BIAS | FILM | RES, tune=50, knobs=NO_BUFA),
    # f32, buffer descriptors: tune 0 takes the direct epilogue where the layer allows it (row05, row07), a per-image FiLM row the LDS-transposed one (row06)
    case("row05", 5, "igemm128x128", *G198, 64, 32, 160, 3, feat=BIAS | FILM | SILU | CH_SCALE | RES),
    case("row06", 6, "igemm128x64", *G198, 64, 0, 96, 4, 2, 1, feat=BIAS | FILM | FILM_PER_IMAGE | SILU | RES),
    case("row07", 7, "igemm128x32", *G198, 96, 0, 20, 1, feat=BIAS | CH_SCALE | RES),
    case("row08", 8, "igemm256x128", *G286, 64, 32, 160, 3, feat=BIAS | SILU | CH_SCALE | RES, tune=3),
    case("row09", 9, "igemm256x256", *G286, 96, 0, 288, 1, feat=BIAS | FILM | SILU | RES, tune=50),
    # f32 with in_scale: generic (tune 6) and buffer descriptors (tune 0)
    case("row10", 10, "igemm128x128", *G198, 96, 0, 160, 1, feat=CONV3, tune=6),
    case("row11", 11, "igemm128x64", *G198, 64, 0, 96, 3, feat=IN_SCALE | BIAS | SILU, tune=6),
    case("row12", 12, "igemm128x32", *G198, 64, 0, 20, 1, feat=CONV3, tune=6),
    case("row13", 13, "igemm128x128", *G198, 96, 0, 160, 1, feat=CONV3),
    case("row14", 14, "igemm128x64", *G198, 64, 0, 96, 3, feat=IN_SCALE | BIAS | FILM | FILM_PER_IMAGE | RES),
    case("row15", 15, "igemm128x32", *G198, 64, 0, 20, 1, feat=CONV3),
    # 16-bit operands on f32 tensors: tune 61 the 128-row tiles (no halo kernel, no narrowing), tune 60 the 256 x 256 tile
    case("row16", 16, "igemm128x128", *G198, 64, 32, 160, 3, mode=BF16, feat=BIAS | FILM | SILU | RES, tune=61),
    case("row17", 17, "igemm128x64", *G198, 64, 0, 96, 1, mode=BF16, feat=CONV5, tune=61),
    case("row18", 18, "igemm128x32", *G198, 64, 0, 20, 3, up=1, mode=BF16, feat=BIAS | FILM | FILM_PER_IMAGE, tune=61),
    case("row19", 19, "igemm256x256", *G286, 96, 0, 288, 1, mode=BF16, feat=BIAS | SILU | RES, tune=60),
    case("row20", 20, "igemm128x128", *G198, 64, 32, 160, 3, mode=FP16, feat=BIAS | FILM | SILU | RES, tune=61),
    case("row21", 21, "igemm128x64", *G198, 64, 0, 96, 1, mode=FP16, feat=CONV5, tune=61),
    case("row22", 22, "igemm128x32", *G198, 64, 0, 20, 3, up=1, mode=FP16, feat=BIAS | FILM | FILM_PER_IMAGE, tune=61),
    case("row23", 23, "igemm256x256", *G286, 96, 0, 288, 1, mode=FP16, feat=BIAS | SILU | RES, tune=60),
    # fp16 operands on fp16 tensors, bf16 operands on bf16 tensors
    case("row24", 24, "igemm128x128", *G198, 32, 32, 160, 3, mode=FP16_ACT, feat=BIAS | FILM | SILU | RES, tune=61),
    case("row25", 25, "igemm128x64", *G198, 64, 0, 96, 1, mode=FP16_ACT, feat=CONV5, tune=61),
    case("row26", 26, "igemm128x32", *G198, 64, 0, 20, 3, mode=FP16_ACT, feat=BIAS | FILM | FILM_PER_IMAGE | RES, tune=61),
    case("row27", 27, "igemm256x256", *G286, 96, 0, 288, 1, mode=FP16_ACT, feat=BIAS | SILU | RES, tune=60),
    case("row28", 28, "igemm128x128", *G198, 32, 32, 160, 3, mode=BF16_ACT, feat=BIAS | FILM | SILU | RES, tune=61),
    case("row29", 29, "igemm128x64", *G198, 64, 0, 96, 1, mode=BF16_ACT, feat=CONV5, tune=61),
    case("row30", 30, "igemm128x32", *G198, 64, 0, 20, 3, mode=BF16_ACT, feat=BIAS | FILM | FILM_PER_IMAGE | RES, tune=61),
    case("row31", 31, "igemm256x256", *G286, 96, 0, 288, 1, mode=BF16_ACT, feat=BIAS | SILU | RES, tune=60),
    # 16-bit operands with in_scale
    case("row32", 32, "igemm128x128", *G198, 96, 0, 160, 1, mode=BF16, feat=CONV3, tune=61),
    case("row33", 33, "igemm128x64", *G198, 64, 0, 96, 3, mode=BF16, feat=IN_SCALE | BIAS | SILU, tune=61),
    case("row34", 34, "igemm128x32", *G198, 64, 0, 20, 1, mode=BF16, feat=CONV3, tune=61),
    case("row35", 35, "igemm128x128", *G198, 96, 0, 160, 1, mode=FP16, feat=CONV3, tune=61),
    case("row36", 36, "igemm128x64", *G198, 64, 0, 96, 3, mode=FP16, feat=IN_SCALE | BIAS | SILU, tune=61),
    case("row37", 37, "igemm128x32", *G198, 64, 0, 20, 1, mode=FP16, feat=CONV3, tune=61),
    case("row38", 38, "igemm128x128", *G198, 96, 0, 160, 1, mode=FP16_ACT, feat=CONV3, tune=61),
    case("row39", 39, "igemm128x64", *G198, 64, 0, 96, 3, mode=FP16_ACT, feat=IN_SCALE | BIAS | SILU, tune=61),
    case("row40", 40, "igemm128x32", *G198, 64, 0, 20, 1, mode=FP16_ACT, feat=CONV3, tune=61),
    # PAIR: 256 x 256 needs 256 tiles (M > 65280 at Cout = 256: 2 x 181 x 181 = 65522 rows, the image boundary inside a tile), 256 x 128 Cout >= 128 and M >= 256,
    # else 128 x 64; the in_scale 256 x 256 instances IRSDE_PAIR_INSCALE256
    case("row41", 41, "pair256x256", 2, 181, 181, 32, 0, 256, 1, mode=PAIR_BF16, feat=BIAS | SILU),
    case("row42", 42, "pair256x128", *G286, 64, 32, 160, 3, mode=PAIR_BF16, feat=BIAS | FILM | SILU | RES),
    case("row43", 43, "pair128x64", *G198, 64, 0, 96, 1, mode=PAIR_BF16, feat=CONV5),
    case("row44", 44, "pair256x256", 2, 181, 181, 32, 0, 256, 1, mode=PAIR_FP16, feat=BIAS | SILU),
    case("row45", 45, "pair256x128", *G286, 64, 32, 160, 3, mode=PAIR_FP16, feat=BIAS | FILM | SILU | RES),
    case("row46", 46, "pair128x64", *G198, 64, 0, 96, 1, mode=PAIR_FP16, feat=CONV5),
    case("row47", 47, "pair256x256", 2, 181, 181, 32, 0, 256, 1, mode=PAIR_BF16, feat=IN_SCALE | BIAS, knobs={"pair_inscale256": 1}),
    case("row48", 48, "pair256x128", *G286, 96, 0, 160, 1, mode=PAIR_BF16, feat=CONV3),
    case("row49", 49, "pair128x64", *G198, 64, 0, 96, 3, mode=PAIR_BF16, feat=IN_SCALE | BIAS | FILM | FILM_PER_IMAGE | SILU),
    case("row50", 50, "pair256x256", 2, 181, 181, 32, 0, 256, 1, mode=PAIR_FP16, feat=IN_SCALE | BIAS, knobs={"pair_inscale256": 1}),
    case("row51", 51, "pair256x128", *G286, 96, 0, 160, 1, mode=PAIR_FP16, feat=CONV3),
    case("row52", 52, "pair128x64", *G198, 64, 0, 96, 3, mode=PAIR_FP16, feat=IN_SCALE | BIAS | FILM | FILM_PER_IMAGE | SILU),
    # the tile-loop kernel: its 1x1 form forced (tune 73: two row tiles per block, both sources), its batch form with all components in one block (tune 71) on
    # 64-row tiles, and on 128-row tiles (IRSDE_ZLOOP_RAGGED64 = 0, Wo > 64 and >= 512 tiles of 128 x 128)
    case("row53_1x1", 53, "zloop1x1_128x128", *G429, 32, 32, 160, 1, feat=BIAS, tune=73),
    case("row54_1x1", 54, "zloop1x1_128x64", *G429, 32, 32, 48, 1, feat=BIAS, tune=73),
    case("row55_batch", 55, "zloop64x128", 1, 1, 100, 64, 0, 160, 1, nz=4, tune=71),
    case("row53_batch", 53, "zloop128x128", 1, 1, 1000, 32, 0, 512, 1, nz=16, tune=71, knobs={"zloop_ragged64": 0}),
    case("row54_batch", 54, "zloop128x64", 1, 1, 1806, 32, 0, 64, 1, nz=36, tune=71, knobs={"zloop_ragged64": 0}),
]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# (b) the feature combinations the engine builds (engine_plan.hip: conv_naf's conv3 / conv4 / conv5, the NAFNet downs / ups, attn_tail's to_out + LayerNorm)
# on one cheap tile per operand mode.  f32 runs every feature twice: tune 0 (the direct epilogue where the layer allows it) and tune 7 (the LDS-transposed
# one).  16-bit operands: tune 61; the fused-LayerNorm layers tune 0 with the DEFAULT knobs written out — the production dispatch, IRSDE_SMALL_BN = 2 included
# (2 or 4 tiles of 128 x Cout are fewer than two per CU on any device: the rule would narrow them at 64 CUs and at 256 alike).
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _matrix():
    out = []
    defaults = dict(zip(KNOB_NAMES, KNOB_DEFAULTS))
    base = {F32: (0, 5, 1), BF16: (61, 16, 2), FP16: (61, 20, 3), FP16_ACT: (61, 24, 3), BF16_ACT: (61, 28, 2), PAIR_FP16: (0, 44, 3), PAIR_BF16: (0, 41, 2)}
    for mode in (F32, BF16, FP16, FP16_ACT, BF16_ACT, PAIR_FP16, PAIR_BF16):
        tune0, r0, _ = base[mode]
        pair, st = mode[2], mode[1]
        for tune in ((0, 7) if mode == F32 else (tune0,)):
            tag = MODE_NAMES[mode] + ("_t7" if tune == 7 else "")
            r64, r128 = (r0 + 2, r0 + 2) if pair else (r0 + 1, r0)       # the 64- and the 128-channel layer's row
            k64, k128 = ("pair128x64", "pair128x64") if pair else ("igemm128x64", "igemm128x128")
            nafnet = st != 1                                             # bf16 tensors take none of the NAFNet fusions: refused
            ri = {F32: 14, BF16: 33, FP16: 36, FP16_ACT: 39, PAIR_FP16: 52, PAIR_BF16: 49}.get(mode)   # the in_scale instance of the 64-wide tile
            add = lambda name, row, kernel, *a, **kw: out.append(case("%s_%s" % (name, tag), row, kernel, *a, mode=mode, tune=kw.pop("tune", tune), **kw))
            add("conv3", ri if nafnet else None, k64, *G198, 64, 0, 64, 1, feat=CONV3)
            add("conv5", r64, k64, *G198, 64, 0, 64, 1, feat=CONV5)
            add("conv4", r128 if nafnet else None, k128, *G198, 64, 0, 128, 1, feat=GATE | BIAS)
            add("conv4_lens", r128 if nafnet else None, k128, *G198, 64, 0, 128, 1, feat=GATE | BIAS | GATE_FILM)
            add("ups", r128 if nafnet else None, k128, *G198, 64, 0, 128, 1, feat=SHUFFLE | RES)
            add("downs", r128, k128, 2, 10, 14, 64, 0, 128, 2, 2, 0, feat=BIAS)
            add("conv3_split3", ri if nafnet else None, k64, *G198, 128, 0, 64, 1, feat=CONV3, splits=3)
            add("conv5_split3", r64, k64, *G198, 128, 0, 64, 1, feat=CONV5, splits=3)
            ln_ok = not pair and st != 2                                 # no fused LayerNorm on the PAIR tiles or on fp16 tensors: refused
            kn = defaults if mode[0] and not pair else None
            add("to_out_ln64", r64 if ln_ok else None, k64, *G198, 64, 0, 64, 1, feat=LN_G | BIAS | RES, tune=7 if tune == 7 else 0, knobs=kn)
            add("to_out_ln128", r128 if ln_ok else None, k128, *G198, 64, 0, 128, 1, feat=LN_G | BIAS | RES, tune=7 if tune == 7 else 0, knobs=kn)
    return out


MATRIX_CASES = _matrix()
CASES = ROW_CASES + MATRIX_CASES
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# inputs and the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def tensors(c):
    """Every input of the case, float32, from its name alone.  in_scale, ch_scale and ln_g are uniform in [0.5, 1.5], the FiLM rows 0.3 N(0, 1); the per-image
    ones differ per image, so that a row or image mix-up costs far more than any tolerance."""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)
    f = lambda *shape: rs.standard_normal(shape).astype(np.float32)
    u = lambda *shape: rs.uniform(0.5, 1.5, shape).astype(np.float32)
    B, H, W, C0, C1, Cout, K, nz, feat = (c[k] for k in ("B", "H", "W", "C0", "C1", "Cout", "K", "nz", "feat"))
    t = {}
    if nz > 1:
        t["x0"] = f(nz, W, C0)
        t["w"] = (f(nz, Cout, C0) / np.float32(np.sqrt(C0))).astype(np.float32)
        return t
    t["x0"] = f(B, C0, H, W)
    if C1:
        t["x1"] = f(B, C1, H, W)
    t["w"] = (f(Cout, C0 + C1, K, K) / np.float32(np.sqrt((C0 + C1) * K * K))).astype(np.float32)
    Ho, Wo = out_hw(c)
    if feat & BIAS:
        t["bias"] = f(Cout)
    if feat & FILM:
        t["film"] = (np.float32(0.3) * f(B if feat & FILM_PER_IMAGE else 1, 2 * Cout)).astype(np.float32)
    if feat & RES:
        t["res"] = f(B, Cout // 4, 2 * Ho, 2 * Wo) if feat & SHUFFLE else f(B, Cout, Ho, Wo)
    if feat & IN_SCALE:
        t["in_scale"] = u(B, C0)
    if feat & CH_SCALE:
        t["ch_scale"] = u(Cout)
    if feat & GATE_FILM:
        t["gate_film"] = (np.float32(0.3) * f(B, Cout)).astype(np.float32)
    if feat & LN_G:
        t["ln_g"] = u(Cout)
    return t


_ROUND = {None: lambda a: a, "bf16": O.round_bf16, "f16": O.round_f16}


class _no_rounding:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _operand_mode(operands):
    return {None: _no_rounding, "bf16": O.bf16_convs, "f16": O.f16_convs}[operands]()


def reference(c, t, operands=None, storage=None, dtype=np.float64):
    """The layer in `dtype` arithmetic.  operands: None / "bf16" / "f16" (the 16-bit MFMA's operand rounding); storage: None / "bf16" / "f16" (tensor storage:
    inputs and residual rounded first, the result rounded once at the end)."""
    st = _ROUND[storage]
    d = lambda a: np.asarray(a, dtype=dtype)
    feat, Cout = c["feat"], c["Cout"]
    if c["nz"] > 1:
        with _operand_mode(operands):
            return np.stack([O.conv2d(d(x).T[None, :, None, :], d(w)[:, :, None, None])[0, :, 0, :].T for x, w in zip(t["x0"], t["w"])])
    x = d(st(t["x0"] if "x1" not in t else np.concatenate([t["x0"], t["x1"]], axis=1)))
    if feat & IN_SCALE:
        x = x * d(t["in_scale"])[:, :, None, None]
    if c["up"]:
        x = O.upsample_nearest2(x)
    with _operand_mode(operands):
        y = O.conv2d(x, d(t["w"]), d(t["bias"]) if feat & BIAS else None, stride=c["stride"], pad=c["pad"])
    res = d(st(t["res"])) if feat & RES else None
    if feat & LN_G:
        y = O.layer_norm_c(y, d(t["ln_g"]).reshape(1, -1, 1, 1))
        return d(st(y if res is None else y + res))
    if feat & FILM:
        f = d(t["film"])
        y = y * (f[:, :Cout, None, None] + 1) + f[:, Cout:, None, None]   # (one row broadcasts over the batch)
    if feat & SILU:
        y = O.silu(y)
    if feat & CH_SCALE:
        y = y * d(t["ch_scale"]).reshape(1, -1, 1, 1)
    if feat & GATE:
        y = F._gate(y, None)
        if feat & GATE_FILM:
            g = d(t["gate_film"])
            y = y * (g[:, :Cout // 2, None, None] + 1) + g[:, Cout // 2:, None, None]
        return d(st(y))
    if feat & SHUFFLE:
        y = O._pixel_shuffle2(y)
    return d(st(y if res is None else y + res))


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
