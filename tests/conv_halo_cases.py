"""The case table of the halo family (csrc/conv_halo.hip: nine kernel instances, two tile orders each), numpy only: layers, inputs and the float64 oracle are
tests/conv_rows_oracle.py's; each case adds what it must REACH: (pixels per block 256 / 512, BN, nslow), checked on the host through
irsde_debug_conv_halo_choice (tests/test_conv_halo_host.py) and on the GPU from the launch's own line (tests/test_gpu_conv_halo.py).

The kernel and the order are forced by the tuning code: 65 / 69 the 256-pixel kernel with the output-channel blocks fastest / slowest, 64 / 68 the 512-pixel
kernel likewise; tune 0 is the production dispatch.  A case's inputs come from its `inputs` name (the case's name without the tuning code), so that the cases of
one layer share their tensors and their reference, and two cases that differ only in the tile order must give the same bits.

Geometries, the smallest at which each mechanism is live:
    GM  2 x 20 x 36   256-pixel kernel: 2 x 3 tiles per image, ragged right and bottom; 512-pixel kernel: 2 x 2; with two column blocks 24 and 16 blocks
    GS  3 x 7 x 9     smaller than one tile, three images
    GE  1 x 16 x 32   both edges exactly on tile boundaries
    GU  1 x 9 x 17    with up = 1: odd source sizes, an 18 x 34 output
    GN  1 x 20 x 40   the natural-rule shape: 6 tiles, 12 blocks with two column blocks (the XCD remap has remainder 4)"""
from conv_rows_oracle import BF16, BF16_ACT, BIAS, FILM, FILM_PER_IMAGE, FP16, MODE_NAMES, RES, SILU, case, out_hw, reference, tensors   # noqa: F401

GM, GS, GE, GU, GN = (2, 20, 36), (3, 7, 9), (1, 16, 32), (1, 9, 17), (1, 20, 40)
MODES = (BF16, FP16, BF16_ACT)
# conv_halo_global_init's order: conv3x3_halo_bf16_kernel<128> / <64> on f32 tensors, on bf16 tensors, with fp16 operands; then conv3x3_halo2_kernel likewise
FORM = {BF16: 0, BF16_ACT: 1, FP16: 2}


def instance(mode, pixels, bn):
    return 6 + FORM[mode] if pixels == 512 else 2 * FORM[mode] + (0 if bn == 128 else 1)


def _layer(stem, geom, C0, C1, Cout, mode, feat, tunes, up=0):
    """One layer under several tuning codes: tunes = {code: (pixels, bn, nslow)}"""
    out = []
    for tune, reach in tunes.items():
        c = case("%s_t%d" % (stem, tune), None, "halo", *geom, C0, C1, Cout, 3, up=up, mode=mode, feat=feat, tune=tune)
        c.update(inputs=stem, reach=reach)
        out.append(c)
    return out


def _cases():
    out = []
    per_image = BIAS | FILM | FILM_PER_IMAGE | SILU | RES
    for mode in MODES:
        m = MODE_NAMES[mode]
        L = lambda what, *a, **kw: out.extend(_layer("%s_%s" % (m, what), *a, **kw))
        # BN = 64 (Cout < 128), the 256-pixel kernel only.  Cout 96 / 100 / 70: the second column block has its upper columns masked and its weight rows clamped;
        # 70 is no multiple of 4: out_stride and res_stride are not either, so every store and residual load takes the scalar path
        L("bn64_film", GM, 32, 32, 96, mode, per_image, {65: (256, 64, 0), 69: (256, 64, 1)})
        L("bn64_onechunk", GS, 32, 0, 64, mode, SILU, {65: (256, 64, 0)})
        L("bn64_c100", GM, 64, 0, 100, mode, RES, {65: (256, 64, 0), 69: (256, 64, 1)})
        L("bn64_c70", GM, 64, 0, 70, mode, BIAS | RES, {65: (256, 64, 0), 69: (256, 64, 1)})
        # BN = 128 on both kernels: 64 + 32 channels = three chunks, the source switches at the odd chunk 2; Cout 160: the second column block holds 32 valid
        # columns; Cout 288: three column blocks (36 / 24 blocks: the XCD remap has a remainder)
        both = lambda slow: {65: (256, 128, 0), 69: (256, 128, slow), 64: (512, 128, 0), 68: (512, 128, slow)}
        L("c160", GM, 64, 32, 160, mode, BIAS | FILM | SILU | RES, both(1))
        L("c288", GM, 64, 32, 288, mode, BIAS | RES, both(1))
        L("onechunk512", GS, 32, 0, 128, mode, BIAS | FILM | FILM_PER_IMAGE, {64: (512, 128, 0)})
        # (one chunk on an image of several ragged tiles: the prologue's clamped weight loads next to the 256-pixel kernel's wrapped last halo pass)
        L("onechunk_tiles", GM, 32, 0, 128, mode, BIAS, {65: (256, 128, 0), 64: (512, 128, 0)})
        L("exact", GE, 64, 0, 256, mode, BIAS | SILU, both(1))
        L("up", GU, 64, 0, 128, mode, BIAS, {65: (256, 128, 0), 64: (512, 128, 0)}, up=1)
        # the production dispatch on a small layer
        L("small", GM, 64, 0, 128, mode, BIAS | SILU, {0: (256, 128, 0)})
    # the natural rule: 2 * 256 * 9 * 896 = 4.13e6 bytes of weights > 4e6 and two column blocks: slow order without being asked (tune 64 forces the kernel only)
    for mode in (BF16, BF16_ACT):
        out.extend(_layer("%s_natural" % MODE_NAMES[mode], GN, 896, 0, 256, mode, BIAS | RES, {0: (256, 128, 1), 64: (512, 128, 1)}))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def geometry(c):
    """(ntile, nblk_n) of the case on the kernel it names"""
    pixels, bn, _ = c["reach"]
    Ho, Wo = out_hw(c)
    tw = 32 if pixels == 512 else 16
    return c["B"] * ((Ho + 15) // 16) * ((Wo + tw - 1) // tw), (c["Cout"] + bn - 1) // bn


def order_pairs():
    """(fast, slow): cases that differ in nothing but the tile order"""
    return [(c["name"], "%s_t%d" % (c["inputs"], c["tune"] + 4)) for c in CASES if c["tune"] in (64, 65) and "%s_t%d" % (c["inputs"], c["tune"] + 4) in BY_NAME]


def case_tensors(c):
    return tensors(dict(c, name=c["inputs"]))
