"""Host-only tests of split3_1x1_choose (csrc/gemm_split.hip) through irsde_debug_split3_1x1_choice: which direct-path layers run on gemm_split3a_kernel (the plain
1x1 convolutions on three bf16 pieces, the activations split inside the GEMM).  The hook reads neither the environment nor a device."""
import ctypes

import pytest

from image_restoration_sde_amd import _lib

CUS = 256
LDS = 2 * (256 * 128 + 128 * 192)
F_BIAS = 1
# feature bits of irsde_debug_conv_choice that refuse the layer (bit 0, the bias, is the one epilogue the kernel has)
REFUSING_BITS = {1: "film", 2: "silu", 3: "res", 4: "in_scale", 5: "ch_scale", 6: "gate", 7: "shuffle", 8: "ln_g"}


def choice(B, H, W, C0, C1, Cout, K=1, stride=1, pad=0, in_shift=0, operand=0, storage=0, pair=0, features=F_BIAS, splits=1, nz=1, flags=0, master=1, knob=2,
           cus=CUS):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().irsde_debug_split3_1x1_choice(B, H, W, C0, C1, Cout, K, stride, pad, in_shift, operand, storage, pair, features, splits, nz, flags,
                                                        master, knob, cus, buf, len(buf)))
    line = buf.value.decode()
    head, why = line.split(" why_not=")
    d = dict(kv.split("=") for kv in head.split())
    return int(d["adopt"]), int(d["grid"]), int(d["lds"]), why


def test_eligible_layer_grid_and_lds():
    # 64 + 32 -> 64 on 2 x 12 x 20: two row tiles, one column tile; XCD 0 .. 7 own units [x 2 / 8, (x + 1) 2 / 8): one unit at most -> 8 blocks
    assert choice(2, 12, 20, 64, 32, 64) == (1, 8, LDS, "")
    assert choice(2, 12, 20, 64, 32, 64, features=0) == (1, 8, LDS, "")           # to_qkv has no bias
    # 16 x 32 x 32, 1536 -> 1024: 64 row tiles x 8 column tiles = 512 items, capped at one block per CU
    assert choice(16, 32, 32, 1024, 512, 1024) == (1, 256, LDS, "")
    assert choice(16, 32, 32, 1024, 512, 1024, cus=64) == (1, 64, LDS, "")


@pytest.mark.parametrize("bit", sorted(REFUSING_BITS))
def test_every_other_feature_bit_refuses(bit):
    adopt, grid, lds, why = choice(2, 12, 20, 64, 32, 64, features=F_BIAS | (1 << bit))
    assert (adopt, grid, lds) == (0, 0, 0) and why == REFUSING_BITS[bit]


def test_geometry_storage_and_range_refuse_with_the_reason_named():
    assert choice(2, 12, 20, 64, 32, 64, K=3, pad=1)[3] == "not a 1x1 convolution"
    assert choice(2, 12, 20, 64, 32, 64, stride=2)[3] == "stride"
    assert choice(2, 12, 20, 64, 32, 64, in_shift=1)[3] == "in_shift"
    assert choice(2, 12, 20, 64, 32, 64, storage=1, operand=1)[3] == "16-bit storage"
    assert choice(2, 12, 20, 64, 32, 64, storage=2, operand=2)[3] == "16-bit storage"
    assert choice(2, 12, 20, 64, 32, 64, operand=1)[3] == "16-bit operands"
    assert choice(2, 12, 20, 64, 32, 64, operand=2, pair=1)[3] == "16-bit operands"
    assert choice(2, 12, 20, 64, 32, 64, splits=2)[3] == "split-K"
    assert choice(1, 1, 480, 64, 0, 64, nz=4)[3] == "batched"
    assert choice(2, 12, 20, 48, 32, 64)[3] == "C0 not a multiple of 32"
    assert choice(2, 12, 20, 64, 16, 64)[3] == "C1 not a multiple of 32"
    # 16 x 512 x 512 pixels of 256 + 32 channels: the first source alone is 4 Gi bytes
    assert choice(16, 512, 512, 256, 32, 128)[3] == "beyond the 32-bit offset range"
    assert choice(16, 512, 512, 128, 0, 128)[0] == 1                                   # 2 GiB: inside


def test_knob_and_master():
    layer = (16, 32, 32, 1024, 512, 1024)
    assert choice(*layer, knob=0)[3] == "IRSDE_SPLIT3_1X1 = 0"
    assert choice(*layer, knob=1)[0] == 1 and choice(*layer, knob=2)[0] == 1
    assert choice(*layer, master=0, knob=2)[3] == "IRSDE_SPLIT3 = 0"                   # the master's mode 0 wins over knob 2
    assert choice(2, 12, 20, 64, 32, 64, master=2, knob=1)[0] == 0                     # its mode 2 does not force anything
    for flag in (_lib.FLAG_NO_SPLIT3, _lib.FLAG_BF16, _lib.FLAG_SPLIT_F16X2, _lib.FLAG_NAIVE_CONV, _lib.FLAG_NO_WINOGRAD):
        assert choice(*layer, flags=flag)[3] == "not the exact-fp32 engine"


# the 1x1 layers of the benchmarked plan (nf = 64, depth = 4, 256 x 256): (H = W, C0, C1, Cout); profiles/split3_1x1.md, section 3
RES_CONV = [(32, 1024, 512, 1024), (64, 512, 256, 512), (128, 256, 128, 256), (256, 128, 64, 128)]
QKV_ADOPTED = [(32, 1024, 0, 384), (64, 512, 0, 384)]
BELOW_THE_FLOP_FLOOR = [(32, 512, 0, 384), (32, 128, 0, 512), (32, 128, 0, 1024), (64, 128, 0, 512)]   # to_qkv 512 -> 384 at 32 x 32 and the to_out layers


def test_the_rule_on_the_benchmarked_shapes():
    for H, C0, C1, Cout in RES_CONV:
        assert choice(16, H, H, C0, C1, Cout, knob=1)[0] == 1, (H, C0, C1, Cout)
        assert choice(16, 2 * H, 2 * H, C0, C1, Cout, knob=1)[0] == 1                  # 16 x 512 x 512
        # the B = 2 shard: 6.4e9 FLOP per layer, below the floor (end to end that plan was slower with them adopted)
        assert choice(2, H, H, C0, C1, Cout, knob=1)[3] == "rule: FLOP"
        assert choice(2, H, H, C0, C1, Cout, knob=2)[0] == 1
    for H, C0, C1, Cout in QKV_ADOPTED:
        assert choice(16, H, H, C0, C1, Cout, knob=1, features=0)[0] == 1, (H, C0, Cout)
    for H, C0, C1, Cout in BELOW_THE_FLOP_FLOOR:
        assert choice(16, H, H, C0, C1, Cout, knob=1)[3] == "rule: FLOP", (H, C0, Cout)
    # the 128 -> 64 res_conv at level 0 (half a column tile, HBM-bound): measured slower, left on the f32 kernel
    assert choice(16, 256, 256, 64, 64, 64, knob=1)[3] == "rule: Cout"
    assert choice(16, 256, 256, 64, 64, 64, knob=2)[0] == 1


def test_the_rule_adopts_no_layer_of_the_small_test_network():
    """nf = 32, depth = 2 on 2 x 24 x 20 (tests/test_gpu_attn_split3.py relies on that plan being the f32 launches): every 1x1 layer has at most 960 rows"""
    B, H, W, nf = 2, 24, 20, 32
    for lvl in range(3):
        h, w, c = H >> lvl, W >> lvl, nf << lvl
        for C0, C1, Cout in ((c, c // 2, c), (c, c, c), (2 * c, c, c), (c, 0, 3 * 128), (c, 0, 3 * c), (128, 0, c)):
            if C0 % 32 or C1 % 32:
                continue
            adopt, _, _, why = choice(B, h, w, C0, C1, Cout, knob=1)
            assert adopt == 0 and why.startswith("rule:"), (lvl, C0, C1, Cout, why)
            assert choice(B, h, w, C0, C1, Cout, knob=2)[0] == 1


def test_the_seven_1x1_rows_of_the_small_test_network_are_eligible():
    """the 1x1 conv rows of the nf = 32, depth = 2, 2 x 24 x 20 plan (tests/test_gpu_split3_1x1.py pins them as marked under knob 2): (H, W, Cin, Cout);
    eligibility does not depend on how Cin is divided between the two sources as long as both are multiples of 32"""
    for H, W, Cin, Cout in ((24, 20, 32, 128), (24, 20, 128, 32), (24, 20, 64, 32), (12, 10, 192, 128), (24, 20, 96, 64)):
        for C0 in range(32, Cin + 1, 32):
            assert choice(2, H, W, C0, Cin - C0, Cout, knob=2)[0] == 1, (H, W, C0, Cin, Cout)
            assert choice(2, H, W, C0, Cin - C0, Cout, knob=1)[3].startswith("rule:")
