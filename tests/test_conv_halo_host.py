"""The halo family's kernel choice (csrc/conv_halo.hip: conv_halo_choose) and the case table tests/conv_halo_cases.py, checked without a device through the
host-only hook irsde_debug_conv_halo_choice: every case reaches the kernel instance and the tile order it names, the table reaches all 18 (instance, order)
pairs with several tiles and several column blocks, the automatic 512-pixel rule and the two tuning knobs do what the source says, and the features the GPU
test relies on are live in the oracle.  tests/test_gpu_conv_halo.py then runs the same table on the GPU."""
import ctypes

import conv_halo_cases as H
import conv_rows_oracle as R
from image_restoration_sde_amd import _lib
from test_conv_choice_host import choose
from test_conv_rows_host import HOOK_BITS, hook_args

_buf = ctypes.create_string_buffer(512)


def parse_halo(text):
    d = dict(kv.split("=") for kv in text.replace(" of ", "/").split())
    return dict(d, pixels=int(d["kernel"][4:]), bn=int(d["bn"]), nslow=int(d["nslow"]), nblk_n=int(d["nblk_n"]), grid=int(d["grid"]))


def halo_choose(layer, tune=0, halo2=1, nslow=-1):
    """layer: (B, H, W, C0, C1, Cout, K, stride, pad, up, op, st, pair, feat, splits, nz) — the hook's line as a dict, or the refusal's message"""
    L = _lib.lib()
    if L.irsde_debug_conv_halo_choice(*layer, tune, halo2, nslow, _buf, len(_buf)) != 0:
        return L.irsde_last_error().decode()
    return parse_halo(_buf.value.decode())


def layer_of(c):
    return hook_args(c, 256)[:16]


def layer(B, H, W, C0, C1, Cout, mode=R.BF16, feat=0, up=0, splits=1, K=3):
    return (B, H, W, C0, C1, Cout, K, 1, K // 2, up) + mode + (feat & HOOK_BITS, splits, 1)


def check_reach(c, d):
    """d: a halo line as a dict — the kernel, BN, order, instance and grid the case names"""
    assert not isinstance(d, str), (c["name"], d)
    pixels, bn, nslow = c["reach"]
    ntile, nblk_n = H.geometry(c)
    got = (d["pixels"], d["bn"], d["nslow"], d["instance"], int(d["op"]), int(d["act"]), d["nblk_n"], d["grid"])
    want = (pixels, bn, nslow, "%d/9" % H.instance(c["mode"], pixels, bn), 3 if c["mode"] == R.FP16 else 2, c["mode"][1], nblk_n, ntile * nblk_n)
    assert got == want, (c["name"], got, want)


def test_every_case_reaches_what_it_names():
    for c in H.CASES:
        check_reach(c, halo_choose(layer_of(c), c["tune"]))
        for cu in (256, 64):   # and conv_choose sends it to the halo family whatever the CU count
            d = choose(hook_args(c, cu))
            assert (d["name"], d["family"], d["row"]) == ("halo", "4", "-1/56"), (c["name"], d)


def test_every_instance_and_order_is_reached_with_several_tiles_and_column_blocks():
    reached = set()
    for c in H.CASES:
        pixels, bn, nslow = c["reach"]
        ntile, nblk_n = H.geometry(c)
        if ntile > 1 and nblk_n > 1:
            reached.add((H.instance(c["mode"], pixels, bn), nslow))
    assert reached == {(i, o) for i in range(9) for o in (0, 1)}, sorted(reached)
    # the slow-order cases a swapped decode would leave holes in: tiles and column blocks differ in number
    assert sum(1 for c in H.CASES if c["reach"][2] and len(set(H.geometry(c))) == 2) >= 18
    # every fast / slow pair differs in nothing but the tuning code
    pairs = H.order_pairs()
    assert len(pairs) >= 18
    for a, b in pairs:
        ca, cb = H.BY_NAME[a], H.BY_NAME[b]
        assert {k for k in ca if ca[k] != cb[k]} <= {"name", "tune", "reach"} and ca["reach"][:2] == cb["reach"][:2]


def test_cases_fit_the_device_budget():
    worst = max(H.CASES, key=R.device_bytes)
    assert R.device_bytes(worst) < 160e6, (worst["name"], R.device_bytes(worst))


def test_automatic_512_pixel_rule_clause_by_clause():
    """conv_halo_choose's rule: blocks >= 256, at most a quarter of padding, and a long K loop: Ctot >= 768, or Ctot >= 256 on fp32 tensors without a residual.
    One shape per clause, refused by its nearest neighbour."""
    k = lambda *a, **kw: halo_choose(layer(*a, **kw))["pixels"]
    # 16 x 16 tiles of 16 x 32 pixels = 256 blocks; one tile row fewer = 240
    assert k(1, 256, 512, 768, 0, 128, R.BF16_ACT) == 512 and k(1, 240, 512, 768, 0, 128, R.BF16_ACT) == 256
    assert k(1, 128, 512, 768, 0, 256, R.BF16_ACT) == 512 and k(1, 128, 512, 768, 0, 128, R.BF16_ACT) == 256   # (column blocks count)
    # padding: one tile column of 32 for W = 26 (32 * 4 <= 26 * 5) but not for W = 25
    assert k(16, 256, 26, 768, 0, 128, R.BF16_ACT) == 512 and k(16, 256, 25, 768, 0, 128, R.BF16_ACT) == 256
    # Ctot >= 768 (with a residual, on bf16 tensors, with fp16 operands)
    for mode in (R.BF16, R.BF16_ACT, R.FP16):
        assert k(1, 256, 512, 768, 0, 128, mode, R.RES) == 512 and k(1, 256, 512, 736, 0, 128, mode, R.RES) == 256
        assert k(1, 256, 512, 512, 256, 128, mode, R.RES) == 512   # (both sources count)
    # Ctot >= 256: fp32 tensors without a residual only
    for mode in (R.BF16, R.FP16):
        assert k(1, 256, 512, 256, 0, 128, mode) == 512 and k(1, 256, 512, 224, 0, 128, mode) == 256
        assert k(1, 256, 512, 256, 0, 128, mode, R.RES) == 256
    assert k(1, 256, 512, 256, 0, 128, R.BF16_ACT) == 256
    # fewer than 128 output channels: never, forced or not
    assert k(4, 256, 512, 768, 0, 96, R.BF16) == 256 and halo_choose(layer(4, 256, 512, 768, 0, 96), 64)["pixels"] == 256
    # a forced kernel ignores the rule both ways
    assert halo_choose(layer(1, 16, 16, 64, 0, 128), 64)["pixels"] == 512 and halo_choose(layer(1, 256, 512, 768, 0, 128), 65)["pixels"] == 256


def test_halo2_and_nslow_knobs():
    """IRSDE_HALO2 = 0: the 512-pixel kernel never by rule (a forced one still runs).  IRSDE_HALO_NSLOW = 0 / 1: the order of every layer, whatever its weights,
    where there are two column blocks at least; the hook's ORDER_N_SLOW (tune 68 / 69) goes before the knob."""
    big = layer(1, 256, 512, 768, 0, 128, R.BF16_ACT)
    assert halo_choose(big)["pixels"] == 512 and halo_choose(big, halo2=0)["pixels"] == 256 and halo_choose(big, 64, halo2=0)["pixels"] == 512
    natural, small, one = layer(1, 20, 40, 896, 0, 256), layer(2, 20, 36, 64, 32, 160), layer(2, 20, 36, 64, 0, 128)
    assert halo_choose(layer(1, 20, 40, 864, 0, 256))["nslow"] == 0   # 3.98e6 bytes of weights
    assert [halo_choose(natural, nslow=v)["nslow"] for v in (-1, 0, 1)] == [1, 0, 1]
    assert [halo_choose(small, nslow=v)["nslow"] for v in (-1, 0, 1)] == [0, 0, 1]
    assert [halo_choose(one, nslow=v)["nslow"] for v in (-1, 0, 1)] == [0, 0, 0]
    for tune in (68, 69):
        assert halo_choose(small, tune, nslow=0)["nslow"] == 1 and halo_choose(one, tune, nslow=1)["nslow"] == 0
    for tune in (64, 65):   # a forced kernel leaves the order to the rule and the knob
        assert [halo_choose(natural, tune, nslow=v)["nslow"] for v in (-1, 0)] == [1, 0]


def test_layers_the_halo_family_never_takes():
    ok = layer(2, 20, 36, 64, 0, 128)
    assert not isinstance(halo_choose(ok), str)
    for what, lay in [("fp16 tensors", layer(2, 20, 36, 64, 0, 128, R.FP16_ACT)), ("in_scale", layer(2, 20, 36, 64, 0, 128, R.FP16, R.IN_SCALE)),
                      ("split-K", layer(2, 20, 36, 64, 0, 128, splits=2)), ("Cout < 64", layer(2, 20, 36, 64, 0, 32)), ("f32", layer(2, 20, 36, 64, 0, 128, R.F32)),
                      ("PAIR", layer(2, 20, 36, 64, 0, 128, R.PAIR_BF16)), ("1x1", layer(2, 20, 36, 64, 0, 128, K=1))]:
        for tune in (0, 64, 65, 68, 69):
            msg = halo_choose(lay, tune)
            assert isinstance(msg, str) and msg.startswith("debug_conv_halo_choice: conv_choose does not send this layer to the halo family"), (what, tune, msg)
    assert halo_choose(ok, 61).startswith("debug_conv_halo_choice: conv_choose does not send")   # the tuning code that switches the family off
    assert halo_choose(layer(2, 20, 36, 48, 0, 128)).startswith("launch_conv: channel counts")   # conv_validate's refusals come first


def test_oracle_features_are_live():
    """Dropping the per-image FiLM rows (all images take row 0), swapping them between the images, or dropping the residual moves the reference by > 1e-2 of
    max|ref|: far more than any bound of the GPU test"""
    n = 0
    for c in H.CASES:
        if not c["feat"] & R.FILM_PER_IMAGE or c["name"].rsplit("_t", 1)[1] not in ("65", "64"):
            continue
        t = H.case_tensors(c)
        ref = R.reference(c, t)
        assert R.relerr(R.reference(c, dict(t, film=t["film"][:1])), ref) > 1e-2, c["name"]
        assert R.relerr(R.reference(c, dict(t, film=t["film"][::-1])), ref) > 1e-2, c["name"]
        if c["feat"] & R.RES:
            assert R.relerr(R.reference(dict(c, feat=c["feat"] & ~R.RES), t), ref) > 1e-2, c["name"]
        n += 1
    assert n == 6
