"""The case table of tests/conv_rows_oracle.py, checked without a device: every case reaches the instance-table row it names whatever the CU count, the per-row
cases cover all 56 rows, no case needs more than 160 MB of device tensors, and the oracle agrees with tests/test_gpu_parity.py's oracle_conv where the two
overlap.  tests/test_gpu_conv_rows.py then runs the same table on the GPU."""
import numpy as np
import pytest

import conv_rows_oracle as R
from test_conv_choice_host import choose

HOOK_BITS = 0x1FF   # what irsde_debug_conv_choice sees of a case's features


def hook_args(c, cu):
    return (c["B"], c["H"], c["W"], c["C0"], c["C1"], c["Cout"], c["K"], c["stride"], c["pad"], c["up"]) + c["mode"] + (c["feat"] & HOOK_BITS, c["splits"], c["nz"], c["tune"], cu)


def check_choice(c, d):
    """d: the choice line as a dict (the host hook's or the launch's own) — the row the case names, and that row's tile, operands, storage and in_scale"""
    tile, op, act, inscale = R.ROWS[c["row"]]
    assert not isinstance(d, str), (c["name"], d)
    got = (d["name"], d["tile"], int(d["op"]), int(d["act"]), int(d["inscale"]), d["row"])
    assert got == (c["kernel"], tile, op, act, inscale, "%d/56" % c["row"]), (c["name"], got)
    assert c["kernel"].endswith(tile)


@pytest.mark.parametrize("cu", [256, 64])
def test_every_case_reaches_its_row(cu):
    for c in R.CASES:
        d = choose(hook_args(c, cu), R.knob_array(c))
        if c["row"] is None:
            assert isinstance(d, str) and d.startswith("launch_conv: "), (c["name"], d)
        else:
            check_choice(c, d)


def test_row_cases_cover_the_instance_tables():
    assert {c["row"] for c in R.ROW_CASES} == set(range(56))
    assert all(c["row"] is not None for c in R.ROW_CASES)


def test_refused_combinations_are_the_documented_ones():
    """bf16 tensors take no NAFNet fusion; the PAIR tiles and fp16 tensors no fused LayerNorm"""
    refused = {c["name"]: choose(hook_args(c, 256), R.knob_array(c)) for c in R.CASES if c["row"] is None}
    assert len(refused) == 5 + 2 + 2 + 2
    for name, msg in refused.items():
        want = ("NAFNet fusions are" if "bf16act" in name else "the fused LayerNorm epilogue" if "pair" in name else "fp16 activation storage needs")
        assert msg.startswith("launch_conv: " + want), (name, msg)


def test_split_k_refuses_gate_and_shuffle():
    """conv_splitk_reduce writes plain rows: a gate or pixel-shuffle layer with split-K is refused, not run"""
    for feat in (R.GATE | R.BIAS, R.SHUFFLE | R.RES):
        for mode in (R.F32, R.FP16, R.PAIR_FP16):
            args = lambda splits: (2, 9, 11, 128, 0, 128, 1, 1, 0, 0) + mode + (feat, splits, 1, 0, 256)
            assert not isinstance(choose(args(1)), str)
            assert choose(args(3)).startswith("launch_conv: split-K has no gate or pixel-shuffle epilogue")


def test_cases_fit_the_device_budget():
    worst = max(R.CASES, key=R.device_bytes)
    assert R.device_bytes(worst) < 160e6, (worst["name"], R.device_bytes(worst))


def test_oracle_agrees_with_the_parity_oracle_on_plain_features():
    """bias / FiLM (shared and per image) / SiLU / residual, concat, upsample, stride: conv_rows_oracle.reference == test_gpu_parity.oracle_conv, bit for bit, in
    float64 and under the operand roundings"""
    from oracle import irsde_oracle as O
    from test_gpu_parity import oracle_conv
    plain = R.BIAS | R.FILM | R.SILU | R.RES | R.FILM_PER_IMAGE
    n = 0
    for c in R.CASES:
        if c["row"] is None or c["nz"] > 1 or c["feat"] & ~plain or R.device_bytes(c) > 4e6:
            continue
        t = R.tensors(c)
        a = (t["x0"], t.get("x1"), t["w"], t.get("bias"), c["stride"], c["pad"], c["up"], t.get("film"), int(bool(c["feat"] & R.SILU)), t.get("res"))
        bstride = 2 * c["Cout"] if c["feat"] & R.FILM_PER_IMAGE else 0
        assert np.array_equal(R.reference(c, t), oracle_conv(*a, film_bstride=bstride)), c["name"]
        with O.bf16_convs():
            want = oracle_conv(*a, film_bstride=bstride)
        assert np.array_equal(R.reference(c, t, operands="bf16"), want), c["name"]
        n += 1
    assert n >= 12


def test_oracle_features_are_live():
    """Each feature moves the reference by far more than any tolerance of the GPU test: dropping it from the case changes the result by > 1e-2 of max|ref|"""
    for name, bit in [("conv3_f32", R.IN_SCALE), ("conv3_f32", R.CH_SCALE), ("conv3_f32", R.RES), ("conv4_lens_f32", R.GATE_FILM), ("row06", R.FILM_PER_IMAGE)]:
        c = R.BY_NAME[name]
        t = R.tensors(c)
        ref = R.reference(c, t)
        if bit == R.FILM_PER_IMAGE:
            t["film"] = t["film"][:1]
        assert R.relerr(R.reference(dict(c, feat=c["feat"] & ~bit), t), ref) > 1e-2, (name, bit)
    c = R.BY_NAME["row14"]   # per-image in_scale: the images' rows swapped
    t = R.tensors(c)
    ref = R.reference(c, t)
    t["in_scale"] = t["in_scale"][::-1]
    assert R.relerr(R.reference(c, t), ref) > 1e-2
