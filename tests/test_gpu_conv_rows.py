"""Every row of launch_conv's instance tables (csrc/conv_igemm.hip: 53 implicit-GEMM / PAIR instances, 3 tile-loop instances) and every epilogue of the
ConvParams contract against the float64 oracle tests/conv_rows_oracle.py: one production launch per case through irsde_debug_conv_features.  The case table is
checked on the host by tests/test_conv_rows_host.py; here each case must report the row it names (the launch's own ConvChoice), write every output element
(the output is pre-filled with NaN) and meet the bound of its mode — the bounds of tests/test_gpu_parity.py's kernel tests, relative to max|ref|:

    f32, PAIR fp16      2e-5 against the float64 oracle                                                  (test_conv_kernel)
    PAIR bf16           2e-4 against the float64 oracle                                                  (test_gpu_split.py's direct PAIR layers)
    16-bit operands     2e-5 against the operand-rounded oracle, and inside the band that says "this really is the reduced-precision product" against the
                        full one: bf16 (1e-4, 2e-2), fp16 (1e-5, 3e-3)                                   (test_conv_kernel_bf16 / _fp16)
    bf16 tensors        every element within 2^-7 |ref| + 1e-6 of the oracle with the same roundings, what comes back is representable in bf16, at most
                        2 % of the elements differ from the rounded oracle                               (test_conv_kernel_bf16_storage)
    fp16 tensors        the same rule with 2^-10 (one fp16 ulp is 2^-11 relative to the value) and fp16

The 2 % cap is a condition on the inputs as much as on the kernel (a different fp32 accumulation order flips a rounding now and then).  Measured on the CPU
for the table's own inputs, a float32 numpy restatement of the layer against the float64 oracle, both rounded to the storage type (profiles/conv_rows.md):
the share of differing elements is at most 0.20 % on the fp16-tensor cases (row26) and 0.016 % on the bf16-tensor cases — the cap leaves a factor of 10
(tools/conv_rows_cpu_figures.py prints them; observed on the MI355X: 0.13 % / 0.016 %).
The fused LayerNorm and the gate product have no bound of their own: they meet the 2e-5 of their mode (float32 restatement against float64 on the CPU:
2.2e-7 / 3.3e-7; measured on the MI355X: 2.0e-7 / 2.8e-7)."""
import ctypes

import numpy as np
import pytest
import torch

import conv_rows_oracle as R
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
from test_conv_rows_host import check_choice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OPERANDS = {0: None, 1: "bf16", 2: "f16"}
BAND = {"bf16": (1e-4, 2e-2), "f16": (1e-5, 3e-3)}
STORE_ULPS = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}
STORE_ROUND = {"bf16": O.round_bf16, "f16": O.round_f16}


def launch(c, t, L=None):
    """One irsde_debug_conv_features call: (output in the reference's layout, NaN where nothing was written; the choice line as a dict) — or, refused,
    (the untouched output, the message)"""
    L = L or _lib.lib()
    feat, B, Cout, nz = c["feat"], c["B"], c["Cout"], c["nz"]
    Ho, Wo = R.out_hw(c)
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(DEV)
    dev = lambda k: torch.from_numpy(np.ascontiguousarray(t[k])).to(DEV) if k in t else None
    host = lambda k: np.ascontiguousarray(t[k], dtype=np.float32).ctypes.data_as(ctypes.c_void_p) if k in t else None
    ptr = lambda d: ctypes.c_void_p(d.data_ptr()) if d is not None else None
    if nz > 1:
        d0, d1, dres = dev("x0"), None, None
        out = torch.full((nz, Wo, Cout), float("nan"), device=DEV)
    else:
        d0, d1, dres = nhwc(t["x0"]), nhwc(t["x1"]) if "x1" in t else None, nhwc(t["res"]) if "res" in t else None
        shape = (B, Ho, Wo, Cout // 2) if feat & R.GATE else (B, 2 * Ho, 2 * Wo, Cout // 4) if feat & R.SHUFFLE else (B, Ho, Wo, Cout)
        out = torch.full(shape, float("nan"), device=DEV)
    dfilm, dscale, dgf = dev("film"), dev("in_scale"), dev("gate_film")
    w = np.ascontiguousarray(t["w"], dtype=np.float32)
    kn = R.knob_array(c)
    line = ctypes.create_string_buffer(512)
    operand, storage, pair = c["mode"]
    torch.cuda.synchronize()
    rc = L.irsde_debug_conv_features(
        ptr(d0), c["C0"], ptr(d1), c["C1"], B, c["H"], c["W"], c["up"], w.ctypes.data_as(ctypes.c_void_p), Cout, c["K"], c["stride"], c["pad"], operand, storage, pair,
        host("bias"), host("ch_scale"), host("ln_g"), ptr(dfilm), 2 * Cout if feat & R.FILM_PER_IMAGE else 0, ptr(dres), ptr(dscale), ptr(dgf), Cout,
        int(bool(feat & R.SILU)), int(bool(feat & R.GATE)), int(bool(feat & R.SHUFFLE)), nz, c["splits"], c["tune"], (ctypes.c_int * 11)(*kn) if kn else None,
        ptr(out), line, len(line), None)
    got = out.cpu().numpy()
    got = got if nz > 1 else got.transpose(0, 3, 1, 2)
    if rc != 0:
        return got, L.irsde_last_error().decode()
    text = line.value.decode()
    head, _, halo = text.partition(" kernel=")   # a launch of the halo family appends its own choice (irsde_debug_conv_halo_choice's line)
    d = dict(kv.split("=") for kv in head.replace(" of ", "/").split())
    if halo:
        d["halo"] = "kernel=" + halo
    return got, d


def figures(c, got, ref, ref_full=None):
    """What the bounds are asserted on ({name: value}): ref is the oracle with the roundings of the case's mode, ref_full the unrounded one (16-bit operands on
    f32 tensors only)"""
    st = OPERANDS[c["mode"][1]]
    fig = {}
    if st:
        err = np.abs(got - ref)
        fig["worst_excess"] = float((err - (np.abs(ref) * STORE_ULPS[st] + 1e-6)).max())
        fig["share_differing"] = float((err > 0).mean())
    else:
        fig["relerr"] = R.relerr(got, ref)
        if ref_full is not None:
            fig["relerr_vs_full"] = R.relerr(got, ref_full)
    return fig


def assert_bounds(c, got, ref, fig):
    """Every output element written, and the bound of the case's mode (the module docstring lists them)"""
    operand, storage, pair = c["mode"]
    ops = None if pair else OPERANDS[operand]
    st = OPERANDS[storage]
    assert got.shape == ref.shape and bool(np.isfinite(got).all()), c["name"]
    if st:
        assert np.array_equal(got, STORE_ROUND[st](got)), c["name"]   # what comes back was stored in the 16-bit type
        assert fig["worst_excess"] <= 0, (c["name"], fig)
        assert fig["share_differing"] < 0.02, (c["name"], fig)
    else:
        assert fig["relerr"] < (2e-4 if pair and operand == 1 else 2e-5), (c["name"], fig)
        if ops:
            lo, hi = BAND[ops]
            assert lo < fig["relerr_vs_full"] < hi, (c["name"], fig)


def check_case(c, L=None):
    """Runs the case and asserts its row and its bound; returns the figures it measured ({name: value}), printed before anything is asserted"""
    t = R.tensors(c)
    got, d = launch(c, t, L)
    if c["row"] is None:   # refused by conv_validate before anything was launched
        assert isinstance(d, str) and d.startswith("launch_conv: ") and np.isnan(got).all(), (c["name"], d)
        return {}
    operand, storage, pair = c["mode"]
    ops = None if pair else OPERANDS[operand]
    st = OPERANDS[storage]
    ref = R.reference(c, t, operands=ops, storage=st)
    fig = figures(c, got, ref, R.reference(c, t) if ops and not st else None)
    print("conv_rows %s row=%s chose=%s written=%d %s" % (c["name"], c["row"], d if isinstance(d, str) else d["name"] + ":" + d["row"], bool(np.isfinite(got).all()),
                                                         " ".join("%s=%.3g" % kv for kv in sorted(fig.items()))))
    check_choice(c, d)
    assert_bounds(c, got, ref, fig)
    return fig


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_conv_row(name):
    check_case(R.BY_NAME[name])


@pytest.mark.parametrize("mode,tune", [(R.BF16, 60), (R.FP16, 60), (R.F32, 50)])
def test_fused_layernorm_on_a_tile_wider_than_cout_is_refused(mode, tune):
    """The LayerNorm epilogue normalises over the tile's columns: a forced 256 x 256 tile on a 128-channel layer is refused by launch_conv itself (the choice
    is legal for conv_choose, the launch is not), before anything runs"""
    c = R.case("ln_wide", None, None, 2, 9, 11, 64, 0, 128, 1, mode=mode, feat=R.LN_G | R.BIAS | R.RES, tune=tune)
    got, msg = launch(c, R.tensors(c))
    assert isinstance(msg, str) and msg.startswith("launch_conv: the fused LayerNorm epilogue needs a column tile as wide as Cout, chosen igemm256x256"), msg
    assert np.isnan(got).all()
