"""Streaming SCAM core, host side (no GPU): the float32 emulation of the kernel's blocked online softmax (tests/scam_stream_oracle.py) against the
float64 restatements, the mutations the GPU bars must be able to see, the wide fixture (tests/golden/stereo_wide.npz,
tools/gen_stereo_wide_golden.py) and the C ABI / Python additions of IRSDE_FLAG_SCAM_STREAM.

Bars: one SCAM 1e-5 of max |SCAM increment| (the GPU bar: the emulation must stay inside it on every kernel shape, every mutation must miss it by
>= 10 x on at least one shape); a network of the wide fixture 1e-4 of max |out| between the float64 restatement and the reference's fp32 result."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle.gen_golden import sub3
import scam_stream_oracle as WS
import stereo_oracle as SO
import stereo_unet_oracle as SU

BAR = 1e-5
# every mutation is measured where it can show: the stale maximum / missing rescales / the neighbouring row's alpha / the shifted boundary from two
# blocks per row, the unmasked tail on a ragged last tile, the swapped directions anywhere
MUTATION_SHAPES = [(2, 5, 10, 64, 16), (1, 2, 17, 32, 16), (1, 2, 130, 64, 64), (1, 2, 509, 128, 256)]

case = WS.case


@pytest.mark.parametrize("shape", WS.STREAM_SHAPES + [WS.C2048_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_emulation_stays_inside_the_bar(shape):
    x, p, want = case(shape)
    e = WS.increment_err(x, want, WS.emulate_stream(p, x, shape[4]))
    print("emulated streaming SCAM %r: %.3g of the increment" % (shape, e))
    assert e < BAR


@pytest.mark.parametrize("mutation", WS.MUTATIONS)
def test_every_mutation_misses_the_bar(mutation):
    errs = {}
    for shape in MUTATION_SHAPES:
        x, p, want = case(shape)
        errs[shape] = WS.increment_err(x, want, WS.emulate_stream(p, x, shape[4], mutation=mutation))
    print(mutation, {k: "%.3g" % v for k, v in errs.items()})
    assert max(errs.values()) >= 10 * BAR, errs


def test_emulation_of_the_quarter_form():
    """The NAFNet form (bicubic quarter-downsample, nearest upsample) at several blocks per row."""
    B, H, W, c = 1, 9, 522, 64   # W' = 130
    x = np.random.RandomState(B * 1000 + W).standard_normal((2 * B, c, H, W)).astype(np.float32)
    p = WS.scam_weights(c, seed=W + c)
    want = SO.scam({k: v.astype(np.float64) for k, v in p.items()}, "f.", x.astype(np.float64))
    assert WS.increment_err(x, want, WS.emulate_stream(p, x, 16, quarter=True)) < BAR
    assert WS.increment_err(x, want, WS.emulate_stream(p, x, 16, mutation="acc_not_rescaled", quarter=True)) >= 10 * BAR


# ---------------------------------------------------------------------------------------------
# the wide fixture
# ---------------------------------------------------------------------------------------------
GOLDEN_SHAPES = {
    "unet_small_1x6x1030/t77": (1, 6, 2, 343), "unet_small_1x6x1030/sensitivity": (),
    "unet_full_1x16x1040/t60": (1, 6, 5, 346), "unet_full_1x16x1040/sensitivity": (),
    "unet_small_sampler_1x6x1030_T5/sde": (1, 6, 2, 343), "unet_small_sampler_1x6x1030_T5/ode": (1, 6, 2, 343),
    "naf_small_1x16x2084/t37": (1, 6, 5, 694), "naf_small_1x16x2084/sensitivity": (),
}


def test_golden_names_and_shapes(golden):
    g = golden.stereo_wide
    assert sorted(g.files) == sorted(GOLDEN_SHAPES)
    for k, shp in GOLDEN_SHAPES.items():
        assert g[k].shape == shp, (k, g[k].shape)
        if k.endswith("sensitivity"):
            assert float(g[k]) >= 0.01, k


@pytest.mark.parametrize("name,cfg,shape,key,t", [("small", WS.UNET_SMALL, (1, 6, 1030), "unet_small_1x6x1030/t77", 77),
                                                  ("full", WS.UNET_FULL, (1, 16, 1040), "unet_full_1x16x1040/t60", 60)])
def test_unet_restatement_follows_the_wide_golden(golden, name, cfg, shape, key, t):
    lq, xT = WS.stereo_inputs(*shape)
    ref = SU.stereo_unet_forward(WS.wide_unet_params(cfg), xT, lq, t, depth=cfg["depth"])
    e = WS.relerr(golden.stereo_wide[key], sub3(ref))
    print("float64 stereo UNet %s vs reference (wide): %.3g" % (name, e))
    assert e < 1e-4


def test_nafnet_restatement_follows_the_wide_golden(golden):
    lq, xT = WS.stereo_inputs(1, 16, 2084)
    cfg = {k: v for k, v in WS.NAF_SMALL.items() if k != "width"}
    ref = SO.stereo_forward(WS.naf_params(), xT, lq, 37, **cfg)
    e = WS.relerr(golden.stereo_wide["naf_small_1x16x2084/t37"], sub3(ref))
    print("float64 stereo NAFNet vs reference (wide): %.3g" % e)
    assert e < 1e-4


# ---------------------------------------------------------------------------------------------
# C ABI and Python surface
# ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("irsde_debug_scam_stream", "irsde_debug_scam_full_stream", "irsde_debug_force_scam_stream")


def test_flag_value_symbols_and_version():
    assert _lib.FLAG_SCAM_STREAM == WS.FLAG_SCAM_STREAM == 2097152
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "irsde_hip.h")).read()
    debug_header = open(os.path.join(root, "include", "irsde_hip_debug.h")).read()
    assert "IRSDE_FLAG_SCAM_STREAM = 2097152" in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert "int %s(" % s in debug_header, s
        assert s in _lib.SYMBOLS, s
        assert hasattr(raw, s), s
        assert getattr(_lib.lib(), s).argtypes is not None, s
    assert _lib.lib().irsde_version() == 107


def _create_unet(flags):
    L = _lib.lib()
    cfg = _lib.Config(3, 3, 32, 2, 0, flags)
    h = ctypes.c_void_p()
    return L, L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)), h


def _create_naf(flags):
    L = _lib.lib()
    cfg = _lib.NafConfig()
    cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
    for i in range(2):
        cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 1
    cfg.device, cfg.flags = 0, flags
    h = ctypes.c_void_p()
    return L, L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h)), h


def _create_latent(flags):
    L = _lib.lib()
    cfg = _lib.LatentConfig()
    cfg.in_ch, cfg.out_ch, cfg.ch, cfg.n_mult, cfg.embed_dim = 3, 3, 32, 2, 4
    cfg.ch_mult[0], cfg.ch_mult[1] = 1, 2
    cfg.device, cfg.flags = 0, flags
    h = ctypes.c_void_p()
    return L, L.irsde_create_latent_unet(ctypes.byref(cfg), ctypes.byref(h)), h


def test_flag_accept_refuse_matrix():
    S = _lib.FLAG_SCAM_STREAM
    for create, flags in ((_create_unet, S | _lib.FLAG_UNET_STEREO), (_create_naf, S | _lib.FLAG_NAF_STEREO),
                          (_create_naf, S | _lib.FLAG_NAF_STEREO | _lib.FLAG_FP16), (_create_latent, 0)):
        L, rc, h = create(flags)
        assert rc == 0, (create.__name__, flags, L.irsde_last_error())
        L.irsde_destroy(h)
    for create, flags in ((_create_unet, S), (_create_unet, S | _lib.FLAG_UNCOND_FULLATTN), (_create_unet, S | _lib.FLAG_BF16),
                          (_create_naf, S), (_create_naf, S | _lib.FLAG_NAF_UNCOND), (_create_naf, S | _lib.FLAG_NAF_INTRO_SKIP),
                          (_create_latent, S)):
        L, rc, h = create(flags)
        assert rc == -1, (create.__name__, flags)   # IRSDE_ERR_INVALID
        assert b"SCAM_STREAM" in L.irsde_last_error(), (create.__name__, flags, L.irsde_last_error())
    # the 16-bit refusals of the stereo UNet are not lifted by the flag
    L, rc, h = _create_unet(S | _lib.FLAG_UNET_STEREO | _lib.FLAG_FP16)
    assert rc == -1 and b"UNET_STEREO" in L.irsde_last_error()


def test_force_scam_stream_argument_check():
    L = _lib.lib()
    try:
        for bad in (17, 8, -16, WS.MAX_BLOCK_W + 16, 1 << 20):
            assert L.irsde_debug_force_scam_stream(bad) == -1, bad   # IRSDE_ERR_INVALID
        for ok in (16, 256, WS.MAX_BLOCK_W):
            assert L.irsde_debug_force_scam_stream(ok) == 0, ok
    finally:
        assert L.irsde_debug_force_scam_stream(0) == 0


def test_set_wide_rows_round_trip():
    for m in (P.stereo_sr.ConditionalUNet(3, 3, 32, depth=2), P.stereo_sr.ConditionalNAFNet(img_channel=3, width=32, enc_blk_nums=[1, 1],
                                                                                              middle_blk_num=1, dec_blk_nums=[1, 1])):
        m.engine_flags = _lib.FLAG_KEEP_ACTIVATIONS
        assert m.set_wide_rows() is m
        assert m.engine_flags == _lib.FLAG_KEEP_ACTIVATIONS | _lib.FLAG_SCAM_STREAM
        assert m.set_wide_rows(True).engine_flags == _lib.FLAG_KEEP_ACTIVATIONS | _lib.FLAG_SCAM_STREAM
        key_on = m._param_key(torch.device("cuda", 0))
        assert m.set_wide_rows(False) is m
        assert m.engine_flags == _lib.FLAG_KEEP_ACTIVATIONS
        assert m._param_key(torch.device("cuda", 0)) != key_on   # the next call builds a fresh engine
        assert m.set_compute_dtype("fp32").set_wide_rows().engine_flags & _lib.FLAG_SCAM_STREAM
    for cls in (P.ConditionalUNet, P.ConditionalNAFNet):
        assert not hasattr(cls, "set_wide_rows")
