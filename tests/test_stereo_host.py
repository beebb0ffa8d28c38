"""stereo-sr network, host side (no GPU): the float64 restatement (tests/stereo_oracle.py) against the reference golden
(tests/golden/stereo.npz, tools/gen_stereo_golden.py), its resampling steps against torch, the fixture's attention sensitivity,
the parameter names of the drop-in module and the C ABI additions."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
import stereo_oracle as SO
from oracle.gen_golden import sub3

SMALL = dict(enc_blk_nums=(1, 1), middle_blk_num=1, dec_blk_nums=(1, 1))
REFUSION = dict(enc_blk_nums=(1, 1, 1, 28), middle_blk_num=1, dec_blk_nums=(1, 1, 1, 1))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def small_params():
    return SO.stereo_synth_params(seed=0, width=32, **SMALL)


def inputs(B, H, W):
    from oracle import irsde_oracle as O
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


@pytest.mark.parametrize("shape", [(10, 14), (5, 7), (16, 16), (20, 28), (4, 4), (7, 9)])
def test_bicubic_quarter_equals_torch(shape):
    x = np.random.RandomState(1).standard_normal((2, 3) + shape)
    want = F.interpolate(torch.from_numpy(x), scale_factor=0.25, mode="bicubic").numpy()
    got = SO.bicubic_quarter(x)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("src,dst", [((3, 3), (14, 14)), ((2, 3), (10, 14)), ((1, 1), (5, 7)), ((5, 7), (20, 28)), ((4, 4), (16, 16)),
                                     ((7, 5), (30, 23))])
def test_nearest_resize_equals_torch(src, dst):
    x = np.random.RandomState(2).standard_normal((1, 2) + src).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x), size=dst).numpy()
    assert np.array_equal(SO.nearest_resize(x, *dst), want)
    if src == (3, 3):   # 3 -> 14 is 0 x5, 1 x5, 2 x4 (not dst // 4)
        assert list(SO.nearest_index(14, 3)) == [0] * 5 + [1] * 5 + [2] * 4


def test_forward_matches_reference_golden(golden):
    g = golden.stereo
    p = small_params()
    lq, xT = inputs(2, 32, 48)
    for key, t in (("t3", 3), ("t77", 77), ("t5_60", [5, 60])):
        e = rel(g["small_2x32x48/" + key], SO.stereo_forward(p, xT, lq, t, **SMALL))
        assert e < 1e-6, (key, e)


def test_forward_matches_reference_golden_refusion(golden):
    """40 NAFBlock + SCAM pairs: the fixture is the reference's fp32 result, whose own rounding reaches ~1e-6 of max |out| here
    (measured 1.04e-6); 5e-6 stays well inside the deraining NAFNet restatement's 2e-5 bar (tests/test_oracle_golden.py)."""
    g = golden.stereo
    p = SO.stereo_synth_params(seed=0, width=64, **REFUSION)
    lq, xT = inputs(1, 64, 64)
    assert rel(g["refusion_1x64x64/t60"], SO.stereo_forward(p, xT, lq, 60, **REFUSION)) < 5e-6
    lq, xT = inputs(1, 80, 112)
    assert rel(g["refusion_1x80x112/t37_sub3"], sub3(SO.stereo_forward(p, xT, lq, 37, **REFUSION))) < 5e-6


def test_block_level_scam_matches_reference_golden(golden):
    g = golden.stereo
    p = {k: v.astype(np.float64) for k, v in small_params().items()}
    got = SO.scam(p, "middle_blks.0.fusion.", g["small_2x32x48/scam_in"].astype(np.float64))
    assert rel(g["small_2x32x48/scam_out_sub3"], sub3(got)) < 1e-6
    p = {k: v.astype(np.float64) for k, v in SO.stereo_synth_params(seed=0, width=64, **REFUSION).items()}
    got = SO.scam(p, "middle_blks.0.fusion.", g["refusion_1x64x64/scam_in"].astype(np.float64))
    assert rel(g["refusion_1x64x64/scam_out"], got) < 1e-6


def test_fixture_is_attention_sensitive(golden):
    """With default-like weights the softmax is nearly uniform and a wrong softmax / direction would hide: the fixture's weights must
    make the uniform-average variant move the output by >= 5 % of its range (recorded from the reference, checked again here)."""
    g = golden.stereo
    assert float(g["small_2x32x48/sensitivity"]) >= 0.05
    p = small_params()
    lq, xT = inputs(2, 32, 48)
    ref = SO.stereo_forward(p, xT, lq, 77, **SMALL)
    uni = SO.stereo_forward(p, xT, lq, 77, uniform=True, **SMALL)
    assert rel(uni, ref) >= 0.05


def test_state_dict_names_equal_reference(golden):
    names = sorted(str(n) for n in golden.stereo["names"])
    m = P.stereo_sr.ConditionalNAFNet(img_channel=3, width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
    assert sorted(m.state_dict()) == names
    shapes = SO.stereo_param_shapes(width=64, **REFUSION)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == shapes[k], k
    # a reference checkpoint loads strictly
    m.load_state_dict({k: torch.from_numpy(v) for k, v in SO.stereo_synth_params(seed=0, width=64, **REFUSION).items()}, strict=True)


def test_define_g_picks_the_stereo_class():
    opt = {"network_G": {"which_model_G": "ConditionalNAFNet", "setting": dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])}}
    m = P.define_G(opt, "stereo-sr")
    assert isinstance(m, P.stereo_sr.ConditionalNAFNet)
    assert m.in_nc == m.out_nc == 6 and m.img_channel == 3
    assert type(P.define_G(opt)) is P.ConditionalNAFNet


def test_cabi_exports_debug_scam_and_keeps_version():
    L = _lib.lib()
    assert "irsde_debug_scam" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "irsde_debug_scam")
    assert L.irsde_version() == 107
    assert _lib.FLAG_NAF_STEREO == 65536


def test_engine_inventory_equals_reference_state_dict(golden):
    """Engine creation and its weight inventory are host-side: the stereo engine's names are the reference state_dict."""
    L = _lib.lib()
    cfg = _lib.NafConfig()
    cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 64, 1, 4, 4
    for i, (a, b) in enumerate(zip([1, 1, 1, 28], [1, 1, 1, 1])):
        cfg.enc_blk_nums[i], cfg.dec_blk_nums[i] = a, b
    cfg.device, cfg.flags = 0, _lib.FLAG_NAF_STEREO
    h = ctypes.c_void_p()
    _lib.check(L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h)))
    try:
        names = sorted(L.irsde_weight_name(h, i).decode() for i in range(L.irsde_num_weights(h)))
    finally:
        L.irsde_destroy(h)
    assert names == sorted(str(n) for n in golden.stereo["names"])


def test_stereo_flag_refusals():
    L = _lib.lib()

    def naf(flags):
        cfg = _lib.NafConfig()
        cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
        for i in range(2):
            cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 1
        cfg.device, cfg.flags = 0, flags
        h = ctypes.c_void_p()
        rc = L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            L.irsde_destroy(h)
        return rc

    S = _lib.FLAG_NAF_STEREO
    assert naf(S) == 0 and naf(S | _lib.FLAG_FP16) == 0
    for f in (_lib.FLAG_NAF_LENS, _lib.FLAG_NAF_INTRO_SKIP, _lib.FLAG_BF16, _lib.FLAG_SPLIT_BF16X2, _lib.FLAG_SPLIT_F16X2):
        assert naf(S | f) == -1, f   # IRSDE_ERR_INVALID
        assert b"NAF_STEREO" in L.irsde_last_error()
    cfg = _lib.Config(3, 3, 32, 2, 0, S)
    h = ctypes.c_void_p()
    assert L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"NAF_STEREO" in L.irsde_last_error()
