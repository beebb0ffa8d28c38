"""stereo-sr ConditionalUNet, host side (no GPU): the float64 restatement (tests/stereo_unet_oracle.py) against the reference golden
(tests/golden/stereo_unet.npz, tools/gen_stereo_unet_golden.py), the fixture's attention sensitivity, the parameter names of the drop-in
module and the C ABI additions.  Bars: those of tests/test_stereo_host.py (forward 5e-6 of max |ref|: the fixture is the reference's
fp32 result; a hooked SCAM 1e-6 of its increment)."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
from oracle.gen_golden import sub3
import stereo_unet_oracle as SU

SMALL = dict(nf=32, depth=2)
FULL = dict(nf=64, depth=4)
TAG = "small_2x22x38"


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


@pytest.fixture(scope="module")
def small_params():
    return SU.stereo_unet_synth_params(seed=0, **SMALL)


def test_forward_matches_reference_golden(golden, small_params):
    g = golden.stereo_unet
    lq, xT = inputs(2, 22, 38)
    for key, t in (("t3", 3), ("t77", 77), ("t5_60", [5, 60])):
        e = rel(SU.stereo_unet_forward(small_params, xT, lq, t, depth=2), g[TAG + "/" + key])
        print("oracle vs reference %s: %.3g" % (key, e))
        assert e <= 5e-6, (key, e)


def test_forward_matches_reference_golden_full(golden):
    g = golden.stereo_unet
    p = SU.stereo_unet_synth_params(seed=0, **FULL)
    lq, xT = inputs(1, 32, 48)
    e = rel(sub3(SU.stereo_unet_forward(p, xT, lq, 60, depth=4)), g["full_1x32x48/t60_sub3"])
    print("oracle vs reference nf64 depth4: %.3g" % e)
    assert e <= 5e-6


@pytest.mark.parametrize("key,prefix", [("mid_fusion", "mid_fusion."), ("ups13", "ups.1.3.")])
def test_hooked_scam_matches_reference_golden(golden, small_params, key, prefix):
    """The fixture keeps the first and the last row of the hooked maps: a SCAM works on one image row at a time."""
    g = golden.stereo_unet
    x, want = g[TAG + "/" + key + "_in"].astype(np.float64), g[TAG + "/" + key + "_out"].astype(np.float64)
    assert x.shape[2] == 2 and x.shape[0] == 4
    got = SU.scam_full(small_params, prefix, x)
    e = float(np.abs(got - want).max() / np.abs(want - x).max())
    print("oracle SCAM %s vs reference: %.3g of the increment" % (key, e))
    assert e <= 1e-6


def test_fixture_is_attention_sensitive(golden, small_params):
    g = golden.stereo_unet
    stored = float(g[TAG + "/sensitivity"])
    assert stored >= 0.01
    lq, xT = inputs(2, 22, 38)
    ref = SU.stereo_unet_forward(small_params, xT, lq, 77, depth=2)
    uni = SU.stereo_unet_forward(small_params, xT, lq, 77, depth=2, uniform=True)
    mine = rel(uni, ref)
    print("sensitivity: stored %.4f, oracle %.4f" % (stored, mine))
    assert abs(mine - stored) <= 1e-3 * stored and mine >= 0.01


def test_define_g_returns_the_stereo_unet():
    opt = {"network_G": {"which_model_G": "ConditionalUNet", "setting": dict(in_nc=3, out_nc=3, nf=32, depth=2)}}
    m = P.define_G(opt, "stereo-sr")
    assert type(m) is P.stereo_sr.ConditionalUNet
    assert m.in_nc == m.out_nc == 6 and m.view_nc == 3
    assert type(P.define_G(opt)) is P.ConditionalUNet   # the deraining task keeps its own class
    with pytest.raises(NotImplementedError):
        P.define_G({"network_G": {"which_model_G": "DiT", "setting": {}}}, "stereo-sr")


def test_state_dict_names_and_shapes_equal_reference(golden):
    names = sorted(str(n) for n in golden.stereo_unet["names"])
    m = P.stereo_sr.ConditionalUNet(3, 3, 64, depth=4, upscale=1, fusion=False)
    assert sorted(m.state_dict()) == names
    shapes = SU.stereo_unet_param_shapes(3, 3, **FULL)
    assert sorted(shapes) == names
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == shapes[k], k
    assert tuple(m.state_dict()["init_conv.weight"].shape) == (64, 6, 3, 3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in SU.stereo_unet_synth_params(seed=0, **FULL).items()}, strict=True)
    assert m.set_compute_dtype("fp32") is m
    for d in ("bf16", "bf16_act", "fp16", "fp32_split", "fp32_split_f16"):
        with pytest.raises(_lib.IrsdeError):
            m.set_compute_dtype(d)


def _create(in_nc, nf, depth, flags):
    L = _lib.lib()
    cfg = _lib.Config(in_nc, in_nc, nf, depth, 0, flags)
    h = ctypes.c_void_p()
    return L, L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)), h


def test_engine_inventory_equals_reference_state_dict(golden):
    """Engine creation and its weight inventory are host-side: the stereo UNet engine lists the reference state_dict."""
    L, rc, h = _create(3, 64, 4, _lib.FLAG_UNET_STEREO)
    assert rc == 0, L.irsde_last_error()
    try:
        n = L.irsde_num_weights(h)
        names = [L.irsde_weight_name(h, i).decode() for i in range(n)]
        shapes = SU.stereo_unet_param_shapes(3, 3, **FULL)
        for i, name in enumerate(names):
            shp, nd = (ctypes.c_int64 * 4)(), ctypes.c_int()
            assert L.irsde_weight_shape(h, i, shp, ctypes.byref(nd)) == 0
            assert tuple(shp[:nd.value]) == shapes[name], name
    finally:
        L.irsde_destroy(h)
    assert sorted(names) == sorted(str(s) for s in golden.stereo_unet["names"])


def test_cabi_additions_keep_the_version():
    L = _lib.lib()
    assert "irsde_debug_scam_full" in _lib.SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "irsde_debug_scam_full")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "irsde_debug_scam")
    assert L.irsde_version() == 107
    assert _lib.FLAG_UNET_STEREO == 262144


def test_flag_refusals():
    S = _lib.FLAG_UNET_STEREO
    for f in (_lib.FLAG_BF16, _lib.FLAG_BF16 | _lib.FLAG_BF16_ACT, _lib.FLAG_BF16_ACT, _lib.FLAG_FP16, _lib.FLAG_SPLIT_BF16X2, _lib.FLAG_SPLIT_F16X2,
              _lib.FLAG_UNCOND_FULLATTN):
        L, rc, h = _create(3, 32, 2, S | f)
        assert rc == -1, f   # IRSDE_ERR_INVALID
        assert b"UNET_STEREO" in L.irsde_last_error(), f
    L, rc, h = _create(3, 32, 2, S)
    assert rc == 0
    L.irsde_destroy(h)
    # the flag belongs to irsde_create
    cfg = _lib.NafConfig()
    cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
    for i in range(2):
        cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 1
    cfg.device, cfg.flags = 0, S
    h = ctypes.c_void_p()
    assert L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"UNET_STEREO" in L.irsde_last_error()
