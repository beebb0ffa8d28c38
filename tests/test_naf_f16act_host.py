"""'fp16_act' (IRSDE_FLAG_F16_ACT: fp16 activation storage for the image-space ConditionalNAFNets), host side (no GPU): the C ABI flag and its refusals,
`set_compute_dtype`, the float64 restatement (tests/naf_f16act_oracle.py) against the existing oracle, and the sensitivity of the GPU test's comparison
to the mistakes a storage-type port of these kernels can make."""
import ctypes

import numpy as np
import pytest

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import dsde_naf_oracle as DN
import naf_f16act_oracle as FA

TAP_BAR = 1e-3   # tests/test_gpu_naf_f16act.py: per-tap bar of the engine against the restatement restarted from the engine's previous tap


def _naf(L, flags, keep=False):
    cfg = _lib.NafConfig()
    cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
    for i in range(2):
        cfg.enc_blk_nums[i], cfg.dec_blk_nums[i] = 1, 1
    cfg.device, cfg.flags = 0, flags
    h = ctypes.c_void_p()
    rc = L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h))
    if rc == 0 and not keep:
        L.irsde_destroy(h)
    return (rc, h) if keep else rc


def test_flag_is_accepted_and_refused_where_the_header_says():
    L = _lib.lib()
    assert L.irsde_version() == 107
    A, F = _lib.FLAG_F16_ACT, _lib.FLAG_FP16
    assert A == 524288
    assert _naf(L, F | A) == 0
    assert _naf(L, _lib.FLAG_NAF_UNCOND | F | A) == 0
    assert _naf(L, A) == 0                                   # the flag implies IRSDE_FLAG_FP16
    assert _naf(L, F | A | _lib.FLAG_KEEP_ACTIVATIONS) == 0
    assert _naf(L, F | A | _lib.FLAG_BF16) == 0              # (_BF16 next to _FP16 is what the fp16 mode sets itself)
    refused = {"intro_skip": _lib.FLAG_NAF_INTRO_SKIP, "lens": _lib.FLAG_NAF_LENS, "stereo": _lib.FLAG_NAF_STEREO, "bf16_act": _lib.FLAG_BF16_ACT,
               "split_bf16x2": _lib.FLAG_SPLIT_BF16X2, "split_f16x2": _lib.FLAG_SPLIT_F16X2, "naive": _lib.FLAG_NAIVE_CONV}
    for name, f in refused.items():
        for base in (F | A, A):
            assert _naf(L, base | f) == -1, name                       # IRSDE_ERR_INVALID
            assert b"IRSDE_FLAG_F16_ACT" in L.irsde_last_error(), (name, L.irsde_last_error())
    assert _naf(L, A | _lib.FLAG_BF16) == -1                             # bf16 operands without the fp16 bit
    assert b"IRSDE_FLAG_F16_ACT" in L.irsde_last_error()
    # every refusal that existed keeps its own text
    assert _naf(L, _lib.FLAG_BF16_ACT) == -1 and L.irsde_last_error() == b"IRSDE_FLAG_BF16_ACT: conditional UNet only"
    assert _naf(L, F | _lib.FLAG_BF16_ACT) == -1 and L.irsde_last_error() == b"IRSDE_FLAG_BF16_ACT: conditional UNet only"
    assert _naf(L, _lib.FLAG_NAF_UNCOND | _lib.FLAG_NAF_LENS) == -1 and b"IRSDE_FLAG_NAF_UNCOND cannot be combined" in L.irsde_last_error()
    # the UNet and the latent UNet refuse it
    h = ctypes.c_void_p()
    for flags in (A, F | A):
        cfg = _lib.Config(3, 3, 32, 2, 0, flags)
        assert L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
        assert b"IRSDE_FLAG_F16_ACT" in L.irsde_last_error()
        lc = _lib.LatentConfig()
        lc.in_ch, lc.out_ch, lc.ch, lc.n_mult, lc.embed_dim, lc.device, lc.flags = 3, 3, 8, 2, 8, 0, flags
        lc.ch_mult[0], lc.ch_mult[1] = 4, 8
        assert L.irsde_create_latent_unet(ctypes.byref(lc), ctypes.byref(h)) == -1
        assert b"IRSDE_FLAG_F16_ACT" in L.irsde_last_error()
    # CNAFNetLocal's window does not apply to an engine that has it
    rc, h = _naf(L, F | A, keep=True)
    assert rc == 0
    try:
        assert L.irsde_nafnet_set_local_pool(h, 24, 24, 16, 16) == -1
        assert b"IRSDE_FLAG_F16_ACT" in L.irsde_last_error()
    finally:
        L.irsde_destroy(h)


def test_set_compute_dtype_sets_both_bits():
    kw = dict(img_channel=3, width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
    both = _lib.FLAG_FP16 | _lib.FLAG_F16_ACT
    for cls in (P.ConditionalNAFNet, P.denoising_sde.ConditionalNAFNet):
        m = cls(**kw)
        m.engine_flags = _lib.FLAG_KEEP_ACTIVATIONS
        assert m.set_compute_dtype("fp16_act") is m
        assert m.engine_flags == both | _lib.FLAG_KEEP_ACTIVATIONS
        m.set_compute_dtype("fp16")
        assert m.engine_flags == _lib.FLAG_FP16 | _lib.FLAG_KEEP_ACTIVATIONS
        m.set_compute_dtype("fp16_act").set_compute_dtype("fp32")
        assert m.engine_flags == _lib.FLAG_KEEP_ACTIVATIONS
        with pytest.raises(_lib.IrsdeError, match="'fp16_act'"):
            m.set_compute_dtype("fp8")
    # the networks the mode does not cover keep their list of names
    for m in (P.ConditionalUNet(3, 3, 32, depth=2), P.latent.ConditionalNAFNet(**kw), P.latent_bokeh.ConditionalNAFNet(**kw)):
        with pytest.raises(_lib.IrsdeError) as ei:
            m.set_compute_dtype("fp16_act")
        assert "fp16_act" not in str(ei.value) and "'fp16'" in str(ei.value)
        assert not m.engine_flags & _lib.FLAG_F16_ACT


@pytest.mark.parametrize("uncond", [False, True])
def test_restatement_without_storage_is_the_fp16_oracle(uncond):
    width, enc, mid, dec, B, H, W = FA.CASES["w32"]
    bp = FA.make_params(width, enc, mid, dec, seed=3, uncond=uncond)
    xt, cond = FA.make_inputs(2, 22, 19, seed=21, uncond=uncond)
    tvec = np.array([5, 60])
    with O.f16_convs():
        ref = DN.forward(bp, xt, tvec, enc, mid, dec) if uncond else O.nafnet_forward(bp, xt, cond, tvec, enc, mid, dec)
    got = FA.forward(bp, xt, tvec, enc, mid, dec, cond=cond, store=False)
    assert np.array_equal(got, ref)
    stored = FA.forward(bp, xt, tvec, enc, mid, dec, cond=cond)
    e = FA.relerr(stored, ref)
    assert 1e-5 < e < 3e-3, e      # the storage roundings are on, and cost no more than the fp16-vs-fp32 network bar


@pytest.mark.parametrize("case", ["w64", "w32"])
def test_tap_comparison_is_sensitive_to_each_mistake(case):
    """The GPU test compares every tap with the restatement restarted from the previous tap at 1e-3 of max|ref|.  Here the CORRECT restatement stands in
    for the engine and each deliberately wrong reference has to miss that bar at least tenfold on some tap (seeds chosen for that; beta / gamma
    ~ 0.5 N(0, 1), sca.1.weight x 8: `make_params`)."""
    width, enc, mid, dec, B, H, W = FA.CASES[case]
    bp = FA.make_params(width, enc, mid, dec, seed=3)
    xt, cond = FA.make_inputs(B, H, W, seed=21)
    tvec = np.array([5, 60, 33])
    taps = {}
    FA.forward(bp, xt, tvec, enc, mid, dec, cond=cond, taps=taps)
    good = FA.restart_taps(bp, taps, tvec, enc, mid, dec)
    assert sorted(good) == sorted(k for k in taps if k != "intro")
    assert all(np.array_equal(good[k], taps[k]) for k in good)      # restarting the right reference from its own taps reproduces them
    for mut in FA.MUTATIONS:
        bad = FA.restart_taps(bp, taps, tvec, enc, mid, dec, mut=mut)
        worst = max(FA.relerr(taps[k], bad[k]) for k in bad)
        print(case, mut, "%.3g" % worst)
        assert worst >= 10 * TAP_BAR, (mut, worst)
