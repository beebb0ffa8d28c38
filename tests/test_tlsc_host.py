"""CNAFNetLocal (TLSC local pooling) on the host: the window rule, the float64 restatement of tests/tlsc_oracle.py against the real
reference's goldens (tests/golden/tlsc.npz, tools/gen_tlsc_golden.py), the pooling sensitivity of those goldens, and the class's surface.
No GPU: nothing here creates an engine.

Networks: enc [1,1], middle 1, dec [1,1], img_channel 3, train sizes (1,3,16,16) -> windows 24 / 12 / 6 and (1,3,20,12) -> 30x18 / 15x9 / 7x4,
at width 16 (w16_*) and at width 32 (w32_*: the engine's smallest width, what tests/test_gpu_tlsc.py runs; the windows depend on depth and
train size only, so they are the same).
"""
import os
import re

import numpy as np
import pytest

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib, latent
from oracle import irsde_oracle as O
import tlsc_oracle as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def make(name, **kw):
    width, train_size = TL.NETS[name]
    args = dict(img_channel=3, width=width, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1], train_size=train_size)
    args.update(kw)
    return P.CNAFNetLocal(**args)


@pytest.mark.parametrize("name", sorted(TL.NETS))
def test_window_rule_vs_reference_kernel_sizes(golden, name):
    """Host rule == the kernel_size lists the reference's conversion forward recorded (module order enc0, enc1, middle, dec0, dec1)."""
    ks = golden.tlsc[name + "/kernel_sizes"].tolist()
    want = TL.WINDOWS[TL.NETS[name][1]]
    lv = latent.tlsc_windows(TL.NETS[name][1], 2)
    assert [tuple(k) for k in ks] == [lv[0], lv[1], lv[2], lv[1], lv[0]]
    assert lv == want == TL.windows(TL.NETS[name][1]) == make(name).kernel_sizes
    assert make(name).base_size == (int(TL.NETS[name][1][2] * 1.5), int(TL.NETS[name][1][3] * 1.5))


def test_window_rule_pads_the_train_size():
    """A train size that is no multiple of 2^n_enc is zero-padded by the conversion forward before the levels halve it."""
    assert latent.tlsc_windows((1, 3, 18, 13), 2) == [(20 * 27 // 18, 16 * 19 // 13), (10 * 27 // 18, 8 * 19 // 13), (5 * 27 // 18, 4 * 19 // 13)]
    assert latent.tlsc_windows((1, 4, 32, 32), 4)[0] == (48, 48)     # nasde.yml's network on 32 x 32 latents


@pytest.mark.parametrize("tag", sorted(TL.FORWARD))
def test_restatement_vs_reference_golden(golden, tag):
    """float64 restatement vs the reference (fp32, prefix sums): <= 1e-5 of max |ref|.  Measured 4.7e-7 .. 7.4e-7 (96 x 128: 7.4e-7)."""
    g = golden.tlsc
    name, B, H, W, ts, stride = TL.FORWARD[tag]
    params = TL.synth_params(name)
    cond, xt = TL.inputs(B, H, W)
    assert list(g[tag + "/ts"]) == list(ts)
    for t in ts:
        ref = g[tag + ("/t%d" % t if stride == 1 else "/t%d_sub%d" % (t, stride))]
        got = TL.forward(params, xt, cond, int(t), TL.NETS[name][1])[..., ::stride, ::stride]
        e = relerr(got, ref)
        print("%s t=%d: %.3g" % (tag, t, e))
        assert e <= 1e-5, (tag, t, e)


@pytest.mark.parametrize("tag", sorted(t for t, v in TL.FORWARD.items() if v[2:4] != (16, 16)))
def test_goldens_are_pooling_sensitive(golden, tag):
    """Replacing the local pool by the global one in the restatement moves the output by >= 1e-2 of max |out| (100 x the parity bar) at every
    local shape -- a global-pool engine cannot pass these goldens.  Measured at t = 7 with SCA_GAIN = 32 and the structured inputs:
    w32_t16 40x56 0.045, 37x50 0.045, 20x56 0.032, 96x128 0.087; w32_t20x12 40x56 0.046, 37x50 0.050; w16_t16 40x56 0.031, 20x56 0.021;
    w16_t20x12 37x50 0.048.  (Plain weights and uniform-noise inputs: 1e-3 .. 5e-3.)"""
    name, B, H, W, ts, stride = TL.FORWARD[tag]
    params = TL.synth_params(name)
    cond, xt = TL.inputs(B, H, W)
    loc = TL.forward(params, xt, cond, 7, TL.NETS[name][1])
    glo = TL.forward(params, xt, cond, 7, TL.NETS[name][1], local=False)
    s = float(np.abs(loc - glo).max() / np.abs(loc).max())
    print("%s: sensitivity %.4f" % (tag, s))
    assert s >= 1e-2, (tag, s)
    key = tag + ("/t7" if stride == 1 else "/t7_sub%d" % stride)
    assert relerr(glo[..., ::stride, ::stride], golden.tlsc[key]) >= 1e-2   # ... and the global-pool network misses the stored golden by as much


def test_covered_shape_is_the_plain_network(golden):
    """16 x 16 with train 16: every window covers its map -> the restatement with local pools equals the global one bit for bit."""
    name, B, H, W, ts, _ = TL.FORWARD["w32_t16_1x16x16"]
    params = TL.synth_params(name)
    cond, xt = TL.inputs(B, H, W)
    a = TL.forward(params, xt, cond, 7, TL.NETS[name][1])
    assert np.array_equal(a, TL.forward(params, xt, cond, 7, TL.NETS[name][1], local=False))
    assert np.array_equal(a, O.nafnet_forward(params, xt, cond, 7, (1, 1), 1, (1, 1), intro_skip=True))


def test_local_pool_definition():
    """The restated pool against the definition written out: m[i][j] = mean x[i:i+k1, j:j+k2], pooled[y][x] = m[clamp(y - top)][clamp(x - left)]."""
    rs = np.random.RandomState(3)
    x = rs.standard_normal((1, 2, 7, 9))
    for K in ((4, 6), (3, 20), (20, 5), (7, 4)):
        got = TL.local_pool(x, K)
        k1, k2 = min(7, K[0]), min(9, K[1])
        top, left = (k1 - 1) // 2, (k2 - 1) // 2
        for y in range(7):
            for xx in range(9):
                i, j = min(max(y - top, 0), 7 - k1), min(max(xx - left, 0), 9 - k2)
                np.testing.assert_allclose(got[0, :, y, xx], x[0, :, i:i + k1, j:j + k2].mean(axis=(1, 2)), rtol=1e-12, atol=1e-14)
    assert TL.local_pool(x, (7, 9)).shape == (1, 2, 1, 1)


@pytest.mark.parametrize("name", sorted(TL.NETS))
def test_state_dict_is_the_latent_networks(golden, name):
    g = golden.tlsc
    width = TL.NETS[name][0]
    plain = latent.ConditionalNAFNet(img_channel=3, width=width, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
    sd, sp = make(name).state_dict(), plain.state_dict()
    assert list(sd) == list(sp)
    assert all(sd[k].shape == sp[k].shape for k in sd)
    assert sorted(sd) == list(g[name + "/names"]) == list(g[name + "/names_plain"])
    assert sorted(sd) == sorted(O.naf_param_shapes(img_channel=3, **TL.cfg_of(name)))


def test_refusals_and_lookup():
    with pytest.raises(_lib.IrsdeError, match="fast_imp"):
        make("w32_t16", fast_imp=True)
    with pytest.raises(_lib.IrsdeError, match="channels"):
        make("w32_t16", train_size=(1, 4, 16, 16))          # the reference's conversion forward fails in intro
    assert P.CNAFNetLocal is latent.CNAFNetLocal and "CNAFNetLocal" in P.__all__
    assert make("w32_t16", train_size=[1, 3, 16, 16]).train_size == (1, 3, 16, 16)
    m = latent.CNAFNetLocal(3, 32, 1, [1, 1], [1, 1])                      # the reference's positional signature and default train size
    assert m.train_size == (1, 3, 128, 128) and m.base_size == (192, 192) and m.kernel_sizes[0] == (192, 192)
    opt = {"network_G": {"which_model": "CNAFNetLocal", "setting": dict(img_channel=4, width=32, enc_blk_nums=[1, 1], middle_blk_num=1,
                                                                        dec_blk_nums=[1, 1], train_size=(1, 4, 32, 32))}}
    net = latent.define_G(opt)
    assert type(net) is latent.CNAFNetLocal and net.kernel_sizes == [(48, 48), (24, 24), (12, 12)]
    opt["network_G"]["which_model"] = "ConditionalNAFNet"
    del opt["network_G"]["setting"]["train_size"]
    assert type(latent.define_G(opt)) is latent.ConditionalNAFNet
    opt["network_G"]["which_model"] = "DiT"
    with pytest.raises(NotImplementedError):
        latent.define_G(opt)


def test_header_and_binding_agree_on_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "irsde_hip.h")).read()
    m = re.search(r"int\s+irsde_nafnet_set_local_pool\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/irsde_hip.h does not declare irsde_nafnet_set_local_pool"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["irsde_engine* e", "int base_h", "int base_w", "int train_h", "int train_w"]
    assert "irsde_nafnet_set_local_pool" in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "image_restoration_sde_amd", "_lib.py")).read()
    assert "lib.irsde_nafnet_set_local_pool.argtypes = [P, c.c_int, c.c_int, c.c_int, c.c_int]" in src
    assert "local_arch.py" in hdr[hdr.index("CNAFNetLocal"):m.start()]         # documented beside the reference lines it replaces
    assert "typedef struct irsde_nafnet_config" in hdr and "local" not in hdr[hdr.index("typedef struct irsde_nafnet_config"):hdr.index("} irsde_nafnet_config;")]
