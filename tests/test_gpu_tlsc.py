"""CNAFNetLocal (TLSC local pooling, csrc/tlsc_pool.hip) on the GPU (run with -m gpu on an MI355X): the engine against the real reference's
goldens (tests/golden/tlsc.npz) and the float64 restatement (tests/tlsc_oracle.py).

Networks: width 32 (the engine's smallest: irsde_create_nafnet refuses widths that are no multiple of 32), enc [1,1], middle 1, dec [1,1],
train sizes (1,3,16,16) -> windows 24 / 12 / 6 and (1,3,20,12) -> 30x18 / 15x9 / 7x4; sca.1.weight x 32 and structured inputs so that a
global-pool engine misses every golden by >= 2e-2 (tests/test_tlsc_host.py::test_goldens_are_pooling_sensitive).

Bars are the sibling rows' of tests/test_gpu_dsde_naf.py: one evaluation vs the reference golden 1e-4, every tap vs the float64 restatement
5e-5, a sampler vs the reference golden 2e-3 (relative to max |ref|); batch vs single images 5e-5; fp16 operand mode vs the fp32 engine 3e-3."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib, latent
from oracle import irsde_oracle as O
import tlsc_oracle as TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NETS = {}
W32 = sorted(t for t in TL.FORWARD if t.startswith("w32"))


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def net(name, flags=0, local=True):
    key = (name, flags, local)
    if key not in _NETS:
        width, train_size = TL.NETS[name]
        kw = dict(img_channel=3, width=width, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
        m = latent.CNAFNetLocal(train_size=train_size, **kw) if local else latent.ConditionalNAFNet(**kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in TL.synth_params(name).items()}, strict=True)
        m.engine_flags = flags
        _NETS[key] = m.to(DEV).eval()
    return _NETS[key]


def dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 18)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine(torch.device(DEV)).h, B, H, W, buf, len(buf)))
    return buf.value.decode()


@pytest.mark.parametrize("tag", W32)
def test_forward_vs_reference_golden(golden, tag):
    g = golden.tlsc
    name, B, H, W, ts, stride = TL.FORWARD[tag]
    m = net(name)
    cond, xt = dev(*TL.inputs(B, H, W))
    for t in ts:
        ref = g[tag + ("/t%d" % t if stride == 1 else "/t%d_sub%d" % (t, stride))]
        e = relerr(m(xt, cond, int(t)).cpu().numpy()[..., ::stride, ::stride], ref)
        print("%s t=%d: %.3g" % (tag, t, e))
        assert e < 1e-4, (tag, int(t), e)


@pytest.mark.parametrize("name,H,W", [("w32_t16", 40, 56), ("w32_t16", 37, 50), ("w32_t16", 20, 56), ("w32_t16", 96, 128), ("w32_t20x12", 37, 50)])
def test_taps_vs_restatement(name, H, W):
    """Every tap and the output against the float64 restatement at 5e-5; 96 x 128 is the drift check of the window sums (48 x 104 windows of a
    96 x 128 map at level 0: a prefix-sum difference in fp32 would carry the error of 12 288 terms, a segment of the running sum carries 7 updates)."""
    m = net(name, flags=_lib.FLAG_KEEP_ACTIVATIONS)
    cond_h, xt_h = TL.inputs(1, H, W)
    taps = {}
    ref = TL.forward(TL.synth_params(name), xt_h, cond_h, 7, TL.NETS[name][1], taps=taps)
    cond, xt = dev(cond_h, xt_h)
    y = m(xt, cond, 7).cpu().numpy()
    errs = {}
    for k, want in taps.items():
        got = m.debug_tap(k).numpy()
        assert got.shape == want.shape, k
        errs[k] = relerr(got, want)
    errs["out"] = relerr(y, ref)
    print("%s %dx%d taps: %s" % (name, H, W, {k: "%.2g" % v for k, v in errs.items()}))
    assert len(taps) == 10 and all(v < 5e-5 for v in errs.values()), errs


def _sample(m, mode, graph, T, cond_h, xt_h, noise=True):
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    sde.set_model(m)
    sde.set_mu(torch.from_numpy(cond_h).to(DEV))
    sde.injected_noise = torch.from_numpy(O.synth_noise(7, T, xt_h.shape)).to(DEV) if noise else None
    sde.use_graph = graph
    sde.seed = 3
    fn = sde.reverse_sde if mode == "sde" else sde.reverse_ode
    return fn(torch.from_numpy(xt_h).to(DEV)).cpu().numpy()


@pytest.mark.parametrize("mode", ["sde", "ode"])
def test_sampler_vs_reference_golden_and_graph_equals_eager(golden, mode):
    name, B, H, W, T = TL.SAMPLER
    cond_h, xt_h = TL.inputs(B, H, W)
    got = _sample(net(name), mode, True, T, cond_h, xt_h)
    e = relerr(got, golden.tlsc["sampler/" + mode])
    print("CNAFNetLocal reverse_%s T=%d: %.3g" % (mode, T, e))
    assert e < 2e-3, (mode, e)
    assert np.array_equal(_sample(net(name), mode, False, T, cond_h, xt_h), got)   # graph replay == eager launches, bit for bit


def test_covered_shape_is_the_plain_network_bit_for_bit():
    """16 x 16 with train 16: every window covers its map -> the plain latent network's plan, row for row, and its bits."""
    loc, plain = net("w32_t16"), net("w32_t16", local=False)
    assert describe(loc, 1, 16, 16).splitlines() == describe(plain, 1, 16, 16).splitlines()
    assert "tlsc" not in describe(loc, 1, 16, 16)
    cond, xt = dev(*TL.inputs(1, 16, 16))
    assert torch.equal(loc(xt, cond, 7), plain(xt, cond, 7))
    # ... and a larger shape on the plain network is unchanged by this engine's existence, while the local one differs there
    cond, xt = dev(*TL.inputs(1, 40, 56))
    assert relerr(loc(xt, cond, 7).cpu().numpy(), plain(xt, cond, 7).cpu().numpy()) > 1e-2


def test_plan_describe_names_the_windows():
    rows = describe(net("w32_t16"), 1, 40, 56).splitlines()
    for win, n in (("tlsc 24x24", 2), ("tlsc 12x12", 2), ("tlsc 6x6", 1)):      # encoder + decoder per level, one middle block
        for part in (" pool ", " sca.1 ", " scale "):
            assert sum(r.startswith(win + part) for r in rows) == n, (win, part, rows)
    assert not any("SCA scale" in r for r in rows)
    rows = describe(net("w32_t16"), 1, 20, 56).splitlines()                      # level 0: 24 >= 20 rows covered, 24 < 56 columns local
    assert sum(r.startswith("tlsc 20x24 pool ") and "-> 1x33" in r for r in rows) == 2, rows
    assert sum(r.startswith("tlsc 10x12 pool ") for r in rows) == 2 and sum(r.startswith("tlsc 5x6 pool ") for r in rows) == 1, rows
    rows = describe(net("w32_t20x12"), 1, 37, 50).splitlines()                   # pads to 40 x 52: maps 40x52 / 20x26 / 10x13
    assert sum(r.startswith("tlsc 30x18 pool ") and "-> 11x35" in r for r in rows) == 2, rows
    assert sum(r.startswith("tlsc 15x9 pool ") for r in rows) == 2 and sum(r.startswith("tlsc 7x4 pool ") for r in rows) == 1, rows


def test_fp16_chain_only_where_the_window_covers():
    """A local block is never part of a NAFBlock chain; covered blocks keep the plan's path, the fp16 chain included (width 64, enc [1,1,1,3]:
    512 channels on the 8 x 8 map of a 64 x 64 input).  train 44 -> every window covers its map at 64 x 64; train 32 -> none does."""
    kw = dict(img_channel=3, width=64, enc_blk_nums=[1, 1, 1, 3], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
    params = O.naf_synth_params(seed=0, img_channel=3, width=64, enc_blk_nums=(1, 1, 1, 3), middle_blk_num=1, dec_blk_nums=(1, 1, 1, 1))
    desc = {}
    for tag, m in (("plain", latent.ConditionalNAFNet(**kw)), ("t44", latent.CNAFNetLocal(train_size=(1, 3, 44, 44), **kw)),
                   ("t32", latent.CNAFNetLocal(train_size=(1, 3, 32, 32), **kw))):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.engine_flags = _lib.FLAG_FP16
        desc[tag] = describe(m.to(DEV).eval(), 2, 64, 64)
    assert desc["plain"].count("naf_chain(fp16)") >= 1
    assert desc["t44"] == desc["plain"]
    assert desc["t32"].count("naf_chain(fp16)") == 0 and desc["t32"].count("window means") == 11
    assert "tlsc 6x6 pool B=2 c=512 hw=8x8" in desc["t32"] and "tlsc 3x3 pool B=2 c=1024 hw=4x4" in desc["t32"]


def test_batch_of_three_equals_single_images():
    m = net("w32_t16")
    cond, xt = dev(*TL.inputs(3, 40, 56))
    yb = m(xt, cond, 7).cpu().numpy()
    scale = np.abs(yb).max()
    worst = max(float(np.abs(m(xt[b:b + 1], cond[b:b + 1], 7).cpu().numpy() - yb[b:b + 1]).max() / scale) for b in range(3))
    print("CNAFNetLocal B=3 vs 3 x B=1 at 40x56: %.3g" % worst)
    assert worst < 5e-5
    assert relerr(yb[0], yb[2]) > 1e-2


def test_graph_replay_equals_eager_with_device_noise():
    """The production sampler path (Philox noise, captured step graph) against eager launches on a shape that is local on both axes."""
    cond_h, xt_h = TL.inputs(2, 40, 56)
    m = net("w32_t20x12")
    a = _sample(m, "sde", True, 5, cond_h, xt_h, noise=False)
    assert np.isfinite(a).all() and np.array_equal(a, _sample(m, "sde", False, 5, cond_h, xt_h, noise=False))


@pytest.mark.parametrize("name,H,W", [("w32_t16", 40, 56), ("w32_t20x12", 37, 50), ("w32_t16", 96, 128)])
def test_fp16_mode_vs_fp32_engine(name, H, W):
    """IRSDE_FLAG_FP16: pool arithmetic fp32, sca.1 on the compact map with the mode's fp16 operands."""
    m16, m32 = net(name, flags=_lib.FLAG_FP16), net(name)
    assert describe(m16, 1, H, W).count(" sca.1 conv(fp16)") == 5 and describe(m32, 1, H, W).count(" sca.1 conv ") == 5
    cond, xt = dev(*TL.inputs(1, H, W))
    e = relerr(m16(xt, cond, 7).cpu().numpy(), m32(xt, cond, 7).cpu().numpy())
    print("CNAFNetLocal fp16 forward vs fp32 %s %dx%d: %.3g" % (name, H, W, e))
    assert 0 < e < 3e-3
    if W == 50:
        cond_h, xt_h = TL.inputs(1, H, W)
        es = relerr(_sample(m16, "ode", True, 20, cond_h, xt_h), _sample(m32, "ode", True, 20, cond_h, xt_h))
        print("CNAFNetLocal fp16 reverse_ode T=20 vs fp32: %.3g" % es)
        assert 0 < es < 3e-3


def test_refused_combinations():
    L = _lib.lib()

    def naf(flags):
        cfg = _lib.NafConfig()
        cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
        for i in range(2):
            cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 1
        cfg.device, cfg.flags = 0, flags
        h = ctypes.c_void_p()
        _lib.check(L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h)))
        return h

    SKIP = _lib.FLAG_NAF_INTRO_SKIP
    for flags in (0, _lib.FLAG_NAF_UNCOND, _lib.FLAG_NAF_STEREO, SKIP | _lib.FLAG_NAF_LENS, SKIP | _lib.FLAG_BF16, SKIP | _lib.FLAG_SPLIT_BF16X2,
                  SKIP | _lib.FLAG_SPLIT_F16X2, SKIP | _lib.FLAG_NAIVE_CONV):
        h = naf(flags)
        assert L.irsde_nafnet_set_local_pool(h, 24, 24, 16, 16) == -1, flags
        assert b"set_local_pool" in L.irsde_last_error()
        L.irsde_destroy(h)
    for flags in (SKIP, SKIP | _lib.FLAG_FP16, SKIP | _lib.FLAG_KEEP_ACTIVATIONS | _lib.FLAG_NO_NAF_CHAIN):
        h = naf(flags)
        assert L.irsde_nafnet_set_local_pool(h, 24, 24, 16, 16) == 0, flags
        for bad in ((0, 24, 16, 16), (24, 24, 0, 16), (24, -1, 16, 16)):
            assert L.irsde_nafnet_set_local_pool(h, *bad) == -1
        L.irsde_destroy(h)
    assert L.irsde_nafnet_set_local_pool(None, 24, 24, 16, 16) == -1
    u = P.ConditionalUNet(3, 3, 32, 2).to(DEV)
    assert L.irsde_nafnet_set_local_pool(u.engine(torch.device(DEV)).h, 24, 24, 16, 16) == -1
    m = latent.CNAFNetLocal(img_channel=3, width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1], train_size=(1, 3, 16, 16)).to(DEV)
    m.set_compute_dtype("bf16")
    with pytest.raises(_lib.IrsdeError, match="set_local_pool"):
        m.engine(torch.device(DEV))


def test_set_local_pool_drops_cached_plans():
    """The per-block choice is baked into a plan: changing the window after a forward rebuilds it."""
    m = latent.CNAFNetLocal(img_channel=3, width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1], train_size=(1, 3, 16, 16))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in TL.synth_params("w32_t16").items()}, strict=True)
    m = m.to(DEV).eval()
    cond, xt = dev(*TL.inputs(1, 37, 50))
    a = m(xt, cond, 7)
    _lib.check(_lib.lib().irsde_nafnet_set_local_pool(m.engine().h, 30, 18, 20, 12))
    b = m(xt, cond, 7)
    assert torch.equal(b, net("w32_t20x12")(xt, cond, 7)) and not torch.equal(a, b)
    assert "tlsc 30x18" in describe(m, 1, 37, 50)
