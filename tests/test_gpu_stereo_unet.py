"""stereo-sr ConditionalUNet on the GPU (run with -m gpu on an MI355X): the full-resolution SCAM kernels (csrc/scam.hip, *_full) against
the float64 restatement (tests/stereo_unet_oracle.py), the network and its samplers against the reference golden
(tests/golden/stereo_unet.npz), graph replay, batch independence and the stereo-sr model wrapper.

Tolerances (those of tests/test_gpu_stereo.py): one SCAM 1e-5 of max |SCAM increment| (the attention part, not the residual that dominates
the output); one network evaluation 1e-4 of max |out|; samplers 2e-3."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
from oracle.gen_golden import sub3
import stereo_unet_oracle as SU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = {"small": dict(nf=32, depth=2), "full": dict(nf=64, depth=4)}
MAX_W = 1024   # kScamFullMaxW (csrc/common.h), stated in include/irsde_hip.h
# Kernel-level SCAM weights: the *_proj1 gain of tests/test_gpu_stereo.py (SO.SCAM_PROJ1_GAIN = 4), whose 1e-5 bar these tests take over.  The bar
# presupposes that gain: score errors grow with its square, and at the network fixture's gain of 8 the fp32 PyTorch reference module itself is
# 1.45e-5 of the increment away from float64 at (1, 2, 509, 128) (7e-6 at c = 1024); at 4 it stays <= 2.6e-6 on every shape below (CPU, measured).
HOOK_PROJ1_GAIN = 4.0


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


_NETS = {}


def unet_model(name, flags=0):
    key = (name, flags)
    if key not in _NETS:
        cfg = CFG[name]
        params = SU.stereo_unet_synth_params(seed=0, **cfg)
        m = P.stereo_sr.ConditionalUNet(3, 3, cfg["nf"], depth=cfg["depth"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.engine_flags = flags
        _NETS[key] = (m.to(DEV).eval(), params)
    return _NETS[key]


def stereo_inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


# ---------------------------------------------------------------------------------------------
# one SCAM through irsde_debug_scam_full
# ---------------------------------------------------------------------------------------------
def scam_weights(c, seed, tie_proj1=False):
    rs = np.random.RandomState(seed)
    p = {}
    pre = "f."
    for n in ("norm_l.g", "norm_r.g"):
        p[pre + n] = rs.uniform(0.5, 1.5, (1, c, 1, 1))
    for n in ("l_proj1", "r_proj1", "l_proj2", "r_proj2"):
        gain = HOOK_PROJ1_GAIN if n.endswith("1") else 1.0
        p[pre + n + ".weight"] = rs.uniform(-gain / np.sqrt(c), gain / np.sqrt(c), (c, c, 1, 1))
        p[pre + n + ".bias"] = rs.uniform(-1 / np.sqrt(c), 1 / np.sqrt(c), (c,))
    p[pre + "beta"] = rs.uniform(-0.5, 0.5, (1, c, 1, 1))
    p[pre + "gamma"] = rs.uniform(-0.5, 0.5, (1, c, 1, 1))
    if tie_proj1:   # identical left / right query projections: a copied image column gives a known score maximum
        p[pre + "r_proj1.weight"] = p[pre + "l_proj1.weight"].copy()
        p[pre + "r_proj1.bias"] = p[pre + "l_proj1.bias"].copy()
        p[pre + "norm_r.g"] = p[pre + "norm_l.g"].copy()
    return {k: v.astype(np.float32) for k, v in p.items()}


def debug_scam_full(x_nchw, p):
    """x [2B, c, H, W] -> the GPU SCAM output [2B, c, H, W]."""
    B2, c, H, W = x_nchw.shape
    x = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).to(DEV)
    out = torch.empty_like(x)
    host = [np.ascontiguousarray(p["f." + n].reshape(-1), dtype=np.float32) for n in
            ("norm_l.g", "norm_r.g", "l_proj1.weight", "l_proj1.bias", "r_proj1.weight", "r_proj1.bias", "l_proj2.weight", "l_proj2.bias",
             "r_proj2.weight", "r_proj2.bias", "beta", "gamma")]
    ptrs = [h.ctypes.data_as(ctypes.c_void_p) for h in host]
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().irsde_debug_scam_full(ctypes.c_void_p(x.data_ptr()), B2 // 2, H, W, c, *ptrs, ctypes.c_void_p(out.data_ptr()),
                                                    _lib.stream_ptr()))
    return out.cpu().numpy().transpose(0, 3, 1, 2)


def scam_err(x, p, got):
    want = SU.scam_full(p, "f.", x)
    return relerr(got - x, want - x)


# (pairs, H, W, c): W = 1, ragged tiles, one / several column tiles per wave (the 4 / 8-tile kernel instances), c up to 1024
SCAM_SHAPES = [(1, 3, 1, 32), (2, 5, 10, 64), (1, 4, 16, 256), (3, 3, 40, 1024), (1, 2, 130, 64), (1, 2, 512, 32), (1, 2, 509, 128)]


@pytest.mark.parametrize("B,H,W,c", SCAM_SHAPES)
def test_debug_scam_full_vs_oracle(B, H, W, c):
    x = np.random.RandomState(B * 1000 + W).standard_normal((2 * B, c, H, W)).astype(np.float32)
    p = scam_weights(c, seed=W + c)
    got = debug_scam_full(x, p)
    e = scam_err(x, p, got)
    print("SCAM(full) B=%d %dx%d c=%d: %.3g" % (B, H, W, c, e))
    assert e < 1e-5


def test_debug_scam_full_width_limit():
    """The widest row runs (the 16-tile kernel instance, 66 KB of LDS); one pixel more raises instead of mis-computing."""
    c = 32
    p = scam_weights(c, seed=3)
    x = np.random.RandomState(4).standard_normal((2, c, 1, MAX_W)).astype(np.float32)
    e = scam_err(x, p, debug_scam_full(x, p))
    print("SCAM(full) W=%d: %.3g" % (MAX_W, e))
    assert e < 1e-5
    x = np.zeros((2, c, 1, MAX_W + 1), np.float32)
    with pytest.raises(_lib.IrsdeError, match="wider than 1024"):
        debug_scam_full(x, p)


def test_debug_scam_full_views_not_swapped():
    """L != R and beta != gamma: the GPU result must match the oracle and be far from the one with the two directions exchanged."""
    B, H, W, c = 2, 3, 40, 64
    rs = np.random.RandomState(5)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[B:] = 2.0 * rs.standard_normal((B, c, H, W)) + 0.5
    p = scam_weights(c, seed=6)
    got = debug_scam_full(x, p)
    assert scam_err(x, p, got) < 1e-5
    sw = dict(p)
    sw["f.beta"], sw["f.gamma"] = p["f.gamma"], p["f.beta"]
    assert scam_err(x, sw, got) > 0.05


def test_debug_scam_full_spike_in_last_tile():
    """W = 509: the softmax maximum lies in the ragged final 16-wide tile in BOTH directions.  The query projections are tied; the last column
    of the left view is a scaled copy of right column 200 (S[508, 200] tops column 200: the left-to-right softmax of right pixel 200 peaks in
    the last tile of its strip) and the last column of the right view a scaled copy of left column 37 (S[37, 508] tops row 37: right-to-left)."""
    B, H, W, c = 1, 2, 509, 64
    rs = np.random.RandomState(W)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[:B, :, :, W - 1] = 3.0 * x[B:, :, :, 200]
    x[B:, :, :, W - 1] = 3.0 * x[:B, :, :, 37]
    p = scam_weights(c, seed=11, tie_proj1=True)
    got = debug_scam_full(x, p)
    e = scam_err(x, p, got)
    print("SCAM(full) spike W=%d: %.3g" % (W, e))
    assert e < 1e-5
    d = {k: v.astype(np.float64) for k, v in p.items()}
    xl, xr = x[:B].astype(np.float64), x[B:].astype(np.float64)
    ql = O.conv2d(O.layer_norm_c(xl, d["f.norm_l.g"]), d["f.l_proj1.weight"], d["f.l_proj1.bias"])[0, :, 0]
    qr = O.conv2d(O.layer_norm_c(xr, d["f.norm_r.g"]), d["f.r_proj1.weight"], d["f.r_proj1.bias"])[0, :, 0]
    S = ql.T @ qr
    assert int(np.argmax(S[:, 200])) == W - 1 and int(np.argmax(S[37, :])) == W - 1


# ---------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------
def forward(m, xT, lq, t):
    tt = t if isinstance(t, int) else torch.tensor(t)
    return m(torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV), tt).cpu().numpy()


def test_forward_small_vs_reference_golden(golden):
    g = golden.stereo_unet
    m, _ = unet_model("small")
    lq, xT = stereo_inputs(2, 22, 38)
    for key, t in (("t3", 3), ("t77", 77), ("t5_60", [5, 60]), ("t77", [77, 77])):
        e = relerr(forward(m, xT, lq, t), g["small_2x22x38/" + key])
        print("stereo UNet small %s (%r): %.3g" % (key, t, e))
        assert e < 1e-4, (key, e)


def test_forward_full_vs_reference_golden(golden):
    g = golden.stereo_unet
    m, _ = unet_model("full")
    lq, xT = stereo_inputs(1, 32, 48)
    e = relerr(sub3(forward(m, xT, lq, 60)), g["full_1x32x48/t60_sub3"])
    print("stereo UNet nf64 depth4 1x6x32x48: %.3g" % e)
    assert e < 1e-4


def test_scam_taps_vs_oracle_and_plan_rows():
    """Every SCAM input and output under IRSDE_FLAG_KEEP_ACTIVATIONS against the float64 restatement; irsde_plan_describe lists the rows."""
    m, params = unet_model("small", flags=_lib.FLAG_KEEP_ACTIVATIONS)
    lq, xT = stereo_inputs(2, 22, 38)
    taps = {}
    ref = SU.stereo_unet_forward(params, xT, lq, [9, 41], depth=2, taps=taps)
    assert relerr(forward(m, xT, lq, [9, 41]), ref) < 1e-4
    names = {"downs.0.3": "downs.0.2", "downs.1.3": "downs.1.2", "mid_fusion": "mid_attn", "ups.0.3": "ups.0.2", "ups.1.3": "ups.1.2"}
    bad = {}
    for out_name, in_name in names.items():
        for tap, want in ((in_name, taps[out_name + ".in"]), (out_name, taps[out_name])):
            got = m.debug_tap(tap).numpy()
            assert got.shape == want.shape, tap
            e = relerr(got, want)
            if not e < 1e-4:
                bad[tap] = e
    assert not bad, bad
    buf = ctypes.create_string_buffer(1 << 20)
    _lib.check(_lib.lib().irsde_plan_describe(unet_model("small")[0].engine().h, 2, 22, 38, buf, len(buf)))
    desc = buf.value.decode()
    assert desc.count("scam_full_core") == 5 and desc.count("scam_full_proj(l)") == 5 and "stereo_unet_pack_pred" in desc
    assert "c=128 hw=12x20" in desc and "c=64 hw=24x40" in desc and "c=32 hw=24x40" in desc and "copy(kept" not in desc


def _sample(m, sde, mode, lq, xT, z, graph):
    sde.set_model(m)
    sde.set_mu(torch.from_numpy(lq).to(DEV))
    sde.injected_noise = None if z is None else torch.from_numpy(z).to(DEV)
    sde.use_graph = graph
    try:
        fn = {"sde": sde.reverse_sde, "ode": sde.reverse_ode, "posterior": sde.reverse_posterior}[mode]
        return fn(torch.from_numpy(xT).to(DEV)).cpu().numpy()
    finally:
        sde.use_graph = True


def test_samplers_vs_reference_golden_and_graph_equals_eager(golden):
    g = golden.stereo_unet
    m, _ = unet_model("small")
    B, H, W, T = 2, 22, 38, 20
    lq, xT = stereo_inputs(B, H, W)
    z = O.synth_noise(7, T, (B, 6, H, W))
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    for mode in ("sde", "ode"):
        got = _sample(m, sde, mode, lq, xT, z, True)
        e = relerr(got, g["small_sampler_2x22x38_T20/" + mode])
        print("stereo UNet sampler %s: %.3g" % (mode, e))
        assert e < 2e-3, (mode, e)
        assert np.array_equal(got, _sample(m, sde, mode, lq, xT, z, False)), mode
    got = _sample(m, sde, "posterior", lq, xT, z, True)
    assert np.isfinite(got).all() and np.array_equal(got, _sample(m, sde, "posterior", lq, xT, z, False))


def test_two_pair_batch_equals_its_single_pairs():
    """Bit for bit: network evaluation and the sampler with the device (keyed Philox) noise, which is drawn per image of the pair tensor."""
    m, _ = unet_model("small")
    lq, xT = stereo_inputs(2, 22, 38)
    both = forward(m, xT, lq, 33)
    for b in range(2):
        assert np.array_equal(both[b:b + 1], forward(m, xT[b:b + 1], lq[b:b + 1], 33)), b
    T = 4
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    sde.seed = 3
    full = _sample(m, sde, "sde", lq, xT, None, True)
    assert np.isfinite(full).all() and not np.array_equal(full[0], full[1])
    sde.image_offset = 0
    assert np.array_equal(full[0:1], _sample(m, sde, "sde", lq[0:1], xT[0:1], None, True))
    sde.image_offset = 1
    try:
        assert np.array_equal(full[1:2], _sample(m, sde, "sde", lq[1:2], xT[1:2], None, True))
    finally:
        sde.image_offset = 0


def test_refusals():
    m, _ = unet_model("small")
    with pytest.raises(_lib.IrsdeError):   # 3-channel tensors are not pairs
        m(torch.zeros(1, 3, 24, 24, device=DEV), torch.zeros(1, 3, 24, 24, device=DEV), 1)
    lq, xT = stereo_inputs(1, 4, MAX_W + 4)
    with pytest.raises(_lib.IrsdeError, match="wider than 1024"):
        forward(m, xT, lq, 10)


def test_stereo_model_wrapper_drop_in():
    """create_model(opt, "stereo-sr") with which_model_G ConditionalUNet: feed_data / test / get_current_visuals, perform_ode both ways."""
    _, params = unet_model("small")
    opt = {"model": "denoising", "network_G": {"which_model_G": "ConditionalUNet", "setting": dict(in_nc=3, out_nc=3, nf=32, depth=2)}, "path": {}}
    model = P.create_model(opt, "stereo-sr")
    assert type(model.model) is P.stereo_sr.ConditionalUNet
    model.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    T = 10
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    sde.set_model(model.model)
    lq, xT = stereo_inputs(1, 22, 38)
    model.feed_data(torch.from_numpy(xT), torch.from_numpy(lq), torch.from_numpy(lq))
    model.test(sde)
    out = model.get_current_visuals()["Output"]
    assert tuple(out.shape) == (6, 22, 38)
    sde.set_mu(torch.from_numpy(lq).to(DEV))
    want = sde.reverse_sde(torch.from_numpy(xT).to(DEV)).cpu()
    assert torch.equal(out, want[0])
    assert np.isfinite(out.numpy()).all()
    L, R = out.chunk(2, dim=0)
    assert not torch.equal(L, R)
    model.test(sde, perform_ode=True)
    assert torch.equal(model.get_current_visuals()["Output"], sde.reverse_ode(torch.from_numpy(xT).to(DEV)).cpu()[0])
