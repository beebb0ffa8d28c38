"""stereo-sr ConditionalNAFNet on the GPU (run with -m gpu on an MI355X): the SCAM kernels (csrc/scam.hip) against the float64
restatement (tests/stereo_oracle.py), the network and its samplers against the reference golden (tests/golden/stereo.npz), the fp16
mode, the refusals and the stereo-sr model wrapper.

Tolerances: one SCAM 1e-5 of max |SCAM increment| (the attention part, not the residual that dominates the output); one network
evaluation 1e-4 of max |out| (the NAFNet bar of tests/test_gpu_parity.py); samplers 2e-3; fp16 vs fp32 engine 3e-3."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import stereo_oracle as SO
from oracle.gen_golden import sub3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
REFUSION = dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def oracle_cfg(cfg):
    return dict(enc_blk_nums=tuple(cfg["enc_blk_nums"]), middle_blk_num=cfg["middle_blk_num"], dec_blk_nums=tuple(cfg["dec_blk_nums"]))


_NETS = {}


def stereo_model(cfg_name, flags=0, dtype="fp32"):
    key = (cfg_name, flags, dtype)
    if key not in _NETS:
        cfg = SMALL if cfg_name == "small" else REFUSION
        params = SO.stereo_synth_params(seed=0, img_channel=3, width=cfg["width"], **oracle_cfg(cfg))
        m = P.stereo_sr.ConditionalNAFNet(img_channel=3, **cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.engine_flags = flags
        m.set_compute_dtype(dtype)
        _NETS[key] = (m.to(DEV).eval(), params)
    return _NETS[key]


def stereo_inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


# ---------------------------------------------------------------------------------------------
# one SCAM through irsde_debug_scam
# ---------------------------------------------------------------------------------------------
def scam_weights(c, seed, tie_proj1=False):
    rs = np.random.RandomState(seed)
    p = {}
    pre = "f."
    for n in ("norm_l.g", "norm_r.g"):
        p[pre + n] = rs.uniform(0.5, 1.5, (1, c, 1, 1))
    for n in ("l_proj1", "r_proj1", "l_proj2", "r_proj2"):
        gain = SO.SCAM_PROJ1_GAIN if n.endswith("1") else 1.0
        p[pre + n + ".weight"] = rs.uniform(-gain / np.sqrt(c), gain / np.sqrt(c), (c, c, 1, 1))
        p[pre + n + ".bias"] = rs.uniform(-1 / np.sqrt(c), 1 / np.sqrt(c), (c,))
    p[pre + "beta"] = rs.uniform(-0.5, 0.5, (1, c, 1, 1))
    p[pre + "gamma"] = rs.uniform(-0.5, 0.5, (1, c, 1, 1))
    if tie_proj1:   # identical left / right query projections: a copied image column gives a known score maximum
        p[pre + "r_proj1.weight"] = p[pre + "l_proj1.weight"].copy()
        p[pre + "r_proj1.bias"] = p[pre + "l_proj1.bias"].copy()
        p[pre + "norm_r.g"] = p[pre + "norm_l.g"].copy()
    return {k: v.astype(np.float32) for k, v in p.items()}


def debug_scam(x_nchw, p):
    """x [2B, c, H, W] -> the GPU SCAM output [2B, c, H, W]."""
    B2, c, H, W = x_nchw.shape
    x = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).to(DEV)
    out = torch.empty_like(x)
    host = [np.ascontiguousarray(p["f." + n].reshape(-1), dtype=np.float32) for n in
            ("norm_l.g", "norm_r.g", "l_proj1.weight", "l_proj1.bias", "r_proj1.weight", "r_proj1.bias", "l_proj2.weight", "l_proj2.bias",
             "r_proj2.weight", "r_proj2.bias", "beta", "gamma")]
    ptrs = [h.ctypes.data_as(ctypes.c_void_p) for h in host]
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().irsde_debug_scam(ctypes.c_void_p(x.data_ptr()), B2 // 2, H, W, c, *ptrs, ctypes.c_void_p(out.data_ptr()),
                                               _lib.stream_ptr()))
    return out.cpu().numpy().transpose(0, 3, 1, 2)


def scam_err(x, p, got):
    want = SO.scam({k: v.astype(np.float64) for k, v in p.items()}, "f.", x.astype(np.float64))
    return relerr(got - x, want - x)


# (pairs, H, W, c): W' = W // 4 in {1, 3, 7, 16, 28, 130, 256, 512}; H / W mostly not multiples of 4
SCAM_SHAPES = [(1, 5, 6, 64), (3, 9, 14, 256), (1, 10, 30, 1024), (3, 13, 66, 64), (1, 22, 113, 256), (1, 9, 522, 64), (1, 8, 1027, 64),
               (3, 7, 1026, 256), (2, 8, 64, 32), (1, 4, 2050, 64), (3, 6, 30, 1024)]


@pytest.mark.parametrize("B,H,W,c", SCAM_SHAPES)
def test_debug_scam_vs_oracle(B, H, W, c):
    x = np.random.RandomState(B * 1000 + W).standard_normal((2 * B, c, H, W)).astype(np.float32)
    p = scam_weights(c, seed=W + c)
    got = debug_scam(x, p)
    e = scam_err(x, p, got)
    print("SCAM B=%d %dx%d c=%d (W'=%d): %.3g" % (B, H, W, c, W // 4, e))
    assert e < 1e-5


def test_debug_scam_views_not_swapped():
    """L != R and beta != gamma: the GPU result must match the oracle and be far from the one with the two directions exchanged."""
    B, H, W, c = 2, 12, 40, 64
    rs = np.random.RandomState(5)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[B:] = 2.0 * rs.standard_normal((B, c, H, W)) + 0.5
    p = scam_weights(c, seed=6)
    got = debug_scam(x, p)
    assert scam_err(x, p, got) < 1e-5
    sw = dict(p)
    sw["f.beta"], sw["f.gamma"] = p["f.gamma"], p["f.beta"]
    assert scam_err(x, sw, got) > 0.05


@pytest.mark.parametrize("W,j_src", [(522, 5), (1027, 200)])
def test_debug_scam_spike_in_last_tile(W, j_src):
    """A score spike whose row / column maximum lies in the LAST 16-wide tile of S: the last downsampled column of the left view is a
    (scaled) copy of column j_src of the right view and the query projections are tied, so S[W' - 1, j_src] = |Q|^2 / sqrt(c) dominates
    column j_src of S (the left-to-right softmax) and row W' - 1 (right-to-left)."""
    B, H, c = 1, 8, 64
    Ws = W // 4
    rs = np.random.RandomState(W)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[:B, :, :, 4 * (Ws - 1):4 * Ws] = 3.0 * x[B:, :, :, 4 * j_src:4 * j_src + 4]
    p = scam_weights(c, seed=11, tie_proj1=True)
    got = debug_scam(x, p)
    e = scam_err(x, p, got)
    print("SCAM spike W'=%d j=%d: %.3g" % (Ws, j_src, e))
    assert e < 1e-5
    # the spike is really the maximum of its column
    d = {k: v.astype(np.float64) for k, v in p.items()}
    xl, xr = SO.bicubic_quarter(x[:B].astype(np.float64)), SO.bicubic_quarter(x[B:].astype(np.float64))
    ql = O.conv2d(O.layer_norm_c(xl, d["f.norm_l.g"]), d["f.l_proj1.weight"], d["f.l_proj1.bias"])[0, :, 0]
    qr = O.conv2d(O.layer_norm_c(xr, d["f.norm_r.g"]), d["f.r_proj1.weight"], d["f.r_proj1.bias"])[0, :, 0]
    S = ql.T @ qr
    assert int(np.argmax(S[:, j_src])) == Ws - 1


# ---------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------
def forward(m, xT, lq, t):
    tt = t if isinstance(t, int) else torch.tensor(t)
    return m(torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV), tt).cpu().numpy()


def test_forward_small_vs_reference_golden(golden):
    g = golden.stereo
    m, _ = stereo_model("small")
    lq, xT = stereo_inputs(2, 32, 48)
    for key, t in (("t3", 3), ("t77", 77), ("t5_60", [5, 60])):
        e = relerr(forward(m, xT, lq, t), g["small_2x32x48/" + key])
        print("stereo small %s: %.3g" % (key, e))
        assert e < 1e-4, (key, e)


def test_forward_refusion_vs_reference_golden(golden):
    g = golden.stereo
    m, _ = stereo_model("refusion")
    lq, xT = stereo_inputs(1, 64, 64)
    e = relerr(forward(m, xT, lq, 60), g["refusion_1x64x64/t60"])
    print("stereo refusion 1x6x64x64: %.3g" % e)
    assert e < 1e-4
    lq, xT = stereo_inputs(1, 80, 112)
    e = relerr(sub3(forward(m, xT, lq, 37)), g["refusion_1x80x112/t37_sub3"])
    print("stereo refusion 1x6x80x112: %.3g" % e)
    assert e < 1e-4


def test_block_taps_vs_oracle():
    """Every block output and every SCAM input (`<path>.fusion.in`) under IRSDE_FLAG_KEEP_ACTIVATIONS against the float64 restatement."""
    m, params = stereo_model("small", flags=_lib.FLAG_KEEP_ACTIVATIONS)
    lq, xT = stereo_inputs(2, 32, 48)
    taps = {}
    ref = SO.stereo_forward(params, xT, lq, [9, 41], taps=taps, **oracle_cfg(SMALL))
    y = forward(m, xT, lq, [9, 41])
    assert relerr(y, ref) < 1e-4
    assert "encoders.0.0.fusion.in" in taps and len(taps) == 10
    bad = {}
    for name, want in taps.items():
        got = m.debug_tap(name).numpy()
        assert got.shape == want.shape, name
        e = relerr(got, want)
        if not e < 1e-4:
            bad[name] = e
    assert not bad, bad


def _sample(m, sde, mode, lq, xT, z, graph):
    sde.set_model(m)
    sde.set_mu(torch.from_numpy(lq).to(DEV))
    sde.injected_noise = None if z is None else torch.from_numpy(z).to(DEV)
    sde.use_graph = graph
    try:
        fn = sde.reverse_sde if mode == "sde" else sde.reverse_ode
        return fn(torch.from_numpy(xT).to(DEV)).cpu().numpy()
    finally:
        sde.use_graph = True


def test_samplers_vs_reference_golden(golden):
    g = golden.stereo
    m, _ = stereo_model("small")
    B, H, W, T = 2, 32, 48, 20
    lq, xT = stereo_inputs(B, H, W)
    z = O.synth_noise(7, T, (B, 6, H, W))
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    for mode in ("sde", "ode"):
        got = _sample(m, sde, mode, lq, xT, z, True)
        e = relerr(got, g["small_sampler_2x32x48_T20/" + mode])
        print("stereo sampler %s: %.3g" % (mode, e))
        assert e < 2e-3, (mode, e)
        assert np.array_equal(got, _sample(m, sde, mode, lq, xT, z, False))


def test_fp16_engine_vs_fp32_and_no_chain():
    m32, _ = stereo_model("refusion")
    m16, _ = stereo_model("refusion", dtype="fp16")
    lq, xT = stereo_inputs(1, 64, 64)
    e = relerr(forward(m16, xT, lq, 60), forward(m32, xT, lq, 60))
    print("stereo fp16 vs fp32: %.3g" % e)
    assert e < 3e-3
    buf = ctypes.create_string_buffer(1 << 20)
    _lib.check(_lib.lib().irsde_plan_describe(m16.engine().h, 2, 64, 64, buf, len(buf)))
    desc = buf.value.decode()
    assert "naf_chain" not in desc
    assert "scam_core" in desc and "scam_proj(l) conv(fp16)" in desc
    # forced concurrent sub-batches: the stereo engine never splits (SCAM couples a pair's two views) -> bit-identical
    L = _lib.lib()
    B, T = 4, 4
    lq, xT = stereo_inputs(B, 64, 64)
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    sde.seed = 3
    outs = []
    try:
        for n in (1, 2):
            L.irsde_debug_force_subbatches(n)
            outs.append(_sample(m16, sde, "sde", lq, xT, None, True))
    finally:
        L.irsde_debug_force_subbatches(0)
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])


def test_refusals():
    m, _ = stereo_model("refusion")
    lq, xT = stereo_inputs(1, 32, 32)   # padded 32 x 32 -> 2 x 2 at the deepest level: the reference's interpolate fails there
    with pytest.raises(_lib.IrsdeError, match="at least 4 rows"):
        forward(m, xT, lq, 10)
    with pytest.raises(_lib.IrsdeError):
        m(torch.zeros(1, 3, 64, 64, device=DEV), torch.zeros(1, 3, 64, 64, device=DEV), 1)
    cfg = _lib.Config(3, 3, 32, 2, 0, _lib.FLAG_NAF_STEREO)
    h = ctypes.c_void_p()
    assert _lib.lib().irsde_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    lens = P.stereo_sr.ConditionalNAFNet(img_channel=3, **SMALL).to(DEV)
    lens.engine_flags = _lib.FLAG_NAF_LENS
    with pytest.raises(_lib.IrsdeError, match="NAF_STEREO"):
        lens.engine()


def test_stereo_model_wrapper_drop_in():
    """create_model(opt, "stereo-sr") with the reference's feed_data / test / get_current_visuals (stereo-sr/test.py:107-115)."""
    _, params = stereo_model("refusion")
    opt = {"model": "denoising", "network_G": {"which_model_G": "ConditionalNAFNet", "setting": dict(REFUSION)}, "path": {}}
    model = P.create_model(opt, "stereo-sr")
    model.model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    T = 100
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    sde.set_model(model.model)
    lq, xT = stereo_inputs(1, 64, 64)
    model.feed_data(torch.from_numpy(xT), torch.from_numpy(lq), torch.from_numpy(lq))
    model.test(sde)
    out = model.get_current_visuals()["Output"]
    assert tuple(out.shape) == (6, 64, 64)
    sde.set_mu(torch.from_numpy(lq).to(DEV))
    want = sde.reverse_sde(torch.from_numpy(xT).to(DEV)).cpu()
    assert torch.equal(out, want[0])
    assert np.isfinite(out.numpy()).all()
    L, R = out.chunk(2, dim=0)
    assert not torch.equal(L, R)
    model.test(sde, perform_ode=True)
    assert torch.equal(model.get_current_visuals()["Output"], sde.reverse_ode(torch.from_numpy(xT).to(DEV)).cpu()[0])
