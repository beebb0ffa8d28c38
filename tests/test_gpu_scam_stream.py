"""The streaming SCAM core on the GPU (run with -m gpu on an MI355X): csrc/scam_stream.hip through irsde_debug_scam_full_stream / irsde_debug_scam_stream
against the float64 restatements, the stereo networks with every SCAM forced onto it (irsde_debug_force_scam_stream) against the existing reference
goldens, and inputs beyond the strip kernels' width under IRSDE_FLAG_SCAM_STREAM (`set_wide_rows()`) against tests/golden/stereo_wide.npz.

Tolerances (those of tests/test_gpu_stereo_unet.py): one SCAM 1e-5 of max |SCAM increment| at the hook weights (proj1 gain 4); one network evaluation
1e-4 of max |out|; samplers 2e-3.  tests/test_scam_stream_host.py shows on the CPU that the kernel's order in float32 stays within 6.2e-6 of the
increment on every shape below and that a stale maximum / a missing rescale / an unmasked tail / exchanged rows, directions or block boundaries miss the
bar by orders of magnitude."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
from oracle.gen_golden import sub3
import scam_stream_oracle as WS
import stereo_oracle as SO
import stereo_unet_oracle as SU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096          # sentinel floats on either side of the output tensor
SENTINEL = -12345.5
relerr = WS.relerr


# ---------------------------------------------------------------------------------------------
# one SCAM through the streaming hooks
# ---------------------------------------------------------------------------------------------
def _weight_ptrs(p):
    host = [np.ascontiguousarray(p["f." + n].reshape(-1), dtype=np.float32) for n in
            ("norm_l.g", "norm_r.g", "l_proj1.weight", "l_proj1.bias", "r_proj1.weight", "r_proj1.bias", "l_proj2.weight", "l_proj2.bias",
             "r_proj2.weight", "r_proj2.bias", "beta", "gamma")]
    return host, [h.ctypes.data_as(ctypes.c_void_p) for h in host]


def debug_stream(x_nchw, p, block_w, hook="irsde_debug_scam_full_stream", prefill=0.0):
    """x [2B, c, H, W] -> the GPU SCAM output [2B, c, H, W]; the output tensor lies between two sentinel guards, which must come back intact."""
    B2, c, H, W = x_nchw.shape
    x = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).to(DEV)
    n = x.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n].view(x.shape)
    out.fill_(prefill)
    host, ptrs = _weight_ptrs(p)
    with torch.cuda.device(DEV):
        _lib.check(getattr(_lib.lib(), hook)(ctypes.c_void_p(x.data_ptr()), B2 // 2, H, W, c, *ptrs, block_w, ctypes.c_void_p(out.data_ptr()),
                                             _lib.stream_ptr()))
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), "the kernel wrote outside its output tensor"
    return got[GUARD:GUARD + n].reshape(B2, H, W, c).transpose(0, 3, 1, 2)


def debug_scam_full(x_nchw, p):
    """The strip kernel (irsde_debug_scam_full) on the same input."""
    B2, c, H, W = x_nchw.shape
    x = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).to(DEV)
    out = torch.empty_like(x)
    host, ptrs = _weight_ptrs(p)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().irsde_debug_scam_full(ctypes.c_void_p(x.data_ptr()), B2 // 2, H, W, c, *ptrs, ctypes.c_void_p(out.data_ptr()),
                                                    _lib.stream_ptr()))
    return out.cpu().numpy().transpose(0, 3, 1, 2)


@pytest.mark.parametrize("shape", WS.STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_full_vs_oracle(shape):
    x, p, want = WS.case(shape)
    got = debug_stream(x, p, shape[4])
    e = WS.increment_err(x, want, got)
    print("SCAM(full, streaming) %r: %.3g" % (shape, e))
    assert e < 1e-5
    assert np.array_equal(got, debug_stream(x, p, shape[4], prefill=7.25)), "the result depends on what the output held"


def test_stream_full_c2048():
    """c = 2048 (16 channel pairs per wave): the float32 emulation sits at the bar's edge here, so the bar is max(1e-5, 2 x the strip kernel's error)."""
    x, p, want = WS.case(WS.C2048_SHAPE)
    e_strip = WS.increment_err(x, want, debug_scam_full(x, p))
    e = WS.increment_err(x, want, debug_stream(x, p, WS.C2048_SHAPE[4]))
    print("SCAM(full) c=2048: streaming %.3g, strip %.3g" % (e, e_strip))
    assert e < max(1e-5, 2 * e_strip)


def _spike_case(W, left_col, left_src, right_col, right_src):
    """Tied query projections; left column left_col is a scaled copy of right column left_src (S[left_col, left_src] tops column left_src: the
    left-to-right softmax of right pixel left_src peaks at left_col) and right column right_col a scaled copy of left column right_src
    (S[right_src, right_col] tops row right_src: right-to-left)."""
    B, H, c = 1, 2, 64
    rs = np.random.RandomState(W)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[:B, :, :, left_col] = 3.0 * x[B:, :, :, left_src]
    x[B:, :, :, right_col] = 3.0 * x[:B, :, :, right_src]
    p = WS.scam_weights(c, seed=11, tie_proj1=True)
    ql, qr = WS.queries(p, x)
    S = ql[0, 0] @ qr[0, 0].T * c ** -0.5   # the scores of image row 0
    return x, p, S


@pytest.mark.parametrize("W,bw", [(130, 64), (1040, 0)])
def test_stream_spike_in_last_block(W, bw):
    """The row maximum lies in the last (ragged) block in both directions: every earlier block is rescaled when it arrives."""
    x, p, S = _spike_case(W, W - 1, 40, W - 1, 37)
    last = (W - 1) // (bw or WS.MAX_BLOCK_W)
    assert int(np.argmax(S[:, 40])) == W - 1 and int(np.argmax(S[37, :])) == W - 1 and last >= 2
    e = WS.increment_err(x, SU.scam_full(p, "f.", x), debug_stream(x, p, bw))
    print("SCAM(full, streaming) spike in the last block W=%d: %.3g" % (W, e))
    assert e < 1e-5


def test_stream_spike_in_first_block():
    """The maximum arrives first and much smaller logits follow: alpha stays 1, the later blocks add almost nothing."""
    W, bw = 130, 64
    x, p, S = _spike_case(W, 3, 100, 7, 90)
    assert int(np.argmax(S[:, 100])) == 3 and int(np.argmax(S[90, :])) == 7
    assert S[3, 100] - np.delete(S[:, 100], 3).max() > 5 and S[90, 7] - np.delete(S[90, :], 7).max() > 5
    e = WS.increment_err(x, SU.scam_full(p, "f.", x), debug_stream(x, p, bw))
    print("SCAM(full, streaming) spike in the first block: %.3g" % e)
    assert e < 1e-5


def test_stream_views_and_scales_not_exchanged():
    """L != R and beta != gamma: the GPU result must match the oracle and be far from the one with the two directions exchanged."""
    B, H, W, c = 2, 3, 40, 64
    rs = np.random.RandomState(5)
    x = rs.standard_normal((2 * B, c, H, W)).astype(np.float32)
    x[B:] = 2.0 * rs.standard_normal((B, c, H, W)) + 0.5
    p = WS.scam_weights(c, seed=6)
    got = debug_stream(x, p, 16)
    assert WS.increment_err(x, SU.scam_full(p, "f.", x), got) < 1e-5
    sw = dict(p)
    sw["f.beta"], sw["f.gamma"] = p["f.gamma"], p["f.beta"]
    assert WS.increment_err(x, SU.scam_full(sw, "f.", x), got) > 0.05


# (pairs, H, W, c, block_w): two shapes of tests/test_gpu_stereo.py::SCAM_SHAPES at 16 (W' = 28, 130) and a quarter-map beyond the strip limit (W' = 521)
NAF_SHAPES = [(1, 22, 113, 256, 16), (1, 9, 522, 64, 16), (1, 8, 2084, 64, 0)]


@pytest.mark.parametrize("B,H,W,c,bw", NAF_SHAPES)
def test_stream_quarter_form_vs_oracle(B, H, W, c, bw):
    x = np.random.RandomState(B * 1000 + W).standard_normal((2 * B, c, H, W)).astype(np.float32)
    p = WS.scam_weights(c, seed=W + c)
    want = SO.scam({k: v.astype(np.float64) for k, v in p.items()}, "f.", x.astype(np.float64))
    e = WS.increment_err(x, want, debug_stream(x, p, bw, hook="irsde_debug_scam_stream"))
    print("SCAM(streaming) B=%d %dx%d c=%d (W'=%d) bw=%d: %.3g" % (B, H, W, c, W // 4, bw, e))
    assert e < 1e-5


def test_hooks_refuse_bad_arguments():
    x, p, _ = WS.case(WS.STREAM_SHAPES[1])
    for bw in (8, 17, WS.MAX_BLOCK_W + 16):
        with pytest.raises(_lib.IrsdeError, match="block_w"):
            debug_stream(x, p, bw)
    with pytest.raises(_lib.IrsdeError):   # 48 channels: not a multiple of 32
        debug_stream(np.zeros((2, 48, 2, 8), np.float32), WS.scam_weights(48, seed=1), 16)


# ---------------------------------------------------------------------------------------------
# the networks
# ---------------------------------------------------------------------------------------------
def unet(cfg, params, flags=0):
    m = P.stereo_sr.ConditionalUNet(3, 3, cfg["nf"], depth=cfg["depth"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m.engine_flags = flags
    return m.to(DEV).eval()


def nafnet(params, flags=0):
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in WS.NAF_SMALL.items()}
    m = P.stereo_sr.ConditionalNAFNet(img_channel=3, **cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m.engine_flags = flags
    return m.to(DEV).eval()


def forward(m, xT, lq, t):
    tt = t if isinstance(t, int) else torch.tensor(t)
    return m(torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV), tt).cpu().numpy()


def describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 20)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return buf.value.decode()


class forced_stream:
    """Plans built inside run every SCAM core on the streaming kernel with this block width (fresh engines only: built plans keep their choice)."""
    def __init__(self, bw):
        self.bw = bw

    def __enter__(self):
        assert _lib.lib().irsde_debug_force_scam_stream(self.bw) == 0

    def __exit__(self, *exc):
        assert _lib.lib().irsde_debug_force_scam_stream(0) == 0


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


def test_forced_streaming_unet_vs_reference_golden_taps_and_plan(golden):
    """The narrow fixture (2 x 22 x 38, SCAM rows 40 and 20 wide) with every SCAM on the streaming kernel at block 16: 2 - 3 blocks per row."""
    g = golden.stereo_unet
    params = SU.stereo_unet_synth_params(seed=0, **WS.UNET_SMALL)
    lq, xT = WS.stereo_inputs(2, 22, 38)
    with forced_stream(16):
        m = unet(WS.UNET_SMALL, params)
        for key, t in (("t3", 3), ("t77", 77), ("t5_60", [5, 60])):
            e = relerr(forward(m, xT, lq, t), g["small_2x22x38/" + key])
            print("stereo UNet small, streaming SCAMs, %s: %.3g" % (key, e))
            assert e < 1e-4, (key, e)
        desc = describe(m, 2, 22, 38)
        assert desc.count("scam_full_stream_core") == 5 and "scam_full_core(" not in desc and desc.count("bw=16") == 5
        mk = unet(WS.UNET_SMALL, params, flags=_lib.FLAG_KEEP_ACTIVATIONS)
        taps = {}
        ref = SU.stereo_unet_forward(params, xT, lq, [9, 41], depth=2, taps=taps)
        assert relerr(forward(mk, xT, lq, [9, 41]), ref) < 1e-4
        bad = {}
        for name in ("downs.0.3", "downs.1.3", "mid_fusion", "ups.0.3", "ups.1.3"):
            e = relerr(mk.debug_tap(name).numpy(), taps[name])
            if not e < 1e-4:
                bad[name] = e
        assert not bad, bad


def test_forced_streaming_nafnet_vs_reference_golden_and_plan(golden):
    params = WS.naf_params()
    lq, xT = WS.stereo_inputs(2, 32, 48)
    with forced_stream(16):
        m = nafnet(params)
        e = relerr(forward(m, xT, lq, 77), golden.stereo["small_2x32x48/t77"])
        print("stereo NAFNet small, streaming SCAMs: %.3g" % e)
        assert e < 1e-4
        desc = describe(m, 2, 32, 48)
        assert desc.count("scam_stream_core") == 5 and "scam_core(" not in desc


@pytest.fixture(scope="module")
def wide_small():
    return unet(WS.UNET_SMALL, WS.wide_unet_params(WS.UNET_SMALL)).set_wide_rows()


def test_wide_unet_small_by_the_flag(golden, wide_small):
    lq, xT = WS.stereo_inputs(1, 6, 1030)
    m = wide_small
    e = relerr(sub3(forward(m, xT, lq, 77)), golden.stereo_wide["unet_small_1x6x1030/t77"])
    print("stereo UNet small 1x6x6x1030 (wide rows): %.3g" % e)
    assert e < 1e-4
    rows = [r for r in describe(m, 1, 6, 1030).splitlines() if "_core(" in r and "scam_full" in r]
    assert len(rows) == 5, rows
    kinds = ["stream" if r.startswith("scam_full_stream_core(") else "strip" if r.startswith("scam_full_core(") else r for r in rows]
    assert kinds == ["stream", "strip", "strip", "strip", "stream"], rows   # downs.0.3, downs.1.3, mid_fusion, ups.0.3, ups.1.3
    assert all("hw=8x1032 bw=512" in r for r in (rows[0], rows[4])) and all("hw=4x516" in r for r in rows[1:4]), rows
    try:
        with pytest.raises(_lib.IrsdeError, match="wider than 1024"):
            forward(m.set_wide_rows(False), xT, lq, 77)
    finally:
        m.set_wide_rows()


def test_wide_unet_full_by_the_flag(golden):
    m = unet(WS.UNET_FULL, WS.wide_unet_params(WS.UNET_FULL)).set_wide_rows()
    lq, xT = WS.stereo_inputs(1, 16, 1040)
    e = relerr(sub3(forward(m, xT, lq, 60)), golden.stereo_wide["unet_full_1x16x1040/t60"])
    print("stereo UNet nf64 depth4 1x6x16x1040 (wide rows): %.3g" % e)
    assert e < 1e-4


def test_wide_nafnet_by_the_flag(golden):
    m = nafnet(WS.naf_params()).set_wide_rows()
    lq, xT = WS.stereo_inputs(1, 16, 2084)
    e = relerr(sub3(forward(m, xT, lq, 37)), golden.stereo_wide["naf_small_1x16x2084/t37"])
    print("stereo NAFNet small 1x6x16x2084 (wide rows): %.3g" % e)
    assert e < 1e-4
    desc = describe(m, 1, 16, 2084)
    assert desc.count("scam_stream_core(") == 2 and desc.count("scam_core(") == 3 and "W'=521 H'=4 bw=512" in desc   # encoders.0.0, decoders.1.0
    try:
        with pytest.raises(_lib.IrsdeError, match="wider than 2051"):
            forward(m.set_wide_rows(False), xT, lq, 37)
    finally:
        m.set_wide_rows()


def test_flag_changes_nothing_below_the_limit():
    params = SU.stereo_unet_synth_params(seed=0, **WS.UNET_SMALL)
    lq, xT = WS.stereo_inputs(2, 22, 38)
    plain, flagged = unet(WS.UNET_SMALL, params), unet(WS.UNET_SMALL, params).set_wide_rows()
    assert np.array_equal(forward(plain, xT, lq, 33), forward(flagged, xT, lq, 33))
    d = describe(plain, 2, 22, 38)
    assert d == describe(flagged, 2, 22, 38) and d.count("scam_full_core(") == 5 and "stream" not in d


def test_wide_samplers_vs_reference_golden_and_graph_equals_eager(golden, wide_small):
    g = golden.stereo_wide
    B, H, W, T = 1, 6, 1030, 5
    lq, xT = WS.stereo_inputs(B, H, W)
    z = O.synth_noise(7, T, (B, 6, H, W))
    sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
    for mode in ("sde", "ode"):
        got = _sample(wide_small, sde, mode, lq, xT, z, True)
        e = relerr(sub3(got), g["unet_small_sampler_1x6x1030_T5/" + mode])
        print("stereo UNet sampler (wide rows) %s: %.3g" % (mode, e))
        assert e < 2e-3, (mode, e)
        assert np.array_equal(got, _sample(wide_small, sde, mode, lq, xT, z, False)), mode


def test_two_pair_batch_equals_its_single_pairs_under_streaming():
    """Bit for bit: network evaluation and the sampler with the device (keyed Philox) noise."""
    params = SU.stereo_unet_synth_params(seed=0, **WS.UNET_SMALL)
    lq, xT = WS.stereo_inputs(2, 22, 38)
    with forced_stream(16):
        m = unet(WS.UNET_SMALL, params)
        both = forward(m, xT, lq, 33)
        for b in range(2):
            assert np.array_equal(both[b:b + 1], forward(m, xT[b:b + 1], lq[b:b + 1], 33)), b
        assert "scam_full_stream_core" in describe(m, 1, 22, 38)
        T = 4
        sde = P.IRSDE(50, T, "cosine", 0.005, device=DEV)
        sde.seed = 3
        full = _sample(m, sde, "sde", lq, xT, None, True)
        assert np.isfinite(full).all() and not np.array_equal(full[0], full[1])
        try:
            for b in range(2):
                sde.image_offset = b
                assert np.array_equal(full[b:b + 1], _sample(m, sde, "sde", lq[b:b + 1], xT[b:b + 1], None, True)), b
        finally:
            sde.image_offset = 0
