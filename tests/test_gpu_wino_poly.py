"""GPU tests of the polyphase Winograd F(4x4,2x2) path of the resampling convolutions (csrc/wino.hip: wino_poly_input_kernel, the component GEMMs of
conv_igemm.hip with 25 / 100 components, wino_poly_output_kernel), through irsde_debug_conv selectors 24 (4x4 stride 2 pad 1) and 25 (nearest x2 + 3x3).

Bar: relerr < 5e-5 against the float64 direct convolution, the project's bar for F(4x4) convolution kernels; the float64 restatement
of the algorithm (tests/wino_poly_oracle.py) is checked against the same direct convolution on the host (tests/test_wino_poly_host.py).
Measured on an MI355X: down 2.3e-6 .. 5.7e-6, up 1.8e-6 .. 6.4e-6 (the direct kernel on the same cases: 4.2e-7 .. 2.2e-6; F(4x4,3x3): 5e-6 .. 1.4e-5); the
smallest golden forward with the path forced on its Downsample and its Upsample: 8.1e-7 / 7.6e-7 against the reference (bar 1e-4).
"""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

import wino_poly_oracle as WP
from test_gpu_parity import DEV, relerr, run_conv, _sample

pytestmark = pytest.mark.gpu

BAR = 5e-5
# NCHW in -> Cout
DOWN = [(2, 32, 16, 16, 64),
        (1, 32, 10, 14, 32),    # 5 x 7 outputs: every edge ragged
        (3, 64, 42, 62, 128),   # 21 x 31 outputs
        (1, 256, 8, 8, 64)]     # K = 1024, one tile per image
UP = [(2, 64, 4, 4, 32),
      (1, 32, 5, 7, 32),
      (2, 128, 21, 31, 64),
      (1, 512, 8, 8, 64)]


def case(shape, K):
    B, C, H, W, O_ = shape
    rs = np.random.RandomState(B * 1000 + C + 7 * H + W + K)
    x = rs.standard_normal((B, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((O_, C, K, K)) / np.sqrt(C * K * K)).astype(np.float32)
    bias = rs.standard_normal(O_).astype(np.float32)
    return x, w, bias


@pytest.mark.parametrize("shape", DOWN)
def test_down_vs_float64_direct(shape):
    x, w, bias = case(shape, 4)
    ref = WP.direct_down(x, w, bias)
    got = run_conv(x, None, w, bias, 2, 1, 0, None, 0, None, naive=24)
    assert got.shape == ref.shape and np.isfinite(got).all()
    e, e_direct = relerr(got, ref), relerr(run_conv(x, None, w, bias, 2, 1, 0, None, 0, None, naive=0), ref)
    print("wino_poly down %s: %.3g (direct kernel %.3g)" % (shape, e, e_direct))
    assert e < BAR, shape
    # no bias: the other epilogue instance
    assert relerr(run_conv(x, None, w, None, 2, 1, 0, None, 0, None, naive=24), WP.direct_down(x, w)) < BAR, shape


@pytest.mark.parametrize("shape", UP)
def test_up_vs_float64_direct(shape):
    x, w, bias = case(shape, 3)
    ref = WP.direct_up(x, w, bias)
    got = run_conv(x, None, w, bias, 1, 1, 1, None, 0, None, naive=25)
    assert got.shape == ref.shape and np.isfinite(got).all()
    e, e_direct = relerr(got, ref), relerr(run_conv(x, None, w, bias, 1, 1, 1, None, 0, None, naive=0), ref)
    print("wino_poly up %s: %.3g (direct kernel %.3g)" % (shape, e, e_direct))
    assert e < BAR, shape
    assert relerr(run_conv(x, None, w, None, 1, 1, 1, None, 0, None, naive=25), WP.direct_up(x, w)) < BAR, shape


def test_selectors_refuse_everything_else():
    """24 runs a 4x4 stride-2 pad-1 layer, 25 an in_shift = 1 3x3 layer, both single source and bias only; anything else is an error, not another path."""
    x, w4, bias = case(DOWN[0], 4)
    _, w3, _ = case((2, 32, 16, 16, 64), 3)
    res = np.zeros((2, 64, 8, 8), np.float32)
    film = np.zeros((1, 128), np.float32)
    bad = [dict(args=(x, None, w3, bias, 1, 1, 0, None, 0, None), naive=24),      # a plain 3x3
           dict(args=(x, None, w3, bias, 1, 1, 0, None, 0, None), naive=25),      # 3x3 without the upsample
           dict(args=(x, None, w4, bias, 2, 1, 0, None, 0, None), naive=25),      # the down layer on the up selector
           dict(args=(x, None, w4, bias, 2, 1, 0, None, 1, None), naive=24),      # SiLU
           dict(args=(x, None, w4, bias, 2, 1, 0, film, 0, None), naive=24),      # FiLM
           dict(args=(x, None, w4, bias, 2, 1, 0, None, 0, res), naive=24),       # residual
           dict(args=(x[:, :16], x[:, 16:], w4, bias, 2, 1, 0, None, 0, None), naive=24)]   # two sources
    for b in bad:
        with pytest.raises(_lib.IrsdeError):
            run_conv(*b["args"], naive=b["naive"])


@pytest.fixture()
def forced_everywhere():
    L = _lib.lib()
    L.irsde_debug_force_wino_poly(2)
    yield
    L.irsde_debug_force_wino_poly(-1)


def _fresh(nf, depth):
    m = P.ConditionalUNet(3, 3, nf, depth=depth)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0, nf=nf, depth=depth).items()}, strict=True)
    return m.to(DEV).eval()


def _describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return buf.value.decode()


def test_network_forced_everywhere_vs_reference_golden(golden, forced_everywhere):
    """The smallest case of the reference golden forward (tests/golden/forward.npz) with the path forced wherever eligible: its Downsample and its Upsample
    both run it (the plan says so), at the one-evaluation bar of 1e-4."""
    g = golden.forward
    tag = "nf32d2_2x24x20"
    nf, depth, B, H, W = (int(v) for v in g[tag + "/cfg"])
    m = _fresh(nf, depth)
    lq, xT = O.synth_inputs(1234, B, H, W)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    d = _describe(m, B, H, W)
    assert d.count("wino_poly_input(down)") == depth - 1 and d.count("wino_poly_input(up)") == depth - 1, d
    assert d.count("conv(winograd F4x2 poly") == 2 * (depth - 1) and d.count("wino_poly_output(") == 2 * (depth - 1), d
    for t in (int(v) for v in g[tag + "/ts"]):
        e = relerr(m(x, c, t).cpu().numpy(), g[tag + "/t%d" % t])
        print("forced polyphase path, %s t=%d vs the reference: %.3g" % (tag, t, e))
        assert e < 1e-4, t


def test_flag_and_rule_keep_small_plans_on_the_old_paths(forced_everywhere):
    """IRSDE_FLAG_NO_WINO_POLY wins over the forced mode; under the rule (mode 1) a plan whose component GEMMs cannot fill the GPU has no polyphase rows."""
    m = _fresh(32, 2)
    m.engine_flags = _lib.FLAG_NO_WINO_POLY
    assert "wino_poly" not in _describe(m, 2, 24, 20)
    _lib.lib().irsde_debug_force_wino_poly(1)
    assert "wino_poly" not in _describe(_fresh(32, 2), 2, 24, 20)


def test_graph_replay_is_bit_identical_to_eager(forced_everywhere):
    """2-step reverse_sde with the path forced: the captured step graph against eager launches, bit for bit."""
    nf, depth, B, H, W, T = 32, 2, 2, 24, 20, 2
    m = _fresh(nf, depth)
    assert "wino_poly_input(down)" in _describe(m, B, H, W)
    lq, xT = O.synth_inputs(5, B, H, W)
    z = O.synth_noise(7, T, (B, 3, H, W))
    eager = _sample(m, "sde", T, lq, xT, z, graph=False)
    graph = _sample(m, "sde", T, lq, xT, z, graph=True)
    assert np.isfinite(eager).all() and np.array_equal(eager, graph)
