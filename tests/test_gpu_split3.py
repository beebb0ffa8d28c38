"""GPU tests of the exact-fp32 engine's three-piece bf16 GEMM path (csrc/gemm_split.hip gemm_split3i_kernel; writers in csrc/wino.hip; plan rule in
csrc/engine_plan.hip): the GEMM alone, single layers through irsde_debug_conv selectors 48 / 26 / 27, and the network with the path forced.

GEMM bar: max-abs error against float64 over max |float64|, below 3 x the error of numpy's float32 A @ B.T on the same inputs (tests/split3_oracle.py;
the host test shows that a lost plane or product lands above that bar).  Layer bar: 5e-5 against the float64 direct convolution, the project's bar for
F(4x4) kernels.  Network bar: 1e-4 against the reference golden forward.  Every test prints its figure next to the native path's before it asserts.
Measured on an MI355X: GEMM 2.0e-7 .. 1.24e-6 against bars 7.0e-7 .. 1.73e-6; F(4x4,3x3) layers 2.8e-6 .. 3.9e-6 (native selector 3: 3.3e-6 .. 4.7e-6); polyphase
down 2.2e-6 (2.5e-6), up 1.8e-6 (1.8e-6); golden forward 8.1e-7.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

import split3_oracle as S3
import wino_poly_oracle as WP
from test_gpu_parity import DEV, relerr, run_conv, oracle_conv, _sample

pytestmark = pytest.mark.gpu

# (M, N, K, ncomp)
GEMM = [(300, 160, 64, 3),      # ragged rows and columns, two K-steps
        (256, 256, 96, 2),      # odd step count
        (130, 512, 32, 36),     # one step, every component
        (512, 256, 1536, 1),    # long accumulation
        (1024, 512, 64, 25)]    # several units per XCD


@pytest.mark.parametrize("shape", GEMM)
def test_gemm_vs_float64(shape):
    M, N, K, ncomp = shape
    A, B = S3.inputs(M, N, K, ncomp)
    ref = np.einsum("zmk,znk->zmn", A.astype(np.float64), B.astype(np.float64))
    bar = S3.bar(A, B, ref)
    dA, dB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    dC = torch.full((ncomp, M, N), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_split_gemm(p(dA), p(dB), p(dC), M, N, K, ncomp, 43, None))
    C = dC.cpu().numpy()
    e = S3.err(C, ref)
    print("three-piece gemm %s: %.3g (bar %.3g = 3 x numpy float32)" % (shape, e, bar))
    assert np.isfinite(C).all() and e < bar


def _layer_case(seed, B, C0, C1, H, W, Cout, K):
    rs = np.random.RandomState(seed)
    x0 = rs.standard_normal((B, C0, H, W)).astype(np.float32)
    x1 = rs.standard_normal((B, C1, H, W)).astype(np.float32) if C1 else None
    w = (rs.standard_normal((Cout, C0 + C1, K, K)) / np.sqrt((C0 + C1) * K * K)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    return rs, x0, x1, w, bias


def _check_layer(what, args, ref, sel, native_sel, **kw):
    got = run_conv(*args, naive=sel, **kw)
    e, e_native = relerr(got, ref), relerr(run_conv(*args, naive=native_sel, **kw), ref)
    print("%s: three-piece %.3g, native selector %d %.3g" % (what, e, native_sel, e_native))
    assert got.shape == ref.shape and np.isfinite(got).all() and e < 5e-5


def test_layer_two_sources_film_silu():
    B, C0, C1, H, W, Cout = 2, 64, 32, 16, 16, 64
    rs, x0, x1, w, bias = _layer_case(1, B, C0, C1, H, W, Cout, 3)
    film = (0.3 * rs.standard_normal((B, 2 * Cout))).astype(np.float32)
    args = (x0, x1, w, bias, 1, 1, 0, film, 1, None)
    _check_layer("F(4x4,3x3) 64+32 -> 64, FiLM + SiLU", args, oracle_conv(*args, film_bstride=2 * Cout), 48, 3, film_bstride=2 * Cout)


def test_layer_silu_residual():
    B, C0, H, W, Cout = 1, 64, 24, 40, 96
    rs, x0, _, w, bias = _layer_case(2, B, C0, 0, H, W, Cout, 3)
    res = rs.standard_normal((B, Cout, H, W)).astype(np.float32)
    args = (x0, None, w, bias, 1, 1, 0, None, 1, res)
    _check_layer("F(4x4,3x3) 64 -> 96, SiLU + residual", args, oracle_conv(*args), 48, 3)


def test_layer_in_shift():
    rs, x0, _, w, bias = _layer_case(3, 1, 64, 0, 8, 8, 64, 3)
    args = (x0, None, w, bias, 1, 1, 1, None, 0, None)
    _check_layer("F(4x4,3x3) 64 -> 64 behind the nearest x2 upsample", args, oracle_conv(*args), 48, 3)


def test_layer_polyphase_down():
    _, x0, _, w, bias = _layer_case(4, 1, 32, 0, 16, 16, 64, 4)
    args = (x0, None, w, bias, 2, 1, 0, None, 0, None)
    _check_layer("polyphase down 32 -> 64", args, WP.direct_down(x0, w, bias), 26, 24)


def test_layer_polyphase_up():
    _, x0, _, w, bias = _layer_case(5, 1, 64, 0, 8, 8, 32, 3)
    args = (x0, None, w, bias, 1, 1, 1, None, 0, None)
    _check_layer("polyphase up 64 -> 32", args, WP.direct_up(x0, w, bias), 27, 25)


@pytest.fixture()
def hooks():
    """Both process-wide hooks back at their defaults afterwards.  The smallest golden network's three-launch F(4x4,3x3) layers are below the plan's general
    256-block floor, so its eligible layers are the polyphase ones: the polyphase path is forced wherever eligible next to the three-piece mode under test."""
    L = _lib.lib()
    L.irsde_debug_force_wino_poly(2)
    yield L
    L.irsde_debug_force_split3(-1)
    L.irsde_debug_force_wino_poly(-1)


def _fresh(nf, depth, flags=0):
    m = P.ConditionalUNet(3, 3, nf, depth=depth)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0, nf=nf, depth=depth).items()}, strict=True)
    m.engine_flags = flags
    return m.to(DEV).eval()


def _describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return buf.value.decode()


def _gemm_rows(d):
    return [l for l in d.splitlines() if "conv(winograd F4 gemm x36" in l or "conv(winograd F4x2 poly" in l]


def test_network_forced_vs_reference_golden_and_plan_marker(golden, hooks):
    g = golden.forward
    tag = "nf32d2_2x24x20"
    nf, depth, B, H, W = (int(v) for v in g[tag + "/cfg"])
    hooks.irsde_debug_force_split3(2)
    m = _fresh(nf, depth)
    rows = _gemm_rows(_describe(m, B, H, W))
    assert len(rows) >= 2 * (depth - 1) and all(r.endswith(" bf16x3") for r in rows), rows     # every eligible layer
    lq, xT = O.synth_inputs(1234, B, H, W)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    for t in (int(v) for v in g[tag + "/ts"]):
        e = relerr(m(x, c, t).cpu().numpy(), g[tag + "/t%d" % t])
        print("three-piece GEMMs forced, %s t=%d vs the reference: %.3g" % (tag, t, e))
        assert e < 1e-4, t
    hooks.irsde_debug_force_split3(0)
    rows0 = _gemm_rows(_describe(_fresh(nf, depth), B, H, W))
    assert len(rows0) == len(rows) and not any("bf16x3" in r for r in rows0), rows0              # and none with mode 0


def test_graph_replay_is_bit_identical_to_eager(hooks):
    nf, depth, B, H, W, T = 32, 2, 2, 24, 20, 2
    hooks.irsde_debug_force_split3(2)
    m = _fresh(nf, depth)
    assert " bf16x3" in _describe(m, B, H, W)
    lq, xT = O.synth_inputs(5, B, H, W)
    z = O.synth_noise(7, T, (B, 3, H, W))
    eager = _sample(m, "sde", T, lq, xT, z, graph=False)
    graph = _sample(m, "sde", T, lq, xT, z, graph=True)
    assert np.isfinite(eager).all() and np.array_equal(eager, graph)


def test_flag_equals_mode_0_bit_for_bit(hooks):
    nf, depth, B, H, W = 32, 2, 2, 24, 20
    lq, xT = O.synth_inputs(1234, B, H, W)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    hooks.irsde_debug_force_split3(2)
    flagged = _fresh(nf, depth, _lib.FLAG_NO_SPLIT3)
    d_flag = _describe(flagged, B, H, W)
    y_flag = flagged(x, c, 50).cpu().numpy()
    y_on = _fresh(nf, depth)(x, c, 50).cpu().numpy()
    hooks.irsde_debug_force_split3(0)
    off = _fresh(nf, depth)
    assert "bf16x3" not in d_flag and d_flag == _describe(off, B, H, W)
    y_off = off(x, c, 50).cpu().numpy()
    assert np.array_equal(y_flag, y_off)
    assert not np.array_equal(y_on, y_off)   # (the forced path is a different arithmetic: the comparison above compares something)
