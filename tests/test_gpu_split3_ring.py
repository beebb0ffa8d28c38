"""GPU tests of the three-piece GEMM's load ring (csrc/gemm_split.hip, gemm_split3i_kernel<ABL, WALK, DRAIN>): the two LDS stages are six units (per K-step
the first and the second 32 rows of every wave's A rows, and the B rows), a K-step is two phases that end in a counted s_waitcnt vmcnt (or none) and a raw
s_barrier, three or nine LDS-DMA wave-loads per wave stay in flight across every barrier of the K loop, and fragment reads run a 16-k sub-step ahead.

Selectors of irsde_debug_split_gemm: 43 the production launch (ring on the persistent walk), 47 the drain twin (the same kernel with vmcnt(0) in front of every
barrier: same issue order, nothing in flight across a barrier), 45 the one-item-per-block launch of the ring.  Per output element all three run the same six
products in the same order over the same K order, so they must agree bit for bit; a mistimed wait reads a unit before its DMA has landed, which shows as a
difference from the drain twin or between two launches on the same buffers.

K = 32 .. 160 = 1 .. 5 K-steps: a step is half the ring, so these are fewer steps than the ring holds (the opening loads are all there is), exactly as many,
the first wrap (the first restaged unit), and odd and even step counts (the last step ends in either stage; the vmcnt(3) phase exists from two steps on).
M = 300, N = 160 is ragged on both sides of the 256 x 128 tile; M = 1024, N = 512 with 36 components is 576 items, so on a 256-CU part every block crosses at
least two item boundaries with the ring full.

float64 bar: tests/split3_oracle.py's, three times the error of numpy's float32 product on the same inputs, as in tests/test_gpu_split3.py.  Layers: the
5e-5 bar of tests/test_gpu_split3.py against the float64 direct convolution, through both triple writers of the polyphase Upsample.
"""
import ctypes

import numpy as np
import pytest
import torch

from image_restoration_sde_amd import _lib

import split3_oracle as S3
import wino_poly_oracle as WP
from test_gpu_parity import DEV, relerr, run_conv, oracle_conv

pytestmark = pytest.mark.gpu

# (M, N, K, ncomp)
RING = [(300, 160, 32, 3), (300, 160, 64, 3), (300, 160, 96, 3), (300, 160, 128, 3), (300, 160, 160, 3), (1024, 512, 64, 36)]
_cache = {}


def _case(shape):
    """Inputs, float64 product and bar of a shape: computed once, shared by the tests, never written to."""
    if shape not in _cache:
        M, N, K, ncomp = shape
        A, B = S3.inputs(M, N, K, ncomp)
        ref = np.einsum("zmk,znk->zmn", A.astype(np.float64), B.astype(np.float64))
        for x in (A, B, ref):
            x.setflags(write=False)
        _cache[shape] = (A, B, ref, S3.bar(A, B, ref))
    return _cache[shape]


def _launch(dA, dB, dC, shape, sel):
    M, N, K, ncomp = shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dC.fill_(float("nan"))
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_split_gemm(p(dA), p(dB), p(dC), M, N, K, ncomp, sel, None))
    return dC.cpu().numpy()


@pytest.mark.parametrize("shape", RING)
def test_ring_vs_float64_and_its_twins_bit_for_bit(shape):
    M, N, K, ncomp = shape
    A, B, ref, bar = _case(shape)
    dA, dB = torch.tensor(A, device=DEV), torch.tensor(B, device=DEV)   # (copies: the shared arrays are read-only)
    dC = torch.empty((ncomp * M + 1, N), device=DEV)   # one guard row behind [ncomp][M][N]
    out = {sel: _launch(dA, dB, dC, shape, sel) for sel in (43, 47, 45)}
    again = _launch(dA, dB, dC, shape, 43)             # a second launch of the production kernel on the same buffers
    ring = out[43][:-1].reshape(ncomp, M, N)
    e = S3.err(ring, ref)
    print("three-piece gemm, ring, %s: %.3g (bar %.3g = 3 x numpy float32)" % (shape, e, bar))
    assert np.isfinite(ring).all() and e < bar
    for sel in (43, 47, 45):
        assert np.isnan(out[sel][-1]).all(), sel        # nothing behind the last row
    assert np.array_equal(out[43], out[47], equal_nan=True)   # the drain twin
    assert np.array_equal(out[43], out[45], equal_nan=True)   # one item per block
    assert np.array_equal(out[43], again, equal_nan=True)


def test_selector_46_is_still_refused():
    """47 is the drain twin (46 / 47 of irsde_debug_conv are other kernels); the hook knows no 46 and no 48"""
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    assert L.irsde_debug_split_gemm(z, z, z, 32, 32, 32, 1, 46, None) != 0
    assert L.irsde_debug_split_gemm(z, z, z, 32, 32, 32, 1, 48, None) != 0


def test_layer_two_sources_on_the_ring():
    """The F(4x4,3x3) two-source layer of tests/test_gpu_split3.py: wino_input's triples into the ring"""
    B, C0, C1, H, W, Cout = 2, 64, 32, 16, 16, 64
    rs = np.random.RandomState(1)
    x0 = rs.standard_normal((B, C0, H, W)).astype(np.float32)
    x1 = rs.standard_normal((B, C1, H, W)).astype(np.float32)
    w = (rs.standard_normal((Cout, C0 + C1, 3, 3)) / np.sqrt((C0 + C1) * 9)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    film = (0.3 * rs.standard_normal((B, 2 * Cout))).astype(np.float32)
    args = (x0, x1, w, bias, 1, 1, 0, film, 1, None)
    ref = oracle_conv(*args, film_bstride=2 * Cout)
    got = run_conv(*args, naive=48, film_bstride=2 * Cout)
    e = relerr(got, ref)
    print("F(4x4,3x3) 64+32 -> 64, FiLM + SiLU on the ring: %.3g" % e)
    assert got.shape == ref.shape and np.isfinite(got).all() and e < 5e-5


def test_layer_polyphase_up_both_writers_on_the_ring():
    """The polyphase up layer of tests/test_gpu_split3.py: whole-line writer (27) and per-thread writer (28) into the ring"""
    rs = np.random.RandomState(5)
    x0 = rs.standard_normal((1, 64, 8, 8)).astype(np.float32)
    w = (rs.standard_normal((32, 64, 3, 3)) / np.sqrt(64 * 9)).astype(np.float32)
    bias = rs.standard_normal(32).astype(np.float32)
    args = (x0, None, w, bias, 1, 1, 1, None, 0, None)
    ref = WP.direct_up(x0, w, bias)
    lines, threads = run_conv(*args, naive=27), run_conv(*args, naive=28)
    e = relerr(lines, ref)
    print("polyphase up 64 -> 32 on the ring: whole-line writer %.3g, per-thread writer %.3g" % (e, relerr(threads, ref)))
    assert lines.shape == ref.shape and np.isfinite(lines).all() and e < 5e-5
    assert np.array_equal(lines, threads)
