"""Host checks of the polyphase Winograd F(4x4,2x2) restatement (tests/wino_poly_oracle.py) that the GPU kernels of csrc/wino.hip are tested against.

The bar of the GPU tests (tests/test_gpu_wino_poly.py) is relerr < 5e-5 against the float64 direct convolution, the project's bar for F(4x4) convolution
kernels.  Here: the algorithm is exact in float64 (1e-12), its float32 evaluation stays under that bar, and each deliberately wrong
variant misses the bar by at least 10x, so the bar can tell them apart.
"""
import numpy as np
import pytest

import wino_poly_oracle as WP

BAR = 5e-5

# (B, C, H, W, Cout): ragged on every edge, odd low-resolution sizes, sizes that are no multiple of the tile, one tile per image
DOWN = [(2, 8, 16, 16, 8), (1, 8, 10, 14, 4), (2, 4, 42, 62, 4), (1, 16, 8, 8, 8)]
UP = [(2, 8, 4, 4, 8), (1, 8, 5, 7, 4), (2, 4, 21, 31, 4), (1, 16, 8, 8, 8)]


def relerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def case(shape, K, seed):
    B, C, H, W, O = shape
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((O, C, K, K)) / np.sqrt(C * K * K)).astype(np.float32)
    bias = rs.standard_normal(O).astype(np.float32)
    return x, w, bias


@pytest.mark.parametrize("shape", DOWN)
def test_down_float64_is_exact(shape):
    x, w, bias = case(shape, 4, 1)
    ref = WP.direct_down(x, w, bias)
    assert relerr(WP.poly_down(x, w, bias), ref) < 1e-12


@pytest.mark.parametrize("shape", UP)
def test_up_float64_is_exact(shape):
    x, w, bias = case(shape, 3, 2)
    ref = WP.direct_up(x, w, bias)
    assert ref.shape[2:] == (2 * shape[2], 2 * shape[3])
    assert relerr(WP.poly_up(x, w, bias), ref) < 1e-12


@pytest.mark.parametrize("shape", DOWN)
def test_down_float32_stays_under_the_gpu_bar(shape):
    x, w, bias = case(shape, 4, 3)
    e = relerr(WP.poly_down(x, w, bias, dtype=np.float32), WP.direct_down(x, w, bias))
    assert e < BAR, e


@pytest.mark.parametrize("shape", UP)
def test_up_float32_stays_under_the_gpu_bar(shape):
    x, w, bias = case(shape, 3, 4)
    e = relerr(WP.poly_up(x, w, bias, dtype=np.float32), WP.direct_up(x, w, bias))
    assert e < BAR, e


@pytest.mark.parametrize("wrong", [v for v in WP.WRONG if v != "unsummed_taps"])   # (the down mode sums no taps)
@pytest.mark.parametrize("shape", [DOWN[1], DOWN[3]])
def test_down_wrong_variants_miss_the_bar(shape, wrong):
    x, w, bias = case(shape, 4, 5)
    e = relerr(WP.poly_down(x, w, bias, wrong=wrong), WP.direct_down(x, w, bias))
    assert e >= 10 * BAR, (wrong, e)


@pytest.mark.parametrize("wrong", WP.WRONG)
@pytest.mark.parametrize("shape", [UP[1], UP[3]])
def test_up_wrong_variants_miss_the_bar(shape, wrong):
    x, w, bias = case(shape, 3, 6)
    e = relerr(WP.poly_up(x, w, bias, wrong=wrong), WP.direct_up(x, w, bias))
    assert e >= 10 * BAR, (wrong, e)


def test_matrices_are_the_toom_cook_ones():
    """A^T [(G g) . (B^T d)] is the 4-output correlation of 2 taps over 5 inputs, for any g and d."""
    rs = np.random.RandomState(7)
    g, d = rs.standard_normal(2), rs.standard_normal(5)
    y = WP.AT @ ((WP.G @ g) * (WP.BT @ d))
    np.testing.assert_allclose(y, [g[0] * d[i] + g[1] * d[i + 1] for i in range(4)], rtol=0, atol=1e-13)
