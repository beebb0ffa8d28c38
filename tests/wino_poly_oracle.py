"""Polyphase Winograd F(4x4,2x2) for the resampling convolutions, restated in numpy (csrc/wino.hip: wino_poly_*).

  down:  Conv2d(4x4, stride 2, pad 1).  out(oy, ox) = sum_{ky,kx} w[ky, kx] in(2 oy - 1 + ky, 2 ox - 1 + kx); with ky = 2a + p, kx = 2b + q this is, for
         each input pixel phase (p, q), a 2x2 correlation with taps w[2a + p, 2b + q] over every second pixel starting at (2 oy - 1 + p, 2 ox - 1 + q).  The
         four phases and Cin add up inside each of the 25 Winograd components (K = 4 Cin); a 4x4 output tile reads a 10x10 input patch.
  up:    nearest x2, then Conv2d(3x3, pad 1).  out(2i + py, 2j + px) is a 2x2 correlation over the LOW-resolution map: rows {i - 1, i} with taps
         {w0, w1 + w2} for py = 0, rows {i, i + 1} with taps {w0 + w1, w2} for py = 1, columns alike: four output phases x 25 components with K = Cin; a
         tile reads a 6x6 low-resolution patch and writes an 8x8 output block.

F(4,2) with the points 0, 1, -1, 2, inf:  y = A^T [(G g) . (B^T d)], 5 products per 4 outputs and axis.

`dtype` is the arithmetic of the transforms and the component products (float64: the algorithm itself; float32: what the kernels do, with U rounded once
from its float64 value as the weight packer does).  The `wrong` argument selects a deliberately broken variant for the sensitivity tests.
"""
import numpy as np

BT = np.array([[2, -1, -2, 1, 0],
               [0, -2, -1, 1, 0],
               [0, 2, -3, 1, 0],
               [0, -1, 0, 1, 0],
               [0, 2, -1, -2, 1]], dtype=np.float64)
G = np.array([[1 / 2, 0],
              [-1 / 2, -1 / 2],
              [-1 / 6, 1 / 6],
              [1 / 6, 1 / 3],
              [0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 0],
               [0, 1, -1, 2, 0],
               [0, 1, 1, 4, 0],
               [0, 1, -1, 8, 1]], dtype=np.float64)

WRONG = ("swapped_parity", "no_offset", "unsummed_taps", "transposed_g")


def direct_down(x, w, bias=None):
    """float64 Conv2d(4x4, stride 2, pad 1); x [B][C][H][W], w [O][C][4][4]."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, C, H, W = x.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    xp = np.zeros((B, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((B, w.shape[0], Ho, Wo))
    for ky in range(4):
        for kx in range(4):
            y += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], w[:, :, ky, kx])
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :, None, None]


def direct_up(x, w, bias=None):
    """float64 nearest x2 upsample followed by Conv2d(3x3, pad 1); x [B][C][H][W], w [O][C][3][3]."""
    x = np.asarray(x, np.float64).repeat(2, axis=2).repeat(2, axis=3)
    w = np.asarray(w, np.float64)
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :, None, None]


def _weights(g, dtype, wrong):
    """U[o][c][5][5] = G g G^T from g [O][C][2][2] (float64), rounded once to `dtype`."""
    if wrong == "transposed_g":   # G applied on the wrong sides: (G g G^T)^T = G g^T G^T
        return np.einsum("ra,ocab,sb->ocsr", G, g, G).astype(dtype)
    return np.einsum("ra,ocab,sb->ocrs", G, g, G).astype(dtype)


def _tiles(xp, y0, x0, step, TH, TW, dtype):
    """V[b][c][ty][tx][5][5] = B^T d B of the 5x5 patches (every `step`-th pixel) whose first pixel is xp[y0 + 4 step ty, x0 + 4 step tx]."""
    B, C = xp.shape[:2]
    d = np.empty((B, C, TH, TW, 5, 5), dtype)
    for r in range(5):
        for s in range(5):
            ys, xs = y0 + step * r, x0 + step * s
            d[..., r, s] = xp[:, :, ys:ys + 4 * step * TH:4 * step, xs:xs + 4 * step * TW:4 * step]
    bt = BT.astype(dtype)
    return np.einsum("ir,bcyxrs,js->bcyxij", bt, d, bt)


def _untile(M, dtype):
    """y[b][o][4 TH][4 TW] = A^T m A of M[b][o][ty][tx][5][5]."""
    at = AT.astype(dtype)
    y = np.einsum("ir,boyxrs,js->boyixj", at, M, at)
    B, O, TH, _, TW, _ = y.shape
    return y.reshape(B, O, 4 * TH, 4 * TW)


def poly_down(x, w, bias=None, dtype=np.float64, wrong=None):
    x = np.asarray(x, dtype)
    w64 = np.asarray(w, np.float64)
    B, C, H, W = x.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    TH, TW = (Ho + 3) // 4, (Wo + 3) // 4
    pad = 2   # xp[y + pad] = x[y]; zeros outside, far enough for every ragged tile
    xp = np.zeros((B, C, pad + 8 * TH + 4, pad + 8 * TW + 4), dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    M = np.zeros((B, w64.shape[0], TH, TW, 5, 5), dtype)
    for p in range(2):
        for q in range(2):
            g = w64[:, :, p::2, q::2]   # taps w[2a + p][2b + q]
            U = _weights(g, dtype, wrong)
            pp, qq = (1 - p, 1 - q) if wrong == "swapped_parity" else (p, q)
            off = 0 if wrong == "no_offset" else -1
            V = _tiles(xp, pad + off + pp, pad + off + qq, 2, TH, TW, dtype)
            M += np.einsum("bcyxrs,ocrs->boyxrs", V, U)
    y = _untile(M, dtype)[:, :, :Ho, :Wo]
    return y if bias is None else y + np.asarray(bias, dtype)[None, :, None, None]


def up_taps(w64, py, px, wrong=None):
    """The phase's 2x2 taps [O][C][2][2], summed in float64."""
    if wrong == "unsummed_taps":
        rows = [[0], [1]] if py == 0 else [[1], [2]]
        cols = [[0], [1]] if px == 0 else [[1], [2]]
    else:
        rows = [[0], [1, 2]] if py == 0 else [[0, 1], [2]]
        cols = [[0], [1, 2]] if px == 0 else [[0, 1], [2]]
    g = np.zeros(w64.shape[:2] + (2, 2))
    for a in range(2):
        for b in range(2):
            g[:, :, a, b] = w64[:, :, rows[a], :][:, :, :, cols[b]].sum(axis=(2, 3))
    return g


def poly_up(x, w, bias=None, dtype=np.float64, wrong=None):
    x = np.asarray(x, dtype)
    w64 = np.asarray(w, np.float64)
    B, C, H, W = x.shape
    TH, TW = (H + 3) // 4, (W + 3) // 4
    pad = 2
    xp = np.zeros((B, C, pad + 4 * TH + 4, pad + 4 * TW + 4), dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, w64.shape[0], 2 * H, 2 * W), dtype)
    for py in range(2):
        for px in range(2):
            U = _weights(up_taps(w64, py, px, wrong), dtype, wrong)
            pp, qq = (1 - py, 1 - px) if wrong == "swapped_parity" else (py, px)
            off = 0 if wrong == "no_offset" else -1
            V = _tiles(xp, pad + off + pp, pad + off + qq, 1, TH, TW, dtype)
            M = np.einsum("bcyxrs,ocrs->boyxrs", V, U)
            y[:, :, py::2, px::2] = _untile(M, dtype)[:, :, :H, :W]
    return y if bias is None else y + np.asarray(bias, dtype)[None, :, None, None]
