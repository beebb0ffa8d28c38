"""Seeded inputs, case lists and a float64 numpy restatement of `imresize` (codes/data/util.py:238-387; degradations.imresize,
csrc/degrade.hip imresize_kernel), for tests/test_imresize_host.py, tests/test_gpu_imresize.py and tools/gen_imresize_golden.py.

The restatement builds the per-axis filter tables from the rules (in the reference's float32, see `tables`) and applies them in float64 to the
symmetric extension of the image:
output x = 1..n_out (n_out = ceil(n_in scale)) is centred at u = x / scale + 0.5 (1 - 1 / scale); the kernel is 4 wide, or 4 / scale with
antialiasing below scale 1; the candidate taps are the P = ceil(width) + 2 pixels from floor(u - width / 2), weighted with the Keys cubic
(a = -0.5) of their distance (antialiasing: scale cubic(distance scale)) and divided by the row's sum; the outer pair of columns is dropped if
the first holds a zero, else the last two if the last holds one; a tap at 0-based p < 0 reads pixel -p - 1, at p >= n pixel 2 n - 1 - p.
Each keyword of `tables` / `imresize` switches ONE rule to a plausible wrong one — the mutation checks of test_imresize_host.py use them.
"""
import math

import numpy as np

# the scales and axis lengths whose reference tables tests/golden/imresize.npz holds (key "tab/<scale index>/<0|1 antialiasing>/<n_in>/...")
SCALES = [1 / 2, 1 / 3, 1 / 4, 1 / 8, 0.3, 0.75, 1.0]
TABLE_N = [7, 9, 10, 21, 33, 40, 131]
ACCEPT_N = list(range(2, 41))   # "accept/<scale index>/<0|1>": the reference's verdict for these axis lengths

# (B, C, H, W, scale, antialiasing): the reference's fp32 outputs are golden "out/<index>"
SHAPES = [
    (2, 3, 40, 136, 1 / 4, True),    # several tiles on both axes; Wo = 34: no 16-byte stores
    (1, 3, 37, 131, 1 / 4, True),    # sizes that are no multiple of 4; Wo = 33
    (1, 1, 7, 7, 1 / 4, True),       # smallest accepted size: both reflections inside one filter
    (2, 3, 21, 70, 1 / 2, True),
    (1, 2, 30, 100, 1 / 3, True),    # odd factor: one exact-zero tap
    (1, 3, 96, 264, 1 / 8, True),    # K = 32
    (1, 3, 33, 47, 0.3, True),       # per-output weights; K = 14
    (1, 3, 9, 10, 1.0, True),
    (1, 3, 18, 67, 1 / 2, False),
    (1, 3, 31, 45, 0.3, False),
    (1, 3, 16, 128, 1 / 4, True),    # Wo = 32: the 16-byte store path
]


def inputs(index):
    """The fp32 input [B, C, H, W] of SHAPES[index]: U(0, 1) noise on a coarse checker of 0 / 1 blocks, so that edges overshoot."""
    B, C, H, W = SHAPES[index][:4]
    rng = np.random.default_rng(1000 + index)
    x = rng.random((B, C, H, W), dtype=np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    checker = (((yy // 5) + (xx // 7)) % 2).astype(np.float32)
    return np.ascontiguousarray((np.float32(0.5) * x + np.float32(0.5) * checker[None, None]).astype(np.float32))


def cubic(d):
    """The Keys cubic (a = -0.5) in the precision of `d`."""
    a = np.abs(d)
    one, two = a.dtype.type(1), a.dtype.type(2)
    a2, a3 = a * a, a * a * a
    near = a.dtype.type(1.5) * a3 - a.dtype.type(2.5) * a2 + one
    far = a.dtype.type(-0.5) * a3 + a.dtype.type(2.5) * a2 - a.dtype.type(4) * a + two
    return near * (a <= one).astype(a.dtype) + far * ((a > one) & (a <= two)).astype(a.dtype)


def tables(n_in, scale, antialiasing=True, *, dtype=np.float32, no_normalise=False, no_half_shift=False, ignore_antialiasing=False,
           skip_start_narrowing=False):
    """(weights float64 [n_out][K], start int64 [n_out]) of one axis; start is the 0-based coordinate of the first tap.

    The coordinates and weights are formed in `dtype`, float32 by default, because the filter the reference applies IS its float32 table: at
    u near 150 the fp32 rounding of u alone moves a weight of the 4-wide kernel by 5e-6 of its value (dtype=np.float64 gives the exact-rule
    table; on the shapes above the two differ by up to 4.6e-6 of max|ref| without antialiasing and 8e-7 with it).  What is done with the table
    afterwards is float64.
    no_normalise: rows not divided by their sum.  no_half_shift: u = x / scale.  ignore_antialiasing: the 4-wide kernel at every scale.
    skip_start_narrowing: the weights lose their first column and the coordinates do not (every tap one pixel to the left)."""
    f = np.dtype(dtype).type
    n_out = math.ceil(n_in * scale)
    widen = scale < 1 and antialiasing and not ignore_antialiasing
    width = 4.0 / scale if widen else 4.0
    x = np.arange(1, n_out + 1).astype(dtype)
    u = x / f(scale)
    if not no_half_shift:
        u = u + f(0.5 * (1.0 - 1.0 / scale))
    left = np.floor(u - f(width / 2.0))
    P = math.ceil(width) + 2
    idx = left[:, None] + np.arange(P).astype(dtype)[None, :]
    d = u[:, None] - idx
    w = f(scale) * cubic(d * f(scale)) if widen else cubic(d)
    if not no_normalise:
        w = w / w.sum(1, dtype=dtype, keepdims=True)
    if np.any(w[:, 0] == 0):
        w = w[:, 1:P - 1]
        idx = idx[:, 0:P - 2] if skip_start_narrowing else idx[:, 1:P - 1]
    elif np.any(w[:, -1] == 0):
        w, idx = w[:, :P - 2], idx[:, :P - 2]
    return w.astype(np.float64), idx[:, 0].astype(np.int64) - 1


def extend(p, n, *, clamp=False, no_edge_repeat=False):
    """Image coordinate a tap at 0-based p reads.  clamp: the edge pixel instead of the symmetric extension.  no_edge_repeat: reflection about
    the edge pixel's centre (p = -1 reads pixel 1), which does not repeat the edge pixel."""
    p = np.asarray(p, dtype=np.int64)
    if clamp:
        return np.clip(p, 0, n - 1)
    if no_edge_repeat:
        q = np.where(p < 0, -p, p)
        q = np.where(q >= n, 2 * n - 2 - q, q)
    else:
        q = np.where(p < 0, -p - 1, p)
        q = np.where(q >= n, 2 * n - 1 - q, q)
    return np.clip(q, 0, n - 1)


def apply_axis(x, w, start, axis, **border):
    """Filter float64 `x` along `axis` with the table (w, start)."""
    n = x.shape[axis]
    K = w.shape[1]
    src = extend(start[:, None] + np.arange(K)[None, :], n, **border)   # [n_out][K]
    xm = np.moveaxis(x, axis, -1)
    out = np.zeros(xm.shape[:-1] + (w.shape[0],))
    for k in range(K):
        out += xm[..., src[:, k]] * w[:, k]
    return np.moveaxis(out, -1, axis)


def imresize(x, scale, antialiasing=True, *, clamp=False, no_edge_repeat=False, **table_rules):
    """x: [..., H, W] -> float64 [..., ceil(H scale), ceil(W scale)]; the H axis first, as the reference (in float64 the order is immaterial)."""
    x = np.asarray(x, dtype=np.float64)
    border = dict(clamp=clamp, no_edge_repeat=no_edge_repeat)
    wH, sH = tables(x.shape[-2], scale, antialiasing, **table_rules)
    wW, sW = tables(x.shape[-1], scale, antialiasing, **table_rules)
    return apply_axis(apply_axis(x, wH, sH, -2, **border), wW, sW, -1, **border)


MUTATIONS = [dict(clamp=True), dict(no_edge_repeat=True), dict(no_normalise=True), dict(no_half_shift=True), dict(ignore_antialiasing=True),
             dict(skip_start_narrowing=True)]
