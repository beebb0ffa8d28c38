"""float64 numpy restatement of the two degradation kernels (csrc/degrade.hip), for tests/test_degrade_host.py and tests/test_gpu_degrade.py.

`upscale` restates PyTorch's `F.interpolate(x, scale_factor=s, mode='bicubic')` (codes/utils/deg_utils.py:38-40) from its rules:
output o samples at src = (o + 0.5) / s - 0.5, i0 = floor(src), t = src - i0; the taps i0 - 1 .. i0 + 2 carry the cubic-convolution
weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with A = -0.75 and are clamped to the image (src is not); separable; no clamp of the result.
Each keyword switches ONE rule to a plausible wrong one — the mutation checks of test_degrade_host.py use them.

`mask_to` restates deg_utils.py:30-34 in the reference's own precisions: mask = float32(m8 / 255.) resized by PyTorch's nearest index
min(floor(dst * float32(in / out)), in - 1), then fp32 mask * x, fp32 1 - mask, fp32 add.
"""
import numpy as np

# (B, C, H, W, scale): odd sizes, one-row and two-column images (every tap clamps), H != W, s = 2 / 3 / 4
SHAPES = [(2, 3, 5, 7, 4), (1, 3, 1, 9, 4), (1, 3, 13, 2, 2), (2, 1, 6, 11, 3), (1, 3, 9, 33, 4)]


def cubic_weights(t, A=-0.75):
    """[..., 4] weights of the taps i0 - 1 .. i0 + 2 at fraction t."""
    t = np.asarray(t, dtype=np.float64)

    def c1(x):   # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def c2(x):   # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

    return np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], axis=-1)


def axis_taps(n_in, s, A=-0.75, align_corners=False, clamp_src=False, reverse_taps=False):
    """(idx [n_in s][4] unclamped tap indices, w [n_in s][4]) of one axis."""
    n_out = n_in * s
    o = np.arange(n_out, dtype=np.float64)
    if align_corners:
        src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros_like(o)
    else:
        src = (o + 0.5) / s - 0.5
    if clamp_src:
        src = np.maximum(src, 0.0)
    i0 = np.floor(src)
    w = cubic_weights(src - i0, A)
    if reverse_taps:
        w = w[:, ::-1]
    return i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], w


def phase_table(s, A=-0.75):
    """The s x 4 table the kernel builds: weights of output phase p = o mod s."""
    idx, w = axis_taps(4, s, A)
    return w[s:2 * s]


def upscale(x, s, A=-0.75, align_corners=False, zero_pad=False, clamp_src=False, swap_tables=False, reverse_taps=False):
    """x: [B, C, H, W] -> float64 [B, C, H s, W s]."""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    kw = dict(A=A, align_corners=align_corners, clamp_src=clamp_src, reverse_taps=reverse_taps)
    ri, rw = axis_taps(H, s, **kw)     # [Ho][4]
    ci, cw = axis_taps(W, s, **kw)     # [Wo][4]
    Ho, Wo = H * s, W * s
    # per output pixel: row taps [Ho][Wo][4], column taps [Ho][Wo][4]
    RI = np.broadcast_to(ri[:, None, :], (Ho, Wo, 4))
    RW = np.broadcast_to(rw[:, None, :], (Ho, Wo, 4))
    CI = np.broadcast_to(ci[None, :, :], (Ho, Wo, 4))
    CW = np.broadcast_to(cw[None, :, :], (Ho, Wo, 4))
    if swap_tables:   # the row filter indexed with the column's phase and the other way round (positions i = o // s stay)
        ph_r = (np.arange(Wo) % s)[None, :] + np.zeros((Ho, 1), dtype=np.int64)
        ph_c = (np.arange(Ho) % s)[:, None] + np.zeros((1, Wo), dtype=np.int64)
        bi, bw = axis_taps(4, s, **dict(kw, align_corners=False))
        di, dw = bi[s:2 * s] - 1, bw[s:2 * s]   # taps relative to i = o // s, per phase
        RI = (np.arange(Ho) // s)[:, None, None] + di[ph_r]
        RW = dw[ph_r]
        CI = (np.arange(Wo) // s)[None, :, None] + di[ph_c]
        CW = dw[ph_c]
    out = np.zeros(x.shape[:-2] + (Ho, Wo))
    for k in range(4):
        r = RI[..., k]
        rv = np.ones_like(r, dtype=np.float64) if not zero_pad else ((r >= 0) & (r < H)).astype(np.float64)
        r = np.clip(r, 0, H - 1)
        for l in range(4):
            c = CI[..., l]
            cv = np.ones_like(c, dtype=np.float64) if not zero_pad else ((c >= 0) & (c < W)).astype(np.float64)
            c = np.clip(c, 0, W - 1)
            out += (RW[..., k] * rv) * (CW[..., l] * cv) * x[..., r, c]
    return out


def nearest_index(n_out, n_in):
    """PyTorch's nearest source index, in float32 arithmetic: min(floor(dst * float32(in / out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def mask_to(x, m8):
    """x: float32 [B, C, H, W]; m8: uint8 [Bm, Hm, Wm, Cm] (Bm in {1, B}, Cm in {1, C}) -> float32 [B, C, H, W]."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    m = (np.asarray(m8).astype(np.float64) / 255.0).astype(np.float32)            # / 255. in float64, .float()
    m = m[:, nearest_index(H, m.shape[1])][:, :, nearest_index(W, m.shape[2])]    # nearest resize
    m = np.broadcast_to(m.transpose(0, 3, 1, 2), x.shape)
    return (m * x).astype(np.float32) + (np.float32(1.0) - m).astype(np.float32)
