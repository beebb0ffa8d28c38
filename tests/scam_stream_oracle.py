"""Streaming SCAM core (csrc/scam_stream.hip), host side: a float32 numpy emulation of the kernel's blocked online-softmax order with the
mutations the tests must be able to see, the kernel-level shapes, and the weights of the wide fixtures.

Test helper (not collected by pytest).  The float64 references stay tests/stereo_unet_oracle.py (`scam_full`) and tests/stereo_oracle.py (`scam`).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import irsde_oracle as O  # noqa: E402
import stereo_oracle as SO  # noqa: E402
import stereo_unet_oracle as SU  # noqa: E402

FLAG_SCAM_STREAM = 2097152
MAX_BLOCK_W = 512        # kScamStreamMaxBlockW (csrc/common.h); block_w = 0 selects it
HOOK_PROJ1_GAIN = 4.0    # the kernel-level gain of tests/test_gpu_stereo_unet.py, whose 1e-5 bar the streaming tests take over

# (pairs, H, W, c, block_w) through irsde_debug_scam_full_stream
STREAM_SHAPES = [(1, 3, 1, 32, 16), (2, 5, 10, 64, 16), (1, 4, 16, 256, 16), (1, 2, 17, 32, 16), (3, 3, 40, 1024, 16), (1, 2, 130, 64, 64),
                 (1, 2, 509, 128, 256), (1, 1, 1040, 32, 0), (1, 1, 2064, 64, 0)]
C2048_SHAPE = (1, 1, 20, 2048, 16)
MUTATIONS = ("stale_max", "acc_not_rescaled", "l_not_rescaled", "tail_unmasked", "alpha_neighbour_row", "directions_swapped", "boundary_off_16")

# The wide UNet fixtures (tests/golden/stereo_wide.npz): at the gains of tests/stereo_unet_oracle.py (proj1 8, proj2 4) a softmax over ~1030 columns
# moves the output by 0.54 % (small) / 0.40 % (full) of max |out| when it is replaced by a plain average, below the 1 % the fixtures must show.  The value
# projections carry gain 8 instead (2.3 % / 2.1 %); the query gain, and with it the sharpness of the scores and the fp32 rounding of the reference, stays.
WIDE_UNET_GAINS = dict(proj1_gain=8.0, proj2_gain=8.0)
UNET_SMALL = dict(nf=32, depth=2)
UNET_FULL = dict(nf=64, depth=4)
NAF_SMALL = dict(width=32, enc_blk_nums=(1, 1), middle_blk_num=1, dec_blk_nums=(1, 1))


def stereo_inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


def wide_unet_params(cfg):
    return SU.stereo_unet_synth_params(seed=0, **cfg, **WIDE_UNET_GAINS)


def naf_params():
    return SO.stereo_synth_params(seed=0, img_channel=3, **NAF_SMALL)


def scam_weights(c, seed, tie_proj1=False, pre="f."):
    """The hook weights of tests/test_gpu_stereo_unet.py::scam_weights (same draws in the same order)."""
    rs = np.random.RandomState(seed)
    p = {}
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


def shape_input(B, H, W, c):
    return np.random.RandomState(B * 1000 + W).standard_normal((2 * B, c, H, W)).astype(np.float32)


_CASES = {}


def case(shape):
    """(x, weights, float64 SCAM output) of one kernel shape (pairs, H, W, c, block_w), computed once per session and never modified."""
    if shape not in _CASES:
        B, H, W, c, _ = shape
        x = shape_input(B, H, W, c)
        p = scam_weights(c, seed=W + c)
        want = SU.scam_full(p, "f.", x)
        for a in (x, want):
            a.setflags(write=False)
        _CASES[shape] = (x, p, want)
    return _CASES[shape]


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def increment_err(x, want, got):
    """Error of a SCAM output relative to max |SCAM increment| (the attention part, not the residual that dominates the output)."""
    return relerr(np.asarray(got, np.float64) - x, np.asarray(want, np.float64) - x)


def queries(p, x, pre="f."):
    """float64 Q_l, Q_r [B, H, W, c] of the full-resolution SCAM on x [2B, c, H, W]."""
    d = {k: np.asarray(v, np.float64) for k, v in p.items()}
    xl, xr = np.split(np.asarray(x, np.float64), 2, axis=0)
    ql = O.conv2d(O.layer_norm_c(xl, d[pre + "norm_l.g"]), d[pre + "l_proj1.weight"], d[pre + "l_proj1.bias"]).transpose(0, 2, 3, 1)
    qr = O.conv2d(O.layer_norm_c(xr, d[pre + "norm_r.g"]), d[pre + "r_proj1.weight"], d[pre + "r_proj1.bias"]).transpose(0, 2, 3, 1)
    return ql, qr


def _stream_rows(q_own, q_oth, v_oth, bw, scale, mutation):
    """One direction of one image row in the kernel's order, float32: q_own / q_oth [W, c], v_oth [W, c] -> F [W, c]."""
    f32 = np.float32
    W, c = q_own.shape
    Wt = (W + 15) // 16 * 16
    qo = np.zeros((Wt, c), f32)
    qo[:W] = q_own                      # padding rows of the last strip: zero operands, results never stored
    qt = np.zeros((Wt + bw + 16, c), f32)
    qt[:W] = q_oth
    vt = np.zeros((Wt + bw + 16, c), f32)
    vt[:W] = v_oth
    m = np.zeros(Wt, f32)
    l = np.zeros(Wt, f32)
    acc = np.zeros((Wt, c), f32)
    nbr = np.arange(Wt) // 16 * 16 + (np.arange(Wt) % 16 + 1) % 16   # the next row of the same 16-row strip
    for blk, j0 in enumerate(range(0, W, bw)):
        nb = min(bw, W - j0)
        nbt = (nb + 15) // 16 * 16
        if mutation == "boundary_off_16" and blk > 0:
            j0 += 16
            nb = max(min(nb, W - j0), 0)
        S = (qo @ qt[j0:j0 + nbt].T).astype(f32) * f32(scale)
        valid = np.arange(nbt) < nb
        nsum = nbt if mutation == "tail_unmasked" else nb
        counted = np.arange(nbt) < nsum
        mb = S[:, valid].max(axis=1) if nb > 0 else np.full(Wt, -np.inf, f32)
        if blk == 0:
            m_new, alpha = mb, np.zeros(Wt, f32)
        else:
            m_new = np.maximum(m, mb)
            alpha = np.exp(m - m_new).astype(f32)
        m_exp = m if (mutation == "stale_max" and blk > 0) else m_new
        Pm = np.where(counted[None, :], np.exp(S - m_exp[:, None]), 0).astype(f32)
        a_use = alpha[nbr] if mutation == "alpha_neighbour_row" else alpha
        l = (l if mutation == "l_not_rescaled" else l * a_use).astype(f32) + Pm.sum(axis=1, dtype=f32)
        acc = (acc if mutation == "acc_not_rescaled" else acc * a_use[:, None]).astype(f32) + (Pm @ vt[j0:j0 + nbt]).astype(f32)
        m = m_new
    return (acc * (f32(1) / l)[:, None])[:W].astype(f32)


def emulate_stream(p, x, block_w, mutation=None, pre="f.", quarter=False):
    """The SCAM output on x [2B, c, H, W] with the core in the streaming kernel's order: float32 statistics and products, column blocks of
    block_w (0: the default), running maximum, alpha = 0 in the first block, accumulators and l rescaled per block, F = acc / l.  Prologue,
    projections and epilogue are taken in float64 and rounded to float32 where the kernels store them.  quarter=True: the NAFNet form
    (bicubic quarter-downsample before, nearest upsample after).  mutation: one of MUTATIONS, what a wrong kernel would compute."""
    assert mutation is None or mutation in MUTATIONS, mutation
    d = {k: np.asarray(v, np.float64) for k, v in p.items() if k.startswith(pre)}
    x64 = np.asarray(x, np.float64)
    c = x64.shape[1]
    xl, xr = np.split(x64, 2, axis=0)
    sl, sr = (SO.bicubic_quarter(xl), SO.bicubic_quarter(xr)) if quarter else (xl, xr)

    def proj(name, v):
        return O.conv2d(v, d[pre + name + ".weight"], d[pre + name + ".bias"]).transpose(0, 2, 3, 1).astype(np.float32)   # B, H', W', c

    Ql, Qr = proj("l_proj1", O.layer_norm_c(sl, d[pre + "norm_l.g"])), proj("r_proj1", O.layer_norm_c(sr, d[pre + "norm_r.g"]))
    Vl, Vr = proj("l_proj2", sl), proj("r_proj2", sr)
    B, Hs, Ws, _ = Ql.shape
    bw = min(block_w or MAX_BLOCK_W, (Ws + 15) // 16 * 16)
    Fl, Fr = np.zeros_like(Ql), np.zeros_like(Qr)
    for b in range(B):
        for h in range(Hs):
            Fl[b, h] = _stream_rows(Ql[b, h], Qr[b, h], Vr[b, h], bw, c ** -0.5, mutation)   # direction 0: F_r2l
            Fr[b, h] = _stream_rows(Qr[b, h], Ql[b, h], Vl[b, h], bw, c ** -0.5, mutation)   # direction 1: F_l2r
    if mutation == "directions_swapped":
        Fl, Fr = Fr, Fl
    Fl = Fl.transpose(0, 3, 1, 2).astype(np.float64) * d[pre + "beta"]
    Fr = Fr.transpose(0, 3, 1, 2).astype(np.float64) * d[pre + "gamma"]
    if quarter:
        H, W = x64.shape[2:]
        Fl, Fr = SO.nearest_resize(Fl, H, W), SO.nearest_resize(Fr, H, W)
    return np.concatenate([xl + Fl, xr + Fr], axis=0)
