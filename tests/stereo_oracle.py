"""Float64 numpy restatement of the stereo-sr ConditionalNAFNet (SCAM after every NAFBlock) and its synthetic weights.

Test helper (not collected by pytest): codes/config/stereo-sr/models/modules/DenoisingNAFNet_arch.py restated on top of
oracle.irsde_oracle's NAFBlock (`naf_block`) and time embedding (`naf_embeddings`).
    SCAM      :15-60
    forward   :199-240 (views stacked on the batch axis [L_0..L_{B-1}, R_0..R_{B-1}], time duplicated likewise)
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import irsde_oracle as O  # noqa: E402

SCAM_PROJ1_GAIN = 4.0   # l_proj1 / r_proj1 ~ U(+-4 / sqrt(c)): scores span several units, so a wrong softmax moves the output visibly


def scam_param_shapes(base_shapes):
    """The SCAM tensors of every NAFBlock found in `base_shapes` (names of oracle.irsde_oracle.naf_param_shapes)."""
    sh = {}
    for name, shp in base_shapes.items():
        if name.endswith("norm1.g"):
            pre, c = name[:-len("norm1.g")] + "fusion.", shp[1]
            sh[pre + "norm_l.g"] = (1, c, 1, 1)
            sh[pre + "norm_r.g"] = (1, c, 1, 1)
            for pr in ("l_proj1.", "r_proj1.", "l_proj2.", "r_proj2."):
                sh[pre + pr + "weight"] = (c, c, 1, 1)
                sh[pre + pr + "bias"] = (c,)
            sh[pre + "beta"] = (1, c, 1, 1)
            sh[pre + "gamma"] = (1, c, 1, 1)
    return sh


def stereo_param_shapes(img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=(1, 1), dec_blk_nums=(1, 1)):
    base = O.naf_param_shapes(img_channel=img_channel, width=width, middle_blk_num=middle_blk_num, enc_blk_nums=tuple(enc_blk_nums),
                              dec_blk_nums=tuple(dec_blk_nums))
    base.update(scam_param_shapes(base))
    return base


def stereo_synth_params(seed=0, img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=(1, 1), dec_blk_nums=(1, 1)):
    """O.naf_synth_params(seed, ...) plus the SCAM tensors (own stream, seed + 1000): beta / gamma ~ U(-0.5, 0.5), LayerNorm gains
    ~ U(0.5, 1.5), *_proj1 ~ U(+-SCAM_PROJ1_GAIN / sqrt(c)), *_proj2 and every bias ~ U(+-1 / sqrt(c))."""
    cfg = dict(img_channel=img_channel, width=width, middle_blk_num=middle_blk_num, enc_blk_nums=tuple(enc_blk_nums), dec_blk_nums=tuple(dec_blk_nums))
    out = O.naf_synth_params(seed=seed, **cfg)
    rs = np.random.RandomState(seed + 1000)
    sh = scam_param_shapes(O.naf_param_shapes(**cfg))
    for name in sorted(sh):
        shp = sh[name]
        if name.endswith(".g"):
            a = rs.uniform(0.5, 1.5, size=shp)
        elif name.endswith("beta") or name.endswith("gamma"):
            a = rs.uniform(-0.5, 0.5, size=shp)
        else:
            c = shp[0]
            bound = (SCAM_PROJ1_GAIN if "_proj1.weight" in name else 1.0) / math.sqrt(c)
            a = rs.uniform(-bound, bound, size=shp)
        out[name] = a.astype(np.float32)
    return out


def bicubic_quarter(x):
    """F.interpolate(x, scale_factor=0.25, mode='bicubic'): output o samples at 4 o + 1.5 -> the separable 4-tap filter
    [-3, 19, 19, -3] / 32 over rows / columns 4 o .. 4 o + 3 (no clamping); size floor(H / 4) x floor(W / 4)."""
    B, C, H, W = x.shape
    Hs, Ws = H // 4, W // 4
    w = np.array([-3.0, 19.0, 19.0, -3.0]) / 32.0
    t = x[:, :, :4 * Hs, :4 * Ws].reshape(B, C, Hs, 4, Ws, 4)
    return np.einsum("bchiwj,i,j->bchw", t, w, w)


def nearest_index(n_out, n_in):
    """PyTorch's nearest source index for F.interpolate(size=...): min(floor(dst * (float)in / out), in - 1) in float32."""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def nearest_resize(x, H, W):
    return x[:, :, nearest_index(H, x.shape[2])][:, :, :, nearest_index(W, x.shape[3])]


def scam(p, pre, x, uniform=False):
    """SCAM.forward (:33-60) on x [2B, c, H, W] (float64); pre = '<block path>.fusion.'.  uniform=True replaces both softmaxes by
    plain averages (the sensitivity check of the fixture)."""
    c = x.shape[1]
    x_l, x_r = np.split(x, 2, axis=0)
    x_ls, x_rs = bicubic_quarter(x_l), bicubic_quarter(x_r)

    def proj(name, v):
        return O.conv2d(v, p[pre + name + ".weight"], p[pre + name + ".bias"])

    Q_l = proj("l_proj1", O.layer_norm_c(x_ls, p[pre + "norm_l.g"])).transpose(0, 2, 3, 1)   # B, H', W', c
    Q_r = proj("r_proj1", O.layer_norm_c(x_rs, p[pre + "norm_r.g"])).transpose(0, 2, 3, 1)
    V_l = proj("l_proj2", x_ls).transpose(0, 2, 3, 1)
    V_r = proj("r_proj2", x_rs).transpose(0, 2, 3, 1)
    S = np.einsum("bhik,bhjk->bhij", Q_l, Q_r) * c ** -0.5

    def softmax(a):
        if uniform:
            return np.full_like(a, 1.0 / a.shape[-1])
        e = np.exp(a - a.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    F_r2l = np.einsum("bhij,bhjc->bhic", softmax(S), V_r).transpose(0, 3, 1, 2) * p[pre + "beta"]
    F_l2r = np.einsum("bhji,bhic->bhjc", softmax(S.transpose(0, 1, 3, 2)), V_l).transpose(0, 3, 1, 2) * p[pre + "gamma"]
    H, W = x.shape[2:]
    return np.concatenate([x_l + nearest_resize(F_r2l, H, W), x_r + nearest_resize(F_l2r, H, W)], axis=0)


def stereo_forward(params, inp, cond, t, enc_blk_nums=(1, 1), middle_blk_num=1, dec_blk_nums=(1, 1), taps=None, uniform=False):
    """ConditionalNAFNet.forward (:199-240) in float64.  t: int (shared by every pair) or [B] values.  taps (dict): for every block,
    '<path>.fusion.in' (SCAM input) and '<path>' (block output), [2B, c, H, W]."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    inp, cond = np.asarray(inp, np.float64), np.asarray(cond, np.float64)
    ic = inp.shape[1] // 2
    xl = np.concatenate([inp[:, :ic] - cond[:, :ic], cond[:, :ic]], axis=1)
    xr = np.concatenate([inp[:, ic:] - cond[:, ic:], cond[:, ic:]], axis=1)
    x = np.concatenate([xl, xr], axis=0)
    tv = np.atleast_1d(np.asarray(t, dtype=np.int64))
    temb, _ = O.naf_embeddings(p, np.concatenate([tv, tv]) if tv.size > 1 else tv, None, np.float64)
    B2, C, H, W = x.shape
    ps = 2 ** len(enc_blk_nums)
    x = np.pad(x, ((0, 0), (0, 0), (0, (ps - H % ps) % ps), (0, (ps - W % ps) % ps)))
    x = O.conv2d(x, p["intro.weight"], p["intro.bias"], pad=1)

    def block(path, x):
        y = O.naf_block(p, path + ".", x, temb)
        z = scam(p, path + ".fusion.", y, uniform)
        if taps is not None:
            taps[path + ".fusion.in"] = y
            taps[path] = z
        return z

    encs = []
    for i, num in enumerate(enc_blk_nums):
        for j in range(num):
            x = block("encoders.%d.%d" % (i, j), x)
        encs.append(x)
        x = O.conv2d(x, p["downs.%d.weight" % i], p["downs.%d.bias" % i], stride=2)
    for j in range(middle_blk_num):
        x = block("middle_blks.%d" % j, x)
    for i, num in enumerate(dec_blk_nums):
        x = O._pixel_shuffle2(O.conv2d(x, p["ups.%d.0.weight" % i])) + encs[len(encs) - 1 - i]
        for j in range(num):
            x = block("decoders.%d.%d" % (i, j), x)
    x = O.conv2d(x, p["ending.weight"], p["ending.bias"], pad=1)[..., :H, :W]
    x_l, x_r = np.split(x, 2, axis=0)
    return np.ascontiguousarray(np.concatenate([x_l, x_r], axis=1))
