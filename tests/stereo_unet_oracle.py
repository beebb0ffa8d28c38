"""Float64 numpy restatement of the stereo-sr ConditionalUNet (a full-resolution SCAM on every level) and its synthetic weights.

Test helper (not collected by pytest): codes/config/stereo-sr/models/modules/DenoisingUNet_arch.py restated on top of
oracle.irsde_oracle's ResBlock (`res_block`), LinearAttention block (`attn_block`), convolution and time embedding.
    SCAM      :18-56   (no downsample / upsample: one W x W score matrix per image row of the level's map)
    forward   :136-196 (views stacked on the batch axis [L_0..L_{B-1}, R_0..R_{B-1}], time duplicated likewise; output xt + cat(x_l, x_r))
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import irsde_oracle as O  # noqa: E402

# The reference initialises beta / gamma to zero and its default scores are flat, so the synthetic SCAM tensors follow tests/stereo_oracle.py:
# beta / gamma ~ U(+-0.5) and l_proj1 / r_proj1 ~ U(+-gain / sqrt(c)).  The gains were tuned on the CPU against the reference until its output
# moves by >= 1 % of max |out| when both softmaxes are replaced by plain averages (tools/gen_stereo_unet_golden.py asserts it).  The output is
# a residual on the state, which hides the attention: proj1 gain alone saturates at 0.5 % (gain 8: 0.21 %, 16: 0.45 %, 128: 0.53 %, one-hot
# softmaxes), so the value projections l_proj2 / r_proj2 carry a gain too (proj1 / proj2 = 8 / 3: 0.6 %, 8 / 4: 1.1 %, 16 / 4: 2.5 %).  8 / 4 is
# kept: with proj1 gain 16 the scores are so sharp that the fp32 reference's own rounding reaches 3e-6 of a SCAM increment, above the 1e-6 its
# hooked SCAMs are compared at (8 / 4: 4e-7).
SCAM_PROJ1_GAIN = 8.0
SCAM_PROJ2_GAIN = 4.0


def scam_shapes(pre, c):
    sh = {pre + "norm_l.g": (1, c, 1, 1), pre + "norm_r.g": (1, c, 1, 1), pre + "beta": (1, c, 1, 1), pre + "gamma": (1, c, 1, 1)}
    for pr in ("l_proj1.", "r_proj1.", "l_proj2.", "r_proj2."):
        sh[pre + pr + "weight"] = (c, c, 1, 1)
        sh[pre + pr + "bias"] = (c,)
    return sh


def stereo_unet_param_shapes(in_nc=3, out_nc=3, nf=32, depth=2):
    """Names / shapes of the reference state_dict: the deraining UNet's with init_conv 3x3, a SCAM at index 3 of every level (the
    down / up-sample moves to index 4) and mid_fusion."""
    base = O.unet_param_shapes(in_nc, out_nc, nf, depth)
    sh = {}
    for name, shp in base.items():
        parts = name.split(".")
        if parts[0] in ("downs", "ups") and parts[2] == "3":
            parts[2] = "4"
        sh[".".join(parts)] = shp
    sh["init_conv.weight"] = (nf, 2 * in_nc, 3, 3)
    for i in range(depth):
        sh.update(scam_shapes("downs.%d.3." % i, nf * 2 ** i))
        sh.update(scam_shapes("ups.%d.3." % (depth - 1 - i), nf * 2 ** (i + 1)))
    sh.update(scam_shapes("mid_fusion.", nf * 2 ** depth))
    return sh


def stereo_unet_synth_params(seed=0, in_nc=3, out_nc=3, nf=32, depth=2, proj1_gain=None, proj2_gain=None):
    """Seeded weights (numpy legacy RandomState): conv / linear tensors ~ U(+-1 / sqrt(fan_in)), LayerNorm gains ~ U(0.5, 1.5); the SCAM
    tensors: beta / gamma ~ U(-0.5, 0.5), *_proj1 weights ~ U(+-SCAM_PROJ1_GAIN / sqrt(c)), *_proj2 weights ~ U(+-SCAM_PROJ2_GAIN / sqrt(c))."""
    rs = np.random.RandomState(seed)
    shapes = stereo_unet_param_shapes(in_nc, out_nc, nf, depth)
    g1 = SCAM_PROJ1_GAIN if proj1_gain is None else proj1_gain
    g2 = SCAM_PROJ2_GAIN if proj2_gain is None else proj2_gain
    out = {}
    for name in sorted(shapes):
        shp = shapes[name]
        if name.endswith(".g"):
            a = rs.uniform(0.5, 1.5, size=shp)
        elif name.endswith(".beta") or name.endswith(".gamma"):
            a = rs.uniform(-0.5, 0.5, size=shp)
        else:
            wshape = shapes[name[:-4] + "weight"] if name.endswith("bias") else shp
            bound = (g1 if "_proj1.weight" in name else g2 if "_proj2.weight" in name else 1.0) / math.sqrt(int(np.prod(wshape[1:])))
            a = rs.uniform(-bound, bound, size=shp)
        out[name] = a.astype(np.float32)
    return out


def scam_full(p, prefix, x, uniform=False):
    """SCAM.forward (:37-56) on x [2B, c, H, W] (float64).  uniform=True replaces both softmaxes by plain averages (the sensitivity
    check of the fixture)."""
    x = np.asarray(x, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in p.items() if k.startswith(prefix)}
    c = x.shape[1]
    x_l, x_r = np.split(x, 2, axis=0)

    def proj(name, v):
        return O.conv2d(v, p[prefix + name + ".weight"], p[prefix + name + ".bias"])

    Q_l = proj("l_proj1", O.layer_norm_c(x_l, p[prefix + "norm_l.g"])).transpose(0, 2, 3, 1)   # B, H, W, c
    Q_r = proj("r_proj1", O.layer_norm_c(x_r, p[prefix + "norm_r.g"])).transpose(0, 2, 3, 1)
    V_l = proj("l_proj2", x_l).transpose(0, 2, 3, 1)
    V_r = proj("r_proj2", x_r).transpose(0, 2, 3, 1)
    S = np.einsum("bhik,bhjk->bhij", Q_l, Q_r) * c ** -0.5

    def softmax(a):
        if uniform:
            return np.full_like(a, 1.0 / a.shape[-1])
        e = np.exp(a - a.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    F_r2l = np.einsum("bhij,bhjc->bhic", softmax(S), V_r).transpose(0, 3, 1, 2) * p[prefix + "beta"]
    F_l2r = np.einsum("bhji,bhic->bhjc", softmax(S.transpose(0, 1, 3, 2)), V_l).transpose(0, 3, 1, 2) * p[prefix + "gamma"]
    return np.concatenate([x_l + F_r2l, x_r + F_l2r], axis=0)


def stereo_unet_forward(params, xt, cond, t, depth=2, taps=None, uniform=False):
    """ConditionalUNet.forward (:136-196) in float64.  t: int (shared by every pair) or [B] values.  taps (dict): '<name>.in' / '<name>' for
    every SCAM (downs.i.3, mid_fusion, ups.j.3), [2B, c, H, W]."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    xt, cond = np.asarray(xt, np.float64), np.asarray(cond, np.float64)
    ic = xt.shape[1] // 2
    xl = np.concatenate([xt[:, :ic], cond[:, :ic]], axis=1)
    xr = np.concatenate([xt[:, ic:], cond[:, ic:]], axis=1)
    x = np.concatenate([xl, xr], axis=0)
    tv = np.atleast_1d(np.asarray(t, dtype=np.int64))
    tv = np.concatenate([tv, tv]) if tv.size > 1 else tv
    H, W = x.shape[2:]
    s = 2 ** depth
    x = np.pad(x, ((0, 0), (0, 0), (0, (s - H % s) % s), (0, (s - W % s) % s)), mode="reflect")
    x = O.conv2d(x, p["init_conv.weight"], pad=1)
    x_ = x
    nf = p["init_conv.weight"].shape[0]
    temb = O.sinusoidal_pos_emb(tv, nf, np.float64)
    temb = O.linear(temb, p["time_mlp.1.weight"], p["time_mlp.1.bias"])
    temb = O.linear(O.gelu(temb), p["time_mlp.3.weight"], p["time_mlp.3.bias"])

    def fusion(name, v):
        z = scam_full(p, name + ".", v, uniform)
        if taps is not None:
            taps[name + ".in"] = v
            taps[name] = z
        return z

    h = []
    for i in range(depth):
        x = O.res_block(p, "downs.%d.0." % i, x, temb)
        h.append(x)
        x = O.res_block(p, "downs.%d.1." % i, x, temb)
        x = O.attn_block(p, "downs.%d.2." % i, x)
        x = fusion("downs.%d.3" % i, x)
        h.append(x)
        if i != depth - 1:
            x = O.conv2d(x, p["downs.%d.4.weight" % i], p["downs.%d.4.bias" % i], stride=2, pad=1)
        else:
            x = O.conv2d(x, p["downs.%d.4.weight" % i], pad=1)
    x = O.res_block(p, "mid_block1.", x, temb)
    x = O.attn_block(p, "mid_attn.", x)
    x = fusion("mid_fusion", x)
    x = O.res_block(p, "mid_block2.", x, temb)
    for j in range(depth):
        x = O.res_block(p, "ups.%d.0." % j, np.concatenate([x, h.pop()], axis=1), temb)
        x = O.res_block(p, "ups.%d.1." % j, np.concatenate([x, h.pop()], axis=1), temb)
        x = O.attn_block(p, "ups.%d.2." % j, x)
        x = fusion("ups.%d.3" % j, x)
        if j != depth - 1:
            x = O.conv2d(O.upsample_nearest2(x), p["ups.%d.4.1.weight" % j], p["ups.%d.4.1.bias" % j], pad=1)
        else:
            x = O.conv2d(x, p["ups.%d.4.weight" % j], pad=1)
    x = O.res_block(p, "final_res_block.", np.concatenate([x, x_], axis=1), temb)
    x = O.conv2d(x, p["final_conv.weight"], p["final_conv.bias"], pad=1)[..., :H, :W]
    x_l, x_r = np.split(x, 2, axis=0)
    return np.ascontiguousarray(xt + np.concatenate([x_l, x_r], axis=1))
