"""Float64 restatement of the 'fp16_act' compute mode of the image-space ConditionalNAFNets (test infrastructure).

IRSDE_FLAG_F16_ACT = the 'fp16' operand mode (`oracle.irsde_oracle.f16_convs`: the operands of every conv2d rounded to IEEE fp16) plus fp16 storage of every
activation tensor between kernels.  This file restates `O.naf_block` / `O.nafnet_forward` (and the unconditional `dsde_naf_oracle.forward`) operation by
operation and puts `O.round_f16` at exactly the engine's stores:

    intro output | per block: conv1's output u, the gated depthwise output, y = x + conv3(.) beta, the gated conv4 output, the block output |
    downs outputs | ups outputs after pixel-shuffle and skip add

Two details of the contract: the SCA pooled mean is taken from the products BEFORE the store rounding, and conv3's operand is round_f16(stored x sca)
(the multiplication by the fp32 scale happens on the stored tensor; the conv's operand rounding does the rest).  The LayerNorm + FiLM output needs no
rounding of its own: its only reader is a conv that rounds it to fp16 anyway.  The prepped input, the FiLM rows, the pooled mean, the SCA vector and
eps_hat are never rounded.

`store=False` switches every storage rounding off; the result is then `O.nafnet_forward` / `dsde_naf_oracle.forward` under `O.f16_convs()` bit for bit
(tests/test_naf_f16act_host.py pins that).  `mut` selects one deliberately wrong reference (the host test's mutation-sensitivity check).
"""
import numpy as np

from oracle import irsde_oracle as O

MUTATIONS = ("no_sca", "swap_gate", "no_beta", "no_skip", "shuffle_transposed", "pool_zeroed_tile", "no_film_shift")

# (width, enc, mid, dec, B, H, W): the shapes of tests/test_gpu_naf_f16act.py
CASES = {
    "w64": (64, (1, 1), 1, (1, 1), 3, 36, 52),     # c = 64 / 128 / 256: the one-piece-K kernels; 5616 / 1404 / 351 pixels, deepest map 13 wide
    "w32": (32, (1, 1), 1, (1, 1), 3, 36, 52),     # c = 32 / 64 / 128: level 0 on the LayerNorm kernel + the implicit GEMM
    "w256": (256, (1, 1), 1, (1, 1), 1, 16, 24),   # c = 256 / 512 / 1024: long K, split-K, residual + ch_scale and in_scale in the implicit GEMM
}


def _st(x, store):
    return O.round_f16(x) if store else x


def _gate(x, mut):
    c = x.shape[1] // 2
    if mut == "swap_gate":   # (the product commutes: a swapped pairing shows as the wrong partner, half a block away)
        return x[:, :c] * np.roll(x[:, c:], c // 2, axis=1)
    return x[:, :c] * x[:, c:]


def naf_block(p, pre, x, temb, store=True, mut=None):
    """`O.naf_block` (NAFBlock.forward, DenoisingNAFNet_arch.py:56-82) with the mode's storage roundings; x is a stored tensor."""
    half = temb.shape[1] // 2
    tt = O.linear(temb[:, :half] * temb[:, half:], p[pre + "mlp.1.weight"], p[pre + "mlp.1.bias"])[:, :, None, None]
    c = x.shape[1]
    shift_att, scale_att, shift_ffn, scale_ffn = (tt[:, i * c:(i + 1) * c] for i in range(4))
    if mut == "no_film_shift":
        shift_att, shift_ffn = shift_att * 0, shift_ffn * 0
    inp = x
    x = O.layer_norm_c(inp, p[pre + "norm1.g"])
    x = x * (scale_att + 1) + shift_att
    x = _st(O.conv2d(x, p[pre + "conv1.weight"], p[pre + "conv1.bias"]), store)                    # u
    x = O._dwconv3x3(x, p[pre + "conv2.weight"], p[pre + "conv2.bias"])
    x = _gate(x, mut)
    if mut == "pool_zeroed_tile":   # one tile of the deterministic two-stage pool (4 image rows) missing from the sum
        z = x.copy()
        z[:, :, :4, :] = 0
        pooled = z.mean(axis=(2, 3), keepdims=True)
    else:
        pooled = x.mean(axis=(2, 3), keepdims=True)                                                # before the store rounding
    x = _st(x, store)                                                                              # the gated depthwise output
    sca = O.conv2d(pooled, p[pre + "sca.1.weight"], p[pre + "sca.1.bias"])
    if mut != "no_sca":
        x = x * sca                                                                                # conv3 rounds the product: round_f16(stored x sca)
    x = O.conv2d(x, p[pre + "conv3.weight"], p[pre + "conv3.bias"])
    y = _st(inp + x * p[pre + "beta"], store) if mut != "no_beta" else _st(inp + x, store)
    x = O.layer_norm_c(y, p[pre + "norm2.g"])
    x = x * (scale_ffn + 1) + shift_ffn
    x = O.conv2d(x, p[pre + "conv4.weight"], p[pre + "conv4.bias"])
    x = _st(_gate(x, mut), store)                                                                  # the gated conv4 output
    x = O.conv2d(x, p[pre + "conv5.weight"], p[pre + "conv5.bias"])
    return _st(y + x * p[pre + "gamma"], store)                                                    # the block output


def _shuffle(x, mut):
    if mut != "shuffle_transposed":
        return O._pixel_shuffle2(x)
    B, C, H, W = x.shape   # dy / dx transposed: channel block (dy, dx) lands at (2y + dx, 2x + dy)
    x = x.reshape(B, C // 4, 2, 2, H, W).transpose(0, 1, 4, 3, 5, 2)
    return np.ascontiguousarray(x.reshape(B, C // 4, 2 * H, 2 * W))


# The network between two taps, as functions of the previous STORED tensor: what the GPU test restarts from the engine's own taps
def down(p, i, x, store=True):
    return _st(O.conv2d(x, p["downs.%d.weight" % i], p["downs.%d.bias" % i], stride=2, pad=0), store)


def up(p, i, x, skip, store=True, mut=None):
    x = _shuffle(O.conv2d(x, p["ups.%d.0.weight" % i]), mut)
    return _st(x if mut == "no_skip" else x + skip, store)


def level(p, path, num, x, temb, store=True, mut=None):
    for j in range(num):
        x = naf_block(p, "%s.%d." % (path, j), x, temb, store, mut)
    return x


def forward(params, x, t, enc_blk_nums, middle_blk_num, dec_blk_nums, cond=None, store=True, mut=None, taps=None, dtype=np.float64):
    """The 'fp16_act' forward under `O.f16_convs()`: cond given = ConditionalNAFNet.forward(xt, cond, time) (`O.nafnet_forward`), cond None = the
    denoising-sde network's forward(x, time) (`dsde_naf_oracle.forward`)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    x = np.asarray(x, dtype=dtype)
    if cond is not None:
        cond = np.asarray(cond, dtype=dtype)
        x = np.concatenate([x - cond, cond], axis=1)
    temb, _ = O.naf_embeddings(p, t, None, dtype)
    B, C, H, W = x.shape
    ps = 2 ** len(enc_blk_nums)
    x = np.pad(x, ((0, 0), (0, 0), (0, (ps - H % ps) % ps), (0, (ps - W % ps) % ps)))
    with O.f16_convs():
        x = _st(O.conv2d(x, p["intro.weight"], p["intro.bias"], pad=1), store)

        def tap(name, v):
            if taps is not None:
                taps[name] = v

        tap("intro", x)
        encs = []
        for i, num in enumerate(enc_blk_nums):
            x = level(p, "encoders.%d" % i, num, x, temb, store, mut)
            tap("encoders.%d" % i, x)
            encs.append(x)
            x = down(p, i, x, store)
            tap("downs.%d" % i, x)
        x = level(p, "middle_blks", middle_blk_num, x, temb, store, mut)
        tap("middle", x)
        for i, num in enumerate(dec_blk_nums):
            x = up(p, i, x, encs[len(encs) - 1 - i], store, mut)
            tap("ups.%d" % i, x)
            x = level(p, "decoders.%d" % i, num, x, temb, store, mut)
            tap("decoders.%d" % i, x)
        x = O.conv2d(x, p["ending.weight"], p["ending.bias"], pad=1)   # eps_hat: fp32 in the engine
    return np.ascontiguousarray(x[..., :H, :W])


def restart_taps(params, got, t, enc_blk_nums, middle_blk_num, dec_blk_nums, mut=None, dtype=np.float64):
    """Every tap after `intro` recomputed from the PREVIOUS tap(s) in `got` (the engine's own stored tensors, or another reference's): {name: expected}."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    g = {k: np.asarray(v, dtype=dtype) for k, v in got.items()}
    temb, _ = O.naf_embeddings(p, t, None, dtype)
    want = {}
    with O.f16_convs():
        prev = "intro"
        for i, num in enumerate(enc_blk_nums):
            want["encoders.%d" % i] = level(p, "encoders.%d" % i, num, g[prev], temb, True, mut)
            want["downs.%d" % i] = down(p, i, g["encoders.%d" % i])
            prev = "downs.%d" % i
        want["middle"] = level(p, "middle_blks", middle_blk_num, g[prev], temb, True, mut)
        prev = "middle"
        n = len(enc_blk_nums)
        for i, num in enumerate(dec_blk_nums):
            want["ups.%d" % i] = up(p, i, g[prev], g["encoders.%d" % (n - 1 - i)], True, mut)
            want["decoders.%d" % i] = level(p, "decoders.%d" % i, num, g["ups.%d" % i], temb, True, mut)
            prev = "decoders.%d" % i
    return want


def make_params(width, enc, mid, dec, seed, uncond=False, sca_gain=8.0):
    """Synthetic weights of the tests: `O.naf_synth_params` (unconditional: `dsde_naf_oracle.synth_params`) with beta / gamma ~ 0.5 N(0, 1), as
    test_naf_chain_blocks_vs_oracle does, and sca.1.weight scaled up so that the SCA branch carries weight (the default pooled products are small next to
    sca.1.bias)."""
    cfg = dict(width=width, enc_blk_nums=tuple(enc), middle_blk_num=mid, dec_blk_nums=tuple(dec))
    if uncond:
        import dsde_naf_oracle as DN
        bp = DN.synth_params(seed=seed, img_channel=3, **cfg)
    else:
        bp = O.naf_synth_params(seed=seed, img_channel=3, **cfg)
    rs = np.random.RandomState(1000 + seed)
    for k in sorted(bp):
        if k.endswith(".beta") or k.endswith(".gamma"):
            bp[k] = (0.5 * rs.standard_normal(bp[k].shape)).astype(np.float32)
        elif k.endswith("sca.1.weight"):
            bp[k] = (bp[k] * np.float32(sca_gain)).astype(np.float32)
    return bp


def make_inputs(B, H, W, seed, uncond=False):
    rs = np.random.RandomState(seed)
    xt = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    cond = None if uncond else rs.standard_normal((B, 3, H, W)).astype(np.float32)
    return xt, cond


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())
