"""Float64 restatement of CNAFNetLocal, the latent ConditionalNAFNet with TLSC local pooling (test infrastructure).

codes/config/latent-dehazing/models/modules/DenoisingNAFNet_arch.py:190-200 + local_arch.py: every NAFBlock's
`sca.0 = AdaptiveAvgPool2d(1)` becomes the mean over a K0 x K1 window, K frozen per block by one forward at the training size,
replicate-padded back to the map.  `naf_block` is `oracle.naf_block` with that one line swapped; everything else -- time MLP,
zero pad, PixelShuffle skips, `ending(x + intro(x))`, crop -- is `oracle.irsde_oracle`'s.  The window sums are formed directly in
float64 (a sliding-window view), not as the reference's difference of fp32 prefix sums.
"""
import numpy as np

from oracle import irsde_oracle as O

ARCH = dict(enc_blk_nums=(1, 1), middle_blk_num=1, dec_blk_nums=(1, 1))
# name -> (width, train_size).  Width 16 is the reference-side configuration of the host tests; the engine's smallest width is 32
# (irsde_create_nafnet: "width must be a positive multiple of 32"), so the GPU tests run the w32 twins: same depth, same train sizes,
# hence the same windows -- 24 / 12 / 6 (even: asymmetric pads) and 30x18 / 15x9 / 7x4 (odd, non-square).
NETS = {"w16_t16": (16, (1, 3, 16, 16)), "w16_t20x12": (16, (1, 3, 20, 12)),
        "w32_t16": (32, (1, 3, 16, 16)), "w32_t20x12": (32, (1, 3, 20, 12))}
WINDOWS = {(1, 3, 16, 16): [(24, 24), (12, 12), (6, 6)], (1, 3, 20, 12): [(30, 18), (15, 9), (7, 4)]}
SCA_GAIN = 32.0   # sca.1.weight of every block is scaled by this: the pooled statistics then steer the block (see `synth_params`)
TS = (1, 7, 20)
# golden forwards: tag -> (net, B, H, W, timesteps, stored stride)
FORWARD = {"w32_t16_1x40x56": ("w32_t16", 1, 40, 56, TS, 1),          # local on both axes at every level
           "w32_t16_1x37x50": ("w32_t16", 1, 37, 50, (7,), 1),        # ragged: zero pad to 40 x 52
           "w32_t16_1x20x56": ("w32_t16", 1, 20, 56, (7,), 1),        # level-0 rows covered (24 >= 20), columns local
           "w32_t16_1x16x16": ("w32_t16", 1, 16, 16, (7,), 1),        # everything covered
           "w32_t16_1x96x128": ("w32_t16", 1, 96, 128, (7,), 2),      # drift check of the window sums (every second pixel stored)
           "w32_t20x12_1x40x56": ("w32_t20x12", 1, 40, 56, TS, 1),
           "w32_t20x12_1x37x50": ("w32_t20x12", 1, 37, 50, (7,), 1),
           "w16_t16_1x40x56": ("w16_t16", 1, 40, 56, (7,), 1),
           "w16_t16_1x20x56": ("w16_t16", 1, 20, 56, (7,), 1),
           "w16_t20x12_1x37x50": ("w16_t20x12", 1, 37, 50, (7,), 1)}
SAMPLER = ("w32_t16", 1, 37, 50, 20)   # net, B, H, W, T: IRSDE(max_sigma 50, T 20, cosine, eps 0.005), injected noise seed 7


def cfg_of(name):
    return dict(width=NETS[name][0], **ARCH)


def windows(train_size, n_enc=2):
    """(K0, K1) per level 0 .. n_enc: what the conversion forward on rand(train_size) freezes (local_arch.py:26-32)."""
    _, _, H, W = train_size
    base = (int(H * 1.5), int(W * 1.5))
    P = 2 ** n_enc
    Hp, Wp = (H + P - 1) // P * P, (W + P - 1) // P * P
    return [((Hp >> l) * base[0] // H, (Wp >> l) * base[1] // W) for l in range(n_enc + 1)]


def synth_params(name, seed=0):
    """`oracle.naf_synth_params` (beta / gamma ~ U(-0.5, 0.5), never zero) with every sca.1.weight scaled by SCA_GAIN: with the
    plain U(+-1/sqrt(c)) weights sca.1's bias dominates the scale vector and the pooled statistics barely matter."""
    p = O.naf_synth_params(seed=seed, img_channel=3, **cfg_of(name))
    for k in p:
        if k.endswith("sca.1.weight"):
            p[k] = (p[k] * np.float32(SCA_GAIN)).astype(np.float32)
    return p


def inputs(B, H, W, seed=1234):
    """(cond, xt) with spatial structure: 8 x 8 blocks of random level, a diagonal ramp and noise (statistics that differ between windows)."""
    rs = np.random.RandomState(seed)
    blocks = rs.uniform(0, 1, size=(B, 3, (H + 7) // 8, (W + 7) // 8))
    img = np.repeat(np.repeat(blocks, 8, axis=2), 8, axis=3)[:, :, :H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (yy / max(H - 1, 1) + xx / max(W - 1, 1)) / 2
    cond = (0.6 * img + 0.3 * ramp[None, None] + 0.1 * rs.uniform(0, 1, size=(B, 3, H, W))).astype(np.float32)
    xt = (cond + rs.standard_normal((B, 3, H, W)).astype(np.float32) * np.float32(50 / 255)).astype(np.float32)
    return cond, xt


def local_pool(x, K):
    """AvgPool2d.forward of local_arch.py:25-72 (fast_imp=False, auto_pad=True) on [B, c, h, w]."""
    h, w = x.shape[2:]
    if K[0] >= h and K[1] >= w:
        return x.mean(axis=(2, 3), keepdims=True)
    k1, k2 = min(h, K[0]), min(w, K[1])
    m = np.lib.stride_tricks.sliding_window_view(x, (k1, k2), axis=(2, 3)).mean(axis=(-2, -1))   # [B, c, h - k1 + 1, w - k2 + 1]
    top, left = (k1 - 1) // 2, (k2 - 1) // 2
    iy = np.clip(np.arange(h) - top, 0, h - k1)
    ix = np.clip(np.arange(w) - left, 0, w - k2)
    return m[:, :, iy][:, :, :, ix]


def naf_block(p, pre, x, temb, K):
    """NAFBlock.forward (DenoisingNAFNet_arch.py:56-84) with sca.0 = the local pool of window K (None: the global mean)."""
    half = temb.shape[1] // 2
    tt = O.linear(temb[:, :half] * temb[:, half:], p[pre + "mlp.1.weight"], p[pre + "mlp.1.bias"])[:, :, None, None]
    c = x.shape[1]
    shift_att, scale_att, shift_ffn, scale_ffn = (tt[:, i * c:(i + 1) * c] for i in range(4))
    inp = x
    x = O.layer_norm_c(inp, p[pre + "norm1.g"])
    x = x * (scale_att + 1) + shift_att
    x = O.conv2d(x, p[pre + "conv1.weight"], p[pre + "conv1.bias"])
    x = O._dwconv3x3(x, p[pre + "conv2.weight"], p[pre + "conv2.bias"])
    x = O._simple_gate(x)
    pooled = x.mean(axis=(2, 3), keepdims=True) if K is None else local_pool(x, K)
    x = x * O.conv2d(pooled, p[pre + "sca.1.weight"], p[pre + "sca.1.bias"])
    x = O.conv2d(x, p[pre + "conv3.weight"], p[pre + "conv3.bias"])
    y = inp + x * p[pre + "beta"]
    x = O.layer_norm_c(y, p[pre + "norm2.g"])
    x = x * (scale_ffn + 1) + shift_ffn
    x = O.conv2d(x, p[pre + "conv4.weight"], p[pre + "conv4.bias"])
    x = O._simple_gate(x)
    x = O.conv2d(x, p[pre + "conv5.weight"], p[pre + "conv5.bias"])
    return y + x * p[pre + "gamma"]


def forward(params, xt, cond, t, train_size, dtype=np.float64, taps=None, local=True):
    """CNAFNetLocal.forward(inp, cond, time); local=False: the plain latent ConditionalNAFNet (global pools) on the same weights."""
    enc, mid, dec = ARCH["enc_blk_nums"], ARCH["middle_blk_num"], ARCH["dec_blk_nums"]
    Ks = windows(train_size, len(enc)) if local else [None] * (len(enc) + 1)
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    xt, cond = np.asarray(xt, dtype=dtype), np.asarray(cond, dtype=dtype)
    x = np.concatenate([xt - cond, cond], axis=1)
    temb, _ = O.naf_embeddings(p, t, None, dtype)
    B, C, H, W = x.shape
    ps = 2 ** len(enc)
    x = np.pad(x, ((0, 0), (0, 0), (0, (ps - H % ps) % ps), (0, (ps - W % ps) % ps)))
    x = O.conv2d(x, p["intro.weight"], p["intro.bias"], pad=1)

    def tap(name, v):
        if taps is not None:
            taps[name] = v

    tap("intro", x)
    intro = x
    encs = []
    for i, num in enumerate(enc):
        for j in range(num):
            x = naf_block(p, "encoders.%d.%d." % (i, j), x, temb, Ks[i])
        tap("encoders.%d" % i, x)
        encs.append(x)
        x = O.conv2d(x, p["downs.%d.weight" % i], p["downs.%d.bias" % i], stride=2, pad=0)
        tap("downs.%d" % i, x)
    for j in range(mid):
        x = naf_block(p, "middle_blks.%d." % j, x, temb, Ks[len(enc)])
    tap("middle", x)
    for i, num in enumerate(dec):
        x = O._pixel_shuffle2(O.conv2d(x, p["ups.%d.0.weight" % i]))
        x = x + encs[len(encs) - 1 - i]
        tap("ups.%d" % i, x)
        for j in range(num):
            x = naf_block(p, "decoders.%d.%d." % (i, j), x, temb, Ks[len(enc) - 1 - i])
        tap("decoders.%d" % i, x)
    x = O.conv2d(x + intro, p["ending.weight"], p["ending.bias"], pad=1)
    return np.ascontiguousarray(x[..., :H, :W])
