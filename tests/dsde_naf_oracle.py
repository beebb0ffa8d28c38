"""Float64 restatement of the denoising-sde ConditionalNAFNet (test infrastructure).

codes/config/denoising-sde/models/modules/DenoisingNAFNet_arch.py differs from the deraining file in four lines: `intro`
takes `img_channel` inputs (:103) and `forward(x, time)` has no condition (:147-150): no `cat(x - cond, cond)`.  Everything
else -- time MLP, zero pad to `padder_size`, NAFBlocks, PixelShuffle skips, crop -- is `oracle.irsde_oracle`'s.
"""
import math

import numpy as np

from oracle import irsde_oracle as O

CFGS = {"refusion": dict(width=64, enc_blk_nums=(1, 1, 1, 28), middle_blk_num=1, dec_blk_nums=(1, 1, 1, 1)),
        "w32_e12": dict(width=32, enc_blk_nums=(1, 2), middle_blk_num=1, dec_blk_nums=(1, 1))}
# tag -> (config, B, H, W) of the forward fixtures; (config, B, H, W, max_sigma, T, sigma) of the sampler fixtures
FORWARD = {"w32_e12_2x22x19": ("w32_e12", 2, 22, 19), "refusion_1x40x56": ("refusion", 1, 40, 56)}
SAMPLER = {"w32_e12_2x22x19": ("w32_e12", 2, 22, 19, 50, 100, 25), "refusion_1x32x32": ("refusion", 1, 32, 32, 70, 1000, 15)}


def param_shapes(img_channel=3, **cfg):
    sh = O.naf_param_shapes(img_channel=img_channel, **cfg)
    sh["intro.weight"] = (cfg["width"], img_channel, 3, 3)
    return sh


def synth_params(seed=0, img_channel=3, **cfg):
    """`oracle.naf_synth_params` with intro.weight replaced by a seeded [width, img_channel, 3, 3] tensor of the same scale
    (U(+-1 / sqrt(fan_in)))."""
    p = O.naf_synth_params(seed=seed, img_channel=img_channel, **cfg)
    bound = 1.0 / math.sqrt(img_channel * 9)
    rs = np.random.RandomState(seed + 7919)
    p["intro.weight"] = rs.uniform(-bound, bound, size=(cfg["width"], img_channel, 3, 3)).astype(np.float32)
    return p


def inputs(B, H, W, sigma=25, seed=1234):
    """(clean, noisy = clean + sigma / 255 * z): the clean image is `oracle.synth_inputs`' LQ, z a seeded normal draw."""
    clean, _ = O.synth_inputs(seed, B, H, W)
    z = np.random.RandomState(5).standard_normal(clean.shape).astype(np.float32)
    return clean, (clean + z * np.float32(sigma / 255)).astype(np.float32)


def forward(params, x, t, enc_blk_nums, middle_blk_num, dec_blk_nums, dtype=np.float64, taps=None):
    """ConditionalNAFNet.forward(x, time) -- denoising-sde DenoisingNAFNet_arch.py:147-183."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    x = np.asarray(x, dtype=dtype)
    temb, _ = O.naf_embeddings(p, t, None, dtype)
    B, C, H, W = x.shape
    ps = 2 ** len(enc_blk_nums)
    x = np.pad(x, ((0, 0), (0, 0), (0, (ps - H % ps) % ps), (0, (ps - W % ps) % ps)))  # zero pad (check_image_size)
    x = O.conv2d(x, p["intro.weight"], p["intro.bias"], pad=1)

    def tap(name, v):
        if taps is not None:
            taps[name] = v

    tap("intro", x)
    encs = []
    for i, num in enumerate(enc_blk_nums):
        for j in range(num):
            x = O.naf_block(p, "encoders.%d.%d." % (i, j), x, temb)
        tap("encoders.%d" % i, x)
        encs.append(x)
        x = O.conv2d(x, p["downs.%d.weight" % i], p["downs.%d.bias" % i], stride=2, pad=0)
        tap("downs.%d" % i, x)
    for j in range(middle_blk_num):
        x = O.naf_block(p, "middle_blks.%d." % j, x, temb)
    tap("middle", x)
    for i, num in enumerate(dec_blk_nums):
        x = O._pixel_shuffle2(O.conv2d(x, p["ups.%d.0.weight" % i]))
        x = x + encs[len(encs) - 1 - i]
        tap("ups.%d" % i, x)
        for j in range(num):
            x = O.naf_block(p, "decoders.%d.%d." % (i, j), x, temb)
        tap("decoders.%d" % i, x)
    x = O.conv2d(x, p["ending.weight"], p["ending.bias"], pad=1)
    return np.ascontiguousarray(x[..., :H, :W])


def sample(params, sch, xT, ode, T, cfg, noise=None, dtype=np.float64):
    """DenoisingSDE.reverse_sde / reverse_ode (sde_utils.py:488-528) around `forward`, with injected noise."""
    x = np.asarray(xT, dtype=dtype).copy()
    for t in range(T, 0, -1):
        eps_hat = forward(params, x, t, cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"], dtype=dtype)
        x = O.dsde_reverse_step(sch, x, eps_hat, None if ode else noise[t], t, ode, dtype)
    return x
