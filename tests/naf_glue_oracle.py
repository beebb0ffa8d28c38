"""Float64 restatements of the NAFBlock glue stages that the kernel-level hooks of include/irsde_hip_debug.h run one at a time
(test infrastructure): conv2 + SimpleGate + SCA (irsde_debug_naf_gate_sca), TLSC pooling (irsde_debug_tlsc), channel LayerNorm + FiLM
(irsde_debug_ln_film) and the one-launch norm / scale + 1x1 convolution kernel (irsde_debug_naf_lnconv).

Every reference works on NCHW like oracle.irsde_oracle and returns, next to its tensors, the error bound its test asserts:
  gated   20 eps S1 S2, S_i = |bias_i| + sum |u| |w| over the 9 taps (9 fused multiply-adds per half, one product)
  mean    mean(bound(gated)) + n eps mean(|gated|), n = 4 run + PP + ceil(ntiles / 4) + 2: the longest addition chain of the pool
          (a lane's 4 rows x run columns, the PP lanes of a tile, a quarter of the tiles, the two-level join and the 1 / HW product)
  s       (c / 64 + 8) eps (|bias| + sum |W| |mean|) + sum |W| bound(mean)
  pooled  (k1 + k2 + 32) eps max |g|  (k - 1 additions of the direct sum, <= 14 roundings of 7 running updates, two passes, one scale)
  scaled  2 ulp of the product
with eps = 2^-24.  LayerNorm and the LayerNorm prologues of the convolution kernel round an fp32 result to fp16 (a legitimate 1-ulp flip):
their bar is 4 x the error of the same operation restated in numpy float32 against this float64 restatement on the test's own inputs,
capped by the project's bars (5e-5 / 1e-3 of max |ref|); the plain prologues round identical operands: 2e-5 (test_conv_kernel_fp16's).
`mut` selects one deliberately wrong variant of a reference (tests/test_naf_glue_host.py shows that each moves the metric >= 10 x its bar).
"""
import functools

import numpy as np

from oracle import irsde_oracle as O
import tlsc_oracle as TL

EPS = 2.0 ** -24

# (B, H, W, c) -> what the shape reaches (tests/test_naf_glue_host.py asserts each claim from the launch rule)
GATE_SHAPES = [(3, 10, 13, 32), (2, 7, 50, 64), (1, 5, 300, 32), (2, 4, 600, 32), (2, 6, 23, 96), (1, 5, 9, 384), (1, 6, 40, 1024),
               (1, 5, 6, 2048), (2, 264, 4, 1024)]
# (B, h, w, c, k1, k2)
TLSC_SHAPES = [(2, 9, 20, 32, 9, 5), (3, 11, 26, 32, 4, 9), (1, 40, 13, 64, 1, 1), (1, 17, 9, 32, 17, 9), (2, 7, 4, 1024, 3, 2),
               (1, 96, 128, 32, 48, 104)]
TLSC_OFFSET = {(1, 96, 128, 32, 48, 104): 100.0}   # long windows: the input offset at which cancellation in a running sum would show
# (B, ppi, C)
LN_SHAPES = [(3, 25, 32), (2, 7, 96), (1, 5, 160), (2, 3, 1024), (1, 9, 1536), (1, 3, 2048), (1, 16387, 1024)]
# (B, ppi, c, Cout, modes)
LNCONV_SHAPES = [(3, 25, 64, 128, (0, 1)), (2, 167, 128, 256, (0, 1)), (1, 64, 256, 512, (0, 1)),
                 (3, 25, 64, 64, (2, 3)), (2, 167, 128, 128, (2, 3)), (3, 25, 256, 256, (2, 3))]
LN_CAP, LNCONV_CAP, PWCONV_BAR = 5e-5, 1e-3, 2e-5
# LayerNorm inputs are N(50, 1) per pixel: a one-pass variance in fp32 then misses the LayerNorm bar 20 - 60 x.  Behind the fp16 rounding of the
# convolution kernel the same mistake moves the metric only 1.3 x its bar at std 1 (the bar is made of legitimate fp16 flips), so the inputs of the
# LayerNorm prologues (modes 0 / 1) keep the mean of 50 and narrow the spread until the one-pass variance misses by more than 10 x.
LNCONV_STD = 0.2


def f32(*a):
    return [np.ascontiguousarray(v, dtype=np.float32) for v in a]


def relerr(a, b):
    """max |a - b| / max |b|; inf where a holds a non-finite value."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if np.isfinite(a).all() else float("inf")


# ---------------------------------------------------------------------------------------------
# launch rules restated (the host test asserts the route of every GPU shape from these)
# ---------------------------------------------------------------------------------------------
def dw_geom(H, W, c):
    """csrc/kernels_misc.hip dw_geom (kDwRows = 4, kDwRun = 16): lanes per tile row PP, columns a lane walks, tiles."""
    G = c >> 2
    gpp = min(G, 256)
    PP = 256 // gpp
    run = min(max(-(-W // PP), 4), 16)
    tiles_x, tiles_y = -(-W // (PP * run)), -(-H // 4)
    return dict(G=G, gpp=gpp, PP=PP, run=run, tiles_x=tiles_x, tiles_y=tiles_y, ntiles=tiles_x * tiles_y, passes=-(-G // gpp))


def sca_two_kernel(ntiles, c):
    """csrc/kernels_misc.hip launch_sca: one launch while ntiles * c <= 65536 (and c <= 4096), else sca_mean_kernel + sca_kernel."""
    return not (ntiles * c <= 65536 and c <= 4096)


def ln_geom(M, C):
    """csrc/kernels_misc.hip launch_ln_t: lanes per pixel L, float4 per lane KV, pixel groups per iteration U, grid-stride trips."""
    L = 1
    while L * 2 <= 64 and L * 2 <= C // 4:
        L *= 2
    need = -(-(C // 4) // L)
    KV = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8
    U = 4 if need <= 2 else 2 if need <= 4 else 1
    ppw = 64 // L
    waves = -(-M // (ppw * U))
    blocks = max(1, min(-(-waves // 4), 256 * 8))
    return dict(L=L, KV=KV, U=U, idle=L * KV - C // 4, trips=-(-M // (blocks * 4 * ppw * U)))


def tlsc_geom(h, w, k1, k2):
    """csrc/tlsc_pool.hip: compact map, pads of the clamped gather, 8-output segments per axis (kTlscSeg)."""
    nh, nw = h - k1 + 1, w - k2 + 1
    seg = lambda n: [min(8, n - j) for j in range(0, n, 8)]
    return dict(nh=nh, nw=nw, top=(k1 - 1) // 2, bottom=k1 - 1 - (k1 - 1) // 2, left=(k2 - 1) // 2, segs_h=seg(nh), segs_w=seg(nw))


# ---------------------------------------------------------------------------------------------
# conv2 + SimpleGate + SCA
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_inputs(B, H, W, c):
    rs = np.random.RandomState(B * 100003 + H * 1009 + W * 31 + c)
    u = rs.standard_normal((B, 2 * c, H, W)) + rs.uniform(1, 2, (B, 2 * c, 1, 1))
    w = rs.uniform(-1 / 3, 1 / 3, (2 * c, 1, 3, 3))
    b = rs.uniform(-1 / 3, 1 / 3, (2 * c,))
    sw = rs.uniform(-4 / np.sqrt(c), 4 / np.sqrt(c), (c, c))
    sb = rs.uniform(-1 / np.sqrt(c), 1 / np.sqrt(c), (c,))
    return dict(zip(("u", "w", "b", "sw", "sb"), f32(u, w, b, sw, sb)))


GATE_MUTATIONS = ("drop_row", "drop_col", "padded_area", "image0", "replicate", "swap_bias")


def gate_mutation_applies(mut, B, H, W, c):
    g = dw_geom(H, W, c)
    if mut == "padded_area":   # identical to the reference where the tiles cover exactly H x W
        return g["tiles_y"] * 4 * g["tiles_x"] * g["PP"] * g["run"] != H * W
    return B > 1 if mut == "image0" else True


def gate_ref(inp, mut=None):
    """-> (ref, bound): dicts of gated [B, c, H, W], mean [B, c], s [B, c] in float64."""
    u, w, b, sw, sb = (inp[k].astype(np.float64) for k in ("u", "w", "b", "sw", "sb"))
    B, c2, H, W = u.shape
    c = c2 // 2
    g = dw_geom(H, W, c)
    if mut == "swap_bias":
        b = np.concatenate([b[c:], b[:c]])
    if mut == "replicate":
        v = O._dwconv3x3(np.pad(u, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge"), w, b)[:, :, 1:-1, 1:-1]
    else:
        v = O._dwconv3x3(u, w, b)
    gated = O._simple_gate(v)
    S = O._dwconv3x3(np.abs(u), np.abs(w), np.abs(b))
    bg = 20 * EPS * O._simple_gate(S)
    pool = gated[:, :, :-1] if mut == "drop_row" else gated[:, :, :, :-1] if mut == "drop_col" else gated
    area = g["tiles_y"] * 4 * g["tiles_x"] * g["PP"] * g["run"] if mut == "padded_area" else H * W
    mean = pool.sum(axis=(2, 3)) / area
    if mut == "image0":
        mean = np.repeat(mean[:1], B, axis=0)
    n = 4 * g["run"] + g["PP"] + -(-g["ntiles"] // 4) + 2
    bm = bg.mean(axis=(2, 3)) + n * EPS * np.abs(gated).mean(axis=(2, 3))
    s = mean @ sw.T + sb
    bs = (c / 64 + 8) * EPS * (np.abs(sb) + np.abs(mean) @ np.abs(sw).T) + bm @ np.abs(sw).T
    return dict(gated=gated, mean=mean, s=s), dict(gated=bg, mean=bm, s=bs)


def _fma32(a, b, acc):
    """fmaf on float32 arrays: the product of two floats is exact in float64; one rounding of the sum."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def gate_emulate_f32(inp):
    """The kernels' fp32 arithmetic in their summation order (dwconv_gate_kernel, sca_mean_kernel / sca_fused_kernel, sca_kernel)."""
    u, w, b, sw, sb = (inp[k] for k in ("u", "w", "b", "sw", "sb"))
    B, c2, H, W = u.shape
    c = c2 // 2
    g = dw_geom(H, W, c)
    up = np.pad(u, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(b.reshape(1, c2, 1, 1), u.shape).astype(np.float32)
    for ky in range(3):
        for kx in range(3):
            acc = _fma32(up[:, :, ky:ky + H, kx:kx + W], np.broadcast_to(w[:, 0, ky, kx].reshape(1, c2, 1, 1), u.shape), acc)
    gated = (acc[:, :c] * acc[:, c:]).astype(np.float32)
    PP, run = g["PP"], g["run"]
    partial = np.zeros((g["ntiles"], B, c), dtype=np.float32)
    for ty in range(g["tiles_y"]):
        for tx in range(g["tiles_x"]):
            lanes = np.zeros((PP, B, c), dtype=np.float32)
            for pl in range(PP):
                x0 = (tx * PP + pl) * run
                for x in range(x0, min(x0 + run, W)):
                    for y in range(ty * 4, min(ty * 4 + 4, H)):
                        lanes[pl] = lanes[pl] + gated[:, :, y, x]
            t = lanes[0]
            for q in range(1, PP):
                t = t + lanes[q]
            partial[ty * g["tiles_x"] + tx] = t
    t4 = np.zeros((4, B, c), dtype=np.float32)
    for q in range(g["ntiles"]):
        t4[q % 4] = t4[q % 4] + partial[q]
    mean = (((t4[0] + t4[1]) + (t4[2] + t4[3])) * np.float32(1.0 / np.float32(H * W))).astype(np.float32)
    lanes = np.zeros((64, B, c), dtype=np.float32)   # [lane][b][o]
    for k in range(c):
        lanes[k % 64] = _fma32(np.broadcast_to(sw[:, k], (B, c)), np.broadcast_to(mean[:, k:k + 1], (B, c)), lanes[k % 64])
    o = 32
    while o:
        lanes = lanes + lanes[np.arange(64) ^ o]
        o >>= 1
    return dict(gated=gated, mean=mean, s=(lanes[0] + sb).astype(np.float32))


# ---------------------------------------------------------------------------------------------
# TLSC
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tlsc_inputs(B, h, w, c, k1, k2):
    rs = np.random.RandomState(B * 100003 + h * 1009 + w * 31 + c + 7 * k1 + k2)
    off = TLSC_OFFSET.get((B, h, w, c, k1, k2), 0.0)
    g = rs.standard_normal((B, c, h, w)) + rs.uniform(1, 2, (B, c, 1, 1)) + off
    scale = rs.uniform(-2, 2, (B, c, h - k1 + 1, w - k2 + 1))
    return dict(zip(("g", "scale"), f32(g, scale)), k=(k1, k2))


TLSC_MUTATIONS = ("drop_row", "drop_col", "image0", "clamp")


def tlsc_mutation_applies(mut, B, h, w, c, k1, k2):
    if mut == "clamp":   # top = k1 / 2 differs from (k1 - 1) / 2 for even windows only (and only where there is something to gather)
        return (k1 % 2 == 0 and h > k1) or (k2 % 2 == 0 and w > k2)
    return B > 1 if mut == "image0" else True


def replicate_pad(m, h, w, k1, k2, top=None, left=None):
    """m [B, c, h - k1 + 1, w - k2 + 1] -> [B, c, h, w] by the clamped gather (local_arch.py's replicate pad: top (k1 - 1) // 2, left (k2 - 1) // 2)."""
    top = (k1 - 1) // 2 if top is None else top
    left = (k2 - 1) // 2 if left is None else left
    iy = np.clip(np.arange(h) - top, 0, h - k1)
    ix = np.clip(np.arange(w) - left, 0, w - k2)
    return m[:, :, iy][:, :, :, ix]


def tlsc_ref(inp, mut=None):
    """-> (ref, bound): pooled [B, c, nh, nw] and scaled [B, c, h, w] in float64."""
    g, scale = inp["g"].astype(np.float64), inp["scale"].astype(np.float64)
    k1, k2 = inp["k"]
    B, c, h, w = g.shape
    nh, nw = h - k1 + 1, w - k2 + 1
    padded = TL.local_pool(g, (k1, k2))
    top, left = (k1 - 1) // 2, (k2 - 1) // 2
    pooled = padded if (k1 >= h and k2 >= w) else padded[:, :, top:top + nh, left:left + nw]
    pooled = np.ascontiguousarray(pooled)
    if mut in ("drop_row", "drop_col"):   # every window loses its last row / column (the divisor stays k1 k2)
        win = np.lib.stride_tricks.sliding_window_view(g, (k1, k2), axis=(2, 3))
        last = win[..., -1, :].sum(axis=-1) if mut == "drop_row" else win[..., :, -1].sum(axis=-1)
        pooled = pooled - last / (k1 * k2)
    if mut == "image0":
        scale = np.repeat(scale[:1], B, axis=0)
    sp = replicate_pad(scale, h, w, k1, k2, *((k1 // 2, k2 // 2) if mut == "clamp" else ()))
    scaled = g * sp
    bound = dict(pooled=np.full(pooled.shape, (k1 + k2 + 32) * EPS * np.abs(g).max()),
                 scaled=2.0 * np.spacing(np.abs(scaled).astype(np.float32)).astype(np.float64))
    return dict(pooled=pooled, scaled=scaled), bound


def _axis_sum_f32(x, k, axis, scale):
    """tlsc_axis_sum_kernel along `axis`: direct sum of k at every 8th output, running add / subtract in between, times scale."""
    x = np.moveaxis(x, axis, 0)
    nout = x.shape[0] - k + 1
    out = np.empty((nout,) + x.shape[1:], dtype=np.float32)
    for j0 in range(0, nout, 8):
        acc = x[j0]
        for t in range(1, k):
            acc = acc + x[j0 + t]
        out[j0] = acc * np.float32(scale)
        for j in range(j0 + 1, min(j0 + 8, nout)):
            acc = (acc + x[j + k - 1]) - x[j - 1]
            out[j] = acc * np.float32(scale)
    return np.moveaxis(out, 0, axis)


def tlsc_emulate_f32(inp):
    k1, k2 = inp["k"]
    g = inp["g"]
    B, c, h, w = g.shape
    rows = _axis_sum_f32(g, k2, 3, 1.0)
    pooled = _axis_sum_f32(rows, k1, 2, np.float32(1.0) / (np.float32(k1) * np.float32(k2)))
    scaled = g * replicate_pad(inp["scale"], h, w, k1, k2)
    return dict(pooled=pooled, scaled=scaled.astype(np.float32))


# ---------------------------------------------------------------------------------------------
# LayerNorm + FiLM
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_inputs(B, ppi, C, mean=50.0):
    rs = np.random.RandomState(B * 100003 + ppi * 31 + C)
    x = rs.standard_normal((B, C, ppi, 1)).astype(np.float32) + np.float32(mean)
    g = rs.uniform(0.5, 1.5, (C,))
    fscale = 0.5 * rs.standard_normal((B, C))
    fshift = rs.standard_normal((B, C))
    return dict(zip(("x", "g", "fscale", "fshift"), f32(x, g, fscale, fshift)))


def _ln_one_pass_f32(x, g):
    """The wrong LayerNorm: var = E[x^2] - E[x]^2 in fp32."""
    x = x.astype(np.float32)
    m = x.mean(axis=1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(axis=1, keepdims=True, dtype=np.float32) - m * m
    return ((x - m) / np.sqrt(var + np.float32(1e-5)) * g.astype(np.float32)).astype(np.float64)


def ln_film(x, g, fscale, fshift, per_image, dtype=np.float64, mut=None):
    """LN(x) * g * (fscale + 1) + fshift on x [B, C, ppi, 1]; the FiLM row of image b is row b (per_image) or row 0."""
    B, C = x.shape[:2]
    x, g, fscale, fshift = (v.astype(dtype) for v in (x, g, fscale, fshift))
    y = _ln_one_pass_f32(x, g.reshape(1, C, 1, 1)).astype(dtype) if mut == "one_pass" else O.layer_norm_c(x, g.reshape(1, C, 1, 1))
    rows = np.arange(B) if per_image and mut != "image0" else np.zeros(B, dtype=int)
    return y * (fscale[rows].reshape(B, C, 1, 1) + dtype(1)) + fshift[rows].reshape(B, C, 1, 1)


def ln_ref(inp, per_image, mut=None):
    """-> (ref float64, bar): bar = min(4 x |float32 restatement - float64 restatement| / max |ref|, 5e-5)."""
    a = (inp["x"], inp["g"], inp["fscale"], inp["fshift"], per_image)
    ref = ln_film(*a)
    self_err = relerr(ln_film(*a, dtype=np.float32), ref)
    return (ln_film(*a, mut=mut) if mut else ref), min(4 * self_err, LN_CAP), self_err


LN_MUTATIONS = ("one_pass", "image0")


def ln_mutation_applies(mut, B, per_image):
    return (B > 1 and per_image) if mut == "image0" else True


# ---------------------------------------------------------------------------------------------
# naf_lnconv_kernel: LayerNorm + FiLM + 1x1 convolution (+ SimpleGate + lens FiLM) / scale + 1x1 convolution + residual
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lnconv_inputs(B, ppi, c, Cout, mode):
    rs = np.random.RandomState(B * 100003 + ppi * 31 + c * 7 + Cout + mode // 2)
    if mode <= 1:   # N(50, LNCONV_STD) per pixel (see LNCONV_STD)
        x = LNCONV_STD * rs.standard_normal((B, c, ppi, 1)) + 50.0
    else:
        x = rs.standard_normal((B, c, ppi, 1)) + rs.uniform(1, 2, (B, c, 1, 1))
    d = dict(x=x, w=rs.standard_normal((Cout, c, 1, 1)) / np.sqrt(c), bias=rs.standard_normal((Cout,)), g=rs.uniform(0.5, 1.5, (c,)),
             fscale=0.5 * rs.standard_normal((B, c)), fshift=rs.standard_normal((B, c)),
             lens=np.concatenate([0.5 * rs.standard_normal((B, Cout // 2)), rs.standard_normal((B, Cout // 2))], axis=1),
             in_scale=rs.uniform(-2, 2, (B, c)), ch_scale=rs.uniform(0.5, 1.5, (Cout,)) * rs.choice([-1.0, 1.0], (Cout,)),
             res=rs.standard_normal((B, Cout, ppi, 1)))
    return {k: f32(v)[0] for k, v in d.items()}


LNCONV_MUTATIONS = ("one_pass", "image0", "scale_before_bias")


def lnconv_mutation_applies(mut, B, mode, lens=False):
    if mut == "one_pass":
        return mode <= 1
    if mut == "image0":   # the FiLM row (modes 0 / 1), the lens row (mode 1) or the in_scale row (mode 2) of image 0 for every image
        return B > 1 and mode != 3
    return mode >= 2      # (acc * ch_scale + bias) instead of (acc + bias) * ch_scale


def lnconv(inp, mode, per_image=True, lens=False, dtype=np.float64, mut=None):
    """The kernel's operation on x [B, c, ppi, 1] -> [B, Cout or Cout / 2, ppi, 1]: the A operand is rounded to fp16 exactly where the kernel
    rounds it (after LayerNorm + FiLM in `dtype`, or after the fp32 product with in_scale), the weights are the engine's fp16 copy, and the
    products are accumulated wide (O.conv2d under O.f16_convs)."""
    B, c = inp["x"].shape[:2]
    w, bias = inp["w"].astype(np.float64), inp["bias"].astype(np.float64)
    Cout = w.shape[0]
    rows = np.zeros(B, dtype=int) if mut == "image0" else np.arange(B)
    if mode <= 1:
        a = ln_film(inp["x"], inp["g"], inp["fscale"], inp["fshift"], per_image, dtype=dtype, mut=mut)
    elif mode == 2:
        a = inp["x"] * inp["in_scale"][rows].reshape(B, c, 1, 1)   # the fp32 product, as staged by the kernel
    else:
        a = inp["x"]
    with O.f16_convs():
        acc = O.conv2d(a.astype(np.float64), w)
    if mode >= 2:
        cs = inp["ch_scale"].astype(np.float64).reshape(1, Cout, 1, 1)
        v = acc * cs + bias.reshape(1, Cout, 1, 1) if mut == "scale_before_bias" else (acc + bias.reshape(1, Cout, 1, 1)) * cs
        return inp["res"].astype(np.float64) + v
    v = acc + bias.reshape(1, Cout, 1, 1)
    if mode == 0:
        return v
    v = O._simple_gate(v)
    if lens:
        f = inp["lens"].astype(np.float64)[rows]
        v = v * (f[:, :Cout // 2].reshape(B, -1, 1, 1) + 1) + f[:, Cout // 2:].reshape(B, -1, 1, 1)
    return v


def lnconv_ref(inp, mode, per_image=True, lens=False, mut=None):
    """-> (ref float64, bar, self_err): modes 0 / 1 min(4 x the float32-LayerNorm restatement's error, 1e-3); modes 2 / 3 2e-5."""
    ref = lnconv(inp, mode, per_image, lens)
    if mode >= 2:
        bar, self_err = PWCONV_BAR, 0.0
    else:
        self_err = relerr(lnconv(inp, mode, per_image, lens, dtype=np.float32), ref)
        bar = min(4 * self_err, LNCONV_CAP)
    return (lnconv(inp, mode, per_image, lens, mut=mut) if mut else ref), bar, self_err


# ---------------------------------------------------------------------------------------------
# the tests' metrics: every value is an error divided by its bar (pass: <= 1)
# ---------------------------------------------------------------------------------------------
def bound_ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / bound).max())


def rel_ratio(got, ref, bound):
    """Per-element error relative to |ref| over the elements with |ref| > 0.1 max |ref|, against the largest bound / |ref| among them."""
    sel = np.abs(ref) > 0.1 * np.abs(ref).max()
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)[sel] / np.abs(ref)[sel]
    return float(e.max() / (bound[sel] / np.abs(ref)[sel]).max())


def gate_metrics(got, ref, bound):
    m = {k: bound_ratio(got[k], ref[k], bound[k]) for k in ("gated", "mean", "s") if k in got}
    m.update({k + "_rel": rel_ratio(got[k], ref[k], bound[k]) for k in ("mean", "s") if k in got})
    return m


def tlsc_metrics(got, ref, bound):
    return {k: bound_ratio(got[k], ref[k], bound[k]) for k in ("pooled", "scaled")}
