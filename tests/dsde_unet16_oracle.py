"""Oracle helpers for the denoising-sde ConditionalUNet in the bf16_act mode (IRSDE_FLAG_UNCOND_FULLATTN | IRSDE_FLAG_BF16_ACT): the full softmax attention
core on bf16 tensors (csrc/full_attn16.hip) and the network around it.  numpy only; shared by tests/test_dsde_unet16_host.py and
tests/test_gpu_dsde_unet16.py.

  attention_reference   float64 softmax attention of a q | k | v tensor: o = sum_j p_ij v_j and A = sum_j p_ij |v_j|
  kernel_bound          the elementwise bar of the kernel against that reference
  full_attention16      the kernel restated in float64 with its rounding points (O.round_bf16)
  emulate_kernel        the kernel's own order in float32: 32-key tiles, online rescale, bf16 P — what the bar has to admit
  dsde_forward_bf16_act the network under O.bf16_convs(store_bf16=True) with the bottleneck the engine runs

The bar.  The kernel rounds P to bf16 (relative error 2^-9 per weight), divides by the sum of the ROUNDED weights and rounds the quotient once.  With p the
float64 softmax: the numerator is off by at most 2^-9 A, the denominator by 2^-9 (relative), which moves the quotient by 2^-9 |o|, and the final rounding adds
another 2^-9 |o|; (1 + 2^-6) covers the products of those terms and 1e-5 A the fp32 exponent, rescale and accumulation:
    |got - o| <= 2^-9 (A + 2 |o|) (1 + 2^-6) + 1e-5 A
"""
import functools

import numpy as np

from oracle import irsde_oracle as O

HEADS, DH = 4, 32
HID = HEADS * DH
SCALE = DH ** -0.5

# (B, N) of the kernel tests: N below, at and just over one 32-key tile; the project's 120-token case; a second work-group with one live wave (130 = 4 full
# query tiles + 2 queries); the bottlenecks of 256 x 256 and 512 x 512 inputs at depth 4
KERNEL_SHAPES = [(1, 1), (1, 31), (2, 32), (1, 33), (3, 120), (1, 130), (2, 1024), (1, 4096)]
# q and k entries of this standard deviation give logits of std 1.5^2 = 2.25: a softmax that is neither flat nor one-hot, so that the scale, the mask, the
# normalisation and the running maximum all show in the output (tests/test_dsde_unet16_host.py::test_mutations_miss_the_bound)
QK_STD = 1.5


def kernel_bound(o, A):
    return 2.0 ** -9 * (A + 2 * np.abs(o)) * (1 + 2.0 ** -6) + 1e-5 * A


def make_qkv(B, N, seed=0, qk_std=QK_STD):
    """[B][N][384] float32 holding bf16 values: q | k rows of std qk_std, v of std 1."""
    rs = np.random.RandomState(1000 * seed + 7 * B + N)
    x = rs.standard_normal((B, N, 3 * HID))
    x[..., :2 * HID] *= qk_std
    return O.round_bf16(x.astype(np.float32))


def _split(qkv):
    B, N, _ = qkv.shape
    return tuple(qkv[..., i * HID:(i + 1) * HID].reshape(B, N, HEADS, DH).transpose(0, 2, 1, 3) for i in range(3))   # [B][heads][N][d]


def _merge(o):
    B, _, N, _ = o.shape
    return np.ascontiguousarray(o.transpose(0, 2, 1, 3).reshape(B, N, HID))


def attention_reference(qkv, scale=SCALE, uniform=False, normalise=True):
    """float64 Attention core (module_util.py:193-204) of qkv [B][N][384] -> (o, A, argmax), o / A [B][N][128], argmax [B][heads][N] the key of the largest logit."""
    q, k, v = (t.astype(np.float64) for t in _split(np.asarray(qkv)))
    B, _, N, _ = q.shape
    o, A, am = np.empty_like(q), np.empty_like(q), np.empty((B, HEADS, N), dtype=np.int64)
    for b in range(B):
        for h in range(HEADS):
            s = (q[b, h] @ k[b, h].T) * scale
            am[b, h] = s.argmax(axis=1)
            p = np.ones_like(s) if uniform else np.exp(s - s.max(axis=1, keepdims=True))
            if normalise:
                p /= p.sum(axis=1, keepdims=True)
            o[b, h], A[b, h] = p @ v[b, h], p @ np.abs(v[b, h])
    return _merge(o), _merge(A), am


@functools.lru_cache(maxsize=None)
def kernel_case(B, N, seed=0):
    """The shared input and float64 reference of one kernel shape (computed once per process; treat as read-only)."""
    qkv = make_qkv(B, N, seed)
    o, A, _ = attention_reference(qkv)
    for a in (qkv, o, A):
        a.setflags(write=False)
    return qkv, o, A


def full_attention16(qkv, uniform=False):
    """The kernel restated in float64: q, k, v as stored (bf16 values), scores scaled after the product, P = exp(s - max) rounded to bf16, the row sum taken over
    the ROUNDED P, the quotient rounded once.  (The kernel forms P against the running maximum of its 32-key tiles and rescales in fp32; here the final maximum is
    used: the same number of roundings, each relative.)  uniform=True: every weight 1 — the average that the sensitivity tests put in the softmax's place."""
    q, k, v = (t.astype(np.float64) for t in _split(np.asarray(qkv)))
    s = np.einsum("bhid,bhjd->bhij", q, k) * SCALE
    p = np.ones_like(s) if uniform else O.round_bf16(np.exp(s - s.max(axis=-1, keepdims=True)))
    o = np.einsum("bhij,bhjd->bhid", p, v) / p.sum(axis=-1, keepdims=True)
    return O.round_bf16(_merge(o))


def emulate_kernel(qkv, mutation=None):
    """The kernel's order of operations in float32 numpy: one pass over 32-key tiles per (image, head) with the running maximum, the fp32 rescale of O and l, P
    rounded to bf16 for the second product and for the row sum, keys behind N masked to -inf, O / l rounded to bf16.  `mutation` injects one bug
    (tests/test_dsde_unet16_host.py::test_mutations_miss_the_bound)."""
    f = np.float32
    q, k, v = _split(np.asarray(qkv, dtype=f))
    if mutation == "kv_swapped":
        k, v = v, k
    B, _, N, _ = q.shape
    scale = f(1.0) if mutation == "no_scale" else f(SCALE)
    out = np.empty_like(q)
    nt = -(-N // 32)
    for b in range(B):
        for h in range(HEADS):
            kp = np.concatenate([k[b, h], np.repeat(k[b, h][-1:], nt * 32 - N, axis=0)])   # the kernel reads row N - 1 for the keys behind the end
            vp = np.concatenate([v[b, h], np.zeros((nt * 32 - N, DH), dtype=f)])              # ... and zeros for their V rows
            m = np.full((N, 1), -np.inf, dtype=f)
            l = np.zeros((N, 1), dtype=f)
            o = np.zeros((N, DH), dtype=f)
            m_first = None
            for t in range(nt):
                s = (q[b, h] @ kp[32 * t:32 * t + 32].T).astype(f) * scale
                if mutation != "tail_unmasked":
                    s[:, max(0, N - 32 * t):] = -np.inf
                if mutation == "uniform":
                    s = np.where(np.isfinite(s), f(0), s)
                mnew = np.maximum(m, s.max(axis=1, keepdims=True))
                with np.errstate(invalid="ignore"):
                    alpha = np.exp(m - mnew).astype(f)
                if t == 0:
                    m_first = mnew
                against = m_first if mutation == "stale_max" else mnew   # stale_max: O and l are rescaled, but P is formed against the first tile's maximum
                p = O.round_bf16(np.exp(s - against).astype(f))
                l = l * alpha + p.sum(axis=1, keepdims=True, dtype=f)
                o = o * alpha + (p @ vp[32 * t:32 * t + 32]).astype(f)
                m = mnew
            out[b, h] = o if mutation == "unnormalised" else o / l
    if mutation == "heads_permuted":
        out = np.roll(out, 1, axis=1)
    return O.round_bf16(_merge(out))


MUTATIONS = ["no_scale", "uniform", "tail_unmasked", "kv_swapped", "heads_permuted", "unnormalised", "stale_max"]


# ---------------------------------------------------------------------------------------------
# the network: denoising-sde ConditionalUNet.forward(x, time) as the engine runs it under IRSDE_FLAG_BF16_ACT
# ---------------------------------------------------------------------------------------------
def mid_attn_bf16_act(p, x, uniform=False):
    """Residual(PreNorm(Attention)) of the bottleneck with the tensors the engine stores (call inside O.bf16_convs(store_bf16=True)): the LayerNorm output, q | k | v,
    the attention output, to_out + residual.  x: NCHW float64 (bf16 values)."""
    B, C, H, W = x.shape
    xn = O._ln_st(x, p["mid_attn.fn.norm.g"])
    qkv = O._st(O.conv2d(xn, p["mid_attn.fn.fn.to_qkv.weight"]))
    a = full_attention16(qkv.reshape(B, 3 * HID, H * W).transpose(0, 2, 1), uniform=uniform)          # [B][N][128], rounded
    a = np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(B, HID, H, W)
    return O._st(O.conv2d(a, p["mid_attn.fn.fn.to_out.weight"], p["mid_attn.fn.fn.to_out.bias"]) + x)


def mid_attn_float64(p, x):
    """The same block with nothing rounded (module_util.py:20-26,82-90,182-204)."""
    return O.full_attention(p, "mid_attn.fn.fn.", O.layer_norm_c(x, p["mid_attn.fn.norm.g"])) + x


def dsde_forward_bf16_act(params, x, t, depth=4, taps=None):
    """O.uncond_unet_forward with the engine's stored tensors: every conv output, ResBlock, attention block rounded to bf16 where the engine keeps a bf16 tensor
    (O.unet_forward does the same for the conditional network), and the bottleneck of mid_attn_bf16_act.  float64 arithmetic."""
    dtype = np.float64
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    x = np.asarray(x, dtype=dtype)
    if np.isscalar(t):
        t = np.array([int(t)])
    H, W = x.shape[2:]
    s = 2 ** depth
    with O.bf16_convs(store_bf16=True):
        x = np.pad(x, ((0, 0), (0, 0), (0, (s - H % s) % s), (0, (s - W % s) % s)), mode="reflect")
        x = O._st(O.conv2d(x, p["init_conv.weight"], pad=3))
        x_ = x
        nf = p["init_conv.weight"].shape[0]
        temb = O.sinusoidal_pos_emb(t, nf, dtype)
        temb = O.linear(O.gelu(O.linear(temb, p["time_mlp.1.weight"], p["time_mlp.1.bias"])), p["time_mlp.3.weight"], p["time_mlp.3.bias"])
        h = []
        for i in range(depth):
            x = O.res_block(p, "downs.%d.0." % i, x, temb)
            h.append(x)
            x = O.res_block(p, "downs.%d.1." % i, x, temb)
            x = O.attn_block(p, "downs.%d.2." % i, x)
            h.append(x)
            if i != depth - 1:
                x = O._st(O.conv2d(x, p["downs.%d.3.weight" % i], p["downs.%d.3.bias" % i], stride=2, pad=1))
            else:
                x = O._st(O.conv2d(x, p["downs.%d.3.weight" % i], pad=1))
        x = O.res_block(p, "mid_block1.", x, temb)
        if taps is not None:
            taps["mid_block1"] = x
        x = mid_attn_bf16_act(p, x)
        if taps is not None:
            taps["mid_attn"] = x
        x = O.res_block(p, "mid_block2.", x, temb)
        for j in range(depth):
            x = O.res_block(p, "ups.%d.0." % j, np.concatenate([x, h.pop()], axis=1), temb)
            x = O.res_block(p, "ups.%d.1." % j, np.concatenate([x, h.pop()], axis=1), temb)
            x = O.attn_block(p, "ups.%d.2." % j, x)
            if j != depth - 1:
                x = O._st(O.conv2d(O.upsample_nearest2(x), p["ups.%d.3.1.weight" % j], p["ups.%d.3.1.bias" % j], pad=1))
            else:
                x = O._st(O.conv2d(x, p["ups.%d.3.weight" % j], pad=1))
        x = O.res_block(p, "final_res_block.", np.concatenate([x, x_], axis=1), temb)
        x = O.conv2d(x, p["final_conv.weight"], p["final_conv.bias"], pad=1)
    return np.ascontiguousarray(x[..., :H, :W])


# Gain on the q and k rows of mid_attn.fn.fn.to_qkv.weight for the block-level tests (as the *_proj1 gain of the SCAM tests).  With default-initialised weights the
# bottleneck's logits have a standard deviation of 0.47 on the nf 32 / depth 2 / 2 x 24 x 20 fixture: the softmax is close to an average, and putting the average
# in its place moves the block by 10.6 block-level bars — on the edge of what a test can see.  A gain g multiplies the logits by g^2: 2 gives logits of std 1.9 and
# 49 bars (tests/test_dsde_unet16_host.py::test_restatement_feels_the_softmax prints both).
MID_QK_GAIN = 2.0


def gained_params(params, gain=MID_QK_GAIN):
    out = dict(params)
    w = np.array(params["mid_attn.fn.fn.to_qkv.weight"], copy=True)
    w[:2 * HID] *= np.asarray(gain, dtype=w.dtype)
    out["mid_attn.fn.fn.to_qkv.weight"] = w
    return out
