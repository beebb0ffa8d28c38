"""Float64 references and the shared input generator of the LinearAttention kernel tests (csrc/linear_attn.hip through the hooks irsde_debug_attn_block /
irsde_debug_attn_core; tests/test_linear_attn_host.py on the CPU, tests/test_gpu_linear_attn.py on the GPU).

References: the block is O.attn_block on a five-key parameter dict with x as [B][C][1][N]; the 16-bit operand modes are O.attn_block_fused16; the core is the
body of O.linear_attention between its two convolutions.  Nothing here restates a kernel: tiles, chunks and the online softmax exist only in the kernels.

Inputs (one generator for both test files): weights U(+-1/sqrt(fan_in)), gains U(0.5, 1.5); to_out.0.weight x N so that the attention branch is O(1) in front of
the bias (the context carries v / N); the k rows of to_qkv.weight x 4 so that k spans enough for the running maximum of the online softmax to move between tiles
and chunks; x standard normal with the LAST pixel of every image x 3: a tail row counted twice, or a mask off by one, then shows in every other pixel.
"""
import functools

import numpy as np

from oracle import irsde_oracle as O

HID = 128          # heads x dim_head
BAR = 5e-5         # fp32-class modes: max error relative to the branch (test_gpu_parity.py::test_fused_attention_block_vs_oracle)
PRE = ""           # prefix of the five keys

# (B, N): less than one tile (three-piece mode: 64 + 8) / four full 128-pixel chunks + an 8-pixel tail, several images / chunk_len 136 (one full tile + an 8-pixel
# tail per chunk, tiles off the 128 grid, partial last chunk)
SHAPES = [(1, 72), (3, 520), (16, 4200)]
PRODUCTION = (16, 7680)   # 80 x 96 images at B = 16: chunk_len 240
HOST_C = (32, 64, 96, 256)
HOST_N = (72, 136, 200, 520)


@functools.lru_cache(maxsize=4)
def make_inputs(C, B, N):
    """float32 arrays: x [B][N][C] (NHWC, pixels flattened) and the five weights in reference layout (flattened 1x1 kernels)."""
    rng = np.random.default_rng([C, B, N, 20])

    def u(shape, fan_in):
        return rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)

    wqkv = u((3 * HID, C), C)
    wqkv[HID:2 * HID] *= 4.0
    d = dict(wqkv=wqkv, wo=u((C, HID), HID) * N, bo=u((C,), HID), g1=rng.uniform(0.5, 1.5, C), g2=rng.uniform(0.5, 1.5, C))
    x = rng.standard_normal((B, N, C))
    x[:, -1, :] *= 3.0
    d["x"] = x
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}


def params_of(inp, dtype=np.float64):
    C = inp["g1"].shape[0]
    return {"fn.norm.g": inp["g1"].astype(dtype).reshape(1, C, 1, 1), "fn.fn.to_qkv.weight": inp["wqkv"].astype(dtype).reshape(3 * HID, C, 1, 1),
            "fn.fn.to_out.0.weight": inp["wo"].astype(dtype).reshape(C, HID, 1, 1), "fn.fn.to_out.0.bias": inp["bo"].astype(dtype),
            "fn.fn.to_out.1.g": inp["g2"].astype(dtype).reshape(1, C, 1, 1)}


def nchw(x_bnc, dtype=np.float64):
    """[B][N][C] -> [B][C][1][N]"""
    return np.ascontiguousarray(x_bnc.astype(dtype).transpose(0, 2, 1))[:, :, None, :]


def bnc(y_nchw):
    """[B][C][1][N] -> [B][N][C]"""
    return np.ascontiguousarray(y_nchw[:, :, 0, :].transpose(0, 2, 1))


def block(inp, x=None, dtype=np.float64):
    """Residual(PreNorm(LinearAttention)) on x [B][N][C] (default: the generator's) -> [B][N][C]"""
    x = inp["x"] if x is None else x
    return bnc(O.attn_block(params_of(inp, dtype), PRE, nchw(x, dtype)))


def block16(inp, f16, store_bf16):
    """The oracle's restatement of the fused kernels' 16-bit operand modes; store_bf16: x is what the bf16 tensor holds"""
    x = O.round_bf16(inp["x"]) if store_bf16 else inp["x"]
    return bnc(O.attn_block_fused16(params_of(inp), PRE, nchw(x), f16=f16, store_bf16=store_bf16))


def core(qkv, dtype=np.float64):
    """The body of O.linear_attention between to_qkv and to_out: qkv [B][N][384] (q | k | v, 4 heads x 32) -> out [B][N][128]"""
    B, N, _ = qkv.shape
    heads, dh = 4, HID // 4
    t = np.ascontiguousarray(qkv.astype(dtype).transpose(0, 2, 1))
    q, k, v = (t[:, i * HID:(i + 1) * HID].reshape(B, heads, dh, N) for i in range(3))
    q = np.exp(q - q.max(axis=2, keepdims=True))
    q = q / q.sum(axis=2, keepdims=True)
    k = np.exp(k - k.max(axis=3, keepdims=True))
    k = k / k.sum(axis=3, keepdims=True)
    q = q * dtype(dh ** -0.5)
    v = v / dtype(N)
    context = np.matmul(k, v.transpose(0, 1, 3, 2))              # "bhdn,bhen->bhde"
    out = np.matmul(context.transpose(0, 1, 3, 2), q)            # "bhde,bhdn->bhen"
    return np.ascontiguousarray(out.reshape(B, HID, N).transpose(0, 2, 1))


def core_inputs(inp):
    """What stands in front of the core on the two tensor routes, as the float32 tensors a plan would hold: xn = PreNorm's LayerNorm of x [B][N][C], and
    qkv = to_qkv(xn) [B][N][384] (its first third is route 1's q tensor)."""
    p = params_of(inp)
    xn = bnc(O.layer_norm_c(nchw(inp["x"]), p["fn.norm.g"])).astype(np.float32)
    qkv = (xn.astype(np.float64) @ inp["wqkv"].astype(np.float64).T).astype(np.float32)
    return xn, qkv


def core_ref_route1(inp, xn, q):
    """float64 core from the float32 tensors route 1 reads: k, v = the k | v rows of to_qkv.weight on xn, q as given"""
    kv = xn.astype(np.float64) @ inp["wqkv"][HID:].astype(np.float64).T
    return core(np.concatenate([q.astype(np.float64), kv], axis=2))


def branch_max(full, x):
    return float(np.abs(full - x).max())


def errors(got, ref, scale):
    d = np.asarray(got, dtype=np.float64) - ref
    return float(np.abs(d).max()) / scale, float(np.sqrt((d * d).mean())) / scale


# the wrong oracles the bar has to tell from the right one (tests/test_linear_attn_host.py)
def wrong_k_row(inp):
    """one k row of to_qkv.weight off by 1 %: the row of the k channel with the widest range over the pixels (largest max - min in any image) — the channel whose
    softmax over N is the most concentrated, the one in which the running maximum moves the most and a wrong weight shows the most.  (A row picked blindly
    gives 1.5e-4 .. 1.3e-3 of the branch at the host test's shapes; this rule 2.7e-4 or more.)"""
    k = core_inputs(inp)[1][..., HID:2 * HID]
    row = int(np.argmax((k.max(axis=1) - k.min(axis=1)).max(axis=0)))
    w = dict(inp)
    w["wqkv"] = inp["wqkv"].copy()
    w["wqkv"][HID + row] *= np.float32(1.01)
    return block(w)


def wrong_v_norm(inp):
    """v / (N + 1) instead of v / N: the branch in front of the bias scaled by N / (N + 1)"""
    N = inp["x"].shape[1]
    w = dict(inp)
    w["wo"] = (inp["wo"].astype(np.float64) * (N / (N + 1.0))).astype(np.float32)
    return block(w)


def wrong_last_pixel(inp):
    """the last pixel of every image replaced by the one in front of it (a tail row read from the wrong place); compare on the OTHER pixels"""
    x = inp["x"].copy()
    x[:, -1] = x[:, -2]
    return block(inp, x)
