"""Numpy restatement of a run of consecutive 512-channel NAFBlocks on 8 x 8 pixels: what naf_chain_kernel (csrc/naf_chain.hip) computes in one
launch and the hook irsde_debug_naf_chain runs on the caller's tensors (test infrastructure).  It follows oracle.irsde_oracle.naf_block
(NAFBlock.forward, DenoisingNAFNet_arch.py:56-83 of the latent-bokeh configuration) but takes the FiLM and lens rows directly: no time MLP.

chain_ref(inp, dtype) has two flavours:
  np.float64  the exact operation: no rounding anywhere, the weights as given
  np.float32  the kernel's arithmetic: fp32 residual stream / LayerNorm (two passes, the kernel's summation order) / depthwise accumulation / gates,
              every GEMM with wide accumulation of fp16 operands, and a rounding to fp16 at every point where the kernel rounds:
                R1 the five weight matrices and the nine depthwise taps (pack_naf_chain_host)
                R2 the LayerNorm + FiLM outputs (operand image of conv1 / conv4)
                R3 the conv1 output + bias in the depthwise staging grid
                R4 the gated tensor of the attention branch (the pool sums the fp32 products, not the rounded ones)
                R5 the pooled mean
                R6 the SCA scale vector sca.1(mean) + bias (four fp32 partial sums of 128 input channels, ((p0 + p1) + p2) + p3)
                R7 the fp16 product of gated tensor and scale on its way into conv3
                R8 the gated (+ lens FiLM) tensor of the FFN branch (operand image of conv5)
The metric of every comparison is max |got - ref| / max |ref| on the BRANCH SUM out - x (the residual stream cannot dilute an error).  The bar of a
case is min(4 x metric(float32 flavour, float64 flavour), CAP): 4 = the margin tests/naf_glue_oracle.py gives legitimate 1-ulp fp16 flips; it is
formed from the two restatements alone.  CAP: profiles/naf_chain_parity.md.
`mut` selects one deliberately wrong variant of the float64 flavour (tests/test_naf_chain_host.py: each misses the bar of every case it applies to
at least tenfold).
"""
import functools

import numpy as np

C, PX, HW = 512, 64, 8
FILM_ROW, CAM_ROW = 4 * C, 2 * C
CAP = 2.0 ** -8
F16_COMFORT = 65504.0 / 16   # every fp16-rounded intermediate stays below this
# The input offset: x = N(0, 1) + a per-image, per-channel offset U(1, 2) + X_MEAN.  LayerNorm removes a pixel's mean, so X_MEAN changes nothing
# for a correct two-pass LayerNorm; a one-pass variance E[x^2] - E[x]^2 in fp32 loses ~2^-23 X_MEAN^2 of a variance of ~1.
X_MEAN = 2000.0

# name -> (groups, B, nblocks, per-image FiLM rows, lens, film_off, cam_off, zeroed residual scale); one per code path (tests/test_gpu_naf_chain.py)
CASES = {
    "g1_b1_shared_nolens": (1, 1, 1, False, False, 0, 0, None),
    "g1_b3_lens": (1, 3, 1, True, True, 0, 0, None),
    "g1_b3_attention_only": (1, 3, 1, True, True, 0, 0, "gamma"),
    "g1_b3_ffn_only": (1, 3, 1, True, True, 0, 0, "beta"),
    "g1_b2_n3_offsets": (1, 2, 3, True, True, 2048 + 64, 1024 + 32, None),
    "g2_b2_n2": (2, 2, 2, True, True, 0, 0, None),
    "g4_b3_n1": (4, 3, 1, True, True, 0, 0, None),
    "g4_b9_n3": (4, 9, 3, True, True, 0, 0, None),
}
WEIGHTS = ("norm1_g", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "sca_w", "sca_b", "conv3_w", "conv3_b", "beta", "norm2_g", "conv4_w", "conv4_b",
           "conv5_w", "conv5_b", "gamma")   # the hook's argument order


def relerr(a, b):
    """max |a - b| / max |b|; inf where a holds a non-finite value."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if np.isfinite(a).all() else float("inf")


def branch_err(out, x, ref_out):
    """The tests' metric: out / ref_out [B, 64, 512] against the same input x, on the branch sums."""
    x = x.astype(np.float64)
    return relerr(np.asarray(out, dtype=np.float64) - x, ref_out.astype(np.float64) - x)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 arrays of case `name`: x [B, 64, 512] (NHWC, pixel = 8 y + x), the weights stacked over the blocks in reference layout,
    film [B or 1, nblocks, 2048] = [shift_att | scale_att | shift_ffn | scale_ffn], cam [B, nblocks, 1024] = [scale | shift] or None."""
    groups, B, nb, per_image, lens, film_off, cam_off, zero = CASES[name]
    rs = np.random.RandomState(1000003 + 101 * B + 7 * nb + (13 if lens else 0) + (1 if per_image else 0) + film_off)
    sgn = lambda *s: rs.choice([-1.0, 1.0], s)
    d = dict(
        x=rs.standard_normal((B, PX, C)) + rs.uniform(1, 2, (B, 1, C)) + X_MEAN,
        norm1_g=rs.uniform(0.5, 1.5, (nb, C)), norm2_g=rs.uniform(0.5, 1.5, (nb, C)),
        conv1_w=rs.standard_normal((nb, 2 * C, C)) / np.sqrt(C), conv1_b=rs.uniform(0.5, 1.5, (nb, 2 * C)) * sgn(nb, 2 * C),
        conv2_w=rs.uniform(-1 / 3, 1 / 3, (nb, 2 * C, 9)), conv2_b=rs.uniform(0.5, 1.5, (nb, 2 * C)) * sgn(nb, 2 * C),
        sca_w=rs.uniform(-4 / np.sqrt(C), 4 / np.sqrt(C), (nb, C, C)), sca_b=rs.uniform(-1, 1, (nb, C)) / np.sqrt(C),
        conv3_w=rs.standard_normal((nb, C, C)) / np.sqrt(C), conv3_b=rs.standard_normal((nb, C)),
        conv4_w=rs.standard_normal((nb, 2 * C, C)) / np.sqrt(C), conv4_b=rs.standard_normal((nb, 2 * C)),
        conv5_w=rs.standard_normal((nb, C, C)) / np.sqrt(C), conv5_b=rs.standard_normal((nb, C)),
        beta=0.5 * rs.standard_normal((nb, C)), gamma=0.5 * rs.standard_normal((nb, C)),
    )
    # FiLM / lens rows: scale halves 0.5 N(0, 1), shift halves N(0, 1), drawn per image AND per block (they differ by O(1) in both)
    film = rs.standard_normal((B if per_image else 1, nb, 4, C)) * np.array([1.0, 0.5, 1.0, 0.5]).reshape(1, 1, 4, 1)
    d["film"] = film.reshape(-1, nb, FILM_ROW)
    cam = rs.standard_normal((B, nb, 2, C)) * np.array([0.5, 1.0]).reshape(1, 1, 2, 1)
    if zero:
        d[zero] = np.zeros((nb, C))
    d = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}
    d["cam"] = np.ascontiguousarray(cam.reshape(B, nb, CAM_ROW), dtype=np.float32) if lens else None
    return d


def row_buffer(rows, off):
    """The device layout of FiLM / lens rows [R, nblocks, L]: image r at r * stride, block i at + off + i * L; NaN everywhere else, so that a
    wrong offset or stride cannot go unnoticed.  -> (flat fp32 buffer, stride; 0 for one shared row)."""
    R, nb, L = rows.shape
    stride = off + nb * L + 64
    buf = np.full((R, stride), np.nan, dtype=np.float32)
    buf[:, off:off + nb * L] = rows.reshape(R, nb * L)
    return buf.reshape(-1), (stride if R > 1 else 0)


# ---------------------------------------------------------------------------------------------
# the two flavours
# ---------------------------------------------------------------------------------------------
def _r16(a):
    return a.astype(np.float16).astype(np.float32)


def _ln_kernel_order(x, g, fscale, fshift):
    """layernorm_to_A in fp32: channel 64 wave + 16 ct + 4 q + i; a lane adds ct = 0 .. 3 of (v0 + v1) + (v2 + v3), the four quarters q are joined
    (t0 + t1) + (t2 + t3), the eight waves ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); two passes; x: [B, 64, 512] float32."""
    f = np.float32

    def tree(v):   # v [..., 8 waves, 4 ct, 4 q, 4 i] -> [...]
        t = np.zeros(v.shape[:-3] + (4,), dtype=f)
        for ct in range(4):
            t = t + ((v[..., ct, :, 0] + v[..., ct, :, 1]) + (v[..., ct, :, 2] + v[..., ct, :, 3]))
        r = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
        return ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))

    lay = x.shape[:-1] + (8, 4, 4, 4)
    mean = tree(x.reshape(lay)) * f(1.0 / C)
    d = x - mean[..., None]
    var = tree((d * d).reshape(lay)) * f(1.0 / C)
    rstd = (f(1.0) / np.sqrt(var + f(1e-5))).astype(f)
    return ((d * rstd[..., None] * g) * (fscale + f(1.0)) + fshift).astype(f)


def _ln_one_pass_f32(x, g):
    """The wrong LayerNorm: var = E[x^2] - E[x]^2 in fp32."""
    x = x.astype(np.float32)
    m = x.mean(axis=-1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(axis=-1, keepdims=True, dtype=np.float32) - m * m
    return ((x - m) / np.sqrt(var + np.float32(1e-5)) * g.astype(np.float32)).astype(np.float64)


def _dwconv(u, taps, bias, replicate=False):
    """Depthwise 3 x 3, pad 1, cross-correlation: u [B, 64, 2c] (pixel = 8 y + x), taps [2c, 9] (ky * 3 + kx); accumulated in float64."""
    B = u.shape[0]
    g = u.reshape(B, HW, HW, -1).astype(np.float64)
    gp = np.pad(g, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge" if replicate else "constant")
    out = np.zeros_like(g) + bias.astype(np.float64)
    for ky in range(3):
        for kx in range(3):
            out += gp[:, ky:ky + HW, kx:kx + HW] * taps[:, ky * 3 + kx].astype(np.float64)
    return out.reshape(B, PX, -1)


MUTATIONS = ("drop_row", "drop_col", "film_image0", "lens_image0", "film_block0", "lens_block0", "film_swap", "lens_swap", "film_no_plus1",
             "lens_no_plus1", "replicate", "gate_adjacent", "sca_per_output", "beta_gamma", "lens_before_gate", "ln_one_pass")
_ATTENTION_ONLY = ("drop_row", "drop_col", "replicate", "sca_per_output")   # mistakes inside the attention branch
_FFN_ONLY = ("lens_image0", "lens_block0", "lens_swap", "lens_no_plus1", "lens_before_gate")


def mutation_applies(mut, name):
    """False where the wrong reference IS the reference by construction."""
    groups, B, nb, per_image, lens, film_off, cam_off, zero = CASES[name]
    if mut.startswith("lens") and not lens:
        return False
    if mut == "film_image0" and not (per_image and B > 1):
        return False
    if mut == "lens_image0" and B == 1:
        return False
    if mut.endswith("block0") and nb == 1:
        return False
    if zero == "beta" and mut in _ATTENTION_ONLY:   # y = inp: the attention branch does not reach the output
        return False
    if zero == "gamma" and mut in _FFN_ONLY:        # out = y: neither does the FFN branch
        return False
    return True


def chain_ref(inp, dtype=np.float64, mut=None, stats=None):
    """-> out [B, 64, 512] in `dtype`.  stats (a dict): receives max |v| of every tensor the kernel holds in fp16, and under "pooled" the
    pooled means [nblocks, B, 512]."""
    k16 = dtype == np.float32
    assert k16 or dtype == np.float64
    assert mut is None or (mut in MUTATIONS and not k16)
    rnd = _r16 if k16 else (lambda a: a)
    wide = lambda a: a.astype(np.float64)

    def note(key, v):
        if stats is not None:
            stats[key] = max(stats.get(key, 0.0), float(np.abs(v).max()))
        return v

    def gemm(a, w):   # a [B, 64, K] (fp16 values in the float32 flavour) x w [O, K]: accumulated wide, delivered in `dtype`
        return (wide(a) @ wide(w).T).astype(dtype)

    x = inp["x"].astype(dtype)
    B, nb = x.shape[0], inp["norm1_g"].shape[0]
    film, cam = inp["film"], inp["cam"]
    for i in range(nb):
        W = {k: inp[k][i] for k in WEIGHTS}
        if mut == "beta_gamma":
            W["beta"], W["gamma"] = W["gamma"], W["beta"]
        fi = 0 if mut == "film_block0" else i
        f = film[:, fi] if film.shape[0] == B and mut != "film_image0" else np.repeat(film[:1, fi], B, axis=0)
        f = f.reshape(B, 1, 4, C).astype(dtype)
        shift_att, scale_att, shift_ffn, scale_ffn = (f[:, :, j] for j in range(4))
        if mut == "film_swap":
            shift_att, scale_att, shift_ffn, scale_ffn = scale_att, shift_att, scale_ffn, shift_ffn
        one = dtype(0.0 if mut == "film_no_plus1" else 1.0)

        def norm(v, g, scale, shift):
            if k16:
                return _ln_kernel_order(v, g, scale, shift)
            if mut == "ln_one_pass":
                y = _ln_one_pass_f32(v, g)
            else:
                m = v.mean(axis=-1, keepdims=True)
                y = (v - m) / np.sqrt(((v - m) ** 2).mean(axis=-1, keepdims=True) + 1e-5) * g
            return y * (scale + one) + shift

        def gate(v):
            return v[..., 0::2] * v[..., 1::2] if mut == "gate_adjacent" else v[..., :C] * v[..., C:]

        # ---- attention branch ----
        a = note("norm1", rnd(norm(x, W["norm1_g"].astype(dtype), scale_att, shift_att)))                       # R2
        u = note("conv1", rnd(gemm(a, rnd(W["conv1_w"])) + W["conv1_b"].astype(dtype)))                          # R1, R3
        v = _dwconv(u, rnd(W["conv2_w"]), W["conv2_b"], replicate=mut == "replicate").astype(dtype)              # R1
        gated = gate(v)
        pool = gated.reshape(B, HW, HW, C)
        pool = pool[:, :-1] if mut == "drop_row" else pool[:, :, :-1] if mut == "drop_col" else pool
        mean = note("mean", rnd((pool.sum(axis=(1, 2), dtype=dtype) * dtype(1.0 / PX)).astype(dtype)))           # R5
        if stats is not None:
            stats.setdefault("pooled", []).append(mean)
        gated = note("gated1", rnd(gated))                                                                       # R4
        sw = rnd(W["sca_w"])
        if k16:   # four fp32 partial sums of 128 input channels each
            p = [gemm(mean[:, 128 * j:128 * j + 128], sw[:, 128 * j:128 * j + 128]) for j in range(4)]
            s = ((p[0] + p[1]) + p[2]) + p[3]
        else:
            s = gemm(mean, sw)
        s = note("sca", rnd(s + W["sca_b"].astype(dtype)))                                                       # R6
        if mut == "sca_per_output":
            acc = gemm(gated, rnd(W["conv3_w"])) * s[:, None, :]
        else:
            acc = gemm(note("gated1*sca", rnd(gated * s[:, None, :])), rnd(W["conv3_w"]))                        # R7
        y = x + (acc + W["conv3_b"].astype(dtype)) * W["beta"].astype(dtype)
        # ---- FFN branch ----
        a = note("norm2", rnd(norm(y, W["norm2_g"].astype(dtype), scale_ffn, shift_ffn)))                       # R2
        v = gemm(a, rnd(W["conv4_w"])) + W["conv4_b"].astype(dtype)
        if cam is not None:
            ci = 0 if mut == "lens_block0" else i
            cr = np.repeat(cam[:1, ci], B, axis=0) if mut == "lens_image0" else cam[:, ci]
            cr = cr.reshape(B, 1, 2, C).astype(dtype)
            cscale, cshift = (cr[:, :, 1], cr[:, :, 0]) if mut == "lens_swap" else (cr[:, :, 0], cr[:, :, 1])
            cone = dtype(0.0 if mut == "lens_no_plus1" else 1.0)
            if mut == "lens_before_gate":
                g2 = (v[..., :C] * (cscale + cone) + cshift) * v[..., C:]
            else:
                g2 = gate(v) * (cscale + cone) + cshift
        else:
            g2 = gate(v)
        g2 = note("gated2", rnd(g2))                                                                             # R8
        x = y + (gemm(g2, rnd(W["conv5_w"])) + W["conv5_b"].astype(dtype)) * W["gamma"].astype(dtype)
        x = x.astype(dtype)
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (ref float64 [B, 64, 512], bar, self_err, stats of the float32 flavour): computed once per case and shared; read-only."""
    inp = inputs(name)
    ref = chain_ref(inp, np.float64)
    stats = {}
    emu = chain_ref(inp, np.float32, stats=stats)
    self_err = branch_err(emu, inp["x"], ref)
    ref.setflags(write=False)
    pooled = np.stack(stats.pop("pooled"))
    return ref, min(4 * self_err, CAP), self_err, dict(stats, pooled=pooled)


# ---------------------------------------------------------------------------------------------
# the weight streams: fragment enumeration of the G-groups-per-image kernel restated (naf_chain_split_order, csrc/naf_chain.hip)
# ---------------------------------------------------------------------------------------------
FRAGS_PER_BLOCK = 448


def one_group_fragments(nblocks):
    """The one-group streams [8 waves][nblocks][448] as (block, conv 0 .. 4, 16-channel tile, k step) per fragment, in pack order."""
    out = []
    for w in range(8):
        for blk in range(nblocks):
            gated = lambda conv: [(blk, conv, hi * 32 + 4 * w + ps, ks) for ps in range(4) for ks in range(16) for hi in (0, 1)]
            plain = lambda conv: [(blk, conv, 4 * w + 2 * ps + t, ks) for ps in range(2) for ks in range(16) for t in (0, 1)]
            sca = [(blk, 1, 4 * w + t, ks) for ks in range(16) for t in range(4)]
            out += gated(0) + sca + plain(2) + gated(3) + plain(4)
    return out


def split_fragments(nblocks, G):
    """The streams [G][8 waves][nblocks][448 / G] of the kernel's passes at G groups per image, as the same tuples."""
    NTW = 4 // G
    NT3 = 2 if NTW >= 2 else 1
    NP3 = NTW // NT3
    out = []
    for g in range(G):
        for w in range(8):
            tile0 = (g * (C // G) + w * 16 * NTW) // 16
            for blk in range(nblocks):
                gated = lambda conv: [(blk, conv, hi * 32 + tile0 + ps, ks) for ps in range(NTW) for ks in range(16) for hi in (0, 1)]
                plain = lambda conv: [(blk, conv, tile0 + NT3 * ps + t, ks) for ps in range(NP3) for ks in range(16) for t in range(NT3)]
                sca = [(blk, 1, 4 * w + t, 4 * (g * (4 // G) + qq) + kk) for qq in range(4 // G) for kk in range(4) for t in range(4)]
                out += gated(0) + sca + plain(2) + gated(3) + plain(4)
    return out
