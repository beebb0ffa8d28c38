"""The denoising-sde ConditionalUNet in the 16-bit modes (run with -m gpu on an MI355X): the bf16 full-attention kernel (csrc/full_attn16.hip) through its debug
hook against the float64 reference under the elementwise bar of tests/dsde_unet16_oracle.py, the bottleneck block, the network and the DenoisingSDE samplers in the
bf16_act mode (IRSDE_FLAG_UNCOND_FULLATTN | IRSDE_FLAG_BF16_ACT) against the oracle's restatement of the mode, and pins for the operand-only modes (bf16 / fp16 with
fp32 storage), which keep the fp32 attention core."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import dsde_unet16_oracle as DU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8   # NaN rows behind the output


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


_MODELS = {}


def dsde_model(nf, depth, dtype="fp32", flags=0, gained=False):
    key = (nf, depth, dtype, flags, gained)
    if key not in _MODELS:
        params = O.uncond_synth_params(seed=0, nf=nf, depth=depth)
        if gained:
            params = DU.gained_params(params)
        m = P.denoising_sde.ConditionalUNet(3, 3, nf, depth=depth)
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
        m.set_compute_dtype(dtype)
        m.engine_flags |= flags
        _MODELS[key] = (m.to(DEV).eval(), params)
    return _MODELS[key]


# ---------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------
def run_kernel(qkv, fill=float("nan")):
    """qkv: numpy [B][N][384] of bf16 values.  Returns (out [B][N][128] float64, guard rows as int16 bit patterns, output bits)."""
    B, N, _ = qkv.shape
    d_in = torch.from_numpy(np.array(qkv, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()
    d_out = torch.full((B * N + GUARD, DU.HID), fill, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_full_attention16(ctypes.c_void_p(d_in.data_ptr()), B, N, ctypes.c_void_p(d_out.data_ptr()), None))
    bits = d_out.view(torch.int16).cpu().numpy()
    out = d_out[:B * N].to(torch.float32).cpu().numpy().astype(np.float64).reshape(B, N, DU.HID)
    return out, bits[B * N:], bits[:B * N]


def check_kernel(qkv, o, A, what):
    got, guard, bits = run_kernel(qkv)
    nan_bits = torch.full((1,), float("nan"), dtype=torch.bfloat16).view(torch.int16).item()
    assert (guard == nan_bits).all(), "%s: rows behind row N were written" % what
    assert np.isfinite(got).all(), what
    ratio = float((np.abs(got - o) / DU.kernel_bound(o, A)).max())
    print("%s: max |got - o| / bound = %.3f, max |got - o| = %.3g" % (what, ratio, float(np.abs(got - o).max())))
    _, guard2, bits2 = run_kernel(qkv, fill=1.0)   # a pre-filled output: nothing of it may survive in, or leak into, the result
    assert np.array_equal(bits, bits2), "%s: the result depends on what the output held" % what
    one_bits = torch.ones(1, dtype=torch.bfloat16).view(torch.int16).item()
    assert (guard2 == one_bits).all(), what
    assert ratio <= 1.0, (what, ratio)
    return got


@pytest.mark.parametrize("B,N", DU.KERNEL_SHAPES)
def test_kernel_vs_float64_reference(B, N):
    """|got - o| <= 2^-9 (A + 2 |o|) (1 + 2^-6) + 1e-5 A elementwise; NaN guard rows behind row N untouched; bit-identical on a pre-filled output."""
    qkv, o, A = DU.kernel_case(B, N)
    check_kernel(qkv, o, A, "B=%d N=%d" % (B, N))


def _spike_qkv(kind):
    """N = 130 (4 full query tiles + 2 queries; 4 full key tiles + 2 keys).  Every 7th query is a fixed vector u.
    'late_max': key 129 = 2 u, so for those queries the largest logit (~25) sits in the ragged last tile and the running maximum rises there.
    'logit80': key 5 = a u and key 100 = -a u with a |u|^2 32^-1/2 = 80: logits of +80 and -80 in one row."""
    qkv = np.array(DU.make_qkv(1, 130, seed=3 if kind == "late_max" else 4), dtype=np.float64)
    rs = np.random.RandomState(11)
    u = rs.standard_normal((DU.HEADS, DU.DH)) * DU.QK_STD
    rows = np.arange(0, 130, 7)
    qkv[0, rows, :DU.HID] = u.reshape(-1)
    k = qkv[0, :, DU.HID:2 * DU.HID].reshape(130, DU.HEADS, DU.DH)
    if kind == "late_max":
        k[129] = 2 * u
    else:
        a = 80.0 / ((u ** 2).sum(axis=1, keepdims=True) * DU.SCALE)
        k[5], k[100] = a * u, -a * u
    return O.round_bf16(qkv.astype(np.float32)), rows


@pytest.mark.parametrize("kind", ["late_max", "logit80"])
def test_kernel_spike_cases(kind):
    qkv, rows = _spike_qkv(kind)
    o, A, am = DU.attention_reference(qkv)
    q, k, _ = DU._split(qkv.astype(np.float64))
    s = np.einsum("bhid,bhjd->bhij", q, k)[0][:, rows] * DU.SCALE
    if kind == "late_max":
        assert (am[0][:, rows] == 129).all()          # the maximum rises in the last, ragged key tile
    else:
        assert 75 < s.max() < 85 and -85 < s.min() < -75
    check_kernel(qkv, o, A, kind)


# ---------------------------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------------------------
def test_bottleneck_block_vs_restatement():
    """taps mid_block1 -> mid_attn of the bf16_act engine (nf 32, depth 2, 2 x 24 x 20: 120 tokens, 128 channels) with the q / k gain of DU.MID_QK_GAIN, against the mode
    restatement fed the engine's own mid_block1 tap: the project's bf16_act block bar, and the restatement explains the kernel (closer to it than the unrounded float64
    block is, by 2x in rms)."""
    nf, depth, B, H, W = 32, 2, 2, 24, 20
    m, params = dsde_model(nf, depth, "bf16_act", flags=_lib.FLAG_KEEP_ACTIVATIONS, gained=True)
    _, xT = O.synth_inputs(1234, B, H, W, max_sigma=25)
    m(torch.from_numpy(xT).to(DEV), 7)
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    assert buf.value.count(b"full_attention (bf16 operands + storage)") == 1
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    xin = m.debug_tap("mid_block1").numpy().astype(np.float64)
    got = m.debug_tap("mid_attn").numpy().astype(np.float64)
    assert xin.shape == (B, 128, 12, 10)
    with O.bf16_convs(store_bf16=True):
        ref = DU.mid_attn_bf16_act(p64, xin)
    full = DU.mid_attn_float64(p64, xin)
    branch = float(np.abs(full - xin).max())
    err = np.abs(got - ref)
    rms_ref, rms_full = float(np.sqrt(((got - ref) ** 2).mean())), float(np.sqrt(((got - full) ** 2).mean()))
    print("bf16_act mid_attn: branch max %.3g; vs the restatement max %.3g rms %.3g (%.3g of the elements differ), vs the unrounded block max %.3g rms %.3g"
          % (branch, float(err.max()), rms_ref, float((err > 0).mean()), float(np.abs(got - full).max()), rms_full))
    assert branch > 0.5
    assert (err <= np.abs(ref) * 2.0 ** -7 + 3e-3 * branch).all(), float((err / (np.abs(ref) * 2.0 ** -7 + 3e-3 * branch)).max())
    assert rms_ref < 0.5 * rms_full, (rms_ref, rms_full)


# ---------------------------------------------------------------------------------------------
# network level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nf32d2_2x24x20", "nf64d4_2x88x80"])
def test_network_bf16_act_mode(golden, tag):
    """forward(x, time) in the bf16_act mode: follows the restatement of the mode (3e-2) and stays close to the fp32 reference golden (above 1e-4: the mode is really
    on; below 5e-2) — the bars of the conditional UNet's test_unet_bf16_act_mode.  nf64d4_2x88x80: 120 bottleneck tokens of 1024 channels."""
    g = golden.dsde
    nf, depth, B, H, W = (int(v) for v in g[tag + "/cfg"])
    m, params = dsde_model(nf, depth, "bf16_act")
    _, xT = O.synth_inputs(1234, B, H, W, max_sigma=25)
    t = int(g[tag + "/ts"][0])
    y = m(torch.from_numpy(xT).to(DEV), t).cpu().numpy()
    ref = DU.dsde_forward_bf16_act(params, xT, t, depth=depth)
    e_oracle, e_fp32 = relerr(y, ref), relerr(y, g[tag + "/t%d" % t])
    print("dsde bf16_act forward %s t=%d: vs the restatement %.3g, vs the fp32 reference %.3g" % (tag, t, e_oracle, e_fp32))
    assert np.isfinite(y).all()
    assert e_oracle < 3e-2
    assert 1e-4 < e_fp32 < 5e-2


def test_network_bf16_act_batch_of_three_with_per_image_timesteps():
    """Image b of a 3-image batch with [B] timesteps against its single-image call (2e-2, the bar of test_unet_bf16_act_batch_and_padding_properties): odd size with
    the reflect pad (48 x 64), 3 x 4 (image, head) groups of 12 tokens in the attention grid."""
    B, H, W = 3, 40, 56
    m, _ = dsde_model(64, 4, "bf16_act")
    _, xT = O.synth_inputs(77, B, H, W, max_sigma=25)
    x = torch.from_numpy(xT).to(DEV)
    ts = torch.tensor([5, 60, 99])
    yb = m(x, ts).cpu().numpy()
    assert np.isfinite(yb).all()
    for b in range(B):
        y1 = m(x[b:b + 1], int(ts[b])).cpu().numpy()
        e = relerr(y1, yb[b:b + 1])
        print("dsde bf16_act image %d of 3 vs its single-image call: %.3g" % (b, e))
        assert e < 2e-2


@pytest.mark.parametrize("tag,key", [("nf32d2_2x24x20", "sampler_2x16x16"), ("nf64d4_1x64x64", "sampler_1x32x32")])
def test_samplers_bf16_act(golden, tag, key):
    """DenoisingSDE.reverse_ode / reverse_sde from get_optimal_timestep(25) in the bf16_act mode: graph replay is bit-identical to eager launches, and the error against
    the fp32 engine is at most 3x that of the bf16 operand-only mode (storage adds about as many roundings as the operands do) and below the project's 5e-2."""
    g = golden.dsde
    nf, depth = (int(v) for v in g[tag + "/cfg"][:2])
    noisy = g["%s/%s/noisy" % (tag, key)]
    x = torch.from_numpy(noisy).to(DEV)
    z = torch.from_numpy(O.synth_noise(7, 100, noisy.shape)).to(DEV)
    outs = {}
    for dtype in ("fp32", "bf16", "bf16_act"):
        m, _ = dsde_model(nf, depth, dtype)
        sde = P.DenoisingSDE(max_sigma=75, T=100, device=DEV)
        sde.set_model(m)
        sde.injected_noise = z
        Topt = sde.get_optimal_timestep(25)
        assert int(Topt) == int(g["%s/%s/T" % (tag, key)])
        for mode, fn in (("ode", sde.reverse_ode), ("sde", sde.reverse_sde)):
            outs[dtype, mode] = fn(x, T=Topt).cpu().numpy()
            if dtype == "bf16_act":
                sde.use_graph = False
                assert np.array_equal(fn(x, T=Topt).cpu().numpy(), outs[dtype, mode]), mode
                sde.use_graph = True
    for mode in ("ode", "sde"):
        assert relerr(outs["fp32", mode], g["%s/%s/%s" % (tag, key, mode)]) < 2e-3   # the yardstick itself is the reference's
        e16, eact = relerr(outs["bf16", mode], outs["fp32", mode]), relerr(outs["bf16_act", mode], outs["fp32", mode])
        print("dsde %s reverse_%s T=%d vs the fp32 engine: bf16 %.3g, bf16_act %.3g" % (tag, mode, int(Topt), e16, eact))
        assert np.isfinite(outs["bf16_act", mode]).all()
        assert eact <= 3 * e16, (mode, eact, e16)
        assert eact < 5e-2


# ---------------------------------------------------------------------------------------------
# pins for the operand-only modes (fp32 storage, fp32 attention core)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol32", [("bf16", 3e-2), ("fp16", 4e-3)])
def test_operand_only_modes_pinned(golden, dtype, tol32):
    g = golden.dsde
    tag = "nf64d4_1x64x64"
    nf, depth, B, H, W = (int(v) for v in g[tag + "/cfg"])
    m, params = dsde_model(nf, depth, dtype)
    _, xT = O.synth_inputs(1234, B, H, W, max_sigma=25)
    t = int(g[tag + "/ts"][0])
    y = m(torch.from_numpy(xT).to(DEV), t).cpu().numpy()
    with (O.bf16_convs() if dtype == "bf16" else O.f16_convs()):
        ref = O.uncond_unet_forward(params, xT, t, depth=depth, dtype=np.float64)
    e_oracle, e_fp32 = relerr(y, ref), relerr(y, g[tag + "/t%d" % t])
    print("dsde %s forward: vs the oracle's restatement %.3g, vs the fp32 reference %.3g" % (dtype, e_oracle, e_fp32))
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    assert b"full_attention (bf16 operands + storage)" not in buf.value
    assert e_oracle < 2e-2
    assert 0 < e_fp32 < tol32
