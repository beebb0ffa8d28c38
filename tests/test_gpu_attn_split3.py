"""GPU tests of the fused LinearAttention kernels' three-piece mode (csrc/linear_attn.hip, AttnMode::Bf16x3 of attn_kv_ctx_kernel / attn_q_out_fused_kernel: the k / v, q and
to_out projections on three bf16 pieces per operand and six products; plan rule Builder::split3_attn_adopts, knob IRSDE_SPLIT3_ATTN, hook
irsde_debug_force_split3_attn).

Block bar: error against the float64 block (O.attn_block) relative to the branch's maximum — at most 2 x what the f32 kernels give on the same inputs in the same
test, and below the 5e-5 of test_gpu_parity.py::test_fused_attention_block_vs_oracle.  The pieces carry all 24 significand bits, so both errors are fp32 rounding
of the same size; the factor 2 covers the different summation order.  Network bar: 1e-4 against the reference golden, as for the f32 kernels.  Every test prints
its figures before it asserts; the measured columns are in profiles/attn_split3.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

from test_gpu_parity import DEV, relerr, _sample, _ATTN_BLOCK_LEVEL

pytestmark = pytest.mark.gpu

TAG = "projection (bf16x3)"


@pytest.fixture()
def hook():
    """The process-wide attention hook (and the GEMMs' master hook) back at their defaults afterwards."""
    L = _lib.lib()
    yield L
    L.irsde_debug_force_split3_attn(-1)
    L.irsde_debug_force_split3(-1)


def _model(params, nf, depth, flags=0):
    m = P.ConditionalUNet(3, 3, nf, depth=depth)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    m.engine_flags |= flags
    return m.to(DEV).eval()


def _describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return buf.value.decode()


def _attn_rows(d):
    return [l for l in d.splitlines() if "linear_attention LayerNorm +" in l and "(fused)" in l]


@pytest.mark.parametrize("size,nb", [((64, 64), 1), ((72, 88), 2)])
def test_block_vs_float64_against_the_f32_kernels(hook, size, nb):
    """Every fused block (C = 64 / 128 / 256, five of them) against the float64 block computed from the block's own input (debug taps), with to_out.0.weight scaled by
    the level's pixel count so that the branch is O(1).  72 x 88 (padded 80 x 96), B = 2: 480 pixels at level 2 — partial 64-pixel tiles and chunk tails at every
    level, more than one image in the grid."""
    nf, depth = 64, 4
    Hp, Wp = -(-size[0] // 16) * 16, -(-size[1] // 16) * 16
    params = dict(O.synth_params(seed=0, nf=nf, depth=depth))
    for pref, lvl in _ATTN_BLOCK_LEVEL.items():
        params[pref + "fn.fn.to_out.0.weight"] = params[pref + "fn.fn.to_out.0.weight"] * np.float32((Hp >> lvl) * (Wp >> lvl))
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    lq, xT = O.synth_inputs(1234, nb, size[0], size[1])
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)

    def errors(m):
        out = {}
        for pref in _ATTN_BLOCK_LEVEL:
            xin = m.debug_tap(pref[:-3] + ".1").numpy().astype(np.float64)
            got = m.debug_tap(pref[:-1]).numpy().astype(np.float64)
            full = O.attn_block(p64, pref, xin)
            branch = float(np.abs(full - xin).max())
            assert branch > 0.5, pref                      # the attention branch is what is being compared
            out[pref] = (xin.shape[1], float(np.abs(got - full).max()) / branch)
        return out

    hook.irsde_debug_force_split3_attn(2)
    m3 = _model(params, nf, depth, _lib.FLAG_KEEP_ACTIVATIONS)
    m3(x, c, 50)
    rows = _attn_rows(_describe(m3, nb, size[0], size[1]))
    assert len(rows) == 10 and all(TAG in r for r in rows), rows     # an instance exists for every fused block
    e3 = errors(m3)
    mf = _model(params, nf, depth, _lib.FLAG_KEEP_ACTIVATIONS | _lib.FLAG_NO_SPLIT3)
    mf(x, c, 50)
    rows = _attn_rows(_describe(mf, nb, size[0], size[1]))
    assert len(rows) == 10 and not any("bf16x3" in r for r in rows), rows
    ef = errors(mf)
    for pref in _ATTN_BLOCK_LEVEL:
        print("%dx%d B=%d %s C=%d: three-piece %.3g, f32 kernels %.3g" % (size[0], size[1], nb, pref, e3[pref][0], e3[pref][1], ef[pref][1]))
    for pref in _ATTN_BLOCK_LEVEL:
        assert e3[pref][1] <= 2 * ef[pref][1] and e3[pref][1] < 5e-5, (pref, e3[pref], ef[pref])


def test_twin_flag_equals_knob_0_and_differs_from_forced(hook):
    nf, depth, B, H, W = 32, 2, 2, 24, 20
    params = O.synth_params(seed=0, nf=nf, depth=depth)
    lq, xT = O.synth_inputs(1234, B, H, W)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    hook.irsde_debug_force_split3_attn(2)
    on = _model(params, nf, depth)
    d_on = _describe(on, B, H, W)
    y_on = on(x, c, 50).cpu().numpy()
    flagged = _model(params, nf, depth, _lib.FLAG_NO_SPLIT3)
    d_flag = _describe(flagged, B, H, W)
    y_flag = flagged(x, c, 50).cpu().numpy()
    hook.irsde_debug_force_split3_attn(0)
    off = _model(params, nf, depth)
    d_off = _describe(off, B, H, W)
    y_off = off(x, c, 50).cpu().numpy()
    assert TAG in d_on and "bf16x3" not in "\n".join(_attn_rows(d_flag)) and "bf16x3" not in "\n".join(_attn_rows(d_off))
    assert _attn_rows(d_flag) == _attn_rows(d_off) and len(_attn_rows(d_off)) == len(_attn_rows(d_on)) > 0
    # (knob 0 leaves the GEMMs' rule alone and this network's GEMMs are below that rule's floor: the two plans are the same launches)
    assert np.array_equal(y_flag, y_off)
    assert np.isfinite(y_on).all() and not np.array_equal(y_on, y_off)   # the forced mode is a different arithmetic: the comparison above compares something
    # the GEMMs' master mode 0 turns the attention mode off too, its mode 2 does not force it
    hook.irsde_debug_force_split3_attn(2)
    hook.irsde_debug_force_split3(0)
    assert "bf16x3" not in _describe(_model(params, nf, depth), B, H, W)
    hook.irsde_debug_force_split3_attn(0)
    hook.irsde_debug_force_split3(2)
    assert "bf16x3" not in "\n".join(_attn_rows(_describe(_model(params, nf, depth), B, H, W)))


def test_graph_replay_is_bit_identical_to_eager(hook):
    nf, depth, B, H, W, T = 32, 2, 2, 24, 20, 2
    hook.irsde_debug_force_split3_attn(2)
    m = _model(O.synth_params(seed=0, nf=nf, depth=depth), nf, depth)
    assert TAG in _describe(m, B, H, W)
    lq, xT = O.synth_inputs(5, B, H, W)
    z = O.synth_noise(7, T, (B, 3, H, W))
    eager = _sample(m, "sde", T, lq, xT, z, graph=False)
    graph = _sample(m, "sde", T, lq, xT, z, graph=True)
    assert np.isfinite(eager).all() and np.array_equal(eager, graph)


def test_attention_sensitive_forward_vs_reference(golden, hook):
    """The REAL reference with attention-sensitive weights (tests/golden/forward_attn.npz) at its smallest tag, every fused block forced onto the three-piece mode."""
    g = golden.forward_attn
    tag = "nf64d4_1x32x32"
    nf, depth, B, H, W, t = (int(v) for v in g[tag + "/cfg"])
    params = O.attn_sensitive_params(O.synth_params(seed=0, nf=nf, depth=depth), H, W, depth)
    hook.irsde_debug_force_split3_attn(2)
    m = _model(params, nf, depth)
    rows = _attn_rows(_describe(m, B, H, W))
    assert len(rows) == 10 and all(TAG in r for r in rows), rows
    lq, xT = O.synth_inputs(1234, B, H, W)
    e = relerr(m(torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV), t).cpu().numpy(), g[tag + "/y"])
    print("attention-sensitive forward %s, three-piece attention forced, vs the reference: %.3g" % (tag, e))
    assert e < 1e-4
