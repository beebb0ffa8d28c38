"""Host-side checks of the denoising-sde ConditionalUNet in the bf16_act mode (no GPU): the engine accepts the flag combination, the debug hook is exported, and the
oracle of tests/dsde_unet16_oracle.py — the elementwise bar of the bf16 attention kernel and the restatement of the mode — admits the kernel's order of operations and
rejects wrong ones."""
import ctypes
import os
import re

import numpy as np
import pytest

from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import dsde_unet16_oracle as DU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(flags, nf=64, depth=4):
    L = _lib.lib()
    cfg = _lib.Config(3, 3, nf, depth, 0, flags)
    h = ctypes.c_void_p()
    return L, L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)), h


def test_engine_creation_accepts_bf16_act_for_the_unconditional_unet():
    U, B16, ACT = _lib.FLAG_UNCOND_FULLATTN, _lib.FLAG_BF16, _lib.FLAG_BF16_ACT
    for flags in (U | B16 | ACT, U | ACT):
        L, rc, h = _create(flags)
        assert rc == 0, (flags, L.irsde_last_error())
        names = [L.irsde_weight_name(h, i).decode() for i in range(L.irsde_num_weights(h))]
        assert "mid_attn.fn.fn.to_out.weight" in names and "mid_attn.fn.fn.to_out.1.g" not in names   # the full Attention inventory
        L.irsde_destroy(h)
    for extra in (0, U):
        L, rc, _ = _create(extra | _lib.FLAG_NAIVE_CONV | ACT)
        assert rc == -1
        assert L.irsde_last_error() == b"IRSDE_FLAG_BF16_ACT: only the conditional UNet on the MFMA kernels stores bf16 activations"
        L, rc, _ = _create(extra | _lib.FLAG_FP16 | ACT)
        assert rc == -1
        assert b"IRSDE_FLAG_FP16" in L.irsde_last_error() and b"IRSDE_FLAG_BF16_ACT" in L.irsde_last_error()
    assert L.irsde_version() == 107


def test_debug_hook_is_exported_and_declared():
    assert "irsde_debug_full_attention16" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "irsde_debug_full_attention16")
    hdr = open(os.path.join(ROOT, "include", "irsde_hip_debug.h")).read()
    assert re.search(r"\bint\s+irsde_debug_full_attention16\s*\(", hdr)


def _ratio(got, o, A):
    return float((np.abs(got.astype(np.float64) - o) / DU.kernel_bound(o, A)).max())


@pytest.mark.parametrize("B,N", DU.KERNEL_SHAPES)
def test_kernel_order_emulation_stays_inside_the_bound(B, N):
    """32-key tiles, online rescale in fp32, P rounded to bf16 for the product and the row sum, the quotient rounded once: inside the bar on every kernel shape."""
    qkv, o, A = DU.kernel_case(B, N)
    r = _ratio(DU.emulate_kernel(qkv), o, A)
    r64 = _ratio(DU.full_attention16(qkv), o, A) if N <= 1024 else float("nan")
    print("B=%d N=%d: |emulation - o| / bound max %.3f; float64 restatement %.3f" % (B, N, r, r64))
    assert r <= 1.0
    assert not r64 > 1.0


# the shapes on which a mutation changes anything: one key has no softmax to get wrong; a full last tile has no tail; one tile has no running maximum
_MUTATION_SHAPES = {
    "no_scale": [s for s in DU.KERNEL_SHAPES if s[1] > 1],
    "uniform": [s for s in DU.KERNEL_SHAPES if s[1] > 1],
    "tail_unmasked": [s for s in DU.KERNEL_SHAPES if s[1] % 32],
    "kv_swapped": DU.KERNEL_SHAPES,
    "heads_permuted": DU.KERNEL_SHAPES,
    "unnormalised": [s for s in DU.KERNEL_SHAPES if s[1] > 1],
    "stale_max": [s for s in DU.KERNEL_SHAPES if s[1] > 32],
}


@pytest.mark.parametrize("mutation", DU.MUTATIONS)
def test_mutations_miss_the_bound(mutation):
    """A kernel with one of these bugs is at least 10 bars away from the reference somewhere, on the tests' own inputs (q, k entries of std DU.QK_STD = 1.5: logits of
    std 2.25; measured 61 bars at the least, the unmasked tail at N = 31)."""
    for B, N in _MUTATION_SHAPES[mutation]:
        qkv, o, A = DU.kernel_case(B, N)
        r = _ratio(DU.emulate_kernel(qkv, mutation), o, A)
        print("%s B=%d N=%d: %.1f bars" % (mutation, B, N, r))
        assert r >= 10.0, (mutation, B, N, r)


def test_restatement_feels_the_softmax():
    """The mode restatement's mid_attn branch, on the block test's fixture (nf 32, depth 2, 2 x 24 x 20, q / k rows of to_qkv times DU.MID_QK_GAIN = 2: logits of
    std 1.9): replacing the softmax by an average moves it by at least 10 x the block-level bar |ref| 2^-7 + 3e-3 branch (49 bars).  Without the gain
    (logits of std 0.47) it is 10.6 bars, on the edge; the gained weights leave a margin."""
    nf, depth, B, H, W = 32, 2, 2, 24, 20
    base = O.uncond_synth_params(seed=0, nf=nf, depth=depth)
    _, xT = O.synth_inputs(1234, B, H, W, max_sigma=25)
    moved = {}
    for gain in (1.0, DU.MID_QK_GAIN):
        params = DU.gained_params(base, gain)
        taps = {}
        DU.dsde_forward_bf16_act(params, xT, 7, depth=depth, taps=taps)
        p64 = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
        x = taps["mid_block1"]
        with O.bf16_convs(store_bf16=True):
            ref = DU.mid_attn_bf16_act(p64, x)
            avg = DU.mid_attn_bf16_act(p64, x, uniform=True)
        assert np.array_equal(ref, taps["mid_attn"])
        branch = float(np.abs(DU.mid_attn_float64(p64, x) - x).max())
        bar = np.abs(ref) * 2.0 ** -7 + 3e-3 * branch
        moved[gain] = float((np.abs(avg - ref) / bar).max())
        xn = O.layer_norm_c(x, p64["mid_attn.fn.norm.g"])
        qkv = O.conv2d(xn, p64["mid_attn.fn.fn.to_qkv.weight"]).reshape(B, 3 * DU.HID, -1).transpose(0, 2, 1)
        q, k, _ = DU._split(qkv)
        logit_std = float((np.einsum("bhid,bhjd->bhij", q, k) * DU.SCALE).std())
        print("gain %g: logits std %.3g, branch %.3g, average instead of softmax moves mid_attn by %.3g bars" % (gain, logit_std, branch, moved[gain]))
    assert moved[DU.MID_QK_GAIN] >= 10.0
    assert moved[DU.MID_QK_GAIN] > 2 * moved[1.0]
