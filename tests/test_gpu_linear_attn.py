"""The LinearAttention kernels of csrc/linear_attn.hip one block at a time against the float64 references of tests/linear_attn_oracle.py (run with -m gpu on an
MI355X): every row of the two instance tables (23 attn_kv_ctx_kernel, 18 attn_q_out_fused_kernel) through irsde_debug_attn_block, the ln_g == nullptr form of
the k / v kernel + attn_out_kernel<float> at stride 128 (route 1) and the three-pass kernels on a q | k | v tensor in f32 and bf16 storage (route 2) through
irsde_debug_attn_core.  The rows come from irsde_debug_attn_choice, not from a list typed in here: a row added to a table is covered, or the last test fails.

Shapes (B, N), geometry asserted in tests/test_linear_attn_host.py: (1, 72) less than one tile (three-piece mode: 64 + 8); (3, 520) four full 128-pixel chunks +
an 8-pixel tail chunk, several images ([B] strides of the workspace); (16, 4200) chunk_len 136 — one full tile + an 8-pixel tail per chunk, tiles that start off
the 128 grid, a partial last chunk; (16, 7680) at C = 64, the production geometry (chunk_len 240).  Every N is a multiple of 4, the least a network level can
produce; the hooks REFUSE any other N (asserted in the host file), so no kernel is claimed to be specified there.

Bars (relative to the branch maximum for the block, to max |ref| for the core), all the project's own:
  F32, PairF16, Bf16x3, routes 1 / 2 in f32: max < 5e-5 (test_gpu_parity.py::test_fused_attention_block_vs_oracle); Bf16x3 also <= 2 x the F32 kernels' error on
    the same inputs (test_gpu_attn_split3.py).
  Bf16 / Fp16 operands against O.attn_block_fused16: max 3e-3 / 6e-4, rms 2e-4 / 4e-5, and rms against the restatement < 0.5 x rms against the unrounded block.
  Bf16 + bf16 storage: |got - ref| <= 2^-7 |ref| + 3e-3 branch, fewer than 25 % of the elements differ from the restatement at all.
  Route 2 in bf16 storage: |got - round_bf16(ref)| <= 2^-7 |ref| + 1e-6, fewer than 2 % of the elements differ at all.
Bit for bit: two calls agree; image b of a batch equals the same image alone where the chunk geometry is the same (the choice hook says where).  Outputs start
as NaN between sentinel guards: every element written, nothing behind row N touched.  Every test prints its figures before it asserts (profiles/attn_parity.md)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import linear_attn_oracle as A
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
from test_linear_attn_host import BF16, BF16X3, F32, FP16, PAIR, choice, table_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 1024, -12345.5
MODE_NAME = {F32: "F32", PAIR: "PairF16", BF16: "Bf16", FP16: "Fp16", BF16X3: "Bf16x3"}

ROWS = table_rows()                                                   # (C, mode, act_bf16, kv_row, qo_row), from the library's tables
FUSED = [r for r in ROWS if r[4] >= 0]                                # both kernels exist: the fused block
KV_F32 = [r for r in ROWS if r[1] == F32]                             # the k / v kernel without LayerNorm: route 1
_launched = {"kv": set(), "qo": set()}                                # table rows this file has launched


def _mode_order(r):   # per (shape, C): the modes that share a reference next to each other, F32 first (the three-piece bar needs its error)
    return (r[0], {F32: 0, PAIR: 1, BF16X3: 2, BF16: 3 + r[2], FP16: 5}[r[1]])


def _id(r, shape):
    return "C%d-%s%s-B%dxN%d" % (r[0], MODE_NAME[r[1]], "+act" if r[2] else "", shape[0], shape[1])


BLOCK_CASES = [pytest.param(r, s, id=_id(r, s), marks=pytest.mark.gpu) for s in A.SHAPES for r in sorted(FUSED, key=_mode_order)]
ROUTE1_CASES = [pytest.param(r, s, id=_id(r, s), marks=pytest.mark.gpu) for s in A.SHAPES for r in KV_F32]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def hptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


class Guarded:
    """An output tensor of `shape` inside a buffer with a sentinel guard on both sides; NaN until written."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[GUARD:GUARD + self.n].fill_(float("nan"))

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def result(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.n:] == SENTINEL).all(), what + ": write outside the tensor"
        out = h[GUARD:GUARD + self.n].reshape(self.shape)
        assert np.isfinite(out).all(), what + ": %d elements not written or not finite" % int((~np.isfinite(out)).sum())
        return out


def run_block(inp, mode, act, x=None):
    """irsde_debug_attn_block on the generator's weights and x [B][N][C] (default: the generator's), twice: the two results must agree bit for bit"""
    x = inp["x"] if x is None else np.ascontiguousarray(x)
    B, N, C = x.shape
    d = choice(C, mode, act, N, B)
    outs = []
    with torch.cuda.device(DEV):
        dx = dev(x)
        for _ in range(2):
            y = Guarded(B, N, C)
            _lib.check(_lib.lib().irsde_debug_attn_block(ctypes.c_void_p(dx.data_ptr()), B, N, C, hptr(inp["g1"]), hptr(inp["wqkv"]), hptr(inp["wo"]), hptr(inp["bo"]),
                                                         hptr(inp["g2"]), mode, act, y.ptr(), _lib.stream_ptr()))
            outs.append(y.result("attn_block C=%d mode=%d act=%d B=%d N=%d" % (C, mode, act, B, N)))
    _launched["kv"].add(d["kv_row"])
    _launched["qo"].add(d["qo_row"])
    assert np.array_equal(outs[0], outs[1]), "two calls differ"
    return outs[0]


def run_core(route, tensor, C=0, wkv=None, q=None, bf16=0):
    """irsde_debug_attn_core, twice; tensor [B][N][C] (route 1: xn) or [B][N][384] (route 2)"""
    B, N = tensor.shape[:2]
    outs = []
    with torch.cuda.device(DEV):
        dt, dq = dev(tensor), (dev(q) if q is not None else None)
        for _ in range(2):
            o = Guarded(B, N, A.HID)
            _lib.check(_lib.lib().irsde_debug_attn_core(route, ctypes.c_void_p(dt.data_ptr()), B, N, C, hptr(wkv) if wkv is not None else None,
                                                        ctypes.c_void_p(dq.data_ptr()) if dq is not None else None, bf16, o.ptr(), _lib.stream_ptr()))
            outs.append(o.result("attn_core route %d C=%d B=%d N=%d bf16=%d" % (route, C, B, N, bf16)))
    if route == 1:
        _launched["kv"].add(choice(C, F32, 0, N, B)["kv_row"])
    assert np.array_equal(outs[0], outs[1]), "two calls differ"
    return outs[0]


def report(route, mode, C, B, N, mx, rms, extra=""):
    print("attn_parity | %s | %s | %d | %d x %d | %.3g | %.3g |%s" % (route, mode, C, B, N, mx, rms, extra))


# references: computed once per (C, shape) and shared by the modes that use them (the cases are ordered so that they follow each other)
@functools.lru_cache(maxsize=2)
def ref_full(C, B, N, stored):
    """float64 block and its branch maximum; stored: from the x a bf16 tensor holds"""
    inp = A.make_inputs(C, B, N)
    x = O.round_bf16(inp["x"]) if stored else inp["x"]
    full = A.block(inp, x)
    return full, A.branch_max(full, x)


_f32_error = {}   # (C, B, N) -> max error of the F32 kernels: the three-piece mode's second bar


def f32_error(C, B, N):
    if (C, B, N) not in _f32_error:
        full, branch = ref_full(C, B, N, False)
        _f32_error[(C, B, N)] = A.errors(run_block(A.make_inputs(C, B, N), F32, 0), full, branch)[0]
    return _f32_error[(C, B, N)]


def check_block(C, mode, act, B, N):
    inp = A.make_inputs(C, B, N)
    got = run_block(inp, mode, act)
    full, branch = ref_full(C, B, N, bool(act))
    name = MODE_NAME[mode] + ("+act" if act else "")
    assert branch > 0.5                                   # the attention branch is what is being compared
    assert np.abs(got - inp["x"]).max() > 0.5
    if mode in (F32, PAIR, BF16X3):
        mx, rms = A.errors(got, full, branch)
        if mode == F32:
            _f32_error[(C, B, N)] = mx
        ef = f32_error(C, B, N) if mode == BF16X3 else None
        report("block", name, C, B, N, mx, rms, " F32 kernels %.3g" % ef if ef is not None else "")
        assert mx < A.BAR, (name, C, B, N, mx)
        if mode == BF16X3:
            assert mx <= 2 * ef, (C, B, N, mx, ef)
        return
    ref = A.block16(inp, f16=mode == FP16, store_bf16=bool(act))
    e_ref, rms_ref = A.errors(got, ref, branch)
    e_full, rms_full = A.errors(got, full, branch)
    if act:
        err = np.abs(got - ref)
        share = float((err > 0).mean())
        report("block", name, C, B, N, e_ref, rms_ref, " differing %.3g; vs the unrounded block max %.3g rms %.3g" % (share, e_full, rms_full))
        assert (err <= np.abs(ref) * 2.0 ** -7 + 3e-3 * branch).all(), (C, B, N, float(err.max()))
        assert share < 0.25, (C, B, N, share)
    else:
        report("block", name, C, B, N, e_ref, rms_ref, " vs the unrounded block max %.3g rms %.3g" % (e_full, rms_full))
        assert e_ref < (6e-4 if mode == FP16 else 3e-3) and rms_ref < (4e-5 if mode == FP16 else 2e-4), (name, C, B, N, e_ref, rms_ref)
        assert rms_ref < 0.5 * rms_full, (name, C, B, N, rms_ref, rms_full)     # the restatement explains the kernel


@pytest.mark.parametrize("row,shape", BLOCK_CASES)
def test_fused_block_row_vs_oracle(row, shape):
    C, mode, act = row[:3]
    check_block(C, mode, act, *shape)


def check_route1(C, B, N):
    inp = A.make_inputs(C, B, N)
    xn, qkv = A.core_inputs(inp)
    q = np.ascontiguousarray(qkv[..., :A.HID])
    wkv = np.ascontiguousarray(inp["wqkv"][A.HID:])
    got = run_core(1, xn, C, wkv, q)
    ref = A.core_ref_route1(inp, xn, q)
    mx, rms = A.errors(got, ref, float(np.abs(ref).max()))
    report("core 1 (k, v from xn; q tensor)", "F32", C, B, N, mx, rms)
    assert mx < A.BAR, (C, B, N, mx)


@pytest.mark.parametrize("row,shape", ROUTE1_CASES)
def test_kv_context_without_layernorm_and_q_out_vs_oracle(row, shape):
    """route 1: attn_kv_ctx_kernel with ln_g == nullptr (the only form of the C = 32, 96, 160, 192, 224 instances; the non-power-of-two staging branch) +
    attn_ctx_finalize_kernel + attn_out_kernel<float> on a q tensor of stride 128"""
    check_route1(row[0], *shape)


def check_route2(B, N, bf16):
    qkv = A.core_inputs(A.make_inputs(64, B, N))[1]
    if bf16:
        qkv = O.round_bf16(qkv)                             # what the hook's bf16 copy holds
    got = run_core(2, qkv, bf16=bf16)
    ref = A.core(qkv)
    scale = float(np.abs(ref).max())
    if not bf16:
        mx, rms = A.errors(got, ref, scale)
        report("core 2 (q | k | v tensor)", "f32 storage", 64, B, N, mx, rms)
        assert mx < A.BAR, (B, N, mx)
        return got
    rref = O.round_bf16(ref)
    err = np.abs(got - rref)
    share = float((err > 0).mean())
    mx, rms = A.errors(got, rref, scale)
    report("core 2 (q | k | v tensor)", "bf16 storage", 64, B, N, mx, rms, " differing %.3g" % share)
    assert (err <= np.abs(ref) * 2.0 ** -7 + 1e-6).all(), (B, N, float(err.max()))
    assert share < 0.02, (B, N, share)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "B%dxN%d" % s)
def test_three_pass_kernels_on_a_qkv_tensor_vs_oracle(shape, bf16):
    """route 2: attn_ctx_partial_kernel<T> + attn_ctx_finalize_kernel + attn_out_kernel<T> at stride 384, T = float / bf16"""
    check_route2(shape[0], shape[1], bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["F32", "Bf16x3", "route1"])
def test_production_geometry(what):
    """80 x 96 images at B = 16: N = 7680, chunk_len 240 = 128 + 112 (three-piece mode: 3 x 64 + 48) — the plain production case, C = 64"""
    B, N = A.PRODUCTION
    if what == "route1":
        check_route1(64, B, N)
    else:
        check_block(64, F32 if what == "F32" else BF16X3, 0, B, N)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [pytest.param(r, id=_id(r, A.SHAPES[1])) for r in sorted(FUSED, key=_mode_order)])
def test_image_of_a_batch_equals_the_image_alone(row):
    """The kernels of an image see nothing of the batch but the chunk geometry: where that is the same (the choice hook says so: 520 pixels at B = 3 and B = 1),
    the last image of the batch equals the same image run alone, bit for bit — a workspace stride taken from the wrong image cannot hide behind a bar."""
    C, mode, act = row[:3]
    B, N = A.SHAPES[1]
    a, b = choice(C, mode, act, N, B), choice(C, mode, act, N, 1)
    assert (a["chunk_len"], a["nch"]) == (b["chunk_len"], b["nch"])
    inp = A.make_inputs(C, B, N)
    batch = run_block(inp, mode, act)
    alone = run_block(inp, mode, act, inp["x"][B - 1:])
    assert np.array_equal(batch[B - 1:], alone)
    # (at 4200 pixels B = 16 and B = 1 chunk differently: other sums, no comparison)
    c, d = choice(C, mode, act, A.SHAPES[2][1], A.SHAPES[2][0]), choice(C, mode, act, A.SHAPES[2][1], 1)
    assert (c["chunk_len"], c["nch"]) != (d["chunk_len"], d["nch"])


@pytest.mark.gpu
def test_core_image_of_a_batch_equals_the_image_alone():
    B, N = A.SHAPES[1]
    inp = A.make_inputs(64, B, N)
    xn, qkv = A.core_inputs(inp)
    q, wkv = np.ascontiguousarray(qkv[..., :A.HID]), np.ascontiguousarray(inp["wqkv"][A.HID:])
    assert np.array_equal(run_core(1, xn, 64, wkv, q)[B - 1:], run_core(1, xn[B - 1:], 64, wkv, q[B - 1:]))
    for bf16 in (0, 1):
        assert np.array_equal(run_core(2, qkv, bf16=bf16)[B - 1:], run_core(2, qkv[B - 1:], bf16=bf16))


@pytest.mark.gpu
def test_every_table_row_was_launched():
    """Runs last: the tests above (the whole file, in order) have launched every row of both instance tables at least once."""
    d = choice(64, F32, 0, 128, 1)
    kv, qo = sorted(_launched["kv"] - {-1}), sorted(_launched["qo"] - {-1})
    print("attn_kv_ctx_kernel rows launched: %d/%d; attn_q_out_fused_kernel rows launched: %d/%d" % (len(kv), d["kv_rows"], len(qo), d["qo_rows"]))
    assert kv == list(range(d["kv_rows"])) and qo == list(range(d["qo_rows"])), (kv, qo)
    assert (d["kv_rows"], d["qo_rows"]) == (23, 18)
