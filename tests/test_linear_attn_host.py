"""What tests/test_gpu_linear_attn.py relies on, shown without a device: the bars of tests/linear_attn_oracle.py tell a right LinearAttention from a wrong one on
the generator's data, the host-only hook irsde_debug_attn_choice reports the two instance tables of csrc/linear_attn.hip (23 k / v rows, 18 q + out rows, their
dynamic LDS), the chunk geometry of every GPU shape is what the GPU tests say it is, and the hooks refuse what the launchers refuse before they touch a device."""
import ctypes

import numpy as np
import pytest

import linear_attn_oracle as A
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

F32, PAIR, BF16, FP16, BF16X3 = range(5)   # AttnMode
_buf = ctypes.create_string_buffer(512)


def choice(C, mode, act, N, B):
    """the hook's line as a dict of ints (rows as (index, table length))"""
    _lib.check(_lib.lib().irsde_debug_attn_choice(C, mode, act, N, B, _buf, len(_buf)))
    words = _buf.value.decode().replace(" of ", "/").split()
    d = dict(w.split("=") for w in words)
    out = {k: int(v) for k, v in d.items() if "/" not in v}
    for k in ("kv_row", "qo_row"):
        out[k], out[k + "s"] = (int(t) for t in d[k].split("/"))
    return out


def table_rows():
    """every (C, mode, act_bf16) with a row in either table, from the hook: [(C, mode, act, kv_row, qo_row)]"""
    rows = []
    for C in range(16, 513, 16):
        for mode in range(5):
            for act in (0, 1):
                d = choice(C, mode, act, 128, 1)
                if d["kv_row"] >= 0 or d["qo_row"] >= 0:
                    rows.append((C, mode, act, d["kv_row"], d["qo_row"]))
    return rows


@pytest.mark.parametrize("C", A.HOST_C)
def test_the_bar_tells_a_wrong_block_from_a_right_one(C):
    """(a) On the generator's data the float32 evaluation of the oracle stays below a tenth of the 5e-5 bar, and three wrong oracles — one k row off by 1 %,
    v / (N + 1), the last pixel replaced (measured on the other pixels) — exceed five times the bar, at every N."""
    for N in A.HOST_N:
        inp = A.make_inputs(C, 1, N)
        full = A.block(inp)
        branch = A.branch_max(full, inp["x"])
        e32 = A.errors(A.block(inp, dtype=np.float32), full, branch)[0]
        ek = A.errors(A.wrong_k_row(inp), full, branch)[0]
        ev = A.errors(A.wrong_v_norm(inp), full, branch)[0]
        el = A.errors(A.wrong_last_pixel(inp)[:, :-1], full[:, :-1], branch)[0]
        print("C=%d N=%d: branch %.3g; float32 oracle %.3g; k row + 1 %% %.3g; v / (N + 1) %.3g; last pixel replaced %.3g" % (C, N, branch, e32, ek, ev, el))
        assert branch > 0.5
        assert e32 < A.BAR / 10, (N, e32)
        assert min(ek, ev, el) > 5 * A.BAR, (N, ek, ev, el)


def test_bf16_storage_core_bar_has_room():
    """The bf16-storage core is compared with round_bf16(float64 core): at most 2 % of the elements may differ at all.  The float32 evaluation of the oracle on
    the same bf16 inputs, rounded the same way, differs in less than a tenth of that — so the cap measures the kernel, not float32."""
    for C, N in ((64, 72), (64, 520), (256, 200)):
        qkv = O.round_bf16(A.core_inputs(A.make_inputs(C, 1, N))[1])
        ref = O.round_bf16(A.core(qkv))
        got = O.round_bf16(A.core(qkv, dtype=np.float32).astype(np.float64))
        share = float((got != ref).mean())
        print("C=%d N=%d: round_bf16(float32 core) differs from round_bf16(float64 core) in %.3g of the elements" % (C, N, share))
        assert share < 0.002
        assert (np.abs(got - ref) <= np.abs(ref) * 2.0 ** -7 + 1e-6).all()


def test_choice_reports_both_tables_completely():
    """(b) over the (C, mode, act_bf16) grid the hook names exactly the rows 0 .. 22 and 0 .. 17, each once"""
    rows = table_rows()
    kv = sorted(r[3] for r in rows if r[3] >= 0)
    qo = sorted(r[4] for r in rows if r[4] >= 0)
    assert kv == list(range(23)) and qo == list(range(18)), (kv, qo)
    d = choice(64, F32, 0, 128, 1)
    assert (d["kv_rows"], d["qo_rows"]) == (23, 18)
    # the k / v table alone holds the f32 widths between the powers of two; everything with a q + out row has a k / v row
    assert sorted(r[0] for r in rows if r[4] < 0) == [32, 96, 160, 192, 224] and all(r[1] == F32 for r in rows if r[4] < 0)
    assert all(r[3] >= 0 for r in rows)
    assert {(r[0], r[1], r[2]) for r in rows if r[4] >= 0} == ({(C, m, 0) for C in (64, 128, 256) for m in range(5)} | {(C, BF16, 1) for C in (64, 128, 256)})


def kv_lds(C, mode):
    """k / v context: the staged tile — f32 rows of C + 4 floats (128 pixels), or one / two / three 16-bit planes with rows of 2 C + 16 bytes (three: 64 pixels)"""
    if mode == F32:
        return 128 * (C + 4) * 4
    return {PAIR: 2 * 128, BF16: 128, FP16: 128, BF16X3: 3 * 64}[mode] * (2 * C + 16)


def qo_lds(C, mode):
    """q + out: one region = max(xn planes, attention-output planes (128 channels), f32 out tile of max(C, 128) + 4 floats per pixel); the three-piece mode has
    64-pixel tiles and adds 4 x 64 floats of LayerNorm partial sums"""
    px, planes = (64, 3) if mode == BF16X3 else (128, {F32: 0, PAIR: 2, BF16: 1, FP16: 1}[mode])
    region = max(planes * px * (2 * C + 16), planes * px * (2 * 128 + 16), px * (max(C, 128) + 4) * 4)
    return region + (4 * 64 * 4 if mode == BF16X3 else 0)


def test_lds_bytes_follow_the_documented_formulas():
    """(c) and every instance fits the 160 KB of a compute unit"""
    for C, mode, act, kv_row, qo_row in table_rows():
        d = choice(C, mode, act, 128, 1)
        assert d["kv_lds"] == kv_lds(C, mode), (C, mode, d)
        assert d["qo_lds"] == (qo_lds(C, mode) if qo_row >= 0 else 0), (C, mode, d)
        assert max(d["kv_lds"], d["qo_lds"]) <= 160 * 1024
        assert (d["kv_tile"], d["qo_tile"]) == ((64, 64) if mode == BF16X3 else (128, 128))


def test_chunk_geometry_of_the_gpu_shapes():
    """(d) what tests/test_gpu_linear_attn.py says about tails and tile grids"""
    def geo(B, N, mode=F32):
        d = choice(64, mode, 0, N, B)
        return d["chunk_len"], d["nch"], N - (d["nch"] - 1) * d["chunk_len"]
    assert A.SHAPES == [(1, 72), (3, 520), (16, 4200)] and A.PRODUCTION == (16, 7680)
    assert geo(1, 72) == (128, 1, 72)              # less than one tile; the 64-pixel tile of the three-piece mode: 64 + 8
    assert geo(3, 520) == (128, 5, 8)              # four full 128-pixel tiles + an 8-pixel tail chunk
    assert geo(16, 4200) == (136, 31, 120)         # one full tile + an 8-pixel tail per chunk, tiles off the 128 grid, a partial last chunk
    assert geo(16, 7680) == (240, 32, 240)         # 80 x 96 at B = 16: 128 + 112 (three-piece: 3 x 64 + 48)
    assert 136 % 128 == 8 and 136 % 64 == 8 and 120 < 128 and 240 % 128 == 112 and 240 % 64 == 48
    assert geo(1, 72, BF16X3) == geo(1, 72)        # the geometry does not depend on the mode
    # image b of a batch against the same image alone: the same chunks at 520 pixels, other chunks at 4200
    assert geo(1, 520)[:2] == geo(3, 520)[:2] and geo(1, 4200)[:2] != geo(16, 4200)[:2]
    for B, N in A.SHAPES + [A.PRODUCTION]:
        assert N % 4 == 0


def test_refusals_come_before_any_launch():
    """(e) with the launchers' own messages; the pointers are host memory nobody may read"""
    L = _lib.lib()
    host = (ctypes.c_float * 16)()
    p = ctypes.cast(host, ctypes.c_void_p)

    def block(C, mode, act, N=72, B=1):
        assert L.irsde_debug_attn_block(p, B, N, C, p, p, p, p, p, mode, act, p, None) != 0
        return L.irsde_last_error().decode()

    for mode, name in ((PAIR, "fp16-pair"), (BF16, "bf16"), (FP16, "fp16"), (BF16X3, "three-piece bf16")):
        assert "no %s kernel for C = 96" % name in block(96, mode, 0)
    for mode in (F32, PAIR, FP16, BF16X3):
        assert "bf16 activation storage goes with bf16 operands" in block(64, mode, 1)
    assert "attention_q_out_fused: no f32 kernel for C = 32" in block(32, F32, 0)
    assert "mode must be 0 .. 4" in block(64, 5, 0)
    # N is a multiple of 4 at every network level: the hooks refuse anything else
    assert "multiple of 4" in block(64, F32, 0, N=131) and "multiple of 4" in block(64, F32, 0, N=1)
    assert L.irsde_debug_attn_core(1, p, 1, 72, 80, p, p, 0, p, None) != 0 and b"no f32 kernel for C = 80" in L.irsde_last_error()
    assert L.irsde_debug_attn_core(1, p, 1, 72, 64, p, p, 1, p, None) != 0 and b"fp32 tensors only" in L.irsde_last_error()
    assert L.irsde_debug_attn_core(3, p, 1, 72, 64, p, p, 0, p, None) != 0 and b"route must be" in L.irsde_last_error()
    assert L.irsde_debug_attn_core(2, p, 1, 70, 0, None, None, 0, p, None) != 0 and b"multiple of 4" in L.irsde_last_error()
    assert L.irsde_debug_attn_choice(64, 7, 0, 72, 1, _buf, len(_buf)) != 0
    assert L.irsde_version() == 107   # hooks outside the drop-in boundary: the ABI version does not move
