"""Host tests of the three-piece bf16 GEMM path (csrc/gemm_split.hip gemm_split3i_kernel): its numpy restatement (tests/split3_oracle.py) against float64,
the mutations the GPU test's bar must catch, the operand layout's index formula and the plumbing that needs no device.

Errors: max-abs against the float64 product over max |float64 product|; bar = 3 x the error of numpy's float32 A @ B.T on the same inputs.
Measured here: six products 1.8e-7 .. 9.4e-7 against bars of 1.0e-6 .. 1.9e-6; the smallest mutation (a lost a0 b2 at K = 1024) 2.1e-6 against 1.6e-6.
"""
import os
import re

import numpy as np
import pytest

import split3_oracle as S3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(96, 80, 64), (160, 96, 1024), (128, 128, 1536)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for M, N, K in SHAPES:
        A, B = S3.inputs(M, N, K)
        A, B = A[0], B[0]
        ref = A.astype(np.float64) @ B.astype(np.float64).T
        out[(M, N, K)] = (A, B, ref, S3.bar(A, B, ref))
    return out


def test_three_pieces_reproduce_every_input_exactly(cases):
    for A, B, _, _ in cases.values():
        for X in (A, B):
            p, res = S3.pieces(X)
            assert not res.any()
            assert np.array_equal((p[2].astype(np.float64) + p[1]) + p[0], X.astype(np.float64))
            for q in p:   # every piece is a bf16: the low 16 bits of its f32 image are zero
                assert not (q.view(np.uint32) & 0xFFFF).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_six_products_pass_the_bar(cases, shape):
    A, B, ref, bar = cases[shape]
    e = S3.err(S3.gemm(A, B), ref)
    print("six products %s: %.3g (bar %.3g)" % (shape, e, bar))
    assert e < bar


@pytest.mark.parametrize("shape", SHAPES)
def test_every_lost_product_and_the_two_piece_scheme_miss_the_bar(cases, shape):
    A, B, ref, bar = cases[shape]
    for drop in range(6):
        prods = [p for i, p in enumerate(S3.PRODUCTS) if i != drop]
        e = S3.err(S3.gemm(A, B, prods), ref)
        print("without a%d b%d %s: %.3g (bar %.3g)" % (S3.PRODUCTS[drop] + (shape, e, bar)))
        assert e > bar, S3.PRODUCTS[drop]
    e = S3.err(S3.gemm(A, B, S3.TWO_PIECE, 2), ref)
    print("two pieces %s: %.3g (bar %.3g)" % (shape, e, bar))
    assert e > bar


@pytest.mark.parametrize("rows,K", [(1, 32), (7, 64), (16, 96), (33, 160)])
def test_layout_round_trip(rows, K):
    """Every (row, k, plane) has its own slot inside the component, a row pair's 32-k block is 384 contiguous bytes, and writer + reader give the input back."""
    r, k, p = np.meshgrid(np.arange(rows), np.arange(K), np.arange(3), indexing="ij")
    idx = S3.index(r, k, p, K).ravel()
    assert idx.min() >= 0 and idx.max() < S3.comp_elems(rows, K) and len(np.unique(idx)) == idx.size
    for row in (0, rows - 1):
        for kb in range(K // 32):
            blk = S3.index(np.full(32, row), kb * 32 + np.arange(32), 0, K)
            base = ((row >> 1) * (K // 32) + kb) * 192
            assert np.array_equal(blk, base + (row & 1) * 96 + np.arange(32)) and base * 2 % 128 == 0   # whole 128-byte lines
    X = np.random.RandomState(rows * K).standard_normal((rows, K)).astype(np.float32)
    img = S3.to_layout(X)
    assert np.array_equal(S3.from_layout(img, rows, K), X)
    if rows & 1:   # the pad row is never written
        pad = S3.index(np.full(K, rows), np.arange(K), 0, K)
        assert (img[pad] == 0xFFFF).all()


def test_layout_formula_matches_the_header():
    src = open(os.path.join(ROOT, "image_restoration_sde_amd", "csrc", "split3_layout.h")).read()
    assert "((row >> 1) * nkb + (k >> 5)) * 192 + (row & 1) * 96 + (size_t)p * 32 + (k & 31)" in src
    assert "(rows + 1) & ~(size_t)1" in src and "split3_rows(rows) * K * 3" in src


def test_flag_knob_and_hook_plumbing():
    from image_restoration_sde_amd import _lib
    assert _lib.FLAG_NO_SPLIT3 == 4194304
    hdr = open(os.path.join(ROOT, "include", "irsde_hip.h")).read()
    assert re.search(r"IRSDE_FLAG_NO_SPLIT3\s*=\s*4194304\b", hdr)
    flags = [int(v) for v in re.findall(r"IRSDE_FLAG_\w+\s*=\s*(\d+)", hdr)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)   # one bit each, none shared
    assert "irsde_debug_force_split3" in _lib.SYMBOLS
    plan = open(os.path.join(ROOT, "image_restoration_sde_amd", "csrc", "engine_plan.hip")).read()
    assert 'tuning_env_int("IRSDE_SPLIT3", 1)' in plan
    assert plan.count('tri ? " bf16x3" : ""') == 2   # the marker is appended behind the existing fields of the two descriptions
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "IRSDE_SPLIT3" in design[design.index("### Tuning knobs"):design.index("### Sampler loop")]
    L = _lib.lib()   # host only: the hook stores a process-wide mode
    assert L.irsde_debug_force_split3(2) == 0 and L.irsde_debug_force_split3(-1) == 0
