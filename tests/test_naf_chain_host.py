"""The kernel-level test of naf_chain_kernel (tests/test_gpu_naf_chain.py) checked without a GPU: the bar of every case comes from the two restatements of
tests/naf_chain_oracle.py alone and stays under the cap, every fp16-held intermediate of the restatement is comfortably inside the fp16 range, every
deliberately wrong reference misses the bar of every case it applies to at least tenfold (and IS the reference where it is said not to apply), and the
fragment order of the 2 / 4-groups-per-image weight streams (naf_chain_split_order, the library's own function) is a permutation of the one-group streams
that hands every pass of the kernel the fragment it expects.  profiles/naf_chain_parity.md quotes this file's printout (pytest -s)."""
import ctypes

import numpy as np
import pytest

from image_restoration_sde_amd import _lib
import naf_chain_oracle as N


@pytest.mark.parametrize("name", list(N.CASES))
def test_bar_and_fp16_range(name):
    groups, B, nb, per_image, lens, film_off, cam_off, zero = N.CASES[name]
    inp = N.inputs(name)
    ref, bar, self_err, stats = N.reference(name)
    held = {k: v for k, v in stats.items() if k != "pooled"}
    print("%-22s float32 flavour vs float64 %.3g -> bar %.3g; max |branch sum| %.3g; fp16-held maxima %s" % (
        name, self_err, bar, np.abs(ref - inp["x"]).max(), {k: "%.3g" % v for k, v in held.items()}))
    assert 0 < self_err and bar == min(4 * self_err, N.CAP)
    assert set(held) == {"norm1", "conv1", "mean", "gated1", "sca", "gated1*sca", "norm2", "gated2"}
    assert max(held.values()) < N.F16_COMFORT, held
    for k in ("conv1_w", "conv2_w", "sca_w", "conv3_w", "conv4_w", "conv5_w"):
        assert np.abs(inp[k]).max() < N.F16_COMFORT
    # the pooled means are O(1) and differ between images; FiLM and lens rows differ by O(1) per image and per block
    pooled = stats["pooled"]
    assert np.abs(pooled).mean() > 0.3
    if B > 1:
        assert np.abs(pooled[:, 0] - pooled[:, -1]).mean() > 0.3
        assert np.abs(inp["film"][0] - inp["film"][-1]).mean() > 0.3 and (not lens or np.abs(inp["cam"][0] - inp["cam"][-1]).mean() > 0.3)
    if nb > 1:
        assert np.abs(inp["film"][:, 0] - inp["film"][:, -1]).mean() > 0.3 and np.abs(inp["cam"][:, 0] - inp["cam"][:, -1]).mean() > 0.3
    if zero:
        assert not inp[zero].any()


@pytest.mark.parametrize("name", list(N.CASES))
def test_mutations_miss_the_bar_tenfold(name):
    inp = N.inputs(name)
    ref, bar, self_err, _ = N.reference(name)
    n = 0
    for mut in N.MUTATIONS:
        e = N.branch_err(N.chain_ref(inp, np.float64, mut=mut), inp["x"], ref)
        if not N.mutation_applies(mut, name):   # the reference by construction: skipped, and shown to be just that
            print("  %-22s %-18s does not apply" % (name, mut))
            assert e == 0.0, (name, mut, e)
            continue
        print("  %-22s %-18s %.3g = %.3g x the bar" % (name, mut, e, e / bar))
        assert e >= 10 * bar, (name, mut, e, bar)
        n += 1
    assert n >= 9


@pytest.mark.parametrize("G,nblocks", [(2, 1), (4, 1), (2, 3), (4, 3)])
def test_split_order_is_a_permutation_of_the_right_fragments(G, nblocks):
    n = 8 * nblocks * N.FRAGS_PER_BLOCK
    order = np.full(n, -1, dtype=np.int32)
    _lib.check(_lib.lib().irsde_debug_naf_chain_split_order(nblocks, G, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n))
    assert np.array_equal(np.sort(order), np.arange(n))
    one, split = N.one_group_fragments(nblocks), N.split_fragments(nblocks, G)
    assert len(one) == len(split) == n and len(set(one)) == n   # every (block, conv, tile, k step) once
    assert [one[i] for i in order] == split
    # refused: a group count the kernel does not have, a wrong length
    L = _lib.lib()
    assert L.irsde_debug_naf_chain_split_order(nblocks, 3, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n) != 0
    assert L.irsde_debug_naf_chain_split_order(nblocks, G, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n - 1) != 0


def test_row_buffer_layout():
    inp = N.inputs("g1_b2_n3_offsets")
    off = N.CASES["g1_b2_n3_offsets"][5]
    buf, stride = N.row_buffer(inp["film"], off)
    assert stride % 4 == 0 and off % 4 == 0 and stride >= off + 3 * N.FILM_ROW
    for b in range(2):
        for i in range(3):
            assert np.array_equal(buf[b * stride + off + i * N.FILM_ROW:][:N.FILM_ROW], inp["film"][b, i])
    assert np.isnan(buf).sum() == 2 * (off + 64)
    assert N.row_buffer(N.inputs("g1_b1_shared_nolens")["film"], 0)[1] == 0
