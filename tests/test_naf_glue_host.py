"""The kernel-level NAFBlock glue tests (tests/test_gpu_naf_glue.py) checked without a GPU: every GPU shape takes the route it was chosen for
(the launch rules restated in tests/naf_glue_oracle.py: dw_geom mirrors csrc/kernels_misc.hip dw_geom, sca_two_kernel the threshold in
launch_sca, ln_geom launch_ln_t, tlsc_geom the segment arithmetic of csrc/tlsc_pool.hip axis_sum), a float32 emulation of the kernels' summation
order stays inside every elementwise bound, and every deliberately wrong reference moves the test's metric to at least 10 x its bar."""
import numpy as np
import pytest

import naf_glue_oracle as G
import tlsc_oracle as TL


# ---------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------
def test_gate_shapes_take_their_routes():
    geo = {s: G.dw_geom(*s[1:]) for s in G.GATE_SHAPES}
    two = {s: G.sca_two_kernel(geo[s]["ntiles"], s[3]) for s in G.GATE_SHAPES}
    assert [s for s in G.GATE_SHAPES if two[s]] == [(2, 264, 4, 1024)]
    g = geo[(3, 10, 13, 32)]
    assert 10 % 4 and g["PP"] == 32 and g["run"] == 4 and g["tiles_x"] == 1 and 13 < g["PP"] * g["run"]          # lanes with x0 >= W
    g = geo[(2, 7, 50, 64)]
    assert g["PP"] == 16 and g["run"] == 4 and 50 - 12 * g["run"] == 2                                          # last working lane: 2 columns
    assert geo[(1, 5, 300, 32)]["run"] == 10 and geo[(1, 5, 300, 32)]["tiles_x"] == 1
    g = geo[(2, 4, 600, 32)]
    assert g["run"] == 16 and g["tiles_x"] == 2 and 600 % (g["PP"] * g["run"]) != 0
    exits = set()   # columns a lane really walks, mod 3: the unrolled slot rotation leaves after its 1st, 2nd or 3rd step
    for (B, H, W, c), g in geo.items():
        for lane in range(g["tiles_x"] * g["PP"]):
            n = min((lane + 1) * g["run"], W) - lane * g["run"]
            if n > 0:
                exits.add(n % 3)
    assert exits == {0, 1, 2}
    for s in [(2, 6, 23, 96), (1, 5, 9, 384)]:
        assert 256 % geo[s]["gpp"] != 0 and geo[s]["PP"] * geo[s]["gpp"] < 256                                  # idle lanes in the LDS reduction
    g = geo[(1, 6, 40, 1024)]
    assert g["PP"] == 1 and g["tiles_x"] == 3 and g["passes"] == 1
    assert geo[(1, 5, 6, 2048)]["passes"] == 2
    g = geo[(2, 264, 4, 1024)]
    assert g["ntiles"] == 66 and g["ntiles"] % 4 and g["ntiles"] * 1024 > 65536


def test_tlsc_shapes_take_their_routes():
    t = {s: G.tlsc_geom(s[1], s[2], s[4], s[5]) for s in G.TLSC_SHAPES}
    g = t[(2, 9, 20, 32, 9, 5)]
    assert g["nh"] == 1 and g["segs_w"] == [8, 8]
    g = t[(3, 11, 26, 32, 4, 9)]
    assert g["segs_h"] == [8] and g["segs_w"] == [8, 8, 2] and (g["top"], g["bottom"]) == (1, 2)
    g = t[(1, 40, 13, 64, 1, 1)]
    assert (g["nh"], g["nw"], g["top"], g["left"]) == (40, 13, 0, 0)
    assert (t[(1, 17, 9, 32, 17, 9)]["nh"], t[(1, 17, 9, 32, 17, 9)]["nw"]) == (1, 1)
    assert t[(2, 7, 4, 1024, 3, 2)]["segs_h"] == [5] and t[(2, 7, 4, 1024, 3, 2)]["segs_w"] == [3]
    g = t[(1, 96, 128, 32, 48, 104)]
    assert len(g["segs_h"]) == 7 and g["segs_w"] == [8, 8, 8, 1]


def test_ln_shapes_take_their_routes():
    geo = {s: G.ln_geom(s[0] * s[1], s[2]) for s in G.LN_SHAPES}
    assert geo[(3, 25, 32)]["KV"] == 1 and geo[(3, 25, 32)]["idle"] == 0
    for s in [(2, 7, 96), (1, 5, 160), (1, 9, 1536)]:
        assert geo[s]["idle"] > 0, s
    assert geo[(2, 3, 1024)]["KV"] == 4
    assert geo[(1, 9, 1536)]["KV"] == 8 and geo[(1, 3, 2048)]["KV"] == 8 and geo[(1, 3, 2048)]["idle"] == 0
    assert all(geo[s]["trips"] == 1 for s in G.LN_SHAPES[:-1]) and geo[(1, 16387, 1024)]["trips"] == 2


def test_lnconv_shapes_straddle_images():
    for B, ppi, c, Cout, modes in G.LNCONV_SHAPES:
        assert c in (64, 128, 256) and Cout % 64 == 0
        if B > 1:
            assert ppi % 64 != 0 and any((b * ppi) // 64 == (b * ppi - 1) // 64 for b in range(1, B))   # one 64-pixel tile holds two images
    assert {c for _, _, c, _, m in G.LNCONV_SHAPES if 0 in m} == {c for _, _, c, _, m in G.LNCONV_SHAPES if 2 in m} == {64, 128, 256}


# ---------------------------------------------------------------------------------------------
# conv2 + SimpleGate + SCA
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.GATE_SHAPES)
def test_gate_sca_emulation_inside_bounds_and_mutations_outside(shape):
    inp = G.gate_inputs(*shape)
    ref, bound = G.gate_ref(inp)
    m = G.gate_metrics(G.gate_emulate_f32(inp), ref, bound)
    print(shape, "float32 emulation / bound:", {k: "%.3g" % v for k, v in m.items()})
    assert max(m.values()) <= 1.0, m
    for mut in G.GATE_MUTATIONS:
        if not G.gate_mutation_applies(mut, *shape):
            continue
        worst = max(G.gate_metrics(G.gate_ref(inp, mut)[0], ref, bound).values())
        print("  %-12s %.3g x the bar" % (mut, worst))
        assert worst >= 10.0, (shape, mut, worst)
    # offsets U(1, 2): the pooled means are O(1) and differ between images
    assert np.abs(ref["mean"]).mean() > 0.3 and (shape[0] == 1 or np.abs(ref["mean"][0] - ref["mean"][-1]).mean() > 0.1)


# ---------------------------------------------------------------------------------------------
# TLSC
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.TLSC_SHAPES)
def test_tlsc_emulation_inside_bounds_and_mutations_outside(shape):
    B, h, w, c, k1, k2 = shape
    inp = G.tlsc_inputs(*shape)
    ref, bound = G.tlsc_ref(inp)
    m = G.tlsc_metrics(G.tlsc_emulate_f32(inp), ref, bound)
    print(shape, "float32 emulation / bound:", {k: "%.3g" % v for k, v in m.items()})
    assert max(m.values()) <= 1.0, m
    for mut in G.TLSC_MUTATIONS:
        if not G.tlsc_mutation_applies(mut, *shape):
            continue
        worst = max(G.tlsc_metrics(G.tlsc_ref(inp, mut)[0], ref, bound).values())
        print("  %-12s %.3g x the bar" % (mut, worst))
        assert worst >= 10.0, (shape, mut, worst)
    # the replicate pad of the compact map is the reference pool's output
    assert np.array_equal(G.replicate_pad(ref["pooled"], h, w, k1, k2), np.broadcast_to(TL.local_pool(inp["g"].astype(np.float64), (k1, k2)), inp["g"].shape))
    if (k1, k2) == (h, w):
        assert np.allclose(ref["pooled"][:, :, 0, 0], inp["g"].astype(np.float64).mean(axis=(2, 3)), rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------
# LayerNorm + FiLM, and the convolution kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("shape", G.LN_SHAPES)
def test_ln_film_bar_and_mutations(shape, per_image):
    B = shape[0]
    inp = G.ln_inputs(*shape)
    ref, bar, self_err = G.ln_ref(inp, per_image)
    print(shape, "float32 restatement %.3g -> bar %.3g" % (self_err, bar))
    assert 0 < self_err and bar <= G.LN_CAP
    for mut in G.LN_MUTATIONS:
        if not G.ln_mutation_applies(mut, B, per_image):
            continue
        e = G.relerr(G.ln_film(inp["x"], inp["g"], inp["fscale"], inp["fshift"], per_image, mut=mut), ref)
        print("  %-12s %.3g = %.3g x the bar" % (mut, e, e / bar))
        assert e >= 10 * bar, (shape, mut, e, bar)


def lnconv_cases():
    for B, ppi, c, Cout, modes in G.LNCONV_SHAPES:
        for mode in modes:
            for lens in ((False, True) if mode == 1 else (False,)):
                yield B, ppi, c, Cout, mode, lens


@pytest.mark.parametrize("B,ppi,c,Cout,mode,lens", list(lnconv_cases()))
def test_lnconv_bar_and_mutations(B, ppi, c, Cout, mode, lens):
    inp = G.lnconv_inputs(B, ppi, c, Cout, mode)
    ref, bar, self_err = G.lnconv_ref(inp, mode, True, lens)
    print((B, ppi, c, Cout), "mode", mode, "lens", lens, "float32 restatement %.3g -> bar %.3g" % (self_err, bar))
    assert bar <= (G.LNCONV_CAP if mode <= 1 else G.PWCONV_BAR)
    n = 0
    for mut in G.LNCONV_MUTATIONS:
        if not G.lnconv_mutation_applies(mut, B, mode, lens):
            continue
        e = G.relerr(G.lnconv(inp, mode, True, lens, mut=mut), ref)
        print("  %-18s %.3g = %.3g x the bar" % (mut, e, e / bar))
        assert e >= 10 * bar, (mode, mut, e, bar)
        n += 1
    assert n >= 1
