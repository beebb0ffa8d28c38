"""The NAFBlock glue kernels one stage at a time against the float64 restatements of tests/naf_glue_oracle.py (run with -m gpu on an MI355X):
dwconv_gate_kernel + the SCA kernels on both routes (irsde_debug_naf_gate_sca), the TLSC kernels (irsde_debug_tlsc), layernorm_kernel with FiLM
(irsde_debug_ln_film) and naf_lnconv_kernel in its three prologues (irsde_debug_naf_lnconv).  Shapes, what each reaches, the derivation of
every bar and the measured errors: profiles/naf_glue.md; tests/test_naf_glue_host.py shows on the CPU that each shape takes its route and that a
wrong pooled mean, pad, clamp, bias order, image row or variance formula misses these bars at least tenfold.

Every output tensor sits between two guards of 1024 sentinel floats and starts as NaN: after the call the guards must be intact (no write
outside the tensor) and the interior finite (no element left unwritten)."""
import ctypes

import numpy as np
import pytest
import torch

from image_restoration_sde_amd import _lib
import naf_glue_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 1024, -12345.5


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None) if not isinstance(t, np.ndarray) else t.ctypes.data_as(ctypes.c_void_p)


class Guarded:
    """An output tensor of `shape` inside a buffer with a sentinel guard on both sides; NaN until written."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.view = self.buf[GUARD:GUARD + self.n]
        self.view.fill_(float("nan"))

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def result(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.n:] == SENTINEL).all(), what + ": write outside the tensor"
        out = h[GUARD:GUARD + self.n].reshape(self.shape)
        assert np.isfinite(out).all(), what + ": %d elements not written or not finite" % int((~np.isfinite(out)).sum())
        return out


def call(fn, *args):
    with torch.cuda.device(DEV):
        _lib.check(fn(*args, _lib.stream_ptr()))


@pytest.mark.parametrize("B,H,W,c", G.GATE_SHAPES)
def test_gate_sca_vs_oracle(B, H, W, c):
    inp = G.gate_inputs(B, H, W, c)
    ref, bound = G.gate_ref(inp)
    u = dev(nhwc(inp["u"]))
    gated, mean, s = Guarded(B, H, W, c), Guarded(B, c), Guarded(B, c)
    call(_lib.lib().irsde_debug_naf_gate_sca, ptr(u), B, H, W, c, ptr(inp["w"]), ptr(inp["b"]), ptr(inp["sw"]), ptr(inp["sb"]), gated.ptr(), mean.ptr(), s.ptr())
    got = dict(gated=gated.result("gated").transpose(0, 3, 1, 2), mean=mean.result("mean"), s=s.result("s"))
    m = G.gate_metrics(got, ref, bound)
    geo = G.dw_geom(H, W, c)
    print("gate+SCA %s (%s route): error / bound %s" % ((B, H, W, c), "two-kernel" if G.sca_two_kernel(geo["ntiles"], c) else "one-launch",
                                                        {k: "%.3g" % v for k, v in m.items()}))
    assert max(m.values()) <= 1.0, m
    # without mean_out the same s (the mean kernel is an observer, not part of the route)
    s2 = Guarded(B, c)
    call(_lib.lib().irsde_debug_naf_gate_sca, ptr(u), B, H, W, c, ptr(inp["w"]), ptr(inp["b"]), ptr(inp["sw"]), ptr(inp["sb"]), gated.ptr(), None, s2.ptr())
    assert np.array_equal(s2.result("s"), got["s"])


@pytest.mark.parametrize("B,h,w,c,k1,k2", G.TLSC_SHAPES)
def test_tlsc_vs_oracle(B, h, w, c, k1, k2):
    inp = G.tlsc_inputs(B, h, w, c, k1, k2)
    ref, bound = G.tlsc_ref(inp)
    nh, nw = h - k1 + 1, w - k2 + 1
    g, scale = dev(nhwc(inp["g"])), dev(nhwc(inp["scale"]))
    pooled, scaled = Guarded(B, nh, nw, c), Guarded(B, h, w, c)
    call(_lib.lib().irsde_debug_tlsc, ptr(g), B, h, w, c, k1, k2, pooled.ptr(), ptr(scale), scaled.ptr())
    got = dict(pooled=pooled.result("pooled").transpose(0, 3, 1, 2), scaled=scaled.result("scaled").transpose(0, 3, 1, 2))
    m = G.tlsc_metrics(got, ref, bound)
    print("TLSC %s: error / bound %s" % ((B, h, w, c, k1, k2), {k: "%.3g" % v for k, v in m.items()}))
    assert max(m.values()) <= 1.0, m
    assert torch.equal(g, dev(nhwc(inp["g"])))   # the input is left alone (the scale runs on the copy)
    if (nh, nw) == (1, 1):
        gm = inp["g"].astype(np.float64).mean(axis=(2, 3))
        assert G.bound_ratio(got["pooled"][:, :, 0, 0], gm, bound["pooled"][:, :, 0, 0]) <= 1.0


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("B,ppi,C", G.LN_SHAPES)
def test_ln_film_vs_oracle(B, ppi, C, per_image):
    inp = G.ln_inputs(B, ppi, C)
    ref, bar, self_err = G.ln_ref(inp, per_image)
    M = B * ppi
    x, fs, fh = dev(nhwc(inp["x"]).reshape(M, C)), dev(inp["fscale"]), dev(inp["fshift"])
    out = Guarded(M, C)
    call(_lib.lib().irsde_debug_ln_film, ptr(x), M, C, ppi, ptr(inp["g"]), ptr(fs), ptr(fh), C if per_image else 0, out.ptr())
    e = G.relerr(out.result("out"), nhwc(ref).reshape(M, C))
    print("LayerNorm+FiLM %s %s rows: float32 restatement %.3g, bar %.3g, measured %.3g" % ((B, ppi, C), "per-image" if per_image else "shared", self_err, bar, e))
    assert e <= bar, (e, bar)


def lnconv_cases():
    for B, ppi, c, Cout, modes in G.LNCONV_SHAPES:
        for mode in modes:
            for lens in ((False, True) if mode == 1 else (False,)):
                yield B, ppi, c, Cout, mode, lens


@pytest.mark.parametrize("B,ppi,c,Cout,mode,lens", list(lnconv_cases()))
def test_naf_lnconv_vs_oracle(B, ppi, c, Cout, mode, lens):
    inp = G.lnconv_inputs(B, ppi, c, Cout, mode)
    ref, bar, self_err = G.lnconv_ref(inp, mode, True, lens)
    M, Co = B * ppi, Cout // 2 if mode == 1 else Cout
    x, fs, fh = dev(nhwc(inp["x"]).reshape(M, c)), dev(inp["fscale"]), dev(inp["fshift"])
    gf = dev(inp["lens"]) if lens else None
    sc, res = dev(inp["in_scale"]), dev(nhwc(inp["res"]).reshape(M, Cout))
    out = Guarded(M, Co)
    call(_lib.lib().irsde_debug_naf_lnconv, mode, ptr(x), M, c, Cout, ppi, ptr(inp["g"]), ptr(fs), ptr(fh), c, ptr(inp["w"]), ptr(inp["bias"]), ptr(gf), Cout if lens else 0,
         ptr(sc), ptr(inp["ch_scale"]), ptr(res), out.ptr())
    e = G.relerr(out.result("out"), nhwc(ref).reshape(M, Co))
    print("lnconv %s mode %d%s: float32 restatement %.3g, bar %.3g, measured %.3g" % ((B, ppi, c, Cout), mode, " + lens FiLM" if lens else "", self_err, bar, e))
    assert e <= bar, (e, bar)


def test_hooks_refuse_bad_shapes():
    """Refused on the host, before any launch: the call fails with an error string and writes nothing."""
    L = _lib.lib()
    t = torch.zeros(4096, device=DEV)
    h = np.zeros(4096, dtype=np.float32)
    p, q = ptr(t), ptr(h)
    s = _lib.stream_ptr()
    assert L.irsde_debug_naf_gate_sca(p, 1, 4, 4, 6, q, q, q, q, p, None, p, s) != 0 and b"debug_naf_gate_sca" in L.irsde_last_error()
    assert L.irsde_debug_naf_gate_sca(p, 0, 4, 4, 8, q, q, q, q, p, None, p, s) != 0
    assert L.irsde_debug_naf_gate_sca(None, 1, 4, 4, 8, q, q, q, q, p, None, p, s) != 0
    assert L.irsde_debug_tlsc(p, 1, 4, 4, 8, 5, 1, p, p, p, s) != 0 and b"tlsc" in L.irsde_last_error()
    assert L.irsde_debug_tlsc(p, 1, 4, 4, 6, 2, 2, p, p, p, s) != 0
    assert L.irsde_debug_ln_film(p, 4, 2052, 4, q, p, p, 0, p, s) != 0 and b"debug_ln_film" in L.irsde_last_error()
    assert L.irsde_debug_ln_film(p, 4, 30, 4, q, p, p, 0, p, s) != 0
    assert L.irsde_debug_ln_film(p, 4, 32, 4, q, p, p, 2, p, s) != 0
    assert L.irsde_debug_naf_lnconv(0, p, 4, 96, 64, 4, q, p, p, 0, q, q, None, 0, None, None, None, p, s) != 0 and b"debug_naf_lnconv" in L.irsde_last_error()
    assert L.irsde_debug_naf_lnconv(4, p, 4, 64, 64, 4, q, p, p, 0, q, q, None, 0, None, None, None, p, s) != 0
    assert L.irsde_debug_naf_lnconv(2, p, 4, 64, 64, 4, None, None, None, 0, q, q, None, 0, None, q, p, p, s) != 0   # mode 2 without in_scale
    assert L.irsde_debug_naf_lnconv(0, p, 4, 64, 96, 4, q, p, p, 0, q, q, None, 0, None, None, None, p, s) != 0
    assert float(t.abs().sum()) == 0.0
