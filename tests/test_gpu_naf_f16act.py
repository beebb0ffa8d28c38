"""'fp16_act' (IRSDE_FLAG_F16_ACT) on the GPU (run with -m gpu on an MI355X): the image-space ConditionalNAFNets with IEEE fp16 storage of every activation
tensor between kernels, against the float64 restatement of the mode (tests/naf_f16act_oracle.py) and against the fp32 engine on the same weights.

Bars.  Per tap: 1e-3 of max|ref| against the restatement restarted from the engine's own previous tap — the bar test_naf_chain_blocks_vs_oracle uses for the
same kind of comparison (fp16 rounding points restated, float64 otherwise); tests/test_naf_f16act_host.py shows that each mistake a storage-type port can make
misses it at least tenfold.  Whole forward against the restatement: 4 x the value measured on an MI355X (room for accumulation-order flips of fp16
roundings), capped at 3e-3, the project's fp16-versus-fp32 network bar.  Against the fp32 engine: finite, above 1e-5 (the mode is on) and below 4 x the
'fp16' mode's own error on the same input.  The measured values are in profiles/naf_fp16_act.md."""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import naf_f16act_oracle as FA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_BAR = 1e-3
F16ACT = _lib.FLAG_FP16 | _lib.FLAG_F16_ACT
TVEC = np.array([5, 60, 33])
# whole forward against the restatement, measured on an MI355X (profiles/naf_fp16_act.md): w64 conditional / w64 unconditional
MEASURED_VS_RESTATEMENT = {("w64", False): 3.42e-4, ("w64", True): 3.40e-4}
_NETS, _REFS = {}, {}


def net(case, flags, uncond=False):
    """The case's network with `make_params` weights (one engine per (case, flags, class) for the whole module)."""
    key = (case, flags, uncond)
    if key not in _NETS:
        width, enc, mid, dec = FA.CASES[case][:4]
        cls = P.denoising_sde.ConditionalNAFNet if uncond else P.ConditionalNAFNet
        m = cls(img_channel=3, width=width, enc_blk_nums=list(enc), middle_blk_num=mid, dec_blk_nums=list(dec))
        bp = FA.make_params(width, enc, mid, dec, seed=3, uncond=uncond)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in bp.items()}, strict=True)
        m.engine_flags = flags
        _NETS[key] = (m.to(DEV).eval(), bp)
    return _NETS[key]


def inputs(case, uncond=False):
    B, H, W = FA.CASES[case][4:]
    xt, cond = FA.make_inputs(B, H, W, seed=21, uncond=uncond)
    return xt, cond, TVEC[:B]


def reference(case, uncond=False):
    """The restatement's forward and taps of the case, computed once and left unchanged."""
    key = (case, uncond)
    if key not in _REFS:
        width, enc, mid, dec = FA.CASES[case][:4]
        bp = FA.make_params(width, enc, mid, dec, seed=3, uncond=uncond)
        xt, cond, tv = inputs(case, uncond)
        taps = {}
        y = FA.forward(bp, xt, tv, enc, mid, dec, cond=cond, taps=taps)
        _REFS[key] = (y, taps)
    return _REFS[key]


def run(m, xt, cond, tv):
    x = torch.from_numpy(xt).to(DEV)
    t = torch.from_numpy(np.asarray(tv)) if np.ndim(tv) else int(tv)
    if cond is None:
        return m(x, t).cpu().numpy()
    return m(x, torch.from_numpy(cond).to(DEV), t).cpu().numpy()


def describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 18)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine(torch.device(DEV)).h, B, H, W, buf, len(buf)))
    return buf.value.decode()


def work_bytes(m, B, H, W):
    out = (ctypes.c_double * 2)()
    _lib.check(_lib.lib().irsde_work_model(m.engine(torch.device(DEV)).h, B, H, W, out))
    return out[1]


@pytest.mark.parametrize("case,uncond", [("w64", False), ("w32", False), ("w256", False), ("w64", True)])
def test_taps_vs_restatement(case, uncond):
    """w64: c = 64 / 128 / 256, every 1x1 on the one-piece-K kernel; w32: c = 32 on the LayerNorm kernel + the implicit GEMM; w256: c = 512 / 1024 on the
    implicit GEMM with split-K, in_scale and ch_scale + residual.  B = 3 images of 36 x 52 with their own timesteps: 5616 / 1404 / 351 pixels, each
    ragged against the 64- and 128-pixel tiles, deepest map 13 wide.  (w64, True): the unconditional network through forward(x, time)."""
    width, enc, mid, dec, B, H, W = FA.CASES[case]
    m, bp = net(case, F16ACT | _lib.FLAG_KEEP_ACTIVATIONS, uncond)
    xt, cond, tv = inputs(case, uncond)
    y = run(m, xt, cond, tv)
    assert np.isfinite(y).all()
    _, rtaps = reference(case, uncond)
    got = {k: m.debug_tap(k).numpy() for k in rtaps}
    for k in rtaps:
        assert got[k].shape == rtaps[k].shape, k
        assert np.array_equal(got[k], got[k].astype(np.float16).astype(np.float32)), k   # the tap is a widened fp16 tensor
    errs = {"intro": FA.relerr(got["intro"], rtaps["intro"])}
    want = FA.restart_taps(bp, got, tv, enc, mid, dec)
    for k in want:
        errs[k] = FA.relerr(got[k], want[k])
    print("fp16_act taps vs restatement (%s%s):" % (case, ", unconditional" if uncond else ""), {k: "%.3g" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TAP_BAR}
    assert not bad, bad


@pytest.mark.parametrize("uncond", [False, True])
def test_whole_forward_vs_restatement_and_fp32_engine(uncond):
    case = "w64"
    xt, cond, tv = inputs(case, uncond)
    ref, _ = reference(case, uncond)
    y = {name: run(net(case, flags, uncond)[0], xt, cond, tv) for name, flags in (("fp32", 0), ("fp16", _lib.FLAG_FP16), ("fp16_act", F16ACT))}
    e_ref = FA.relerr(y["fp16_act"], ref)
    e_act = FA.relerr(y["fp16_act"], y["fp32"].astype(np.float64))
    e_16 = FA.relerr(y["fp16"], y["fp32"].astype(np.float64))
    print("fp16_act whole forward (w64%s): vs restatement %.3g, vs fp32 engine %.3g ('fp16' mode vs fp32 engine: %.3g)"
          % (", unconditional" if uncond else "", e_ref, e_act, e_16))
    assert np.isfinite(y["fp16_act"]).all()
    assert e_ref < min(4 * MEASURED_VS_RESTATEMENT[(case, uncond)], 3e-3), e_ref
    assert 1e-5 < e_act < 4 * e_16, (e_act, e_16)


def test_plan_rows_and_work_model():
    """Every conv row of the plan carries the storage tag; no level runs as the per-image chain (which the 'fp16' engine of the same four-level network
    does at 8 x 8); the work model counts 2 bytes per stored element: 28 c against 56 c bytes per pixel and block, plus weights and the fp32 ends."""
    m, _ = net("w64", F16ACT)
    rows = [r for r in describe(m, 2, 64, 64).splitlines() if r]
    convs = [r for r in rows if r.startswith("conv")]
    assert len(convs) >= 5 * 4 + 6 and all("(fp16 operands + storage" in r for r in convs), [r for r in convs if "storage" not in r]
    assert not any("naf_chain" in r for r in rows)
    b_act, b_16 = work_bytes(m, 2, 64, 64), work_bytes(net("w64", _lib.FLAG_FP16)[0], 2, 64, 64)
    print("work model bytes 2x3x64x64: fp16_act %.4g, fp16 %.4g (ratio %.3f)" % (b_act, b_16, b_act / b_16))
    assert 0 < b_act < 0.6 * b_16
    # four levels: 512 channels on an 8 x 8 map — the 'fp16' plan runs two chains there, this mode's plan none
    deep = {}
    for name, flags in (("fp16", _lib.FLAG_FP16), ("fp16_act", F16ACT)):
        mm = P.ConditionalNAFNet(img_channel=3, width=64, enc_blk_nums=[1, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
        bp = O.naf_synth_params(seed=0, img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 1), dec_blk_nums=(1, 1, 1, 1))
        mm.load_state_dict({k: torch.from_numpy(v) for k, v in bp.items()}, strict=True)
        mm.engine_flags = flags
        deep[name] = describe(mm.to(DEV).eval(), 2, 64, 64)
    assert deep["fp16"].count("naf_chain(fp16)") == 2 and "naf_chain" not in deep["fp16_act"]
    assert all("(fp16 operands + storage" in r for r in deep["fp16_act"].splitlines() if r.startswith("conv"))


def test_samplers_graph_eager_and_repeat_are_bit_identical():
    """reverse_sde / reverse_posterior (T = 8, the engine's Philox noise): graph replay == eager launches, two runs with one seed are identical; the error
    against the fp32 engine is finite (recorded in profiles/naf_fp16_act.md).  DenoisingSDE.reverse_ode runs on the unconditional network."""
    case, T = "w64", 8
    xt, cond, _ = inputs(case)
    x, mu = torch.from_numpy(xt).to(DEV), torch.from_numpy(cond).to(DEV)
    outs = {}
    for name, flags in (("fp32", 0), ("fp16_act", F16ACT)):
        m, _ = net(case, flags)
        sde = P.IRSDE(10, T, "cosine", 0.005, device=DEV)
        sde.set_model(m)
        sde.set_mu(mu)
        sde.seed = 11
        for mode, fn in (("sde", sde.reverse_sde), ("posterior", sde.reverse_posterior)):
            sde.use_graph = True
            a = fn(mu + x).cpu().numpy()
            b = fn(mu + x).cpu().numpy()
            sde.use_graph = False
            c = fn(mu + x).cpu().numpy()
            assert np.isfinite(a).all()
            assert np.array_equal(a, b), (name, mode, "two runs with one seed differ")
            assert np.array_equal(a, c), (name, mode, "graph replay and eager launches differ")
            outs[(name, mode)] = a
    for mode in ("sde", "posterior"):
        e = FA.relerr(outs[("fp16_act", mode)], outs[("fp32", mode)].astype(np.float64))
        print("fp16_act reverse_%s T=%d vs fp32 engine: %.3g" % (mode, T, e))
        assert np.isfinite(e) and e > 0
    mu_, _ = net(case, F16ACT, uncond=True)
    dsde = P.DenoisingSDE(max_sigma=50, T=100, device=DEV)
    dsde.set_model(mu_)
    noisy = torch.from_numpy((0.5 + 0.1 * xt).astype(np.float32)).to(DEV)
    out = dsde.reverse_ode(noisy, T=8).cpu().numpy()
    assert out.shape == xt.shape and np.isfinite(out).all()


def test_batch_images_equal_their_single_image_calls():
    case = "w64"
    m, _ = net(case, F16ACT)
    xt, cond, tv = inputs(case)
    yb = run(m, xt, cond, tv)
    scale = float(np.abs(yb).max())
    worst = max(float(np.abs(run(m, xt[b:b + 1], cond[b:b + 1], int(tv[b])) - yb[b:b + 1]).max() / scale) for b in range(xt.shape[0]))
    print("fp16_act B=3 vs 3 x B=1 at 36x52: %.3g" % worst)
    assert worst < TAP_BAR
    assert FA.relerr(yb[0], yb[2].astype(np.float64)) > 1e-2   # (the images differ)
