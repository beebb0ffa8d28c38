"""LPIPS v0.1 / AlexNet on the GPU (csrc/lpips.hip through metrics.LPIPS, irsde_lpips and irsde_debug_lpips_tap) against the float64 oracle
tests/lpips_oracle.py, on synthetic weights.

The bar, for every per-tap feature map (of max |ref|) and for EACH of the five terms (relative), is 5e-5: the project's bar for an fp32
convolution against its float64 oracle (tests/test_gpu_parity.py).  The terms are compared one by one because tap 1 carries 80 - 92 % of the
total with these weights and taps 3 - 5 about 1 % each: the sum alone would pass with a broken deep layer.  Every test prints its figures before
it asserts; the measured ones are in profiles/lpips.md.

Shapes: (1, 31, 31) the minimum, taps 3 - 5 are 1 x 1 maps; (2, 64, 48) non-square; (3, 97, 130) every floor division inexact, ragged M tiles at
every tap; (1, 256, 256) the benchmark's image size.  Inputs are seeded torch.rand images: an independent pair (a, b) and a near pair
(a, clamp(a + 0.02 randn)).

Values on the published weights are unpinned and blocked on assets (tests/test_lpips_host.py)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import lpips_oracle as LO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 5e-5
SHAPES = [(1, 31, 31), (2, 64, 48), (3, 97, 130), (1, 256, 256)]
W = LO.synth_weights(0)

_CASES = {}
_MODEL = []


def model():
    if not _MODEL:
        _MODEL.append(P.LPIPS(net="alex").load_state_dict(LO.lpips_layout(W)))
    return _MODEL[0]


def case(shape):
    """Inputs and float64 references of one shape, computed once and shared: a, b, near; terms of (a, b) and (a, near); the five maps of a."""
    if shape not in _CASES:
        g = torch.Generator().manual_seed(1000 + shape[1] * 7 + shape[2])
        a = torch.rand(shape[0], 3, shape[1], shape[2], generator=g)
        b = torch.rand(shape[0], 3, shape[1], shape[2], generator=g)
        near = (a + 0.02 * torch.randn(a.shape, generator=g)).clamp(0, 1)
        t_ind, maps = LO.lpips_terms(W, a, b)
        t_near, _ = LO.lpips_terms(W, a, near)
        _CASES[shape] = dict(a=a, b=b, near=near, independent=t_ind, near_terms=t_near, maps=[f.numpy() for f in maps])
    return _CASES[shape]


def gpu_terms(x, y, normalize=False):
    m = model()
    t = m.terms(x.to(DEV), y.to(DEV), normalize=normalize)
    return t, m.last_dist.copy()


def sum5(t):
    return (((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]) + t[:, 4]   # the order irsde_lpips adds the terms in


def gpu_tap(x, tap, normalize=False):
    m = model()
    xd = x.to(DEV).contiguous()
    h = m._engine(xd.device)
    L = _lib.lib()
    B, _, H, Wd = xd.shape
    dims = (ctypes.c_int64 * 4)()
    _lib.check(L.irsde_debug_lpips_tap(h, ctypes.c_void_p(xd.data_ptr()), B, H, Wd, int(normalize), tap, None, dims, _lib.stream_ptr()))
    out = torch.empty(tuple(dims), dtype=torch.float32, device=DEV)
    _lib.check(L.irsde_debug_lpips_tap(h, ctypes.c_void_p(xd.data_ptr()), B, H, Wd, int(normalize), tap, ctypes.c_void_p(out.data_ptr()), dims,
                                       _lib.stream_ptr()))
    return out.permute(0, 3, 1, 2).cpu().numpy()   # NHWC -> NCHW


@pytest.mark.parametrize("shape", SHAPES)
def test_tap_feature_maps_against_the_oracle(shape):
    c = case(shape)
    want_shapes = LO.feature_shapes(shape[1], shape[2])
    worst = 0.0
    for tap in range(1, 6):
        ref = c["maps"][tap - 1]
        got = gpu_tap(c["a"], tap)
        assert got.shape == ref.shape == (shape[0],) + want_shapes[tap - 1]
        assert ref.max() > 0 and (ref.reshape(ref.shape[0], ref.shape[1], -1).max(2) > 0).any()   # the tap is alive
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("lpips tap %d of %s: max err / max |ref| = %.2e" % (tap, shape, err))
        worst = max(worst, err)
    assert worst <= BAR, worst


@pytest.mark.parametrize("pair", ["independent", "near"])
@pytest.mark.parametrize("shape", SHAPES)
def test_each_term_against_the_oracle(shape, pair):
    c = case(shape)
    ref = c["independent"] if pair == "independent" else c["near_terms"]
    got, dist = gpu_terms(c["a"], c["b"] if pair == "independent" else c["near"])
    assert got.shape == ref.shape == (shape[0], 5) and got.dtype == np.float64
    assert (ref > 0).all()
    rel = np.abs(got - ref) / ref
    print("lpips terms %s %s: rel err per term (worst image) = %s; share of tap 1 = %.2f" %
          (shape, pair, " ".join("%.2e" % v for v in rel.max(0)), float((ref[:, 0] / ref.sum(1)).min())))
    assert rel.max() <= BAR, rel
    assert np.array_equal(dist, sum5(got))   # dist is the float64 sum of its five terms


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_properties(shape):
    c = case(shape)
    taa, daa = gpu_terms(c["a"], c["a"])
    assert np.array_equal(taa, np.zeros_like(taa)) and np.array_equal(daa, np.zeros_like(daa))   # lpips(a, a) == 0
    tab, dab = gpu_terms(c["a"], c["b"])
    tba, dba = gpu_terms(c["b"], c["a"])
    assert np.array_equal(tab, tba) and np.array_equal(dab, dba)                                 # lpips(a, b) == lpips(b, a)
    tab2, dab2 = gpu_terms(c["a"], c["b"])
    assert np.array_equal(tab, tab2) and np.array_equal(dab, dab2)                               # deterministic


def test_an_image_of_a_batch_equals_the_image_alone():
    c = case((3, 97, 130))
    tb, db = gpu_terms(c["a"], c["b"])
    for k in range(3):
        t1, d1 = gpu_terms(c["a"][k:k + 1], c["b"][k:k + 1])
        assert np.array_equal(t1[0], tb[k]) and d1[0] == db[k], k
    for tap in (1, 3, 5):
        full = gpu_tap(c["a"], tap)
        assert np.array_equal(gpu_tap(c["a"][2:3], tap)[0], full[2]), tap


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_normalize_folds_2x_minus_1(shape):
    c = case(shape)   # a, b are in [0, 1]
    t01, _ = gpu_terms(c["a"], c["b"], normalize=True)
    tpm, _ = gpu_terms(c["a"] * 2 - 1, c["b"] * 2 - 1, normalize=False)
    rel = np.abs(t01 - tpm) / tpm
    print("lpips normalize=True vs 2x-1 %s: rel diff per term = %s" % (shape, " ".join("%.2e" % v for v in rel.max(0))))
    assert rel.max() <= BAR
    ref, _ = LO.lpips_terms(W, c["a"] * 2 - 1, c["b"] * 2 - 1)
    assert (np.abs(t01 - ref) / ref).max() <= BAR


def test_call_returns_a_b111_float32_device_tensor():
    c = case((2, 64, 48))
    m = model()
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    d = m(a, b)
    assert isinstance(d, torch.Tensor) and d.shape == (2, 1, 1, 1) and d.dtype == torch.float32 and d.device.type == "cuda"
    t = m.terms(a, b)
    assert np.array_equal(d.cpu().numpy().reshape(-1), sum5(t).astype(np.float32))
    # the reference's own line (deraining/test.py:149-154), one pair
    GT, SR = (a[:1] + 1) / 2, (b[:1] + 1) / 2
    lp = m(GT.to(DEV) * 2 - 1, SR.to(DEV) * 2 - 1).squeeze().item()
    assert isinstance(lp, float) and abs(lp - c["independent"][0].sum()) <= 2 * BAR * c["independent"][0].sum()
    with pytest.raises(P.IrsdeError):
        m(a[:, :2], b[:, :2])                       # C != 3
    with pytest.raises(P.IrsdeError):
        m(a, b[:1])                                 # shape mismatch
    with pytest.raises(P.IrsdeError, match="31"):
        m(a[:, :, :30], b[:, :, :30])               # below the minimum size
    with pytest.raises(P.IrsdeError, match="no weights"):
        P.LPIPS()(a, b)


def test_evaluate_batch_adds_the_key_and_changes_nothing_else():
    c = case((2, 64, 48))
    out, gt = c["near"].to(DEV), c["a"].to(DEV)
    plain = P.metrics.evaluate_batch(out, gt, crop_border=4)
    with_lp = P.metrics.evaluate_batch(out, gt, crop_border=4, lpips=model())
    assert set(plain) == {"psnr", "ssim", "psnr_y", "ssim_y"} and set(with_lp) == set(plain) | {"lpips"}
    for k in plain:
        assert np.array_equal(plain[k], with_lp[k]), k
    ref, _ = LO.lpips_terms(W, c["near"] * 2 - 1, c["a"] * 2 - 1)   # on the full, unquantised images in [0, 1]: normalize=True
    assert with_lp["lpips"].shape == (2,) and (np.abs(with_lp["lpips"] - ref.sum(1)) / ref.sum(1)).max() <= BAR


def test_eval_folder_prints_the_average_lpips_line(tmp_path, capsys):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("eval_folder", os.path.join(ROOT, "tools", "eval_folder.py"))
    ef = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ef)
    rs = np.random.RandomState(5)
    for d in ("LQ", "GT"):
        (tmp_path / d).mkdir()
    gts = []
    for i in range(3):
        g = rs.randint(0, 256, size=(64, 48, 3), dtype=np.uint8)
        lq = np.clip(g.astype(np.int32) + rs.randint(-20, 21, size=g.shape), 0, 255).astype(np.uint8)
        Image.fromarray(g).save(str(tmp_path / "GT" / ("img%02d.png" % i)))
        Image.fromarray(lq).save(str(tmp_path / "LQ" / ("img%02d.png" % i)))
        gts.append(torch.from_numpy(np.ascontiguousarray(g.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))))
    params = O.synth_params(seed=0, nf=32, depth=2)   # the small UNet of tests/test_gpu_degrade.py
    torch.save({"module." + k: torch.from_numpy(v) for k, v in params.items()}, tmp_path / "G.pth")
    files = LO.files_layout(W)   # as the two published files
    torch.save({k: v for k, v in files.items() if not k.startswith("lin")}, tmp_path / "alexnet.pth")
    torch.save({k: v for k, v in files.items() if k.startswith("lin")}, tmp_path / "alex.pth")
    # --task sisr --scale 1 is the LQ / GT loop (the upscale by 1 copies) with the hook that hands out the sampler's device tensors
    argv = ["--task", "sisr", "--scale", "1", "--lq", str(tmp_path / "LQ"), "--gt", str(tmp_path / "GT"), "--weights", str(tmp_path / "G.pth"),
            "--nf", "32", "--depth", "2", "--T", "4", "--batch", "3", "--seed", "3"]
    seen = []
    summary = ef.main(argv + ["--lpips-weights", str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")],
                      on_batch=lambda idx, LQ, out: seen.append((list(idx), out.cpu())))
    text = capsys.readouterr().out
    assert [s[0] for s in seen] == [[0, 1, 2]]
    out = seen[0][1]
    ref, _ = LO.lpips_terms(W, out * 2 - 1, torch.stack(gts) * 2 - 1)
    want = float(ref.sum(1).mean())
    with capsys.disabled():
        print("eval_folder average LPIPS %.9f, oracle %.9f" % (summary["lpips"], want))
    assert set(summary) == {"psnr", "ssim", "psnr_y", "ssim_y", "lpips"}
    assert abs(summary["lpips"] - want) <= BAR * want
    assert "----average LPIPS\t: %.6f" % summary["lpips"] in text
    per_image = re.findall(r"^img\s*\d+:img0\d\s+- PSNR: [\d.]+ dB; SSIM: [-\d.]+; LPIPS: ([\d.]+); PSNR_Y", text, re.M)
    assert len(per_image) == 3 and all(abs(float(v) - r) <= 1e-6 + BAR * r for v, r in zip(per_image, ref.sum(1)))
    # without the flag: the same run, no LPIPS anywhere, the other numbers unchanged
    plain = ef.main(argv)
    text = capsys.readouterr().out
    assert "LPIPS" not in text and set(plain) == {"psnr", "ssim", "psnr_y", "ssim_y"}
    assert all(plain[k] == summary[k] for k in plain)
