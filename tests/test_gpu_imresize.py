"""imresize on the GPU (csrc/degrade.hip imresize_kernel through degradations.imresize): the kernel against the float64 restatement
(tests/imresize_oracle.py) and against the reference's own fp32 outputs (tests/golden/imresize.npz, tools/gen_imresize_golden.py), its
exactness properties, and tools/eval_folder.py --task sisr --lq-from-gt against the same steps made on the API.

Measured on an MI355X (max |gpu - ref| / max |ref|; the bar is 1e-5): profiles/degradations.md."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import degradations as D
from oracle import irsde_oracle as O
import imresize_oracle as IO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5   # of max |ref|: the bar tests/test_gpu_degrade.py holds the upscale kernel to
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "imresize.npz"))

_REF = {}


def case(i):
    """(input, float64 restatement) of IO.SHAPES[i], computed once."""
    if i not in _REF:
        x = IO.inputs(i)
        ref = IO.imresize(x, IO.SHAPES[i][4], IO.SHAPES[i][5])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[i] = (x, ref)
    return _REF[i]


def gpu(x, scale, aa=True):
    return D.imresize(torch.tensor(x, device=DEV), scale, aa).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("i", range(len(IO.SHAPES)))
def test_kernel_matches_the_restatement_and_the_reference(i):
    x, ref = case(i)
    gold = GOLDEN["out/%d" % i].astype(np.float64)
    got = gpu(x, IO.SHAPES[i][4], IO.SHAPES[i][5])
    assert got.shape == ref.shape and got.dtype == np.float32
    e_ref = float(np.abs(got - ref).max() / np.abs(ref).max())
    e_gold = float(np.abs(got - gold).max() / np.abs(gold).max())
    print("imresize %s: %.2e of max|ref| from the restatement, %.2e from the reference's fp32 output (range %.3f .. %.3f)" %
          (IO.SHAPES[i], e_ref, e_gold, ref.min(), ref.max()))
    assert e_ref < BAR
    assert e_gold < BAR


@pytest.mark.parametrize("shape", [(1, 2, 150, 70, 1 / 4, True), (2, 1, 70, 150, 1 / 2, True), (1, 1, 61, 45, 0.3, False)], ids=str)
def test_more_than_one_tile_of_rows(shape):
    """A tile holds up to 16 output rows and 32 columns; the golden shapes have at most 12 rows.  Ho = 38 / 35 / 19: two or three tiles of rows,
    the last one partial, on up to three tiles of columns — against the restatement."""
    x = np.random.default_rng(sum(shape[:4])).random(shape[:4], dtype=np.float32)
    ref = IO.imresize(x, shape[4], shape[5])
    got = gpu(x, shape[4], shape[5])
    assert got.shape == ref.shape and ref.shape[2] > 16
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("imresize %s: %.2e of max|ref| from the restatement" % (shape, e))
    assert e < BAR


def test_scale_one_is_the_input_bit_for_bit():
    x = np.random.default_rng(5).standard_normal((2, 3, 9, 10)).astype(np.float32)   # finite and non-zero: 0 * x and + 0 keep every bit
    for aa in (True, False):
        assert np.array_equal(bits(gpu(x, 1.0, aa)), bits(x))


def test_interior_impulse_is_the_product_of_the_tables():
    """A unit impulse away from the borders: the H pass leaves wH[i][k] (a sum of zeros and one exact product with 1), the W pass one fmaf of
    it with wW[j][l] onto zero, i.e. the fp32 product rounded once; outputs no tap reaches are zero."""
    H, W, y, x = 40, 136, 17, 70   # x beyond the first tile's columns
    img = np.zeros((1, 1, H, W), dtype=np.float32)
    img[0, 0, y, x] = 1.0
    got = gpu(img, 1 / 4)[0, 0]
    (wH, sH, _, _), (wW, sW, _, _) = D.imresize_tables(H, 1 / 4), D.imresize_tables(W, 1 / 4)

    def seen(w, s, p):   # [n_out] weight of the tap that reads pixel p, 0 where none does (p is out of every reflection's reach)
        w, s = w.numpy(), s.numpy()
        k = p - s
        ok = (k >= 0) & (k < w.shape[1])
        return np.where(ok, w[np.arange(len(s)), np.clip(k, 0, w.shape[1] - 1)], np.float32(0)).astype(np.float32), ok

    (a, oka), (b, okb) = seen(wH, sH, y), seen(wW, sW, x)
    want = a[:, None] * b[None, :]           # fp32 x fp32 -> fp32: one rounding
    reached = oka[:, None] & okb[None, :]
    assert want.dtype == np.float32 and oka.sum() == 4 and okb.sum() == 4
    assert np.array_equal(bits(got)[reached & (want != 0)], bits(want)[reached & (want != 0)])
    assert np.all(got[~reached | (want == 0)] == 0)
    assert np.count_nonzero(got) >= 12


@pytest.mark.parametrize("corner", ["first", "last"])
def test_corner_impulse_sums_the_direct_and_the_reflected_tap(corner):
    H, W = 40, 136
    y, x = (0, 0) if corner == "first" else (H - 1, W - 1)
    img = np.zeros((1, 1, H, W), dtype=np.float32)
    img[0, 0, y, x] = 1.0
    ref = IO.imresize(img, 1 / 4)[0, 0]
    got = gpu(img, 1 / 4)[0, 0].astype(np.float64)
    assert np.abs(got - ref).max() < BAR * np.abs(ref).max()
    # the corner output: the edge pixel is read by its own tap and by the tap one beyond the edge
    (wH, sH, _, _), (wW, sW, _, _) = D.imresize_tables(H, 1 / 4), D.imresize_tables(W, 1 / 4)

    def both(w, s, n, first):
        o = 0 if first else len(s) - 1
        p_direct, p_mirror = (0, -1) if first else (n - 1, n)
        row = w[o].numpy().astype(np.float64)
        return row[p_direct - int(s[o])] + row[p_mirror - int(s[o])]

    first = corner == "first"
    want = both(wH, sH, H, first) * both(wW, sW, W, first)
    o = got[0, 0] if first else got[-1, -1]
    assert abs(o - want) < BAR * np.abs(ref).max() and abs(want) > 0.01


def test_planes_do_not_mix():
    x, _ = case(0)
    only = np.zeros_like(x)
    only[1, 1] = x[1, 1]
    got = gpu(only, 1 / 4)
    whole = gpu(x, 1 / 4)
    for b in range(2):
        for c in range(3):
            if (b, c) == (1, 1):
                assert np.array_equal(bits(got[b, c]), bits(whole[b, c]))
            else:
                assert np.all(got[b, c] == 0), (b, c)


def test_entry_forms_agree_bit_for_bit():
    x, _ = case(1)   # (1, 3, 37, 131)
    t4 = D.imresize(torch.tensor(x, device=DEV), 1 / 4)
    t3 = D.imresize(torch.tensor(x[0], device=DEV), 1 / 4)
    hwc = D.imresize(np.ascontiguousarray(x[0].transpose(1, 2, 0)), 1 / 4)
    assert tuple(t4.shape) == (1, 3, 10, 33) and tuple(t3.shape) == (3, 10, 33) and t3.dtype == torch.float32
    assert isinstance(hwc, np.ndarray) and hwc.shape == (10, 33, 3) and hwc.dtype == np.float32
    assert torch.equal(t4[0], t3)
    assert np.array_equal(bits(hwc.transpose(2, 0, 1)), bits(t3.cpu().numpy()))


def test_two_calls_return_identical_bits():
    x, _ = case(6)   # scale 0.3: per-output weights
    a = gpu(x, 0.3)
    n_tables = len(D._DEVICE_TABLES)
    b = gpu(x, 0.3)
    assert np.array_equal(bits(a), bits(b)) and len(D._DEVICE_TABLES) == n_tables   # the second call took the cached device tables


# ---------------------------------------------------------------------------------------------
# tools/eval_folder.py --task sisr --lq-from-gt
# ---------------------------------------------------------------------------------------------
T, SEED, MAX_SIGMA = 4, 3, 10   # as tests/test_gpu_degrade.py


def test_eval_folder_lq_from_gt(tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("eval_folder", os.path.join(ROOT, "tools", "eval_folder.py"))
    ef = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ef)
    (tmp_path / "HR").mkdir()
    rs = np.random.RandomState(2)
    imgs = [rs.randint(0, 256, size=hw + (3,), dtype=np.uint8) for hw in ((30, 43), (30, 43), (29, 50))]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(str(tmp_path / "HR" / ("img%02d.png" % i)))
    hr = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))) for im in imgs]
    params = O.synth_params(seed=0, nf=32, depth=2)   # the small UNet of tests/test_gpu_degrade.py
    torch.save({"module." + k: torch.from_numpy(v) for k, v in params.items()}, tmp_path / "G.pth")
    model = P.ConditionalUNet(3, 3, 32, depth=2)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to(DEV).eval()
    seen = []
    summary = ef.main(["--task", "sisr", "--gt", str(tmp_path / "HR"), "--lq-from-gt", "--scale", "4", "--weights", str(tmp_path / "G.pth"), "--nf", "32",
                       "--depth", "2", "--T", str(T), "--batch", "2", "--seed", str(SEED), "--max-sigma", str(MAX_SIGMA), "--out", str(tmp_path / "res")],
                      on_batch=lambda idx, LQ, out: seen.append((list(idx), LQ.clone(), out.clone())))
    assert set(summary) == {"psnr", "ssim", "psnr_y", "ssim_y"} and all(np.isfinite(v) for v in summary.values())
    assert [s[0] for s in seen] == [[0, 1], [2]]   # two size groups after modcrop: 28 x 40 twice, 28 x 48
    for name, hw in (("img00", (28, 40)), ("img01", (28, 40)), ("img02", (28, 48))):
        for suffix in ("", "_LQ", "_HQ"):
            assert Image.open(str(tmp_path / "res" / (name + suffix + ".png"))).size == (hw[1], hw[0]), (name, suffix)
    metrics = {k: [] for k in summary}
    for idx, LQ, out in seen:
        GT = torch.stack([D.modcrop(hr[i], 4) for i in idx]).to(DEV)
        small = D.imresize(GT, 1 / 4, True)
        assert tuple(small.shape[2:]) == (GT.shape[2] // 4, GT.shape[3] // 4)
        want_lq = D.upscale(small, 4)
        assert LQ.shape == GT.shape and torch.equal(LQ, want_lq)
        sde = P.IRSDE(max_sigma=MAX_SIGMA, T=T, schedule="cosine", eps=0.005, device=torch.device(DEV))
        sde.set_model(model)
        sde.seed = SEED
        noise = torch.stack([torch.randn(want_lq.shape[1:], generator=torch.Generator().manual_seed(SEED * 1000003 + i)) for i in idx])
        sde.image_offset = idx[0]
        sde.set_mu(want_lq)
        want = sde.reverse_sde(want_lq + (noise * sde.max_sigma).to(DEV))
        assert torch.equal(out, want)
        m = P.metrics.evaluate_batch(want, GT, crop_border=4)
        for k in metrics:
            metrics[k].extend(float(v) for v in m[k])
    want_summary = P.metrics.reduce_metrics({k: np.asarray(v, dtype=np.float64) for k, v in metrics.items()})
    assert {k: float(v) for k, v in summary.items()} == {k: float(v) for k, v in want_summary.items()}
