"""Degradation front ends on the GPU (csrc/degrade.hip through degradations.py): the bicubic upscale against the float64 restatement
(tests/degrade_oracle.py, itself within 2e-6 of torch's CPU `F.interpolate`: tests/test_degrade_host.py), its exactness properties, the mask
composite bit for bit against the reference's three lines on the CPU, and one run of each new task of tools/eval_folder.py.

Measured on an MI355X (max |gpu - restatement| / max |restatement|; the bar is 1e-5): profiles/degradations.md."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_sde_amd as P
from oracle import irsde_oracle as O
import degrade_oracle as DO
import stereo_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5   # of max |ref|: the bar tests/test_gpu_stereo.py holds the SCAM kernels to, whose prologue is this filter at t = 0.5
# the host shapes + an output (148 x 280) that crosses every tile edge up to 128 in both axes + the largest factor
SHAPES = DO.SHAPES + [(1, 3, 37, 70, 4), (1, 2, 3, 3, 8)]
SMALL = dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])   # the SMALL network of tests/test_gpu_stereo.py

_REF = {}


def case(shape):
    """(input, float64 restatement) of a shape, computed once."""
    if shape not in _REF:
        x = np.random.default_rng(sum(shape)).random(shape[:4], dtype=np.float32)
        ref = DO.upscale(x, shape[4])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[shape] = (x, ref)
    return _REF[shape]


def gpu_upscale(x, s):
    return P.degradations.upscale(torch.tensor(x, device=DEV), s).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_upscale_matches_the_restatement(shape):
    x, ref = case(shape)
    got = gpu_upscale(x, shape[4])
    assert got.shape == ref.shape and got.dtype == np.float32
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("upscale %s: %.2e of max|ref| (range %.3f .. %.3f)" % (shape, e, ref.min(), ref.max()))
    assert e < BAR


def test_upscale_scale_one_is_the_input_bit_for_bit():
    x = np.random.default_rng(5).standard_normal((2, 3, 7, 9)).astype(np.float32)
    x[0, 0, 0, :3] = [-0.0, np.float32(1e-42), -np.inf]   # signed zero, a denormal, an infinity: a copy keeps them
    assert np.array_equal(gpu_upscale(x, 1).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_upscale_keeps_a_constant_image(s):
    x = np.full((1, 2, 5, 37), 0.7, dtype=np.float32)
    got = gpu_upscale(x, s)
    assert got.shape == (1, 2, 5 * s, 37 * s)
    assert np.abs(got.astype(np.float64) - np.float64(np.float32(0.7))).max() <= 1e-6


@pytest.mark.parametrize("s", [3, 4])
def test_upscale_of_an_impulse_is_the_weight_table(s):
    """A unit impulse at (iy, ix) comes out as the outer product of the phase table's taps: three fp32 roundings (both table entries, their
    product) of a value <= 1, i.e. <= 3 * 2^-24 = 1.8e-7 absolute; zero wherever the restatement is zero."""
    H, W, iy, ix = 9, 40, 4, 33   # ix beyond the first 32-column tile
    x = np.zeros((1, 1, H, W), dtype=np.float32)
    x[0, 0, iy, ix] = 1.0
    got = gpu_upscale(x, s)[0, 0].astype(np.float64)
    ref = DO.upscale(x, s)[0, 0]
    assert np.abs(got - ref).max() <= 2e-7
    assert np.array_equal(got == 0.0, np.abs(ref) < 1e-300)
    # the table itself, entry by entry, down the output column of phase s // 2 through the impulse (that phase has d = 0 and sees it with tap 1)
    tab = DO.phase_table(s)
    col = got[:, s * ix + s // 2]
    for p in range(s):
        d = -1 if 2 * p + 1 < s else 0
        for k in range(4):   # tap k of phase p reads input row i + d + k - 1: the impulse is seen from i = iy - d - k + 1
            assert abs(col[s * (iy - d - k + 1) + p] - tab[p, k] * tab[s // 2, 1]) <= 2e-7, (p, k)


def test_upscale_planes_do_not_mix():
    x, _ = case((2, 3, 5, 7, 4))
    whole = gpu_upscale(x, 4)
    for b in range(2):
        for c in range(3):
            assert np.array_equal(gpu_upscale(x[b:b + 1, c:c + 1], 4)[0, 0], whole[b, c]), (b, c)
    assert np.array_equal(P.degradations.upscale(torch.from_numpy(x[1].copy()).to(DEV), 4).cpu().numpy(), whole[1])   # [C, H, W] form


@pytest.mark.parametrize("Cm", [1, 3])
@pytest.mark.parametrize("Bm", [1, 2])
@pytest.mark.parametrize("sizes", [((256, 256), (37, 53)), ((8, 8), (20, 28)), ((16, 16), (16, 16))], ids=["down", "up", "same"])
def test_mask_to_is_the_reference_bit_for_bit(sizes, Bm, Cm):
    (Hm, Wm), (H, W) = sizes
    rng = np.random.default_rng(Hm + 3 * Bm + Cm)
    m8 = rng.choice(np.array([0, 77, 255], dtype=np.uint8), size=(Bm, Hm, Wm, Cm))
    tensor = torch.from_numpy(rng.random((2, 3, H, W), dtype=np.float32))
    mask = torch.tensor(m8 / 255.).permute(0, 3, 1, 2).float()           # deg_utils.py:30
    mask = F.interpolate(mask, size=tensor.shape[2:], mode="nearest")    # :32
    masked_tensor = mask * tensor                                        # :33
    ref = (masked_tensor + (1. - mask)).numpy()                          # :34
    got = P.degradations.mask_to(tensor.to(DEV), masks=m8).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(DO.mask_to(tensor.numpy(), m8), ref)
    got_t = P.degradations.mask_to(tensor.to(DEV), masks=torch.from_numpy(m8).to(DEV)).cpu().numpy()   # masks already on the device
    assert np.array_equal(got_t, ref)


def test_mask_to_reads_mask_files_like_cv2(tmp_path):
    """mask_id >= 0: '%06d.png' for the whole batch; a colour PNG (RGB on disk) is applied in BGR order, as cv2.imread returns it."""
    from PIL import Image
    rng = np.random.default_rng(2)
    rgb = rng.choice(np.array([0, 77, 255], dtype=np.uint8), size=(16, 24, 3))
    Image.fromarray(rgb).save(str(tmp_path / "000007.png"))
    tensor = torch.from_numpy(rng.random((2, 3, 13, 18), dtype=np.float32))
    got = P.degradations.mask_to(tensor.to(DEV), str(tmp_path), mask_id=7).cpu().numpy()
    assert np.array_equal(got, DO.mask_to(tensor.numpy(), rgb[None, :, :, ::-1]))


# ---------------------------------------------------------------------------------------------
# tools/eval_folder.py --task sisr | inpainting | stereo-sr
# ---------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("eval_folder", os.path.join(ROOT, "tools", "eval_folder.py"))
    ef = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ef)
    return ef


def _pngs(folder, n, h, w, seed):
    from PIL import Image
    folder.mkdir()
    rs = np.random.RandomState(seed)
    imgs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(str(folder / ("img%02d.png" % i)))
    return [np.ascontiguousarray(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)) for im in imgs]


def _unet(tmp_path):
    params = O.synth_params(seed=0, nf=32, depth=2)
    torch.save({"module." + k: torch.from_numpy(v) for k, v in params.items()}, tmp_path / "G.pth")
    m = P.ConditionalUNet(3, 3, 32, depth=2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(DEV).eval(), ["--weights", str(tmp_path / "G.pth"), "--nf", "32", "--depth", "2"]


T, SEED, MAX_SIGMA = 4, 3, 10


def _direct(model, LQ, idx):
    """The steps of the loop on the API: the per-image seeded noise_state draw, reverse_sde."""
    sde = P.IRSDE(max_sigma=MAX_SIGMA, T=T, schedule="cosine", eps=0.005, device=torch.device(DEV))
    sde.set_model(model)
    sde.seed = SEED
    noise = torch.stack([torch.randn(LQ.shape[1:], generator=torch.Generator().manual_seed(SEED * 1000003 + i)) for i in idx])
    sde.image_offset = idx[0]
    sde.set_mu(LQ)
    return sde.reverse_sde(LQ + (noise * sde.max_sigma).to(DEV))


def _run(ef, args, out_dir):
    seen = []
    summary = ef.main(args + ["--T", str(T), "--batch", "2", "--seed", str(SEED), "--max-sigma", str(MAX_SIGMA), "--out", str(out_dir)],
                      on_batch=lambda idx, LQ, out: seen.append((list(idx), LQ.clone(), out.clone())))
    assert all(np.isfinite(v) for v in summary.values()), summary
    return summary, seen


def _check_pngs(out_dir, names, hw):
    from PIL import Image
    for n in names:
        for suffix in ("", "_LQ", "_HQ"):
            assert Image.open(str(out_dir / (n + suffix + ".png"))).size == (hw[1], hw[0]), (n, suffix)


def test_eval_folder_sisr(tmp_path):
    lq = _pngs(tmp_path / "LQ", 3, 8, 12, seed=1)
    _pngs(tmp_path / "GT", 3, 32, 48, seed=2)
    model, wargs = _unet(tmp_path)
    summary, seen = _run(_tool(), ["--task", "sisr", "--lq", str(tmp_path / "LQ"), "--gt", str(tmp_path / "GT"), "--scale", "4"] + wargs, tmp_path / "res")
    assert set(summary) == {"psnr", "ssim", "psnr_y", "ssim_y"} and [s[0] for s in seen] == [[0, 1], [2]]
    _check_pngs(tmp_path / "res", ["img00", "img01", "img02"], (32, 48))
    for idx, LQ, out in seen:
        want_lq = P.degradations.upscale(torch.from_numpy(np.stack([lq[i] for i in idx])).to(DEV), 4)
        assert tuple(LQ.shape) == (len(idx), 3, 32, 48) and torch.equal(LQ, want_lq)
        assert torch.equal(out, _direct(model, want_lq, idx))


def test_eval_folder_inpainting(tmp_path):
    from PIL import Image
    gt = _pngs(tmp_path / "GT", 3, 32, 48, seed=4)
    (tmp_path / "masks").mkdir()
    rs = np.random.RandomState(5)
    masks = [rs.choice(np.array([0, 255], dtype=np.uint8), size=(16, 16)) for _ in range(3)]
    for i, m in enumerate(masks):
        Image.fromarray(m).save(str(tmp_path / "masks" / ("%06d.png" % i)))
    model, wargs = _unet(tmp_path)
    summary, seen = _run(_tool(), ["--task", "inpainting", "--gt", str(tmp_path / "GT"), "--mask-root", str(tmp_path / "masks")] + wargs, tmp_path / "res")
    assert set(summary) == {"psnr", "ssim", "psnr_y", "ssim_y"} and [s[0] for s in seen] == [[0, 1], [2]]
    _check_pngs(tmp_path / "res", ["img00", "img01", "img02"], (32, 48))
    for idx, LQ, out in seen:
        x = torch.from_numpy(np.stack([gt[i] for i in idx])).to(DEV)
        want_lq = P.degradations.mask_to(x, masks=np.stack([masks[i] for i in idx])[..., None])   # mask_id = the global image index
        assert torch.equal(LQ, want_lq)
        assert np.array_equal(LQ.cpu().numpy(), DO.mask_to(x.cpu().numpy(), np.stack([masks[i] for i in idx])[..., None]))
        assert torch.equal(out, _direct(model, want_lq, idx))


def test_eval_folder_stereo_sr(tmp_path):
    lq = _pngs(tmp_path / "LQ", 4, 8, 12, seed=6)     # L0, R0, L1, R1 in sorted order
    _pngs(tmp_path / "GT", 4, 32, 48, seed=7)
    cfg = dict(enc_blk_nums=tuple(SMALL["enc_blk_nums"]), middle_blk_num=SMALL["middle_blk_num"], dec_blk_nums=tuple(SMALL["dec_blk_nums"]))
    params = SO.stereo_synth_params(seed=0, img_channel=3, width=SMALL["width"], **cfg)
    torch.save({k: torch.from_numpy(v) for k, v in params.items()}, tmp_path / "S.pth")
    model = P.stereo_sr.ConditionalNAFNet(img_channel=3, **SMALL)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model = model.to(DEV).eval()
    args = ["--task", "stereo-sr", "--lq", str(tmp_path / "LQ"), "--gt", str(tmp_path / "GT"), "--weights", str(tmp_path / "S.pth"),
            "--naf-width", "32", "--naf-enc", "1,1", "--naf-mid", "1", "--naf-dec", "1,1"]
    summary, seen = _run(_tool(), args, tmp_path / "res")
    assert set(summary) == {"psnr", "ssim"} and [s[0] for s in seen] == [[0, 1]]
    _check_pngs(tmp_path / "res", ["img00", "img01", "img02", "img03"], (32, 48))
    idx, LQ, out = seen[0]
    views = [P.degradations.upscale(torch.from_numpy(np.stack([lq[2 * i + v] for i in idx])).to(DEV), 4) for v in range(2)]
    want_lq = torch.cat(views, dim=1)
    assert tuple(LQ.shape) == (2, 6, 32, 48) and torch.equal(LQ, want_lq)
    assert torch.equal(out, _direct(model, want_lq, idx))
    # the saved right view of pair 1 is channels 3..5 of the output
    from PIL import Image
    png = np.asarray(Image.open(str(tmp_path / "res" / "img03.png")))
    assert np.array_equal(png[..., ::-1], P.metrics.tensor2img_batch(out[1:2, 3:6])[0])
