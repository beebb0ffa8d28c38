"""Degradation front ends (csrc/degrade.hip, degradations.py, tools/eval_folder.py --task sisr | inpainting | stereo-sr), host side (no GPU):
the float64 restatement against torch's own CPU `F.interpolate` (the reference's arithmetic, codes/utils/deg_utils.py), its sensitivity to
each rule of the filter, the C ABI additions and the evaluation tool's help."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
import degrade_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_BAR = 1e-5   # tests/test_gpu_degrade.py: kernel vs restatement, relative to max |ref|


def _x(shape, seed=0):
    return np.random.default_rng(seed).random(shape[:4], dtype=np.float32)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("shape", DO.SHAPES)
def test_restatement_matches_torch_bicubic(shape):
    x = _x(shape)
    ref = F.interpolate(torch.from_numpy(x), scale_factor=shape[4], mode="bicubic").numpy()
    got = DO.upscale(x, shape[4])
    assert got.shape == ref.shape
    e = _rel(got, ref)
    print("restatement vs torch-CPU bicubic %s: %.2e of max|ref| (max|ref| %.3f, min %.3f)" % (shape, e, np.abs(ref).max(), ref.min()))
    assert e < 2e-6


def test_phase_table_and_identity():
    assert np.array_equal(DO.phase_table(1), [[0.0, 1.0, 0.0, 0.0]])
    x = _x((1, 2, 5, 6))
    assert np.array_equal(DO.upscale(x, 1), x.astype(np.float64))
    for s in range(1, 9):
        tab = DO.phase_table(s)
        assert tab.shape == (s, 4) and np.allclose(tab.sum(1), 1.0, atol=1e-15)
    # the t = 0.5 phase is the filter scam_prologue_kernel hard-codes: [-3, 19, 19, -3] / 32
    assert np.allclose(DO.cubic_weights(0.5), np.array([-3.0, 19.0, 19.0, -3.0]) / 32.0, atol=1e-15)


@pytest.mark.parametrize("mutation", [dict(A=-0.5), dict(align_corners=True), dict(zero_pad=True), dict(clamp_src=True),
                                      dict(swap_tables=True), dict(reverse_taps=True)], ids=lambda m: next(iter(m)))
def test_restatement_is_sensitive_to_every_rule(mutation):
    """A kernel with one rule wrong misses the GPU bar at least tenfold on at least one of the test shapes."""
    worst = 0.0
    for shape in DO.SHAPES:
        x = _x(shape)
        worst = max(worst, _rel(DO.upscale(x, shape[4], **mutation), DO.upscale(x, shape[4])))
    print("mutation %s: %.2e of max|ref|" % (mutation, worst))
    assert worst >= 10 * GPU_BAR


@pytest.mark.parametrize("sizes", [((256, 256), (37, 53)), ((256, 256), (256, 256)), ((256, 256), (300, 500)), ((8, 8), (20, 28)), ((16, 16), (16, 16))])
def test_nearest_index_and_mask_to_match_torch(sizes):
    (Hm, Wm), (H, W) = sizes
    rng = np.random.default_rng(1)
    m8 = rng.choice(np.array([0, 77, 255], dtype=np.uint8), size=(2, Hm, Wm, 3))
    x = rng.random((2, 3, H, W), dtype=np.float32)
    mask = torch.tensor(m8 / 255.).permute(0, 3, 1, 2).float()           # deg_utils.py:30
    mask = F.interpolate(mask, size=(H, W), mode="nearest")             # :32
    ref = (mask * torch.from_numpy(x) + (1. - mask)).numpy()            # :33-34
    assert np.array_equal(DO.mask_to(x, m8), ref)


def test_abi_additions():
    L = _lib.lib()
    assert L.irsde_version() == 107
    for name in ("irsde_upscale_bicubic", "irsde_mask_to"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # never dereferenced: every call below is refused on its arguments
    assert L.irsde_upscale_bicubic(None, p, 1, 3, 4, 4, 4, None) == -1 and b"null" in L.irsde_last_error()
    assert L.irsde_upscale_bicubic(p, None, 1, 3, 4, 4, 4, None) == -1 and b"null" in L.irsde_last_error()
    for scale in (0, -2, 9):
        assert L.irsde_upscale_bicubic(p, p, 1, 3, 4, 4, scale, None) == -1 and b"scale" in L.irsde_last_error()
    for dims in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, -1, 4), (1, 3, 4, 0)):
        assert L.irsde_upscale_bicubic(p, p, *dims, 4, None) == -1 and b"positive" in L.irsde_last_error()
    assert L.irsde_mask_to(None, p, 1, 4, 4, 1, p, 1, 3, 4, 4, None) == -1 and b"null" in L.irsde_last_error()
    assert L.irsde_mask_to(p, None, 1, 4, 4, 1, p, 1, 3, 4, 4, None) == -1 and b"null" in L.irsde_last_error()
    assert L.irsde_mask_to(p, p, 1, 4, 4, 1, None, 1, 3, 4, 4, None) == -1 and b"null" in L.irsde_last_error()
    assert L.irsde_mask_to(p, p, 2, 4, 4, 1, p, 3, 3, 4, 4, None) == -1 and b"Bm" in L.irsde_last_error()
    assert L.irsde_mask_to(p, p, 1, 4, 4, 2, p, 3, 3, 4, 4, None) == -1 and b"Cm" in L.irsde_last_error()
    assert L.irsde_mask_to(p, p, 1, 0, 4, 1, p, 1, 3, 4, 4, None) == -1 and b"positive" in L.irsde_last_error()
    assert L.irsde_mask_to(p, p, 1, 4, 4, 1, p, 1, 3, 4, 0, None) == -1 and b"positive" in L.irsde_last_error()


def test_python_surface_refuses_what_is_not_built():
    assert "degradations" in P.__all__ and P.degradations.add_noise is P.denoising_sde.add_noise
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(P.IrsdeError, match="no CPU fallback"):
        P.degradations.upscale(x, 4)
    with pytest.raises(P.IrsdeError, match="no CPU fallback"):
        P.degradations.mask_to(x, masks=np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(P.IrsdeError, match="bicubic"):
        P.degradations.upscale(x, 4, mode="bilinear")
    for scale in (2.5, 0.5, 0, 9, -1):
        with pytest.raises(P.IrsdeError, match="integer in 1..8"):
            P.degradations.upscale(x, scale)


def test_eval_folder_help_names_the_new_tasks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("sisr", "inpainting", "stereo-sr", "--mask-root", "--wide-rows"):
        assert word in r.stdout, word
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--task", "inpainting", "--gt", "x", "--weights", "x.pth"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--mask-root" in r.stderr
