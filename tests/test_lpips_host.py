"""LPIPS (metrics.LPIPS, irsde_create_lpips / irsde_lpips) without a GPU: checkpoint key mapping, the engine's weight inventory, the error
paths that need no device, the oracle's shape function, and the command-line / signature surface.

Values on real weights (the reference README's LPIPS column) are unpinned and blocked on assets, like the Rain100H PSNR gate: the published
AlexNet and lpips weight files are not available where this suite was written.  Everything here and in tests/test_gpu_lpips.py runs on
tests/lpips_oracle.py's synthetic weights."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib, metrics as M
import lpips_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lpips_layout, files_layout = LO.lpips_layout, LO.files_layout


def test_both_layouts_load_to_the_same_15_tensors():
    w = LO.synth_weights(0)
    a = M.lpips_map_state_dict(lpips_layout(w))
    b = M.lpips_map_state_dict({"module." + k: v for k, v in files_layout(w).items()})
    c = M.lpips_map_state_dict({"module.module." + k: v for k, v in lpips_layout(w).items()})
    assert sorted(a) == sorted(b) == sorted(c) == sorted(w) and len(a) == 15
    for k in w:
        assert a[k].dtype == torch.float32 and tuple(a[k].shape) == w[k].shape
        assert np.array_equal(a[k].numpy(), w[k]) and np.array_equal(b[k].numpy(), w[k]) and np.array_equal(c[k].numpy(), w[k])
    m = P.metrics.LPIPS(net="alex").load_state_dict(lpips_layout(w))
    assert sorted(m.weights) == sorted(w)


def test_from_files_merges_the_two_files(tmp_path):
    w = LO.synth_weights(1)
    full = files_layout(w)
    torch.save({k: v for k, v in full.items() if not k.startswith("lin")}, tmp_path / "alexnet.pth")
    torch.save({k: v for k, v in full.items() if k.startswith("lin")}, tmp_path / "alex.pth")
    m = M.LPIPS.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))
    assert all(np.array_equal(m.weights[k].numpy(), w[k]) for k in w)
    with pytest.raises(P.IrsdeError, match="missing"):
        M.LPIPS.from_files(str(tmp_path / "alexnet.pth"))


def test_missing_tensor_wrong_shape_and_wrong_scaling_layer_raise():
    w = LO.synth_weights(0)
    sd = lpips_layout(w)
    del sd["net.slice3.6.bias"]
    with pytest.raises(P.IrsdeError, match="conv3.bias"):
        M.lpips_map_state_dict(sd)
    sd = lpips_layout(w)
    sd["scaling_layer.scale"] = torch.tensor([.458, .448, .5]).view(1, 3, 1, 1)
    with pytest.raises(P.IrsdeError, match="scaling_layer.scale"):
        M.lpips_map_state_dict(sd)
    sd = lpips_layout(w)
    sd["lin2.model.1.weight"] = sd["lin2.model.1.weight"][:, :100]
    with pytest.raises(P.IrsdeError, match="shape"):
        M.lpips_map_state_dict(sd)


def test_constructor_refuses_what_is_not_built():
    for kw in (dict(net="vgg"), dict(net="squeeze"), dict(spatial=True), dict(version="0.0")):
        with pytest.raises(P.IrsdeError):
            M.LPIPS(**kw)
    assert M.LPIPS is P.metrics.LPIPS and P.LPIPS is M.LPIPS


def _inventory(L, h):
    out = {}
    for i in range(L.irsde_num_weights(h)):
        shape = (ctypes.c_int64 * 4)()
        nd = ctypes.c_int()
        assert L.irsde_weight_shape(h, i, shape, ctypes.byref(nd)) == 0
        out[L.irsde_weight_name(h, i).decode()] = tuple(shape[k] for k in range(nd.value))
    return out


def test_engine_inventory_is_the_15_names_and_shapes():
    L = _lib.lib()
    assert L.irsde_version() == 107
    h = ctypes.c_void_p()
    assert L.irsde_create_lpips(ctypes.byref(h)) == 0
    try:
        inv = _inventory(L, h)
        assert inv == M.LPIPS_SHAPES and len(inv) == 15
        assert inv == {k: v.shape for k, v in LO.synth_weights(0).items()}
        # a wrong shape and an unknown name are refused as for every engine
        bad = np.zeros((64, 3, 11, 10), np.float32)
        shape = (ctypes.c_int64 * 4)(*bad.shape)
        assert L.irsde_load_weight(h, b"conv1.weight", bad.ctypes.data_as(ctypes.c_void_p), shape, 4) == -4
        assert L.irsde_load_weight(h, b"conv6.weight", bad.ctypes.data_as(ctypes.c_void_p), shape, 4) == -4
    finally:
        L.irsde_destroy(h)
    assert L.irsde_create_lpips(None) < 0


def test_calls_fail_cleanly_before_finalize_and_on_a_unet_engine():
    L = _lib.lib()
    dist = (ctypes.c_double * 1)()
    dims = (ctypes.c_int64 * 4)()
    fake = ctypes.c_void_p(256)   # never dereferenced: every check below comes first
    h = ctypes.c_void_p()
    assert L.irsde_create_lpips(ctypes.byref(h)) == 0
    try:
        assert L.irsde_lpips(h, fake, fake, 1, 64, 64, 0, dist, None, None) < 0
        assert b"not finalized" in L.irsde_last_error()
        assert L.irsde_debug_lpips_tap(h, fake, 1, 64, 64, 0, 1, None, dims, None) < 0
        assert b"not finalized" in L.irsde_last_error()
        assert L.irsde_lpips(h, None, fake, 1, 64, 64, 0, dist, None, None) < 0
        # the score-network calls refuse an LPIPS engine
        t = (ctypes.c_int64 * 1)(1)
        assert L.irsde_unet_forward(h, fake, fake, t, 1, 1, 32, 32, fake, None) < 0
        coef = (ctypes.c_float * (12 * 3))()
        assert L.irsde_set_schedule(h, 2, coef) < 0
        assert b"LPIPS engine" in L.irsde_last_error()
    finally:
        L.irsde_destroy(h)
    u = ctypes.c_void_p()
    cfg = _lib.Config(3, 3, 32, 2, 0, 0)
    assert L.irsde_create(ctypes.byref(cfg), ctypes.byref(u)) == 0
    try:
        assert L.irsde_lpips(u, fake, fake, 1, 64, 64, 0, dist, None, None) < 0
        assert b"not an LPIPS engine" in L.irsde_last_error()
        assert L.irsde_debug_lpips_tap(u, fake, 1, 64, 64, 0, 1, None, dims, None) < 0
        assert b"not an LPIPS engine" in L.irsde_last_error()
    finally:
        L.irsde_destroy(u)


def test_cpu_tensors_and_bad_shapes_raise():
    m = M.LPIPS().load_state_dict(lpips_layout(LO.synth_weights(0)))
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(P.IrsdeError, match="no CPU fallback"):
        m(x, x)
    with pytest.raises(P.IrsdeError):
        m.terms(x, x)
    with pytest.raises(P.IrsdeError):
        P.metrics.evaluate_batch(x, x, lpips=m)


@pytest.mark.parametrize("hw", [(31, 31), (64, 48), (97, 130), (256, 256)])
def test_feature_shapes_agree_with_the_oracle_maps(hw):
    w = LO.synth_weights(0)
    x = torch.zeros(1, 3, *hw, dtype=torch.float32)
    maps = LO.features(w, x, torch.float32)
    assert [tuple(f.shape[1:]) for f in maps] == LO.feature_shapes(*hw)
    if hw == (256, 256):
        assert LO.feature_shapes(*hw) == [(64, 63, 63), (192, 31, 31), (384, 15, 15), (256, 15, 15), (256, 15, 15)]
    if hw == (31, 31):
        assert LO.feature_shapes(*hw)[2:] == [(384, 1, 1), (256, 1, 1), (256, 1, 1)]


def test_eval_folder_help_shows_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--lpips-weights" in r.stdout and "LPIPS" in r.stdout
    assert "LPIPS is not computed" not in r.stdout


def test_evaluate_batch_leaves_lpips_off_by_default():
    sig = inspect.signature(P.metrics.evaluate_batch)
    assert list(sig.parameters) == ["output", "gt", "crop_border", "lpips"]
    assert sig.parameters["lpips"].default is None and sig.parameters["crop_border"].default == 0
