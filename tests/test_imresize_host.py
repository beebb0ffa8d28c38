"""imresize (degradations.imresize_tables / imresize / modcrop, csrc/degrade.hip imresize_kernel, tools/eval_folder.py --lq-from-gt), host side
(no GPU): the filter tables bit for bit against the reference's (tests/golden/imresize.npz, written by tools/gen_imresize_golden.py from the
real codes/data/util.py), the refusal rule against the reference's accept set, the float64 restatement (tests/imresize_oracle.py) against the
reference's outputs and its sensitivity to each rule, modcrop, the C ABI addition and the evaluation tool's flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from image_restoration_sde_amd import degradations as D
import imresize_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "imresize.npz"))
CASES = [(s, aa) for s in range(len(IO.SCALES)) for aa in (True, False)]


def _accepted(n, scale, aa):
    try:
        D.imresize_tables(n, scale, aa)
        return True
    except P.IrsdeError:
        return False


@pytest.mark.parametrize("s,aa", CASES)
def test_tables_are_the_reference_tables_bit_for_bit(s, aa):
    scale, seen = IO.SCALES[s], 0
    for n in IO.TABLE_N:
        key = "tab/%d/%d/%d/" % (s, int(aa), n)
        if key + "weights" not in GOLDEN:
            assert not _accepted(n, scale, aa), (scale, aa, n)
            continue
        w, start, sym_s, sym_e = D.imresize_tables(n, scale, aa)
        ref_w, ref_idx = GOLDEN[key + "weights"], GOLDEN[key + "indices"]
        assert w.dtype == torch.float32 and start.dtype == torch.int32 and tuple(w.shape) == ref_w.shape and tuple(start.shape) == ref_w.shape[:1]
        assert np.array_equal(w.numpy().view(np.uint32), ref_w.view(np.uint32)), (scale, aa, n)
        assert [sym_s, sym_e] == GOLDEN[key + "sym"].tolist(), (scale, aa, n)
        # the reference's indices address the axis extended by sym_s pixels in front: image coordinate + sym_s
        assert np.array_equal(start.numpy().astype(np.int64)[:, None] + np.arange(w.shape[1])[None, :] + sym_s, ref_idx), (scale, aa, n)
        assert np.all(np.diff(start.numpy()) >= 0)   # what the kernel's tile span relies on
        seen += 1
    assert seen or (scale == 1 / 8 and not aa)   # the reference runs 1/8 without antialiasing at no size


@pytest.mark.parametrize("s,aa", CASES)
def test_refusal_rule_is_the_reference_accept_set(s, aa):
    want = GOLDEN["accept/%d/%d" % (s, int(aa))].astype(bool).tolist()
    assert [_accepted(n, IO.SCALES[s], aa) for n in IO.ACCEPT_N] == want


def test_accept_set_examples_and_refused_arguments():
    assert not any(_accepted(n, 1 / 4, False) for n in range(4, 41, 4))
    assert not any(_accepted(n, 1 / 8, False) for n in IO.ACCEPT_N)
    assert [_accepted(n, 1 / 4, True) for n in (5, 6, 7, 8)] == [False, False, True, True]
    for aa in (True, False):
        for scale in IO.SCALES:
            with pytest.raises(P.IrsdeError, match="one pixel"):
                D.imresize_tables(1, scale, aa)
    with pytest.raises(P.IrsdeError, match="use upscale"):
        D.imresize_tables(16, 2, True)
    with pytest.raises(P.IrsdeError, match="use upscale"):
        D.imresize_tables(16, 1.0001, True)
    with pytest.raises(P.IrsdeError, match="below 1/8"):
        D.imresize_tables(400, 0.1, True)
    for scale in (0, 0.0, -0.25, float("nan")):
        with pytest.raises(P.IrsdeError, match="positive"):
            D.imresize_tables(16, scale, True)
    with pytest.raises(P.IrsdeError, match="number"):
        D.imresize_tables(16, "0.25", True)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("i", range(len(IO.SHAPES)))
def test_restatement_matches_the_reference_outputs(i):
    """Measured with the seeded inputs (max |restatement - reference fp32| / max |reference|; the bar is 1e-6): 1.9e-7, 1.9e-7, 6.1e-8,
    1.9e-7, 3.1e-7, 4.2e-7, 3.0e-7, 0, 1.0e-7, 1.6e-7, 1.8e-7 in the order of imresize_oracle.SHAPES."""
    B, C, H, W, scale, aa = IO.SHAPES[i]
    ref = GOLDEN["out/%d" % i]
    got = IO.imresize(IO.inputs(i), scale, aa)
    assert got.shape == ref.shape and ref.dtype == np.float32
    e = _rel(got, ref.astype(np.float64))
    print("restatement vs reference %s: %.2e of max|ref| (range %.3f .. %.3f)" % (IO.SHAPES[i], e, ref.min(), ref.max()))
    assert e < 1e-6
    # the same sum over the product's own tables (bit-identical to the reference's): the restatement's tables are the rules, not a copy
    (wH, sH, _, _), (wW, sW, _, _) = D.imresize_tables(H, scale, aa), D.imresize_tables(W, scale, aa)
    x = IO.inputs(i).astype(np.float64)
    via = IO.apply_axis(IO.apply_axis(x, wH.numpy().astype(np.float64), sH.numpy().astype(np.int64), -2), wW.numpy().astype(np.float64),
                        sW.numpy().astype(np.int64), -1)
    assert _rel(via, ref.astype(np.float64)) < 1e-6


@pytest.mark.parametrize("mutation", IO.MUTATIONS, ids=lambda m: next(iter(m)))
def test_restatement_is_sensitive_to_every_rule(mutation):
    worst = 0.0
    for i, (B, C, H, W, scale, aa) in enumerate(IO.SHAPES):
        x = IO.inputs(i)
        worst = max(worst, _rel(IO.imresize(x, scale, aa, **mutation), IO.imresize(x, scale, aa)))
    print("mutation %s: %.2e of max|ref|" % (mutation, worst))
    assert worst > 1e-3


def test_scale_one_tables_are_the_identity():
    w, start, sym_s, sym_e = D.imresize_tables(9, 1.0, True)
    assert np.array_equal(w.numpy(), np.tile(np.array([0, 1, 0, 0], dtype=np.float32), (9, 1)))
    assert start.tolist() == list(range(-1, 8)) and (sym_s, sym_e) == (1, 2)


def test_modcrop_equals_slicing():
    rng = np.random.default_rng(0)
    t = torch.from_numpy(rng.random((2, 3, 30, 43), dtype=np.float32))
    assert torch.equal(D.modcrop(t, 4), t[:, :, :28, :40])
    assert torch.equal(D.modcrop(t[0], 7), t[0, :, :28, :42])
    assert torch.equal(D.modcrop(t[0, 0], 5), t[0, 0, :30, :40])
    assert D.modcrop(t, 1).shape == t.shape
    hwc = rng.random((29, 50, 3), dtype=np.float32)
    got = D.modcrop(hwc, 4)
    assert np.array_equal(got, hwc[:28, :48, :]) and not np.shares_memory(got, hwc)
    assert np.array_equal(D.modcrop(hwc[:, :, 0], 3), hwc[:27, :48, 0])
    with pytest.raises(P.IrsdeError, match="ndim"):
        D.modcrop(np.zeros((2, 3, 4, 5)), 2)
    for scale in (0, 2.0, True):
        with pytest.raises(P.IrsdeError, match="positive integer"):
            D.modcrop(t, scale)


def test_abi_addition():
    L = _lib.lib()
    assert L.irsde_version() == 107
    assert "irsde_imresize" in _lib.SYMBOLS and hasattr(L, "irsde_imresize")
    with open(os.path.join(ROOT, "include", "irsde_hip.h")) as f:
        assert "int irsde_imresize(" in f.read()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # never dereferenced: every call below is refused on its arguments

    def call(ptrs=(p,) * 6, dims=(1, 3, 8, 8, 2, 2), KH=16, KW=16):
        i, o, wH, sH, wW, sW = ptrs
        return L.irsde_imresize(i, o, *dims, wH, sH, KH, wW, sW, KW, None)

    for k in range(6):
        assert call(ptrs=tuple(None if j == k else p for j in range(6))) == -1 and b"null" in L.irsde_last_error(), k
    for k in range(6):
        for bad in (0, -1):
            dims = [1, 3, 8, 8, 2, 2]
            dims[k] = bad
            assert call(dims=tuple(dims)) == -1 and b"positive" in L.irsde_last_error(), (k, bad)
    for bad in (0, -1, 33):
        assert call(KH=bad) == -1 and b"taps" in L.irsde_last_error()
        assert call(KW=bad) == -1 and b"taps" in L.irsde_last_error()


def test_python_surface():
    assert "imresize" in D.__all__ and "modcrop" in D.__all__
    with pytest.raises(P.IrsdeError, match="no CPU fallback"):
        D.imresize(torch.zeros(1, 3, 16, 16), 1 / 4)
    with pytest.raises(P.IrsdeError, match="no CPU fallback"):
        D.imresize(torch.zeros(3, 16, 16), 1 / 2, False)


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py")] + list(args), capture_output=True, text=True)


def test_eval_folder_flag():
    r = _tool("--help")
    assert r.returncode == 0 and "--lq-from-gt" in r.stdout and "imresize" in r.stdout
    r = _tool("--lq-from-gt", "--gt", "x", "--lq", "y", "--weights", "x.pth")                       # without --task sisr
    assert r.returncode == 2 and "--task sisr" in r.stderr
    r = _tool("--task", "inpainting", "--lq-from-gt", "--gt", "x", "--mask-root", "m", "--weights", "x.pth")
    assert r.returncode == 2 and "--task sisr" in r.stderr
    r = _tool("--task", "sisr", "--lq-from-gt", "--gt", "x", "--lq", "y", "--weights", "x.pth")    # with --lq
    assert r.returncode == 2 and "--lq must be absent" in r.stderr
    r = _tool("--task", "sisr", "--lq-from-gt", "--weights", "x.pth")                               # without --gt
    assert r.returncode == 2 and "--gt" in r.stderr
    r = _tool("--task", "sisr", "--gt", "x", "--weights", "x.pth")                                  # as before: sisr without --lq
    assert r.returncode == 2 and "--lq" in r.stderr
