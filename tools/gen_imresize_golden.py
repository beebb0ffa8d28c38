"""Generate tests/golden/imresize.npz from the REAL reference `imresize` (test infrastructure only; needs the reference tree).

codes/data/util.py is loaded by path with a stub `cv2` module in sys.modules (the file imports cv2 at the top and the resize never calls it),
and its `calculate_weights_indices` and `imresize` run on CPU tensors.  What they compute is stored, arrays only:

    tab/<s>/<a>/<n>/weights, indices, sym   the tables of calculate_weights_indices(n, ceil(n scale), scale, 'cubic', 4, antialiasing) for
                                            scale = SCALES[s], antialiasing = bool(a), n in TABLE_N, wherever imresize accepts an n x n image:
                                            weights fp32 [n_out][K], indices int64 [n_out][K] (into the extended axis, as returned), sym = [sym_s, sym_e]
    accept/<s>/<a>                          uint8 [len(ACCEPT_N)]: 1 where imresize runs an n x n image without raising
    out/<i>                                 imresize(inputs(i), scale, antialiasing) of tests/imresize_oracle.SHAPES[i], fp32 [B, C, Ho, Wo]

Usage:  python tools/gen_imresize_golden.py --ref <reference root>
Read by tests/test_imresize_host.py and tests/test_gpu_imresize.py, which rebuild the inputs from the seeded generator.
"""
import argparse
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imresize_oracle as IO  # noqa: E402


def load_util(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    path = os.path.join(ref, "codes", "data", "util.py")
    spec = importlib.util.spec_from_file_location("reference_data_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def accepts(util, n, scale, aa):
    try:
        util.imresize(torch.zeros(1, n, n), scale, aa)
        return True
    except Exception:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    util = load_util(args.ref)
    out = {}
    for s, scale in enumerate(IO.SCALES):
        for aa in (True, False):
            tag = "%d/%d" % (s, int(aa))
            verdict = [accepts(util, n, scale, aa) for n in IO.ACCEPT_N]
            out["accept/" + tag] = np.array(verdict, dtype=np.uint8)
            kept = []
            for n in IO.TABLE_N:
                if not accepts(util, n, scale, aa):
                    continue
                w, idx, sym_s, sym_e = util.calculate_weights_indices(n, math.ceil(n * scale), scale, "cubic", 4, aa)
                out["tab/%s/%d/weights" % (tag, n)] = w.numpy().astype(np.float32)
                out["tab/%s/%d/indices" % (tag, n)] = idx.numpy().astype(np.int64)
                out["tab/%s/%d/sym" % (tag, n)] = np.array([sym_s, sym_e], dtype=np.int64)
                kept.append(n)
            print("scale %.4g aa %d: accepts %d of %d, tables for %s" % (scale, aa, sum(verdict), len(verdict), kept), flush=True)
    for i, (B, C, H, W, scale, aa) in enumerate(IO.SHAPES):
        x = IO.inputs(i)
        y = util.imresize(torch.from_numpy(x), scale, aa).numpy()
        assert y.dtype == np.float32 and y.shape == (B, C, math.ceil(H * scale), math.ceil(W * scale)), (y.dtype, y.shape)
        out["out/%d" % i] = y
        r = IO.imresize(x, scale, aa)
        print("shape %s: range %.3f .. %.3f, reference vs float64 restatement %.2e of max|ref|" %
              ((B, C, H, W, scale, aa), y.min(), y.max(), np.abs(y - r).max() / np.abs(r).max()), flush=True)
    path = os.path.join(ROOT, "tests", "golden", "imresize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
