"""Generate tests/golden/stereo_wide.npz from the REAL reference stereo-sr networks (test infrastructure only; needs the reference tree).

Rows wider than the SCAM strip kernels hold in LDS (ConditionalUNet: level-0 width > 1024; ConditionalNAFNet: quarter-map width > 512): what
IRSDE_FLAG_SCAM_STREAM / `set_wide_rows()` runs on the streaming core.  The reference networks of codes/config/stereo-sr/models/modules run on
CPU with the seeded weights of tests/stereo_unet_oracle.py / tests/stereo_oracle.py; every network output is stored as its sub3 (every third
pixel, oracle.gen_golden.sub3).  The UNets take those weights with the value-projection gain 8 (tests/scam_stream_oracle.py, WIDE_UNET_GAINS): at the
narrow fixtures' gain of 4 a softmax over ~1030 columns moves the output by only 0.4 - 0.5 % of max |out|, and the fixtures must show >= 1 %:

    unet_small_1x6x1030/t77         ConditionalUNet nf 32, depth 2, 1 pair x 6 x 6 x 1030 (reflect-padded to 8 x 1032: SCAM widths 1032 and 516)
    unet_small_1x6x1030/sensitivity max |out(softmax -> uniform average) - out| / max |out| at t = 77; asserted >= 0.01 here
    unet_full_1x16x1040/t60         nf 64, depth 4, 1 pair x 6 x 16 x 1040 (SCAM widths 1040, 520, 260, 130)
    unet_full_1x16x1040/sensitivity the same measure at t = 60
    unet_small_sampler_1x6x1030_T5/sde, /ode   IRSDE(max_sigma 50, T 5, cosine, eps 0.005) with injected noise (seed 7)
    naf_small_1x16x2084/t37         ConditionalNAFNet width 32, enc [1, 1], middle 1, dec [1, 1], 1 pair x 6 x 16 x 2084 (quarter-map widths 521, 260, 130)
    naf_small_1x16x2084/sensitivity the same measure at t = 37
Inputs: oracle.irsde_oracle.synth_inputs per view (left: seed 1234, right: seed 1235), concatenated on channels.

Usage:  python tools/gen_stereo_wide_golden.py --ref <reference root>
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from oracle import irsde_oracle as O  # noqa: E402
from oracle.gen_golden import InjectedIRSDE, load_reference, load_task_modules, sub3  # noqa: E402
import gen_stereo_golden as GN  # noqa: E402
import gen_stereo_unet_golden as GU  # noqa: E402
import scam_stream_oracle as WS  # noqa: E402


def with_sensitivity(out, tag, key, net, xT, lq, t, run):
    ref = run(net, xT, lq, t)
    out[tag + "/" + key] = sub3(ref)
    sm = torch.softmax
    torch.softmax = lambda a, dim: torch.full_like(a, 1.0 / a.shape[dim])   # SCAM's two softmaxes -> plain averages
    try:
        uni = run(net, xT, lq, t)
    finally:
        torch.softmax = sm
    sens = float(np.abs(uni - ref).max() / np.abs(ref).max())
    out[tag + "/sensitivity"] = np.array(sens)
    print("%s: sensitivity (uniform softmax) %.4f of max|out|" % (tag, sens))
    assert sens >= 0.01, "the fixture must be attention-sensitive: " + tag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    sde_utils, _ = load_reference(args.ref)
    task = os.path.join(args.ref, "codes/config/stereo-sr")
    _, unet_arch = load_task_modules(task, ["module_util", "DenoisingUNet_arch"])
    _, naf_arch = load_task_modules(task, ["module_util", "DenoisingNAFNet_arch"])
    assert "stereo-sr" in unet_arch.__file__ and "stereo-sr" in naf_arch.__file__
    out = {}

    small = GU.build(unet_arch, dict(GU.SMALL, **WS.WIDE_UNET_GAINS))
    B, H, W = 1, 6, 1030
    lq, xT = GU.stereo_inputs(B, H, W)
    with_sensitivity(out, "unet_small_1x6x1030", "t77", small, xT, lq, 77, GU.run)

    class Shared(torch.nn.Module):   # the reference sampler passes an int step: one time for every pair
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x, cond, t):
            return self.net(x, cond, torch.full((x.shape[0],), int(t)))

    T = 5
    z = O.synth_noise(7, T, (B, 6, H, W))
    Inj = InjectedIRSDE.make(sde_utils)
    sde = Inj(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(z)
    sde.set_model(Shared(small))
    sde.set_mu(torch.from_numpy(lq))
    for mode in ("sde", "ode"):
        with torch.no_grad():
            fn = sde.reverse_sde if mode == "sde" else sde.reverse_ode
            out["unet_small_sampler_1x6x1030_T5/" + mode] = sub3(fn(torch.from_numpy(xT)).numpy())

    full = GU.build(unet_arch, dict(GU.FULL, **WS.WIDE_UNET_GAINS))
    lq, xT = GU.stereo_inputs(1, 16, 1040)
    with_sensitivity(out, "unet_full_1x16x1040", "t60", full, xT, lq, 60, GU.run)

    naf = GN.build(naf_arch, GN.SMALL)
    lq, xT = GN.stereo_inputs(1, 16, 2084)
    with_sensitivity(out, "naf_small_1x16x2084", "t37", naf, xT, lq, 37, GN.run)

    for k, v in out.items():
        if v.dtype == np.float64:
            out[k] = v.astype(np.float32) if v.ndim else v
    path = os.path.join(ROOT, "tests", "golden", "stereo_wide.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
