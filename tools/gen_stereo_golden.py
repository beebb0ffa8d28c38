"""Generate tests/golden/stereo.npz from the REAL reference stereo-sr network (test infrastructure only; needs the reference tree).

The reference `ConditionalNAFNet` of codes/config/stereo-sr/models/modules/DenoisingNAFNet_arch.py (NAFBlocks + SCAM) runs on CPU
with the seeded synthetic weights of tests/stereo_oracle.py (oracle.irsde_oracle.naf_synth_params + SCAM tensors whose *_proj1 are
scaled up so the cross-view scores span several units), and its outputs are stored as fixtures:

    names                         the reference state_dict names of the ssr refusion.yml config (width 64, enc [1,1,1,28], middle 1, dec [1,1,1,1])
    small_2x32x48/t3, /t77        small net (width 32 -- the engine's smallest width --, enc [1,1], middle 1, dec [1,1]), 2 pairs x 6 x 32 x 48,
                                  one time for both pairs (the reference's int path needs B = 1: these call it with a [B] tensor of equal entries)
    small_2x32x48/t5_60           the same with per-pair times [5, 60]
    small_2x32x48/scam_in, /scam_out_sub3
                                  middle_blks.0.fusion input (full) and output (every third pixel, tools' sub3) at t = 77, forward hooks
    small_2x32x48/sensitivity     max |out(softmax -> uniform average) - out| / max |out| at t = 77
    refusion_1x64x64/t60          refusion config, 1 pair x 6 x 64 x 64 (SCAM maps down to 1 x 1)
    refusion_1x64x64/scam_in, /scam_out   middle_blks.0.fusion (c = 1024, 4 x 4 map, W' = 1)
    refusion_1x80x112/t37_sub3    refusion config, 1 pair x 6 x 80 x 112 (non-multiple-of-4 SCAM maps 5 x 7 -> 1 x 1), every third pixel
    small_sampler_2x32x48_T20/sde, /ode   IRSDE(max_sigma 50, T 20, cosine, eps 0.005; ssr refusion.yml) with injected noise (seed 7),
                                  reverse_sde and reverse_ode (the stereo test() switch), the int step time shared by both pairs
Inputs: oracle.irsde_oracle.synth_inputs(1234, B, H, W) per view (left: seed 1234, right: seed 1235), concatenated on channels.

Usage:  python tools/gen_stereo_golden.py --ref <reference root>
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
from oracle import irsde_oracle as O  # noqa: E402
from oracle.gen_golden import InjectedIRSDE, load_reference, load_task_modules, sub3  # noqa: E402
import stereo_oracle as SO  # noqa: E402

SMALL = dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
REFUSION = dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def stereo_inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


def build(arch, cfg, seed=0):
    params = SO.stereo_synth_params(seed=seed, img_channel=3, width=cfg["width"], middle_blk_num=cfg["middle_blk_num"],
                                    enc_blk_nums=tuple(cfg["enc_blk_nums"]), dec_blk_nums=tuple(cfg["dec_blk_nums"]))
    net = arch.ConditionalNAFNet(img_channel=3, **cfg).eval()
    sd = net.state_dict()
    assert set(sd) == set(params), set(sd) ^ set(params)
    for k in sd:
        assert tuple(sd[k].shape) == params[k].shape, (k, sd[k].shape, params[k].shape)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return net


def run(net, x, lq, t):
    tt = torch.as_tensor(np.broadcast_to(np.atleast_1d(t), (x.shape[0],)).copy())
    with torch.no_grad():
        return net(torch.from_numpy(x), torch.from_numpy(lq), tt).numpy()


def hooked(net, x, lq, t, module):
    got = {}
    h = module.register_forward_hook(lambda m, i, o: got.update(inp=i[0].detach().numpy().copy(), out=o.detach().numpy().copy()))
    try:
        run(net, x, lq, t)
    finally:
        h.remove()
    return got["inp"], got["out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    sde_utils, _ = load_reference(args.ref)
    _, arch = load_task_modules(os.path.join(args.ref, "codes/config/stereo-sr"), ["module_util", "DenoisingNAFNet_arch"])
    out = {}
    out["names"] = np.array(sorted(arch.ConditionalNAFNet(img_channel=3, **REFUSION).state_dict()))

    small = build(arch, SMALL)
    lq, xT = stereo_inputs(2, 32, 48)
    for t in (3, 77):
        out["small_2x32x48/t%d" % t] = run(small, xT, lq, t)
    out["small_2x32x48/t5_60"] = run(small, xT, lq, np.array([5, 60]))
    sin, sout = hooked(small, xT, lq, 77, small.middle_blks[0].fusion)
    out["small_2x32x48/scam_in"], out["small_2x32x48/scam_out_sub3"] = sin, sub3(sout)
    ref = out["small_2x32x48/t77"]
    sm = torch.softmax
    torch.softmax = lambda a, dim: torch.full_like(a, 1.0 / a.shape[dim])   # SCAM's two softmaxes -> plain averages
    try:
        uni = run(small, xT, lq, 77)
    finally:
        torch.softmax = sm
    out["small_2x32x48/sensitivity"] = np.array(float(np.abs(uni - ref).max() / np.abs(ref).max()))
    print("sensitivity (uniform softmax) %.3f of max|out|" % out["small_2x32x48/sensitivity"])

    big = build(arch, REFUSION)
    lq, xT = stereo_inputs(1, 64, 64)
    out["refusion_1x64x64/t60"] = run(big, xT, lq, 60)
    out["refusion_1x64x64/scam_in"], out["refusion_1x64x64/scam_out"] = hooked(big, xT, lq, 60, big.middle_blks[0].fusion)
    lq, xT = stereo_inputs(1, 80, 112)
    out["refusion_1x80x112/t37_sub3"] = sub3(run(big, xT, lq, 37))

    class Shared(torch.nn.Module):   # the reference sampler passes an int step: one time for every pair
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x, cond, t):
            return self.net(x, cond, torch.full((x.shape[0],), int(t)))

    B, H, W, T = 2, 32, 48, 20
    lq, xT = stereo_inputs(B, H, W)
    z = O.synth_noise(7, T, (B, 6, H, W))
    Inj = InjectedIRSDE.make(sde_utils)
    sde = Inj(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(z)
    sde.set_model(Shared(small))
    sde.set_mu(torch.from_numpy(lq))
    key = "small_sampler_%dx%dx%d_T%d" % (B, H, W, T)
    for mode in ("sde", "ode"):
        with torch.no_grad():
            fn = sde.reverse_sde if mode == "sde" else sde.reverse_ode
            out[key + "/" + mode] = fn(torch.from_numpy(xT)).numpy()
    for k, v in out.items():
        if v.dtype == np.float64:
            out[k] = v.astype(np.float32) if v.ndim else v
    path = os.path.join(ROOT, "tests", "golden", "stereo.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
