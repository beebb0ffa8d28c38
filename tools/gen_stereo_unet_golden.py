"""Generate tests/golden/stereo_unet.npz from the REAL reference stereo-sr UNet (test infrastructure only; needs the reference tree).

The reference `ConditionalUNet` of codes/config/stereo-sr/models/modules/DenoisingUNet_arch.py (a full-resolution SCAM on every level) runs
on CPU with the seeded synthetic weights of tests/stereo_unet_oracle.py (beta / gamma ~ U(+-0.5), *_proj1 scaled up so the cross-view
scores are far from flat), and its outputs are stored as fixtures:

    names                          the reference state_dict names at nf = 64, depth = 4
    small_2x22x38/t3, /t77         small net (nf 32, depth 2), 2 pairs x 6 x 22 x 38 (reflect-padded to 24 x 40: SCAM widths 40 and 20 — the last down level keeps its size), one
                                   time for both pairs (the reference's int path needs B = 1: these call it with a [B] tensor of equal entries)
    small_2x22x38/t5_60            the same with per-pair times [5, 60]
    small_2x22x38/mid_fusion_in, /mid_fusion_out, /ups13_in, /ups13_out
                                   forward-hook input / output of mid_fusion (c = 128, 12 x 20) and ups.1.3 (c = 64, 24 x 40) at t = 77; a SCAM
                                   works on one image row at a time, so only the map's first and last row are kept ([2B, c, 2, W])
    small_2x22x38/sensitivity      max |out(softmax -> uniform average) - out| / max |out| at t = 77; asserted >= 0.01 here
    full_1x32x48/t60_sub3          nf 64, depth 4, 1 pair x 6 x 32 x 48, every third pixel (oracle.gen_golden.sub3)
    small_sampler_2x22x38_T20/sde, /ode   IRSDE(max_sigma 50, T 20, cosine, eps 0.005) with injected noise (seed 7), reverse_sde / reverse_ode
Inputs: oracle.irsde_oracle.synth_inputs per view (left: seed 1234, right: seed 1235), concatenated on channels.

Usage:  python tools/gen_stereo_unet_golden.py --ref <reference root>
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
import stereo_unet_oracle as SU  # noqa: E402

SMALL = dict(nf=32, depth=2)
FULL = dict(nf=64, depth=4)


def stereo_inputs(B, H, W):
    lq_l, x_l = O.synth_inputs(1234, B, H, W, max_sigma=50)
    lq_r, x_r = O.synth_inputs(1235, B, H, W, max_sigma=50)
    return np.concatenate([lq_l, lq_r], axis=1), np.concatenate([x_l, x_r], axis=1)


def build(arch, cfg, seed=0):
    params = SU.stereo_unet_synth_params(seed=seed, **cfg)
    net = arch.ConditionalUNet(3, 3, cfg["nf"], depth=cfg["depth"]).eval()
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


def end_rows(a):
    return np.ascontiguousarray(a[:, :, [0, a.shape[2] - 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    sde_utils, _ = load_reference(args.ref)
    _, arch = load_task_modules(os.path.join(args.ref, "codes/config/stereo-sr"), ["module_util", "DenoisingUNet_arch"])
    assert "stereo-sr" in arch.__file__
    out = {}
    out["names"] = np.array(sorted(arch.ConditionalUNet(3, 3, **FULL).state_dict()))

    small = build(arch, SMALL)
    B, H, W = 2, 22, 38
    tag = "small_%dx%dx%d" % (B, H, W)
    lq, xT = stereo_inputs(B, H, W)
    for t in (3, 77):
        out[tag + "/t%d" % t] = run(small, xT, lq, t)
    out[tag + "/t5_60"] = run(small, xT, lq, np.array([5, 60]))
    for key, mod in (("mid_fusion", small.mid_fusion), ("ups13", small.ups[1][3])):
        sin, sout = hooked(small, xT, lq, 77, mod)
        out[tag + "/" + key + "_in"], out[tag + "/" + key + "_out"] = end_rows(sin), end_rows(sout)
    ref = out[tag + "/t77"]
    sm = torch.softmax
    torch.softmax = lambda a, dim: torch.full_like(a, 1.0 / a.shape[dim])   # SCAM's two softmaxes -> plain averages
    try:
        uni = run(small, xT, lq, 77)
    finally:
        torch.softmax = sm
    sens = float(np.abs(uni - ref).max() / np.abs(ref).max())
    out[tag + "/sensitivity"] = np.array(sens)
    print("sensitivity (uniform softmax) %.4f of max|out|" % sens)
    assert sens >= 0.01, "the fixture must be attention-sensitive: raise SCAM_PROJ1_GAIN in tests/stereo_unet_oracle.py"

    full = build(arch, FULL)
    lq, xT = stereo_inputs(1, 32, 48)
    out["full_1x32x48/t60_sub3"] = sub3(run(full, xT, lq, 60))

    class Shared(torch.nn.Module):   # the reference sampler passes an int step: one time for every pair
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x, cond, t):
            return self.net(x, cond, torch.full((x.shape[0],), int(t)))

    T = 20
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
    path = os.path.join(ROOT, "tests", "golden", "stereo_unet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
