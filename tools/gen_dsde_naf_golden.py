"""Generate tests/golden/dsde_naf.npz from the REAL reference denoising-sde network (test infrastructure only; needs the reference tree).

The reference `ConditionalNAFNet` of codes/config/denoising-sde/models/modules/DenoisingNAFNet_arch.py (forward(x, time): no condition
input) and `DenoisingSDE` of codes/utils/sde_utils.py run on the CPU with the seeded synthetic weights of tests/dsde_naf_oracle.py
(oracle.irsde_oracle.naf_synth_params with a [width, 3, 3, 3] intro.weight), and their outputs are stored as fixtures:

    <cfg>/names, <cfg>/shapes     the reference state_dict inventory (cfg = refusion: width 64, enc [1,1,1,28], middle 1, dec [1,1,1,1] --
                                  denoising-sde/options/test/refusion.yml; w32_e12: width 32, enc [1,2], middle 1, dec [1,1])
    w32_e12_2x22x19/ts, /t<t>     forward at t in {1, 7, T_opt}, 2 x 3 x 22 x 19 (zero pad to 24 x 20: ragged on both axes)
    refusion_1x40x56/ts, /t<t>    the same for the refusion config, 1 x 3 x 40 x 56 (pads to 48 x 64)
    w32_e12_2x22x19/sampler/{T, noisy, ode, sde}
                                  DenoisingSDE(max_sigma 50, T 100), sigma 25: T = get_optimal_timestep(25), reverse_ode and reverse_sde
                                  (injected noise, seed 7) from noisy = clean + sigma / 255 z
    refusion_1x32x32/sampler/{T, noisy, ode}
                                  the shipped config's schedule DenoisingSDE(max_sigma 70, T 1000), sigma 15, reverse_ode from T_opt
Inputs: tests/dsde_naf_oracle.py `inputs` (clean = oracle.synth_inputs(1234, ...)'s LQ).

Usage:  python tools/gen_dsde_naf_golden.py --ref <reference root>      (15 s of CPU wall time; the file is 159 KB)
Read by tests/test_dsde_naf_host.py and tests/test_gpu_dsde_naf.py; the tests rebuild weights, inputs and injected noise from the seeded
generators and read only the reference's outputs (and the stored noisy sampler inputs) from the file.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import irsde_oracle as O  # noqa: E402
from oracle.gen_golden import load_reference, load_task_modules  # noqa: E402
import dsde_naf_oracle as DN  # noqa: E402


def build(arch, cfg):
    kw = dict(width=cfg["width"], enc_blk_nums=list(cfg["enc_blk_nums"]), middle_blk_num=cfg["middle_blk_num"], dec_blk_nums=list(cfg["dec_blk_nums"]))
    params = DN.synth_params(seed=0, img_channel=3, **cfg)
    net = arch.ConditionalNAFNet(img_channel=3, **kw).eval()
    sd = net.state_dict()
    assert set(sd) == set(params), set(sd) ^ set(params)
    for k in sd:
        assert tuple(sd[k].shape) == params[k].shape, (k, sd[k].shape, params[k].shape)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    tic = time.time()
    sde_utils, _ = load_reference(args.ref)
    (arch,) = load_task_modules(os.path.join(args.ref, "codes/config/denoising-sde"), ["DenoisingNAFNet_arch"])
    assert "denoising-sde" in arch.__file__, arch.__file__

    class Inj(sde_utils.DenoisingSDE):   # the injected-noise subclass of oracle/gen_golden.py: gen_dsde
        noise = None

        def dispersion(self, x, t):
            return self.sigmas[t] * (self.noise[t] * math.sqrt(self.dt)).to(self.device)

    out = {}
    nets = {}
    for name, cfg in DN.CFGS.items():
        nets[name] = build(arch, cfg)
        sd = nets[name].state_dict()
        names = sorted(sd)
        out[name + "/names"] = np.array(names)
        shapes = np.zeros((len(names), 4), dtype=np.int64)
        for i, k in enumerate(names):
            shapes[i, :sd[k].dim()] = list(sd[k].shape)
        out[name + "/shapes"] = shapes

    topt = {}
    for tag, (name, B, H, W, max_sigma, T, sigma) in DN.SAMPLER.items():
        net = nets[name]
        sde = Inj(max_sigma=max_sigma, T=T, device="cpu")
        sde.set_model(net)
        Topt = int(sde.get_optimal_timestep(sigma))
        topt[name] = Topt
        _, noisy = DN.inputs(B, H, W, sigma)
        key = tag + "/sampler"
        out[key + "/T"] = np.int64(Topt)
        out[key + "/noisy"] = noisy
        with torch.no_grad():
            out[key + "/ode"] = sde.reverse_ode(torch.from_numpy(noisy), T=Topt).numpy()
            print(key, "ode", Topt, float(np.abs(out[key + "/ode"]).max()), "%.0f s" % (time.time() - tic), flush=True)
            if T <= 100:
                sde.noise = torch.from_numpy(O.synth_noise(7, T, (B, 3, H, W)))
                out[key + "/sde"] = sde.reverse_sde(torch.from_numpy(noisy), T=Topt).numpy()

    for tag, (name, B, H, W) in DN.FORWARD.items():
        sigma = 25 if name == "w32_e12" else 15
        _, noisy = DN.inputs(B, H, W, sigma)
        ts = [1, 7, topt[name]]
        out[tag + "/ts"] = np.array(ts, dtype=np.int64)
        for t in ts:
            with torch.no_grad():
                out[tag + "/t%d" % t] = nets[name](torch.from_numpy(noisy), t).numpy()
            print(tag, t, float(np.abs(out[tag + "/t%d" % t]).max()), flush=True)

    for k, v in out.items():
        if v.dtype == np.float64:
            out[k] = v.astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "dsde_naf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; wall %.0f s" % (time.time() - tic))


if __name__ == "__main__":
    main()
