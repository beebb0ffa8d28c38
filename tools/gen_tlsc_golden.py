"""Generate tests/golden/tlsc.npz from the REAL reference CNAFNetLocal (test infrastructure only; needs the reference tree).

The reference `CNAFNetLocal` of codes/config/latent-dehazing/models/modules/DenoisingNAFNet_arch.py:190-200 (with local_arch.py: TLSC, every
NAFBlock's global average pool replaced by a windowed mean) and `IRSDE` of codes/utils/sde_utils.py run on the CPU with the seeded synthetic
weights of tests/tlsc_oracle.py (oracle.irsde_oracle.naf_synth_params, sca.1.weight scaled by SCA_GAIN), and what they compute is stored:

    <net>/names                   the reference state_dict names of CNAFNetLocal (net = w16_t16, w16_t20x12, w32_t16, w32_t20x12: width 16 / 32,
                                  enc [1,1], middle 1, dec [1,1], train_size (1,3,16,16) / (1,3,20,12))
    <net>/names_plain             ... of the latent ConditionalNAFNet with the same arguments
    <net>/kernel_sizes            [5][2]: the kernel_size the conversion forward froze in encoders.0.0, encoders.1.0, middle_blks.0, decoders.0.0,
                                  decoders.1.0 (module order)
    <tag>/ts, <tag>/t<t>          forward(xt, cond, t) for the tags of tlsc_oracle.FORWARD (1x40x56, 1x37x50, 1x20x56, 1x16x16, 1x96x128; the last
                                  stored as every second pixel, key <tag>/t<t>_sub2)
    sampler/sde, sampler/ode      IRSDE(max_sigma 50, T 20, cosine, eps 0.005) reverse_sde (injected noise, seed 7) and reverse_ode on tlsc_oracle.SAMPLER
Inputs: tests/tlsc_oracle.py `inputs` (blocks + ramp + noise).  Arrays only.

Usage:  python tools/gen_tlsc_golden.py --ref <reference root>
Read by tests/test_tlsc_host.py and tests/test_gpu_tlsc.py, which rebuild weights, inputs and noise from the seeded generators.
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
from oracle.gen_golden import InjectedIRSDE, load_reference, load_task_modules  # noqa: E402
import tlsc_oracle as TL  # noqa: E402


def build(arch, name):
    width, train_size = TL.NETS[name]
    kw = dict(img_channel=3, width=width, enc_blk_nums=list(TL.ARCH["enc_blk_nums"]), middle_blk_num=TL.ARCH["middle_blk_num"],
              dec_blk_nums=list(TL.ARCH["dec_blk_nums"]))
    params = TL.synth_params(name)
    net = arch.CNAFNetLocal(train_size=train_size, fast_imp=False, **kw).eval()
    sd = net.state_dict()
    assert set(sd) == set(params), set(sd) ^ set(params)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    plain = arch.ConditionalNAFNet(**kw)
    blocks = [net.encoders[0][0], net.encoders[1][0], net.middle_blks[0], net.decoders[0][0], net.decoders[1][0]]
    ks = np.array([list(b.sca[0].kernel_size) for b in blocks], dtype=np.int64)
    return net, np.array(sorted(sd)), np.array(sorted(plain.state_dict())), ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    sde_utils, _ = load_reference(args.ref)
    (arch,) = load_task_modules(os.path.join(args.ref, "codes/config/latent-dehazing"), ["DenoisingNAFNet_arch"])
    assert "latent-dehazing" in arch.__file__, arch.__file__
    out, nets = {}, {}
    for name in TL.NETS:
        nets[name], out[name + "/names"], out[name + "/names_plain"], out[name + "/kernel_sizes"] = build(arch, name)
        print(name, out[name + "/kernel_sizes"].tolist())
    for tag, (name, B, H, W, ts, stride) in TL.FORWARD.items():
        cond, xt = TL.inputs(B, H, W)
        out[tag + "/ts"] = np.array(ts, dtype=np.int64)
        for t in ts:
            with torch.no_grad():
                y = nets[name](torch.from_numpy(xt), torch.from_numpy(cond), int(t)).numpy()
            out[tag + ("/t%d" % t if stride == 1 else "/t%d_sub%d" % (t, stride))] = np.ascontiguousarray(y[..., ::stride, ::stride])
            print(tag, t, float(np.abs(y).max()), flush=True)
    name, B, H, W, T = TL.SAMPLER
    cond, xt = TL.inputs(B, H, W)
    sde = InjectedIRSDE.make(sde_utils)(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(O.synth_noise(7, T, (B, 3, H, W)))
    sde.set_model(nets[name])
    sde.set_mu(torch.from_numpy(cond))
    for mode in ("sde", "ode"):
        with torch.no_grad():
            out["sampler/" + mode] = (sde.reverse_sde if mode == "sde" else sde.reverse_ode)(torch.from_numpy(xt)).numpy()
    for k, v in out.items():
        if v.dtype == np.float64:
            out[k] = v.astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "tlsc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
