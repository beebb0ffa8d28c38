"""Cost of one evaluation of the stereo-sr ConditionalUNet (GPU box): ms per network evaluation (nf 64, depth 4, fp32) on B pairs x 6 x H x W
from graph-replayed reverse-SDE steps (warm-up, then the median of --reps timed calls of a --T step sampler), the per-kernel share of the
scam_full_* rows from irsde_op_profile (event-timed eager launches), and for comparison the deraining ConditionalUNet (the same network
without SCAM, 7x7 init_conv) on the 2B views as plain images: the difference is the price of the SCAM.

Usage:  python tools/stereo_unet_bench.py [--cases 2x128x128 1x256x256] [--reps 20] [--T 5]
Prints one JSON line per case."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_restoration_sde_amd as P  # noqa: E402
from image_restoration_sde_amd import _lib  # noqa: E402
from oracle import irsde_oracle as O  # noqa: E402
import stereo_unet_oracle as SU  # noqa: E402


def timed(sde, xT, reps, T):
    sde.reverse_sde(xT, T=T)   # plan, graph capture
    sde.reverse_sde(xT, T=T)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sde.reverse_sde(xT, T=T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / T)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2x128x128", "1x256x256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--T", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    m = P.stereo_sr.ConditionalUNet(3, 3, 64, depth=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in SU.stereo_unet_synth_params(seed=0, nf=64, depth=4).items()}, strict=True)
    m = m.to(dev).eval()
    plain = P.ConditionalUNet(3, 3, 64, depth=4)
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0, nf=64, depth=4).items()}, strict=True)
    plain = plain.to(dev).eval()
    for case in args.cases:
        B, H, W = (int(v) for v in case.split("x"))
        rs = np.random.RandomState(B)
        lq = torch.from_numpy(rs.uniform(0, 1, (B, 6, H, W)).astype(np.float32)).to(dev)
        sde = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
        sde.set_model(m)
        sde.set_mu(lq)
        xT = sde.noise_state(lq)
        med, lo, hi = timed(sde, xT, args.reps, args.T)
        sde.profile = True
        sde.reverse_sde(xT, T=3)
        torch.cuda.synchronize()
        sde.profile = False
        buf = ctypes.create_string_buffer(1 << 20)
        _lib.check(_lib.lib().irsde_op_profile(m.engine().h, buf, len(buf)))
        tot = scam = 0.0
        per, levels = {}, {}
        for line in buf.value.decode().splitlines():
            if " ms " not in line:
                continue
            ms = float(line.split()[0])
            tot += ms
            desc = line.split("ms", 1)[1].strip()
            if desc.startswith("scam_full_"):
                scam += ms
                kind = desc.split("(")[0] if "proj" not in desc else "scam_full_proj"
                per[kind] = per.get(kind, 0.0) + ms
                if "core" in desc:
                    levels[desc.split(" B=")[1].split(" ", 1)[1]] = levels.get(desc.split(" B=")[1].split(" ", 1)[1], 0.0) + ms
        sde2 = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
        sde2.set_model(plain)
        views = torch.cat([lq[:, :3], lq[:, 3:]], 0).contiguous()
        sde2.set_mu(views)
        pmed, plo, phi = timed(sde2, torch.cat([xT[:, :3], xT[:, 3:]], 0).contiguous(), args.reps, args.T)
        print(json.dumps({"case": case, "reps": args.reps, "T": args.T, "eval_ms_median": round(med, 3), "eval_ms_min_max": [round(lo, 3), round(hi, 3)],
                          "plain_unet_2B_views_eval_ms_median": round(pmed, 3), "plain_min_max": [round(plo, 3), round(phi, 3)],
                          "scam_price_ms": round(med - pmed, 3), "eval_ms_profiled_eager": round(tot, 3), "scam_ms_profiled": round(scam, 3),
                          "scam_kernels_ms": {k: round(v, 3) for k, v in sorted(per.items())},
                          "scam_core_ms_by_level": {k: round(v, 3) for k, v in levels.items()}}), flush=True)


if __name__ == "__main__":
    main()
