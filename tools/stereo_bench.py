"""Throughput of the stereo-sr sampler (GPU box): pairs / s of the full 100-step reverse SDE of the ssr refusion.yml network
(ConditionalNAFNet width 64, enc [1,1,1,28], middle 1, dec [1,1,1,1], SCAM after every block) on B pairs x 6 x H x W, and the share
of one network evaluation spent in the SCAM ops: from irsde_op_profile (event-timed eager launches, lines named scam_*), and from
the sampler itself against the deraining ConditionalNAFNet (the same network without SCAM) on the 2B views as plain images.

Usage:  python tools/stereo_bench.py [--pairs 1 4] [--size 256 512] [--dtypes fp32 fp16] [--reps 2]
Prints one JSON line per (dtype, pairs) and the per-op profile of the SCAM ops."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_restoration_sde_amd as P  # noqa: E402
from image_restoration_sde_amd import _lib  # noqa: E402
import stereo_oracle as SO  # noqa: E402

CFG = dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--size", type=int, nargs=2, default=[256, 512])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--T", type=int, default=100)
    args = ap.parse_args()
    dev = "cuda:0"
    H, W = args.size
    params = SO.stereo_synth_params(seed=0, img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 28), dec_blk_nums=(1, 1, 1, 1))
    for dtype in args.dtypes:
        m = P.stereo_sr.ConditionalNAFNet(img_channel=3, **CFG)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.set_compute_dtype(dtype)
        m = m.to(dev).eval()
        for B in args.pairs:
            rs = np.random.RandomState(B)
            lq = torch.from_numpy(rs.uniform(0, 1, (B, 6, H, W)).astype(np.float32)).to(dev)
            sde = P.IRSDE(50, args.T, "cosine", 0.005, device=dev)
            sde.set_model(m)
            sde.set_mu(lq)
            xT = sde.noise_state(lq)
            sde.reverse_sde(xT)   # plan, graph capture
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = sde.reverse_sde(xT)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert torch.isfinite(out).all()
            # per-op profile of one evaluation (event-instrumented eager steps)
            sde.profile = True
            sde.reverse_sde(xT, T=3)
            torch.cuda.synchronize()
            sde.profile = False
            buf = ctypes.create_string_buffer(1 << 20)
            _lib.check(_lib.lib().irsde_op_profile(m.engine().h, buf, len(buf)))
            tot = scam = 0.0
            per = {}
            for line in buf.value.decode().splitlines():
                if " ms " not in line:
                    continue
                ms = float(line.split()[0])
                tot += ms
                desc = line.split("ms", 1)[1].strip()
                if desc.startswith("scam_"):
                    scam += ms
                    # level of the op: c of the SCAM (the projection GEMMs name their 2c output channels)
                    c = int(desc.split(" c=")[1].split()[0]) if " c=" in desc else int(desc.split("Cout=")[1].split()[0]) // 2
                    key = "c=%d %s" % (c, desc.split("(")[0])
                    ms_sum, n = per.get(key, (0.0, 0))
                    per[key] = (ms_sum + ms, n + 1)
            best = min(times)
            # the same sampler on the deraining ConditionalNAFNet (no SCAM) over the 2B views as plain images: the SCAM's share of a
            # graph-replayed step is 1 - t_plain / t_stereo
            plain = P.ConditionalNAFNet(3, **CFG)
            plain.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if ".fusion." not in k}, strict=True)
            plain.set_compute_dtype(dtype)
            plain = plain.to(dev).eval()
            sde2 = P.IRSDE(50, args.T, "cosine", 0.005, device=dev)
            sde2.set_model(plain)
            views = torch.cat([lq[:, :3], lq[:, 3:]], 0).contiguous()
            sde2.set_mu(views)
            xv = torch.cat([xT[:, :3], xT[:, 3:]], 0).contiguous()
            sde2.reverse_sde(xv)
            torch.cuda.synchronize()
            tp = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                sde2.reverse_sde(xv)
                torch.cuda.synchronize()
                tp.append(time.perf_counter() - t0)
            del plain, sde2
            print(json.dumps({"dtype": dtype, "pairs": B, "H": H, "W": W, "T": args.T, "sampler_s": round(best, 4),
                              "sampler_s_all": [round(t, 4) for t in times], "pairs_per_s": round(B / best, 4),
                              "plain_nafnet_2B_views_s": round(min(tp), 4), "scam_share_sampler": round(1 - min(tp) / best, 4),
                              "eval_ms_profiled": round(tot, 3), "scam_ms": round(scam, 3), "scam_share": round(scam / max(tot, 1e-9), 4),
                              "scam_ops_ms_count": {k: [round(v[0], 3), v[1]] for k, v in sorted(per.items(), key=lambda kv: int(kv[0].split()[0][2:]))}}),
                  flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
