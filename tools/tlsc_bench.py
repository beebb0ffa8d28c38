"""Cost of TLSC local pooling (GPU box): one network evaluation of the nasde.yml score network (latent-dehazing: img_channel 8, width 64,
enc [1,1,1,28], middle 1, dec [1,1,1,1]) as CNAFNetLocal with train latent 32 x 32 on a 1 x 8 x 96 x 128 latent, against the same weights and
shape through the plain latent ConditionalNAFNet (global pools) of the same build.

Measured: ms per evaluation of both networks = wall time of a T-step reverse_ode (graph replay, ends in a device synchronise) / T, `--reps`
calls each, alternating, after one warm-up call per network; their difference; per-launch-group ms of the "tlsc" rows from one
event-instrumented sampler call (IRSDE_SAMPLE_PROFILE: a hipEvent pair around every launch group).
Derived: the added launches' algorithmic bytes per block -- the gated tensor read once (4 B h w c), the compact map of window means written and
read (2 x 4 B nh nw c), the compact scale map written and read (2 x 4 B nh nw c), the gated tensor rescaled (read + write: 8 B h w c); the row
sums between the two pool passes (written and read: 8 B h nw c) are this implementation's own traffic and are listed separately -- and the
bandwidth = those bytes / the measured ms of the rows.

Usage:  python tools/tlsc_bench.py [--shape 1x96x128] [--train 32] [--dtypes fp32 fp16] [--T 50] [--reps 5] [--md profiles/tlsc_table.md]
Prints one JSON line per dtype and, with --md, appends the table rows in markdown."""
import argparse
import ctypes
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_restoration_sde_amd as P  # noqa: E402
from image_restoration_sde_amd import _lib, latent  # noqa: E402
from oracle import irsde_oracle as O  # noqa: E402

CFG = dict(img_channel=8, width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x96x128")
    ap.add_argument("--train", type=int, default=32)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = (int(v) for v in args.shape.split("x"))
    params = O.naf_synth_params(seed=0, img_channel=8, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 28), dec_blk_nums=(1, 1, 1, 1))
    rs = np.random.RandomState(0)
    mu = torch.from_numpy(rs.uniform(0, 1, (B, 8, H, W)).astype(np.float32)).to(dev)
    xT = mu + torch.from_numpy(rs.standard_normal((B, 8, H, W)).astype(np.float32)).to(dev) * (50 / 255)
    rows_md = []
    for dtype in args.dtypes:
        nets, sdes = {}, {}
        for tag in ("local", "global"):
            m = latent.CNAFNetLocal(train_size=(1, 8, args.train, args.train), **CFG) if tag == "local" else latent.ConditionalNAFNet(**CFG)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
            m.set_compute_dtype(dtype)
            nets[tag] = m.to(dev).eval()
            sde = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
            sde.set_model(nets[tag])
            sde.set_mu(mu)
            sdes[tag] = sde
            sde.reverse_ode(xT, T=args.T)   # warm-up: plan build, graph capture
            torch.cuda.synchronize()
        times = {"local": [], "global": []}
        for _ in range(args.reps):
            for tag in ("local", "global"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = sdes[tag].reverse_ode(xT, T=args.T)
                torch.cuda.synchronize()
                times[tag].append(1e3 * (time.perf_counter() - t0) / args.T)
                assert torch.isfinite(out).all()
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        # per launch group: one event-instrumented call on the local network
        sde = sdes["local"]
        sde.profile = True
        sde.reverse_ode(xT, T=5)
        torch.cuda.synchronize()
        sde.profile = False
        buf = ctypes.create_string_buffer(1 << 20)
        _lib.check(_lib.lib().irsde_op_profile(nets["local"].engine().h, buf, len(buf)))
        groups = {}
        for line in buf.value.decode().splitlines():
            mm = re.match(r"\s*([\d.]+) ms\s+tlsc (\d+)x(\d+) (pool|sca\.1|scale) (.*)", line)
            if not mm:
                continue
            ms, k1, k2, part, rest = float(mm.group(1)), int(mm.group(2)), int(mm.group(3)), mm.group(4), mm.group(5)
            g = groups.setdefault((k1, k2), {"pool": 0.0, "sca.1": 0.0, "scale": 0.0, "blocks": 0})
            g[part] += ms
            if part == "pool":
                c, h, w, nh, nw = (int(v) for v in re.search(r"c=(\d+) hw=(\d+)x(\d+) -> (\d+)x(\d+)", rest).groups())
                g.update(c=c, h=h, w=w, nh=nh, nw=nw)
                g["blocks"] += 1
        tot_ms = tot_bytes = tot_extra = 0.0
        per_window = []
        for (k1, k2), g in sorted(groups.items(), reverse=True):
            n, c, h, w, nh, nw = g["blocks"], g["c"], g["h"], g["w"], g["nh"], g["nw"]
            algo = n * 4.0 * B * c * (h * w + 2 * nh * nw + 2 * nh * nw + 2 * h * w)
            extra = n * 8.0 * B * c * h * nw
            ms = g["pool"] + g["sca.1"] + g["scale"]
            tot_ms, tot_bytes, tot_extra = tot_ms + ms, tot_bytes + algo, tot_extra + extra
            per_window.append({"window": "%dx%d" % (k1, k2), "blocks": n, "map": "%dx%dx%d" % (h, w, c), "compact": "%dx%d" % (nh, nw),
                               "pool_ms": round(g["pool"], 4), "sca1_ms": round(g["sca.1"], 4), "scale_ms": round(g["scale"], 4),
                               "algorithmic_MB": round(algo / 1e6, 3), "rowsum_MB": round(extra / 1e6, 3), "GBps": round(algo / ms / 1e6, 1)})
        res = {"dtype": dtype, "B": B, "H": H, "W": W, "train": args.train, "T": args.T,
               "eval_ms_local_all": [round(t, 4) for t in times["local"]], "eval_ms_global_all": [round(t, 4) for t in times["global"]],
               "eval_ms_local": round(med["local"], 4), "eval_ms_global": round(med["global"], 4), "eval_ms_added": round(med["local"] - med["global"], 4),
               "tlsc_rows_ms": round(tot_ms, 4), "tlsc_algorithmic_MB": round(tot_bytes / 1e6, 3), "tlsc_rowsum_MB": round(tot_extra / 1e6, 3),
               "tlsc_GBps": round(tot_bytes / max(tot_ms, 1e-9) / 1e6, 1), "per_window": per_window}
        print(json.dumps(res), flush=True)
        for r in per_window:
            rows_md.append("| %s | %s | %d | %s | %s | %.4f | %.4f | %.4f | %.3f | %.3f | %.1f |" % (
                dtype, r["window"], r["blocks"], r["map"], r["compact"], r["pool_ms"], r["sca1_ms"], r["scale_ms"], r["algorithmic_MB"], r["rowsum_MB"], r["GBps"]))
        rows_md.append("| %s | all | | | | | | %.4f (sum) | %.3f | %.3f | %.1f |" % (dtype, tot_ms, tot_bytes / 1e6, tot_extra / 1e6, res["tlsc_GBps"]))
        rows_md.append("| %s | evaluation | local %.4f ms | global %.4f ms | added %.4f ms | | | | | | |" % (dtype, med["local"], med["global"], med["local"] - med["global"]))
        del nets, sdes
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| dtype | window | blocks | map h x w x c | compact map | pool ms | sca.1 ms | scale ms | algorithmic MB | row sums MB | GB/s |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            f.write("\n".join(rows_md) + "\n")


if __name__ == "__main__":
    main()
