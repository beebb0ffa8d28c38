"""Cost of one evaluation of the stereo-sr ConditionalUNet (GPU box): ms per network evaluation (nf 64, depth 4, fp32) on B pairs x 6 x H x W
from graph-replayed reverse-SDE steps (warm-up, then the median of --reps timed calls of a --T step sampler), the per-kernel share of the
scam_full_* rows from irsde_op_profile (event-timed eager launches), and for comparison the deraining ConditionalUNet (the same network
without SCAM, 7x7 init_conv) on the 2B views as plain images: the difference is the price of the SCAM.

Usage:  python tools/stereo_unet_bench.py [--cases 2x128x128 1x256x256] [--hw H W] [--wide] [--force-stream BW [--runs 3]] [--reps 20] [--T 5]
    --hw H W           one more case: 1 pair x 6 x H x W
    --wide             set_wide_rows() (IRSDE_FLAG_SCAM_STREAM): rows beyond 1024 run the streaming SCAM core (csrc/scam_stream.hip)
    --force-stream BW  A/B of the two SCAM cores in one process: a second engine whose plans run EVERY SCAM core on the streaming kernel at block width BW
                       (irsde_debug_force_scam_stream) against the engine of the rule, --runs alternating measurements of each (rule, forced, rule, ...);
                       prints the median over the runs of ms per evaluation and of every *_core row, both variants side by side
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


def profiled(sde, m, xT):
    """(eager total, SCAM rows total, per launch group, core rows per level) in ms from a 3-step profiled sampler call."""
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
                key = desc.split(" B=")[1].split(" ", 1)[1]
                levels[key] = levels.get(key, 0.0) + ms
    return tot, scam, per, levels


def stereo_net(dev, wide):
    m = P.stereo_sr.ConditionalUNet(3, 3, 64, depth=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in SU.stereo_unet_synth_params(seed=0, nf=64, depth=4).items()}, strict=True)
    if wide:
        m.set_wide_rows()
    return m.to(dev).eval()


def ab_cores(args, dev, case, lq):
    """The rule's engine against one with every SCAM core on the streaming kernel, alternating in one process."""
    nets = {"rule": stereo_net(dev, args.wide), "stream": stereo_net(dev, args.wide)}
    sdes, xT = {}, None
    for name, m in nets.items():
        sde = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
        sde.set_model(m)
        sde.set_mu(lq)
        xT = sde.noise_state(lq) if xT is None else xT
        sdes[name] = sde
    if _lib.lib().irsde_debug_force_scam_stream(args.force_stream) != 0:
        raise SystemExit("--force-stream: the block width must be a multiple of 16 in [16, 512]")
    try:   # plans keep the choice made when they are built: build the forced engine's (sampler and profiled) here
        timed(sdes["stream"], xT, 1, args.T)
        profiled(sdes["stream"], nets["stream"], xT)
    finally:
        _lib.lib().irsde_debug_force_scam_stream(0)
    runs = {"rule": [], "stream": []}
    for _ in range(args.runs):
        for name in ("rule", "stream"):
            med, _, _ = timed(sdes[name], xT, args.reps, args.T)
            runs[name].append((med,) + profiled(sdes[name], nets[name], xT))
    out = {"case": case, "reps": args.reps, "T": args.T, "runs": args.runs, "force_stream_bw": args.force_stream, "wide": args.wide}
    for name, rs in runs.items():
        out[name] = {"eval_ms_median_of_runs": round(statistics.median(r[0] for r in rs), 3), "eval_ms_runs": [round(r[0], 3) for r in rs],
                     "scam_core_ms_total": round(statistics.median(sum(r[4].values()) for r in rs), 3),
                     "scam_core_ms_by_level": {k: round(statistics.median(r[4][k] for r in rs), 3) for k in rs[0][4]}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2x128x128", "1x256x256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--T", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, metavar=("H", "W"), help="one more case: 1 pair x 6 x H x W")
    ap.add_argument("--wide", action="store_true", help="set_wide_rows(): rows beyond 1024 on the streaming SCAM core")
    ap.add_argument("--force-stream", type=int, default=0, metavar="BW", help="A/B: every SCAM core on the streaming kernel at this block width against the rule")
    ap.add_argument("--runs", type=int, default=3, help="alternating measurements per variant of --force-stream")
    args = ap.parse_args()
    if args.hw:
        args.cases = (args.cases if "--cases" in sys.argv else []) + ["1x%dx%d" % tuple(args.hw)]
    dev = "cuda:0"
    m = stereo_net(dev, args.wide)
    plain = P.ConditionalUNet(3, 3, 64, depth=4)
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0, nf=64, depth=4).items()}, strict=True)
    plain = plain.to(dev).eval()
    for case in args.cases:
        B, H, W = (int(v) for v in case.split("x"))
        rs = np.random.RandomState(B)
        lq = torch.from_numpy(rs.uniform(0, 1, (B, 6, H, W)).astype(np.float32)).to(dev)
        if args.force_stream:
            ab_cores(args, dev, case, lq)
            continue
        sde = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
        sde.set_model(m)
        sde.set_mu(lq)
        xT = sde.noise_state(lq)
        med, lo, hi = timed(sde, xT, args.reps, args.T)
        tot, scam, per, levels = profiled(sde, m, xT)
        sde2 = P.IRSDE(50, 100, "cosine", 0.005, device=dev)
        sde2.set_model(plain)
        views = torch.cat([lq[:, :3], lq[:, 3:]], 0).contiguous()
        sde2.set_mu(views)
        pmed, plo, phi = timed(sde2, torch.cat([xT[:, :3], xT[:, 3:]], 0).contiguous(), args.reps, args.T)
        print(json.dumps({"case": case, "wide": args.wide, "reps": args.reps, "T": args.T, "eval_ms_median": round(med, 3), "eval_ms_min_max": [round(lo, 3), round(hi, 3)],
                          "plain_unet_2B_views_eval_ms_median": round(pmed, 3), "plain_min_max": [round(plo, 3), round(phi, 3)],
                          "scam_price_ms": round(med - pmed, 3), "eval_ms_profiled_eager": round(tot, 3), "scam_ms_profiled": round(scam, 3),
                          "scam_kernels_ms": {k: round(v, 3) for k, v in sorted(per.items())},
                          "scam_core_ms_by_level": {k: round(v, 3) for k, v in levels.items()}}), flush=True)


if __name__ == "__main__":
    main()
