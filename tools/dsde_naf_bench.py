"""Throughput of the denoising-sde Refusion config (GPU box): denoising-sde/options/test/refusion.yml -- ConditionalNAFNet width 64,
enc [1,1,1,28], middle 1, dec [1,1,1,1], DenoisingSDE(max_sigma 70, T 1000), sigma 15 -> reverse_ode from T_opt = 158 -- on B x 3 x H x W:
images / s and ms per network evaluation (graph replay, one warm-up call, `--reps` timed calls, all of them printed), the size and build
time of the FiLM table of the T = 1000 schedule, and the plan-build time per shape.

`--network cond` runs the same number of reverse_ode steps of the conditional (deraining) refusion network with IRSDE(70, 1000) on the
same shapes: the yardstick (the unconditional network does the same work minus half of the intro's K).  IRSDE_LIB_PATH selects the
library build, so the yardstick can be another build's in the same session.

Usage:  python tools/dsde_naf_bench.py [--network uncond|cond] [--shapes 1x512x512 8x512x512 1x481x321] [--dtypes fp32 fp16 fp16_act] [--reps 3]
Prints one JSON line per (dtype, shape)."""
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
from oracle import irsde_oracle as O  # noqa: E402

CFG = dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default="uncond", choices=["uncond", "cond"])
    ap.add_argument("--shapes", nargs="+", default=["1x512x512", "8x512x512", "1x481x321"])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    params = O.naf_synth_params(seed=0, img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 28), dec_blk_nums=(1, 1, 1, 1))
    if args.network == "uncond":
        import dsde_naf_oracle as DN
        params = DN.synth_params(seed=0, **DN.CFGS["refusion"])
    dsde = P.DenoisingSDE(max_sigma=70, T=1000, device=dev)
    Topt = int(dsde.get_optimal_timestep(args.sigma))
    for dtype in args.dtypes:
        m = (P.denoising_sde.ConditionalNAFNet if args.network == "uncond" else P.ConditionalNAFNet)(img_channel=3, **CFG)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.set_compute_dtype(dtype)
        m = m.to(dev).eval()
        sde = dsde if args.network == "uncond" else P.IRSDE(70, 1000, "cosine", 0.005, device=dev)
        sde.set_model(m)
        eng = m.engine(dev)
        film_row = sum(4 * b.conv3.weight.shape[0] for b in m.modules() if hasattr(b, "conv3"))
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(dev)[0]
        t0 = time.perf_counter()
        _lib.check(L.irsde_set_schedule(eng.h, sde.T, ctypes.c_void_p(sde._coef.data_ptr())))
        torch.cuda.synchronize()
        sched_s = time.perf_counter() - t0
        film_mb_measured = (free0 - torch.cuda.mem_get_info(dev)[0]) / 2 ** 20
        eng.schedule_key = ("dsde", sde.T, sde.schedule, sde.max_sigma) if args.network == "uncond" else None
        for shape in args.shapes:
            B, H, W = (int(v) for v in shape.split("x"))
            rs = np.random.RandomState(B)
            clean = torch.from_numpy(rs.uniform(0, 1, (B, 3, H, W)).astype(np.float32)).to(dev)
            noisy = clean + torch.randn(clean.shape, generator=torch.Generator().manual_seed(1)).to(dev) * (args.sigma / 255)
            buf = ctypes.create_string_buffer(1 << 18)
            t0 = time.perf_counter()
            _lib.check(L.irsde_plan_describe(eng.h, B, H, W, buf, len(buf)))
            torch.cuda.synchronize()
            plan_s = time.perf_counter() - t0
            if args.network == "cond":
                sde.set_mu(clean)
            t0 = time.perf_counter()
            sde.reverse_ode(noisy, T=Topt)   # (cond: sets the schedule once more through the Python path), graph capture
            torch.cuda.synchronize()
            first_s = time.perf_counter() - t0
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = sde.reverse_ode(noisy, T=Topt)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert torch.isfinite(out).all()
            best, med = min(times), sorted(times)[len(times) // 2]
            print(json.dumps({"network": args.network, "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "dtype": dtype, "B": B, "H": H, "W": W,
                              "steps": Topt, "sampler_s_all": [round(t, 4) for t in times], "sampler_s_median": round(med, 4),
                              "images_per_s": round(B / med, 4), "eval_ms": round(1e3 * med / Topt, 4), "eval_ms_best": round(1e3 * best / Topt, 4),
                              "spread_pct": round(100 * (max(times) - best) / best, 2), "plan_build_s": round(plan_s, 3),
                              "first_call_s": round(first_s, 3), "set_schedule_s": round(sched_s, 3), "film_row_floats": film_row,
                              "film_table_MiB": round((sde.T + 1) * film_row * 4 / 2 ** 20, 1), "set_schedule_device_MiB": round(film_mb_measured, 1)}),
                  flush=True)
        del m, eng
        sde.set_model(None)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
