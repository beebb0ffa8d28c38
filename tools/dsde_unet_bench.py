"""Throughput of the denoising-sde ConditionalUNet (GPU box): images / s of a 100-step DenoisingSDE.reverse_ode (max_sigma 50, T 100) on B x 3 x H x W (default
16 x 3 x 256 x 256, nf 64, depth 4: 16 x 16 = 256 bottleneck tokens of 1024 channels per image) in the compute modes fp32, bf16
(bf16 MFMA operands, fp32 storage) and bf16_act (+ bf16 storage of every activation tensor: the full softmax attention of the bottleneck on the bf16 MFMA,
csrc/full_attn16.hip) — graph replay, one warm-up call, the median of `--reps` timed calls — and the event-timed row of the bottleneck attention core from
irsde_op_profile (eager launches of a 3-step profiled call), with the LayerNorm / to_qkv / to_out rows around it.

`--kernel N [N ...]` additionally times the bf16 kernel alone through irsde_debug_full_attention16 on B x N x 384 random tokens (events around `--iters` calls of
the hook, which synchronises: the figure includes that; the op-profile row does not).

IRSDE_LIB_PATH selects the library build, so another build's rates can be taken in the same session.

Usage:  python tools/dsde_unet_bench.py [--shape 16x256x256] [--dtypes fp32 bf16 bf16_act] [--reps 3] [--steps 100]
Prints one JSON line per dtype."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import image_restoration_sde_amd as P  # noqa: E402
from image_restoration_sde_amd import _lib  # noqa: E402
from oracle import irsde_oracle as O  # noqa: E402


def profile_rows(L, m, sde, x, steps=3):
    """irsde_op_profile of an eager, event-timed `steps`-step call: [(ms, description)] of one network evaluation."""
    eng = m.engine(x.device)
    out = torch.empty_like(x)
    B, _, H, W = x.shape
    _lib.check(L.irsde_sample(eng.h, _lib.MODE["dsde_ode"], ctypes.c_void_p(x.data_ptr()), None, None, 0, 0, B, H, W, steps, 0,
                              ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr(), _lib.SAMPLE_PROFILE))
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 20)
    _lib.check(L.irsde_op_profile(eng.h, buf, len(buf)))
    rows = []
    for line in buf.value.decode().splitlines():
        if " ms " in line:
            rows.append((float(line.split()[0]), line.split("ms", 1)[1].strip()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16x256x256")
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16", "bf16_act"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--kernel", nargs="*", type=int, default=[])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B, H, W = (int(v) for v in args.shape.split("x"))
    params = O.uncond_synth_params(seed=0, nf=args.nf, depth=args.depth)
    rs = np.random.RandomState(B)
    clean = torch.from_numpy(rs.uniform(0, 1, (B, 3, H, W)).astype(np.float32)).to(dev)
    noisy = clean + torch.randn(clean.shape, generator=torch.Generator().manual_seed(1)).to(dev) * (25 / 255)
    mid = args.nf << args.depth
    for dtype in args.dtypes:
        m = P.denoising_sde.ConditionalUNet(3, 3, args.nf, depth=args.depth)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.set_compute_dtype(dtype)
        m = m.to(dev).eval()
        sde = P.DenoisingSDE(max_sigma=50, T=100, device=dev)
        sde.set_model(m)
        t0 = time.perf_counter()
        sde.reverse_ode(noisy, T=args.steps)   # plan build + graph capture
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = sde.reverse_ode(noisy, T=args.steps)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        assert torch.isfinite(out).all()
        med = sorted(times)[len(times) // 2]
        rows = profile_rows(L, m, sde, noisy)
        # the bottleneck: LayerNorm, the to_qkv convolution (the first with Cin = nf 2^depth and Cout = 384; the second is ups.0's LinearAttention), the core, to_out
        i_qkv = [i for i, (_, d) in enumerate(rows) if d.startswith("conv") and "Cout=384 " in d and "Cin=%d " % mid in d]
        assert len(i_qkv) == 2 and rows[i_qkv[0] + 2][1].startswith("conv") and "Cin=128 " in rows[i_qkv[0] + 2][1], [d for _, d in rows]
        i = i_qkv[0]
        if dtype == "bf16_act":
            assert rows[i + 1][1].startswith("full_attention (bf16 operands + storage)"), rows[i + 1]
        print(json.dumps({"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "dtype": dtype, "B": B, "H": H, "W": W, "nf": args.nf, "depth": args.depth,
                          "steps": args.steps, "sampler_s_all": [round(t, 4) for t in times], "sampler_s_median": round(med, 4),
                          "images_per_s": round(B / med, 4), "eval_ms": round(1e3 * med / args.steps, 4), "first_call_s": round(first_s, 3),
                          "eval_ms_profiled_eager": round(sum(ms for ms, _ in rows), 4), "bottleneck_tokens": (H >> args.depth) * (W >> args.depth),
                          "attention_core_us": round(1e3 * rows[i + 1][0], 2), "attention_core_row": rows[i + 1][1],
                          "layernorm_us": round(1e3 * rows[i - 1][0], 2), "to_qkv_us": round(1e3 * rows[i][0], 2), "to_out_us": round(1e3 * rows[i + 2][0], 2)}),
              flush=True)
        del m
        sde.set_model(None)
        torch.cuda.empty_cache()
    for N in args.kernel:
        qkv = torch.randn((B, N, 384), device=dev).to(torch.bfloat16)
        o = torch.empty((B, N, 128), device=dev, dtype=torch.bfloat16)
        call = lambda: _lib.check(L.irsde_debug_full_attention16(ctypes.c_void_p(qkv.data_ptr()), B, N, ctypes.c_void_p(o.data_ptr()), _lib.stream_ptr()))
        call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(args.iters):
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        print(json.dumps({"kernel": "full_attention16", "B": B, "N": N, "launch_us_best_of_%d" % args.iters: round(1e3 * best, 2),
                          "flops": 4.0 * B * 4 * N * N * 32}), flush=True)


if __name__ == "__main__":
    main()
