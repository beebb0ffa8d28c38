"""lpips_bench.py — what LPIPS costs in the evaluation loop: irsde_lpips for 16 pairs of 256 x 256 (55.7 GFLOP executed) beside, in the same
process, ONE evaluation of the fp32 ConditionalUNet (nf 64, depth 4) on the same batch, of which the sampler runs 100 per batch.  Device events
around every call after a warm-up, the median of --repeat calls; the per-kernel split of the last LPIPS call comes from the events irsde_lpips
records around its launches (`LPIPS.last_profile`).  The figures of profiles/lpips.md come from here.

    python tools/lpips_bench.py [--batch 16] [--size 256] [--repeat 20]

The condition: LPIPS for the batch costs no more than one network evaluation of that batch (then it adds at most 1 % to a 100-step run)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import image_restoration_sde_amd as P
    import lpips_oracle as LO   # synthetic weights: the time does not depend on the values
    if not torch.cuda.is_available():
        sys.exit("lpips_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    y = torch.rand(B, 3, S, S, generator=g).to(dev)

    def timed(fn):
        """(median, min, max) device milliseconds and the median wall milliseconds of one call"""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms), float(np.median(wall))

    lp = P.LPIPS(net="alex").load_state_dict(LO.lpips_layout(LO.synth_weights(0)))
    t_lp = timed(lambda: lp.terms(x, y, normalize=True))
    split = lp.last_profile()
    shapes = LO.feature_shapes(S, S)
    macs = 0
    for (co, ci, k, _, _), (_, h, w) in zip(LO.LAYERS, shapes):
        macs += 2 * B * h * w * co * (4 if ci == 3 else ci) * k * k   # executed: conv1 runs on 4 input channels
    net = P.ConditionalUNet(3, 3, 64, depth=4).to(dev).eval()
    with torch.no_grad():
        t_net = timed(lambda: net(x, y, 50))

    print("LPIPS, %d pairs of %d x %d (%.1f GFLOP executed):  %.3f ms  (min %.3f, max %.3f; wall %.3f ms per call)  %.1f TFLOP/s" %
          (B, S, S, 2 * macs / 1e9, t_lp[0], t_lp[1], t_lp[2], t_lp[3], 2 * macs / t_lp[0] / 1e9))
    print("one ConditionalUNet(nf 64, depth 4) fp32 evaluation of the same batch:  %.3f ms  (min %.3f, max %.3f; wall %.3f ms)" % t_net)
    print("ratio LPIPS / network evaluation: %.3f  -> condition (<= 1): %s" % (t_lp[0] / t_net[0], "met" if t_lp[0] <= t_net[0] else "NOT met"))
    print("per-kernel split of the last LPIPS call (events around every launch group):")
    total = sum(ms for ms, _ in split)
    for ms, desc in split:
        print("  %9.4f ms  %5.1f %%  %s" % (ms, 100.0 * ms / total, desc))
    print("  %9.4f ms  sum" % total)
    return t_lp[0] <= t_net[0]


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
