"""The three-piece GEMM (csrc/gemm_split.hip, gemm_split3i_kernel) alone on the component shapes of profiles/split3_walk.md section 2 (GPU box, PROBES build):
irsde_bench_conv 490 the production launch, 500 the drain twin, 495 one item per block, 491 / 493 / 494 the production launch without the K loop's loads /
its MFMAs / its output stores.  Every variant is timed REPS times, the variants interleaved; prints the median and the spread (max - min) of each, and the
line fit (slope per 512 of K, intercept) of the T = 1024, N = 1024 shapes.  A tree that lacks a variant prints nan for it.
usage: python tools/split3_ring_bench.py [variant ...]      (default: 490 500 495 491 493 494)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from image_restoration_sde_amd import _lib
L = _lib.probes_lib()
VARIANTS = [int(v) for v in sys.argv[1:]] or [490, 500, 495, 491, 493, 494]
REPS = 3
cases = [  # name, B, H = W, Cin, Cout        T = B (H / 4)^2
    ("512->1024 T=1024", 16, 32, 512, 1024), ("1024->1024 T=1024", 16, 32, 1024, 1024), ("1536->1024 T=1024", 16, 32, 1536, 1024),
    ("768->512 T=4096", 16, 64, 768, 512), ("512->512 T=4096", 16, 64, 512, 512), ("512->512 T=1024", 16, 32, 512, 512),
    ("1024->1024 T=256", 4, 32, 1024, 1024), ("1024->1024 T=128", 2, 32, 1024, 1024), ("768->512 T=1024", 4, 64, 768, 512), ("1024->512 T=512", 2, 64, 1024, 512),
]
def run(v, B, H, Cin, Cout):
    ms = ctypes.c_double()
    rc = L.irsde_bench_conv(v, B, H, H, Cin, Cout, 3, 1, 0, 2, 20, ctypes.byref(ms))
    return ms.value if rc == 0 else float("nan")
print("%-18s | " % "layer" + " | ".join("%4d med  spread" % v for v in VARIANTS))
line = {}
for name, B, H, Cin, Cout in cases:
    t = {v: [] for v in VARIANTS}
    for _ in range(REPS):
        for v in VARIANTS:
            t[v].append(run(v, B, H, Cin, Cout))
    med = {v: sorted(t[v])[REPS // 2] for v in VARIANTS}
    print("%-18s | " % name + " | ".join("%8.4f %7.4f" % (med[v], max(t[v]) - min(t[v])) for v in VARIANTS), flush=True)
    if B == 16 and H == 32 and Cout == 1024:
        line[Cin] = med
for v in VARIANTS:   # least squares through K = 512, 1024, 1536
    ks = sorted(line)
    ys = [line[k][v] for k in ks]
    slope = (ys[2] - ys[0]) / 2.0
    print("%d: %.4f ms per 512 of K, intercept %.4f ms" % (v, slope, sum(ys) / 3.0 - 2.0 * slope))
