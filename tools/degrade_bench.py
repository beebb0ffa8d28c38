"""degrade_bench.py — time per call of the degradation kernels (csrc/degrade.hip) beside a device-to-device hipMemcpyAsync of the output's
bytes, the yardstick of a kernel that mostly writes (imresize, which mostly reads: of its input's bytes).  Device events around `--iters` back-to-back calls on one stream, after a warm-up; the
figures of profiles/degradations.md come from here.

    python tools/degrade_bench.py [--iters 500] [--repeat 5]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("sisr batch 16x3x64x64 -> 256x256", (16, 3, 64, 64), 4), ("stereo view 1x3x94x312 -> 376x1248", (1, 3, 94, 312), 4),
         ("1x3x94x313 x3 (element-per-lane rows)", (1, 3, 94, 313), 3), ("16x3x128x128 x2", (16, 3, 128, 128), 2), ("4x3x64x64 x8", (4, 3, 64, 64), 8)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args(argv)
    import torch
    import image_restoration_sde_amd as P
    from image_restoration_sde_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("degrade_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3   # hipMemcpyDeviceToDevice

    def timed(fn):
        """median over --repeat windows of the microseconds per call of --iters back-to-back calls"""
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return sorted(us)[len(us) // 2], min(us), max(us)

    s = _lib.stream_ptr()
    print("%-42s %10s %22s %22s %8s" % ("case", "out MB", "kernel us (min..max)", "D2D copy us (min..max)", "GB/s"))
    for name, shape, scale in CASES:
        x = torch.rand(shape, device=dev)
        B, C, H, W = shape
        out = torch.empty((B, C, H * scale, W * scale), device=dev)
        out2 = torch.empty_like(out)
        nbytes = out.numel() * 4

        def up():
            _lib.check(L.irsde_upscale_bicubic(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, C, H, W, scale, s))

        def cp():
            assert hip.hipMemcpyAsync(out2.data_ptr(), out.data_ptr(), nbytes, D2D, s) == 0

        k, c = timed(up), timed(cp)
        assert torch.equal(out, P.degradations.upscale(x, scale))
        print("%-42s %10.2f %8.2f (%6.2f..%6.2f) %8.2f (%6.2f..%6.2f) %8.0f" %
              ("upscale " + name, nbytes / 1e6, k[0], k[1], k[2], c[0], c[1], c[2], (nbytes + x.numel() * 4) / k[0] / 1e3))
    # the mask composite at the inpainting config's size (256 x 256 images, 256 x 256 masks)
    x = torch.rand((16, 3, 256, 256), device=dev)
    m = torch.randint(0, 2, (16, 256, 256, 3), device=dev, dtype=torch.uint8) * 255
    out = torch.empty_like(x)
    out2 = torch.empty_like(x)
    nbytes = out.numel() * 4

    def mk():
        _lib.check(L.irsde_mask_to(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(m.data_ptr()), 16, 256, 256, 3, ctypes.c_void_p(out.data_ptr()),
                                   16, 3, 256, 256, s))

    def cp2():
        assert hip.hipMemcpyAsync(out2.data_ptr(), out.data_ptr(), nbytes, D2D, s) == 0

    k, c = timed(mk), timed(cp2)
    print("%-42s %10.2f %8.2f (%6.2f..%6.2f) %8.2f (%6.2f..%6.2f) %8.0f" %
          ("mask_to 16x3x256x256, masks 16x256x256x3", nbytes / 1e6, k[0], k[1], k[2], c[0], c[1], c[2], (2 * nbytes + m.numel()) / k[0] / 1e3))
    # imresize x1/4 of a batch of 1024 x 1024 images (LQ from GT): it reads 16 times what it writes, so its yardstick is a copy of its INPUT
    del x, m, out, out2
    x = torch.rand((16, 3, 1024, 1024), device=dev)
    x2 = torch.empty_like(x)
    P.degradations.imresize(x[:1], 1 / 4)   # builds and uploads the tables
    (wH, sH), (wW, sW) = (P.degradations._device_tables(n, 1 / 4, True, x.device) for n in (1024, 1024))
    out = torch.empty((16, 3, 256, 256), device=dev)
    in_bytes = x.numel() * 4

    def rs():
        _lib.check(L.irsde_imresize(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), 16, 3, 1024, 1024, 256, 256,
                                    ctypes.c_void_p(wH.data_ptr()), ctypes.c_void_p(sH.data_ptr()), wH.shape[1],
                                    ctypes.c_void_p(wW.data_ptr()), ctypes.c_void_p(sW.data_ptr()), wW.shape[1], s))

    def cp3():
        assert hip.hipMemcpyAsync(x2.data_ptr(), x.data_ptr(), in_bytes, D2D, s) == 0

    k, c = timed(rs), timed(cp3)
    assert torch.equal(out, P.degradations.imresize(x, 1 / 4))
    print("%-42s %10.2f %8.2f (%6.2f..%6.2f) %8.2f (%6.2f..%6.2f) %8.0f   (copy of the %.1f MB input; GB/s = input + output bytes)" %
          ("imresize 16x3x1024x1024 x1/4 -> 256x256", out.numel() * 4 / 1e6, k[0], k[1], k[2], c[0], c[1], c[2],
           (in_bytes + out.numel() * 4) / k[0] / 1e3, in_bytes / 1e6))


if __name__ == "__main__":
    main()
