"""Evaluation tail on the device — the metric block of the reference's test scripts
(/root/reference/codes/config/deraining/test.py:110-178) without cv2 and without leaving the GPU:
`util.tensor2img`, `util.calculate_psnr`, `util.calculate_ssim` (codes/utils/img_utils.py:136-234) and the Y-channel
variants through `bgr2ycbcr` (codes/data/util.py:177-198).  All arithmetic runs in libirsde_hip.so
(csrc/eval_metrics.hip); there is no CPU fallback.  `LPIPS` is the loops' third metric, `lpips.LPIPS(net='alex')`
(test.py:74, 149-154), on csrc/lpips.hip with the user's weight files.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _f32_cuda(t):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.IrsdeError("metrics run on CUDA(HIP) tensors only (no CPU fallback)")
    t = t.detach().to(torch.float32)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise _lib.IrsdeError("expected (B,C,H,W) or (C,H,W)")
    return t.contiguous()


def tensor2img(tensor, out_type=np.uint8, min_max=(0, 1)):
    """util.tensor2img for a (C,H,W) / (1,C,H,W) device tensor: numpy HWC uint8, BGR channel order."""
    if out_type != np.uint8 or tuple(min_max) != (0, 1):
        raise _lib.IrsdeError("only the uint8 / (0,1) form used by the test scripts is implemented")
    t = _f32_cuda(tensor)
    B, C, H, W = t.shape
    if B != 1:
        raise _lib.IrsdeError("tensor2img takes one image (use tensor2img_batch)")
    return tensor2img_batch(t)[0]


def tensor2img_batch(tensor):
    """(B,C,H,W) device tensor -> numpy (B,H,W,C) uint8 BGR (C == 1: (B,H,W))."""
    t = _f32_cuda(tensor)
    B, C, H, W = t.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().irsde_tensor2img(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, C, H, W,
                                               _lib.stream_ptr()))
    a = out.cpu().numpy()
    return a[..., 0] if C == 1 else a


def evaluate_batch(output, gt, crop_border=0, lpips=None):
    """Per-image metrics of a batch: dict of float64 arrays psnr, ssim, psnr_y, ssim_y (deraining/test.py:137-178;
    crop_border as `opt["crop_border"]`).  With an `LPIPS` object also "lpips": the distance of the full, unquantised
    `output` / `gt` in [0, 1] (normalize=True), as test.py:149-154 computes it (no crop border there)."""
    o, g = _f32_cuda(output), _f32_cuda(gt)
    if o.shape != g.shape or o.device != g.device:
        raise _lib.IrsdeError("output / GT shape or device mismatch")
    B, C, H, W = o.shape
    m = (ctypes.c_double * (4 * B))()
    with torch.cuda.device(o.device):
        _lib.check(_lib.lib().irsde_eval_metrics(ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(g.data_ptr()), B, C, H, W,
                                                 int(crop_border), m, _lib.stream_ptr()))
    a = np.array(m, dtype=np.float64).reshape(B, 4)
    res = {"psnr": a[:, 0], "ssim": a[:, 1], "psnr_y": a[:, 2], "ssim_y": a[:, 3]}
    if lpips is not None:
        res["lpips"] = lpips.terms(o, g, normalize=True).sum(axis=1)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# LPIPS v0.1, net='alex' — the third number of the reference's test loops (deraining/test.py:12, 74, 149-154), which take it
# from the pip package `lpips`.  Here: an AlexNet feature tower and the distance as HIP kernels (csrc/lpips.hip) behind
# irsde_create_lpips / irsde_lpips; the published weights come from the user as files.
# ----------------------------------------------------------------------------------------------------------------------
LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)


def _lpips_name_table():
    """THE name table: engine tensor -> the checkpoint keys it is read from (first match wins; `module.` prefixes are stripped
    before the lookup).  Per tensor, in this order: the key of `lpips.LPIPS(net='alex').state_dict()`; the key of the two
    published files (torchvision's AlexNet `features.N.*`, and lpips' `alex.pth`, whose lin keys are the state_dict's).
    These keys are written from memory of lpips 0.1.4 and torchvision — neither package is
    installed where this was written, so nobody could check them against the real files: a wrong one is a one-line fix here."""
    table = {}
    for n, idx in ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10)):   # slice / conv number, index inside torchvision's `features`
        for p in ("weight", "bias"):
            table["conv%d.%s" % (n, p)] = ("net.slice%d.%d.%s" % (n, idx, p), "features.%d.%s" % (idx, p))
        table["lin%d.weight" % n] = ("lin%d.model.1.weight" % (n - 1),)
    return table


LPIPS_SHAPES = {"conv1.weight": (64, 3, 11, 11), "conv2.weight": (192, 64, 5, 5), "conv3.weight": (384, 192, 3, 3),
                "conv4.weight": (256, 384, 3, 3), "conv5.weight": (256, 256, 3, 3), "conv1.bias": (64,), "conv2.bias": (192,),
                "conv3.bias": (384,), "conv4.bias": (256,), "conv5.bias": (256,), "lin1.weight": (1, 64, 1, 1),
                "lin2.weight": (1, 192, 1, 1), "lin3.weight": (1, 384, 1, 1), "lin4.weight": (1, 256, 1, 1), "lin5.weight": (1, 256, 1, 1)}


def lpips_map_state_dict(sd):
    """Checkpoint dict (either layout of `_lpips_name_table`, or both files merged) -> the engine's 15 float32 CPU tensors.
    Ignored: `lins.*` (lpips registers the lin layers twice), `classifier.*`, any other key the table does not name.
    `scaling_layer.shift` / `.scale`, when present, must hold the constants the kernels use.  A missing tensor raises."""
    flat = {}
    for k, v in sd.items():
        while k.startswith("module."):
            k = k[len("module."):]
        flat[k] = v
    for key, want in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
        if key in flat:
            got = torch.as_tensor(flat[key]).detach().to("cpu", torch.float64).flatten()
            if got.numel() != 3 or not torch.allclose(got, torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-6):
                raise _lib.IrsdeError("LPIPS: %s is %s, the kernels are built for %s" % (key, got.tolist(), list(want)))
    out, missing = {}, []
    for name, keys in _lpips_name_table().items():
        src = next((k for k in keys if k in flat), None)
        if src is None:
            missing.append("%s (looked for %s)" % (name, " / ".join(keys)))
            continue
        t = torch.as_tensor(flat[src]).detach().to("cpu", torch.float32).contiguous()
        if tuple(t.shape) != LPIPS_SHAPES[name]:
            raise _lib.IrsdeError("LPIPS: %s has shape %s, expected %s" % (src, tuple(t.shape), LPIPS_SHAPES[name]))
        out[name] = t
    if missing:
        raise _lib.IrsdeError("LPIPS: missing tensors: " + "; ".join(missing))
    return out


class LPIPS:
    """`lpips.LPIPS(net='alex')` on the HIP engine: `m(in0, in1)` with inputs in [-1, 1] (or [0, 1] with normalize=True) returns
    a float32 device tensor (B, 1, 1, 1), so the reference's line
    `lpips_fn(GT.to(device) * 2 - 1, SR_img.to(device) * 2 - 1).squeeze().item()` runs unchanged.  Weights: `load_state_dict` /
    `LPIPS.from_files` (see `_lpips_name_table` for the accepted keys).  fp32 throughout; no CPU path, no gradients."""

    def __init__(self, net="alex", version="0.1", spatial=False):
        if net != "alex":
            raise _lib.IrsdeError("LPIPS: only net='alex' is built (got %r)" % (net,))
        if str(version) != "0.1":
            raise _lib.IrsdeError("LPIPS: only version '0.1' is built (got %r)" % (version,))
        if spatial:
            raise _lib.IrsdeError("LPIPS: spatial=True is not built")
        self.weights = None
        self._engines = {}   # device index -> irsde_engine handle

    @classmethod
    def from_files(cls, *paths):
        """The published files (torchvision's AlexNet checkpoint + lpips' alex.pth) or one saved `state_dict()`."""
        sd = {}
        for p in paths:
            d = torch.load(p, map_location="cpu")
            if not isinstance(d, dict):
                raise _lib.IrsdeError("LPIPS: %s does not hold a dict of tensors" % (p,))
            sd.update(d)
        m = cls()
        m.load_state_dict(sd)
        return m

    def load_state_dict(self, sd):
        self.weights = lpips_map_state_dict(sd)
        self._release()
        return self

    def _release(self):
        for h in getattr(self, "_engines", {}).values():   # (a constructor that raised leaves no table)
            try:
                _lib.lib().irsde_destroy(h)
            except Exception:
                pass
        self._engines = {}

    def __del__(self):
        self._release()

    def _engine(self, device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._engines:
            if self.weights is None:
                raise _lib.IrsdeError("LPIPS: no weights loaded (load_state_dict / LPIPS.from_files)")
            L = _lib.lib()
            h = ctypes.c_void_p()
            _lib.check(L.irsde_create_lpips(ctypes.byref(h)))
            try:
                for i in range(L.irsde_num_weights(h)):
                    name = L.irsde_weight_name(h, i).decode()
                    t = self.weights[name]
                    shape = (ctypes.c_int64 * t.dim())(*t.shape)
                    _lib.check(L.irsde_load_weight(h, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()))
                with torch.cuda.device(idx):
                    _lib.check(L.irsde_finalize_weights(h))
            except Exception:
                L.irsde_destroy(h)
                raise
            self._engines[idx] = h
        return self._engines[idx]

    def terms(self, in0, in1, normalize=False):
        """The five per-tap terms of every pair: numpy float64 [B, 5] (their sum is the distance)."""
        a, b = _f32_cuda(in0), _f32_cuda(in1)
        if a.shape != b.shape or a.device != b.device:
            raise _lib.IrsdeError("LPIPS: in0 / in1 shape or device mismatch")
        B, C, H, W = a.shape
        if C != 3:
            raise _lib.IrsdeError("LPIPS: expected 3 channels (RGB), got %d" % C)
        h = self._engine(a.device)
        dist = (ctypes.c_double * B)()
        terms = (ctypes.c_double * (5 * B))()
        with torch.cuda.device(a.device):
            _lib.check(_lib.lib().irsde_lpips(h, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), B, H, W,
                                              1 if normalize else 0, dist, terms, _lib.stream_ptr()))
        self.last_dist = np.array(dist, dtype=np.float64)
        return np.array(terms, dtype=np.float64).reshape(B, 5)

    def __call__(self, in0, in1, normalize=False):
        self.terms(in0, in1, normalize=normalize)
        dev = in0.device
        return torch.from_numpy(self.last_dist.astype(np.float32)).reshape(-1, 1, 1, 1).to(dev)

    def last_profile(self, device=None):
        """(milliseconds, kernel) pairs of the last call on `device` (irsde_op_profile: events around every launch group)."""
        idx = torch.device(device).index if device is not None else next(iter(self._engines))
        buf = ctypes.create_string_buffer(1 << 14)
        _lib.check(_lib.lib().irsde_op_profile(self._engines[idx], buf, len(buf)))
        rows = []
        for line in buf.value.decode().splitlines():
            ms, _, desc = line.strip().partition(" ms  ")
            rows.append((float(ms), desc))
        return rows


def reduce_metrics(metrics):
    """Dataset averages across ranks: all_reduce of (sum, count) per metric (the optional scalar
    reduction); single-process when torch.distributed is not initialised."""
    import torch.distributed as dist
    keys = sorted(metrics)
    local = torch.tensor([[float(np.sum(metrics[k])), float(len(metrics[k]))] for k in keys], dtype=torch.float64)
    if dist.is_available() and dist.is_initialized():
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        buf = local.to(dev)
        dist.all_reduce(buf)
        local = buf.cpu()
    return {k: float(local[i, 0] / max(local[i, 1], 1.0)) for i, k in enumerate(keys)}
