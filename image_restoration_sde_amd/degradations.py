"""Degradation front ends of the reference's test loops — codes/utils/deg_utils.py on the device:

    upscale    deg_utils.py:38-40  F.interpolate(tensor, scale_factor=scale, mode='bicubic')   (sisr/test.py:102, stereo-sr/test.py:105-109)
    mask_to    deg_utils.py:19-34  mask * tensor + (1 - mask), masks from '%06d.png' files       (inpainting/test.py:103)
    add_noise  deg_utils.py:13-15  re-exported from denoising_sde                                (denoising-sde/test.py:104)

and the front end of the image-space datasets, codes/data/util.py:

    imresize   util.py:238-387     MATLAB-style antialiased cubic resize by a factor <= 1       (LQGT_dataset.py:106-130: LQ made from GT)
    modcrop    util.py:221-234     crop height and width down to multiples of the scale          (LQGT_dataset.py:94-96)

All arithmetic runs in libirsde_hip.so (csrc/degrade.hip); there is no CPU / PyTorch fallback.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .denoising_sde import add_noise  # noqa: F401

__all__ = ["upscale", "mask_to", "add_noise", "imresize", "modcrop"]


def _f32_cuda(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.IrsdeError("%s runs on CUDA(HIP) tensors only (no CPU fallback)" % what)
    if t.dim() not in (3, 4):
        raise _lib.IrsdeError("%s needs a [B, C, H, W] or [C, H, W] tensor" % what)
    x = t.detach().to(torch.float32)
    return (x if x.dim() == 4 else x[None]).contiguous()


def upscale(tensor, scale=4, mode="bicubic"):
    """util.upscale: bicubic (align_corners=False, A = -0.75) upscale by an integer factor 1..8 of a [B, C, H, W] or [C, H, W] device
    tensor.  Other modes, non-integer or down-scaling factors raise `IrsdeError`."""
    if mode != "bicubic":
        raise _lib.IrsdeError("upscale: only mode='bicubic' is built, not %r" % (mode,))
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or int(scale) != scale or not 1 <= scale <= 8:
        raise _lib.IrsdeError("upscale: the scale must be an integer in 1..8, not %r" % (scale,))
    x = _f32_cuda(tensor, "upscale")
    B, C, H, W = x.shape
    s = int(scale)
    out = torch.empty((B, C, H * s, W * s), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().irsde_upscale_bicubic(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, C, H, W, s,
                                                    _lib.stream_ptr()))
    return out if tensor.dim() == 4 else out[0]


def read_mask(path):
    """One mask file as `cv2.imread(path)` returns it: uint8 [H, W, 3], BGR channel order (a gray file repeats its plane).  Read with Pillow
    and reversed."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(a[:, :, ::-1])


def mask_to(tensor, mask_root="data/datasets/gt_keep_masks/genhalf", mask_id=-1, n=100, *, masks=None):
    """util.mask_to: `mask * tensor + (1 - mask)` with the uint8 mask / 255. resized to the tensor by nearest interpolation.
    mask_id >= 0: the file '%06d.png' % mask_id of `mask_root` for the whole batch; mask_id < 0: one id per image, drawn with
    `np.random.randint(0, n, batch)` as the reference draws it.  `masks=`: a uint8 array / tensor [Bm, Hm, Wm, Cm] or [Hm, Wm, Cm] or
    [Hm, Wm] instead of files (Bm 1 or B, Cm 1 or C; mask channel k goes with tensor channel k)."""
    x = _f32_cuda(tensor, "mask_to")
    B, C, H, W = x.shape
    if masks is None:
        ids = [int(mask_id)] if mask_id >= 0 else np.random.randint(0, n, B)
        m = np.stack([read_mask(os.path.join(mask_root, "%06d.png" % int(i))) for i in ids])
        if C != 3:   # cv2.imread always returns three planes: a gray mask is one plane repeated
            if not (np.array_equal(m[..., 0], m[..., 1]) and np.array_equal(m[..., 0], m[..., 2])):
                raise _lib.IrsdeError("mask_to: a colour mask needs a 3-channel tensor, not %d channels" % C)
            m = m[..., :1]
        masks = m
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(masks))
    if m.dtype != torch.uint8:
        raise _lib.IrsdeError("mask_to: masks must be uint8 (the values cv2.imread returns), not %s" % m.dtype)
    if m.dim() == 2:
        m = m[None, :, :, None]
    elif m.dim() == 3:
        m = m[None]
    if m.dim() != 4:
        raise _lib.IrsdeError("mask_to: masks must be [Bm, Hm, Wm, Cm], [Hm, Wm, Cm] or [Hm, Wm]")
    m = m.to(x.device).contiguous()
    Bm, Hm, Wm, Cm = m.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().irsde_mask_to(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(m.data_ptr()), Bm, Hm, Wm, Cm,
                                            ctypes.c_void_p(out.data_ptr()), B, C, H, W, _lib.stream_ptr()))
    return out if tensor.dim() == 4 else out[0]


# ---------------------------------------------------------------------------------------------
# imresize: the filter tables of one axis on the host, the filter itself in imresize_kernel
# ---------------------------------------------------------------------------------------------
IMRESIZE_MAX_TAPS = 32   # the kernel's weight tiles hold 32 taps per output: scales down to 1/8 with antialiasing


def _cubic(d):
    """The Keys cubic (a = -0.5) of a float32 tensor of distances, in the operation order of util.py:240-248 (the tables are bit-identical to the
    reference's only when every rounding is)."""
    a1 = torch.abs(d)
    a2 = a1 ** 2
    a3 = a1 ** 3
    near = (a1 <= 1).type_as(a1)
    far = ((a1 > 1) * (a1 <= 2)).type_as(a1)
    return (1.5 * a3 - 2.5 * a2 + 1) * near + (-0.5 * a3 + 2.5 * a2 - 4 * a1 + 2) * far


_TABLES = {}
_DEVICE_TABLES = {}


def imresize_tables(n_in, scale, antialiasing=True):
    """The separable filter of `imresize` along one axis of n_in pixels: (weights float32 [n_out][K], start int32 [n_out], sym_s, sym_e), built
    with torch CPU float32 operations in the order of util.py:251-303 and therefore bit-identical to the reference's tables.

    Output i (coordinate x = i + 1 of 1..n_out, n_out = ceil(n_in scale)) is centred at u = x / scale + 0.5 (1 - 1 / scale).  The kernel is 4 wide,
    or 4 / scale when the scale is below 1 and antialiasing is on; the candidate taps are the P = ceil(width) + 2 pixels from floor(u - width / 2);
    their weights cubic(u - idx) (antialiasing: scale cubic((u - idx) scale)) are divided by the row's sum.  Two columns of the P are then
    dropped as the reference drops them: the outer pair if the first column holds a zero, else the last two if the last column holds one.
    `start[i]` is the 0-based image coordinate of row i's first tap and may be negative: a tap at p < 0 reads pixel -p - 1 and a tap at p >= n_in
    reads 2 n_in - 1 - p (symmetric extension, util.py:342-353).  sym_s / sym_e are the widths of that extension at the two ends; the reference
    runs only where 0 <= sym_s <= n_in and 1 <= sym_e <= n_in, and everything else raises `IrsdeError`."""
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
        raise _lib.IrsdeError("imresize: the scale must be a number, not %r" % (scale,))
    if isinstance(n_in, bool) or not isinstance(n_in, (int, np.integer)) or n_in < 1:
        raise _lib.IrsdeError("imresize: the axis length must be a positive integer, not %r" % (n_in,))
    scale, n_in, antialiasing = float(scale), int(n_in), bool(antialiasing)
    if not scale > 0:
        raise _lib.IrsdeError("imresize: the scale must be positive, not %r" % (scale,))
    if scale > 1:
        raise _lib.IrsdeError("imresize: scale %r enlarges; use upscale" % (scale,))
    if scale < 1 / 8:
        raise _lib.IrsdeError("imresize: scale %r is below 1/8 (more than %d taps per output)" % (scale, IMRESIZE_MAX_TAPS))
    if n_in == 1:
        raise _lib.IrsdeError("imresize: an axis of one pixel has no symmetric extension")
    key = (n_in, scale, antialiasing)
    if key in _TABLES:
        return _TABLES[key]
    n_out = math.ceil(n_in * scale)
    widen = scale < 1 and antialiasing
    width = 4 / scale if widen else 4
    x = torch.linspace(1, n_out, n_out)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - width / 2)
    P = math.ceil(width) + 2
    idx = left.view(n_out, 1).expand(n_out, P) + torch.linspace(0, P - 1, P).view(1, P).expand(n_out, P)
    dist = u.view(n_out, 1).expand(n_out, P) - idx
    w = scale * _cubic(dist * scale) if widen else _cubic(dist)
    w = w / torch.sum(w, 1).view(n_out, 1).expand(n_out, P)
    zeros = torch.sum((w == 0), 0)
    if int(zeros[0]) != 0:        # both narrowings take P - 2 columns of the original P: after this one the next changes nothing
        idx, w = idx.narrow(1, 1, P - 2), w.narrow(1, 1, P - 2)
    if int(zeros[-1]) != 0:
        idx, w = idx.narrow(1, 0, P - 2), w.narrow(1, 0, P - 2)
    sym_s, sym_e = int(-idx.min() + 1), int(idx.max() - n_in)
    if not (0 <= sym_s <= n_in and 1 <= sym_e <= n_in):
        raise _lib.IrsdeError("imresize: an axis of %d pixels at scale %r (antialiasing %s) needs a symmetric extension of %d / %d pixels, which "
                              "the reference cannot run either" % (n_in, scale, antialiasing, sym_s, sym_e))
    if w.shape[1] > IMRESIZE_MAX_TAPS:
        raise _lib.IrsdeError("imresize: %d taps per output, the kernel holds %d" % (w.shape[1], IMRESIZE_MAX_TAPS))
    start = (idx[:, 0] - 1).to(torch.int32).contiguous()
    _TABLES[key] = (w.contiguous(), start, sym_s, sym_e)
    return _TABLES[key]


def _device_tables(n_in, scale, antialiasing, device):
    key = (int(n_in), float(scale), bool(antialiasing), str(device))
    if key not in _DEVICE_TABLES:
        w, start, _, _ = imresize_tables(n_in, scale, antialiasing)
        _DEVICE_TABLES[key] = (w.to(device), start.to(device))
    return _DEVICE_TABLES[key]


def imresize(img, scale, antialiasing=True):
    """util.imresize: the MATLAB-style cubic resize by a factor in [1/8, 1] (the same for both axes) of a [B, C, H, W] or [C, H, W] device
    tensor; returns the same rank as float32, overshoot kept (no clamp, no rounding).  An HWC numpy array is uploaded to the current device and
    an HWC numpy array comes back, as the reference returns it.  The H axis is filtered first, as there."""
    if isinstance(img, np.ndarray):
        if img.ndim != 3:
            raise _lib.IrsdeError("imresize needs an [H, W, C] numpy array")
        if not torch.cuda.is_available():
            raise _lib.IrsdeError("imresize runs on CUDA(HIP) devices only (no CPU fallback)")
        t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()
        return np.ascontiguousarray(imresize(t, scale, antialiasing).cpu().numpy().transpose(1, 2, 0))
    x = _f32_cuda(img, "imresize")
    B, C, H, W = x.shape
    wH, sH = _device_tables(H, scale, antialiasing, x.device)
    wW, sW = _device_tables(W, scale, antialiasing, x.device)
    Ho, Wo = wH.shape[0], wW.shape[0]
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().irsde_imresize(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, C, H, W, Ho, Wo,
                                             ctypes.c_void_p(wH.data_ptr()), ctypes.c_void_p(sH.data_ptr()), wH.shape[1],
                                             ctypes.c_void_p(wW.data_ptr()), ctypes.c_void_p(sW.data_ptr()), wW.shape[1], _lib.stream_ptr()))
    return out if img.dim() == 4 else out[0]


def modcrop(img, scale):
    """util.modcrop: height and width cropped down to multiples of `scale` — the trailing two dimensions of a tensor, or the leading two of an
    HW / HWC numpy array (a copy, as the reference returns)."""
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale < 1:
        raise _lib.IrsdeError("modcrop: the scale must be a positive integer, not %r" % (scale,))
    if isinstance(img, np.ndarray):
        if img.ndim not in (2, 3):
            raise _lib.IrsdeError("modcrop: wrong img ndim: [%d]" % img.ndim)
        H, W = img.shape[:2]
        return np.copy(img[:H - H % scale, :W - W % scale])
    if not isinstance(img, torch.Tensor) or img.dim() < 2:
        raise _lib.IrsdeError("modcrop needs a tensor of at least two dimensions or an HW / HWC numpy array")
    H, W = img.shape[-2:]
    return img[..., :H - H % scale, :W - W % scale]
