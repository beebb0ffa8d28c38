"""Degradation front ends of the reference's test loops — codes/utils/deg_utils.py on the device:

    upscale    deg_utils.py:38-40  F.interpolate(tensor, scale_factor=scale, mode='bicubic')   (sisr/test.py:102, stereo-sr/test.py:105-109)
    mask_to    deg_utils.py:19-34  mask * tensor + (1 - mask), masks from '%06d.png' files       (inpainting/test.py:103)
    add_noise  deg_utils.py:13-15  re-exported from denoising_sde                                (denoising-sde/test.py:104)

All arithmetic runs in libirsde_hip.so (csrc/degrade.hip); there is no CPU / PyTorch fallback.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .denoising_sde import add_noise  # noqa: F401

__all__ = ["upscale", "mask_to", "add_noise"]


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
