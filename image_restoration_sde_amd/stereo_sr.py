"""stereo-sr score networks: `ConditionalNAFNet` whose NAFBlocks end in a stereo cross-attention module (SCAM), and `ConditionalUNet`
(below) with a full-resolution SCAM on every level.  The NAFNet:

Reference: codes/config/stereo-sr/models/modules/DenoisingNAFNet_arch.py
    :15-60   SCAM(c): bicubic quarter-downsample, LayerNorm + 1x1 projections per view, one W' x W' score matrix per image row,
             softmax over both axes (right -> left and left -> right), beta / gamma scale, nearest upsample, residual
    :63-134  NAFBlock = the deraining block followed by `x = self.fusion(x)`
    :137-240 ConditionalNAFNet: inp / cond [B, 6, H, W] (left view channels 0-2, right 3-5), the views stacked on the batch axis
and models/denoising_model.py:171-184 (`test(sde, perform_ode=False, save_states=False)`).

Same HIP engine as the other NAFNets (IRSDE_FLAG_NAF_STEREO): the SCAM runs on csrc/scam.hip plus the engine's 1x1 GEMM, the
sampler state / mu / noise stay [B][6][H][W] per pair.  Unlike the reference (whose int-time path only works for one pair, as
`tensor([t])` is concatenated to two rows) an int `time` is shared by every pair of the batch; a [B] tensor gives each pair its own.
Padded H and W must be >= 4 * 2**len(enc_blk_nums) (the reference's interpolate fails on an empty map): smaller inputs raise.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from .denoising_model import DenoisingModel
from .nafnet import ConditionalNAFNet as _ImageNAFNet, _NAFBlock
from .unet import ConditionalUNet as _ImageUNet, _Gain, _ResBlock, _Residual, _upsample


class _SCAM(nn.Module):  # DenoisingNAFNet_arch.py:15-31 (parameter container)
    def __init__(self, c):
        super().__init__()
        self.scale = c ** -0.5
        self.norm_l = _Gain(c)
        self.norm_r = _Gain(c)
        self.l_proj1 = nn.Conv2d(c, c, 1)
        self.r_proj1 = nn.Conv2d(c, c, 1)
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)))
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)))
        self.l_proj2 = nn.Conv2d(c, c, 1)
        self.r_proj2 = nn.Conv2d(c, c, 1)


class _StereoNAFBlock(_NAFBlock):
    def __init__(self, c, time_emb_dim):
        super().__init__(c, time_emb_dim)
        self.fusion = _SCAM(c)


class _WideRows:
    def set_wide_rows(self, enable=True):
        """Lift the width limit (IRSDE_FLAG_SCAM_STREAM): SCAMs whose score rows are wider than the strip kernels hold in LDS (ConditionalUNet: padded
        width > 1024; ConditionalNAFNet: > 2051) run the streaming online-softmax core of csrc/scam_stream.hip; narrower inputs compute exactly what
        they compute without it.  The next call builds a fresh engine."""
        if enable:
            self.engine_flags |= _lib.FLAG_SCAM_STREAM
        else:
            self.engine_flags &= ~_lib.FLAG_SCAM_STREAM
        return self


class ConditionalNAFNet(_WideRows, _ImageNAFNet):
    _fp16_act = False   # fp16 activation storage covers the image-space network only (the engine refuses it here too)

    def __init__(self, img_channel=3, width=16, middle_blk_num=1, enc_blk_nums=[], dec_blk_nums=[], upscale=1):
        nn.Module.__init__(self)
        self.upscale = upscale
        self.img_channel = img_channel
        self.in_nc = self.out_nc = 2 * img_channel   # a stereo pair: [left | right]
        self.width = width
        self.enc_blk_nums, self.dec_blk_nums, self.middle_blk_num = list(enc_blk_nums), list(dec_blk_nums), middle_blk_num
        time_dim = width * 4
        self.time_mlp = nn.Sequential(nn.Identity(), nn.Linear(width, time_dim * 2), nn.Identity(), nn.Linear(time_dim, time_dim))
        self.intro = nn.Conv2d(img_channel * 2, width, 3, padding=1)
        self.ending = nn.Conv2d(width, img_channel, 3, padding=1)
        self.encoders, self.decoders = nn.ModuleList(), nn.ModuleList()
        self.ups, self.downs = nn.ModuleList(), nn.ModuleList()
        chan = width
        for num in self.enc_blk_nums:
            self.encoders.append(nn.Sequential(*[_StereoNAFBlock(chan, time_dim) for _ in range(num)]))
            self.downs.append(nn.Conv2d(chan, 2 * chan, 2, 2))
            chan *= 2
        self.middle_blks = nn.Sequential(*[_StereoNAFBlock(chan, time_dim) for _ in range(middle_blk_num)])
        for num in self.dec_blk_nums:
            self.ups.append(nn.Sequential(nn.Conv2d(chan, chan * 2, 1, bias=False), nn.Identity()))
            chan //= 2
            self.decoders.append(nn.Sequential(*[_StereoNAFBlock(chan, time_dim) for _ in range(num)]))
        self.padder_size = 2 ** len(self.encoders)
        self._engine = None
        self._engine_key = None
        self.engine_flags = 0

    def _create_handle(self, L, device_index, flags):
        cfg = _lib.NafConfig()
        cfg.img_channel, cfg.width, cfg.middle_blk_num = self.img_channel, self.width, self.middle_blk_num
        cfg.n_enc, cfg.n_dec = len(self.enc_blk_nums), len(self.dec_blk_nums)
        for i, v in enumerate(self.enc_blk_nums):
            cfg.enc_blk_nums[i] = v
        for i, v in enumerate(self.dec_blk_nums):
            cfg.dec_blk_nums[i] = v
        cfg.device, cfg.flags = device_index, flags | _lib.FLAG_NAF_STEREO
        h = ctypes.c_void_p()
        _lib.check(L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h)))
        return h

    def forward(self, inp, cond, time):
        """noise = model(inp, cond, time) on stereo pairs [B, 2 img_channel, H, W] — DenoisingNAFNet_arch.py:199-240."""
        if inp.dim() != 4 or inp.shape[1] != self.in_nc or tuple(cond.shape) != tuple(inp.shape):
            raise _lib.IrsdeError("stereo ConditionalNAFNet.forward needs inp and cond of shape [B, %d, H, W]" % self.in_nc)
        return super().forward(inp, cond, time)


class ConditionalUNet(_WideRows, _ImageUNet):
    """The IR-SDE (UNet) score network of stereo-sr: codes/config/stereo-sr/models/modules/DenoisingUNet_arch.py
        :18-56   SCAM(c) WITHOUT the quarter-downsample / upsample of the NAFNet's: one W x W score matrix per image row at full resolution
        :59-196  ConditionalUNet(in_nc, out_nc, nf, depth=4, upscale=1, fusion=False): init_conv 3x3 on cat(xt_v, cond_v) (no xt - cond);
                 every level is ResBlock, ResBlock, Residual(PreNorm(LinearAttention)), SCAM, down / up-sample; mid_fusion between
                 mid_attn and mid_block2; output xt + cat(x_l, x_r).
    Parameter container under the reference's state_dict names; the arithmetic runs on the HIP engine (IRSDE_FLAG_UNET_STEREO, fp32 only;
    padded width <= 1024 unless `set_wide_rows()`).  xt / cond are [B, 2 in_nc, H, W] pairs; an int `time` is shared by every pair, a [B] tensor gives each its own."""

    def __init__(self, in_nc, out_nc, nf, depth=4, upscale=1, fusion=False):
        nn.Module.__init__(self)
        if in_nc != out_nc:
            raise _lib.IrsdeError("stereo ConditionalUNet: in_nc must equal out_nc (the output is a residual on the state)")
        self.view_nc, self.nf, self.depth = in_nc, nf, depth
        self.in_nc = self.out_nc = 2 * in_nc   # a stereo pair: [left | right]
        self.upscale, self.fusion = upscale, fusion   # stored and unused, as in the reference (:63-64)
        time_dim = nf * 4
        self.init_conv = nn.Conv2d(in_nc * 2, nf, 3, padding=1, bias=False)
        self.time_mlp = nn.Sequential(nn.Identity(), nn.Linear(nf, time_dim), nn.GELU(), nn.Linear(time_dim, time_dim))
        self.downs = nn.ModuleList([])
        self.ups = nn.ModuleList([])
        for i in range(depth):
            di, do = nf * 2 ** i, nf * 2 ** (i + 1)
            self.downs.append(nn.ModuleList([
                _ResBlock(di, di, time_dim), _ResBlock(di, di, time_dim), _Residual(di), _SCAM(di),
                nn.Conv2d(di, do, 4, 2, 1) if i != depth - 1 else nn.Conv2d(di, do, 3, padding=1, bias=False)]))
            self.ups.insert(0, nn.ModuleList([
                _ResBlock(do + di, do, time_dim), _ResBlock(do + di, do, time_dim), _Residual(do), _SCAM(do),
                _upsample(do, di) if i != 0 else nn.Conv2d(do, di, 3, padding=1, bias=False)]))
        mid = nf * 2 ** depth
        self.mid_block1 = _ResBlock(mid, mid, time_dim)
        self.mid_attn = _Residual(mid)
        self.mid_fusion = _SCAM(mid)
        self.mid_block2 = _ResBlock(mid, mid, time_dim)
        self.final_res_block = _ResBlock(nf * 2, nf, time_dim)
        self.final_conv = nn.Conv2d(nf, out_nc, 3, 1, 1)
        self._engine = None
        self._engine_key = None
        self.engine_flags = 0

    def _create_handle(self, L, device_index, flags):
        cfg = _lib.Config(self.view_nc, self.view_nc, self.nf, self.depth, device_index, flags | _lib.FLAG_UNET_STEREO)
        h = ctypes.c_void_p()
        _lib.check(L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)))
        return h

    def set_compute_dtype(self, dtype):
        """fp32 only: the other operand modes are not covered for the full-resolution SCAM network (the engine refuses them too)."""
        if dtype not in ("fp32", "f32", torch.float32):
            raise _lib.IrsdeError("stereo ConditionalUNet runs in fp32 only, not %r" % (dtype,))
        return _ImageUNet.set_compute_dtype(self, dtype)

    def forward(self, xt, cond, time):
        """out = model(xt, cond, time) on stereo pairs [B, 2 in_nc, H, W] — DenoisingUNet_arch.py:136-196."""
        if xt.dim() != 4 or xt.shape[1] != self.in_nc or tuple(cond.shape) != tuple(xt.shape):
            raise _lib.IrsdeError("stereo ConditionalUNet.forward needs xt and cond of shape [B, %d, H, W]" % self.in_nc)
        return super().forward(xt, cond, time)


class StereoDenoisingModel(DenoisingModel):
    """The stereo-sr wrapper (models/denoising_model.py): `test(sde, perform_ode=False, save_states=False)` runs reverse_sde, or
    reverse_ode with perform_ode; `get_current_visuals()["Output"]` is the [2 img_channel, H, W] pair that test.py chunks into L / R."""
    task = "stereo-sr"

    def test(self, sde=None, perform_ode=False, save_states=False):
        return DenoisingModel.test(self, sde, mode="ode" if perform_ode else "sde", save_states=save_states)
