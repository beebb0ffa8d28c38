"""stereo-sr score network: `ConditionalNAFNet` whose NAFBlocks end in a stereo cross-attention module (SCAM).

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
from .unet import _Gain


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


class ConditionalNAFNet(_ImageNAFNet):
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


class StereoDenoisingModel(DenoisingModel):
    """The stereo-sr wrapper (models/denoising_model.py): `test(sde, perform_ode=False, save_states=False)` runs reverse_sde, or
    reverse_ode with perform_ode; `get_current_visuals()["Output"]` is the [2 img_channel, H, W] pair that test.py chunks into L / R."""
    task = "stereo-sr"

    def test(self, sde=None, perform_ode=False, save_states=False):
        return DenoisingModel.test(self, sde, mode="ode" if perform_ode else "sde", save_states=save_states)
