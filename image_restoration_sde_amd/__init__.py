"""image-restoration-sde_amd: the IR-SDE reverse-diffusion sampler of Algolzw/image-restoration-sde,
rebuilt for MI355X (gfx950): hand-written HIP kernels behind a C ABI (include/irsde_hip.h,
csrc/ -> libirsde_hip.so) with the reference's own Python interface on top:

    IRSDE              codes/utils/sde_utils.py:80-361
    ConditionalUNet    codes/config/deraining/models/modules/DenoisingUNet_arch.py:18-134
    ConditionalNAFNet  codes/config/deraining/models/modules/DenoisingNAFNet_arch.py:85-187 (Refusion)
    DenoisingSDE, denoising_sde.ConditionalUNet / ConditionalNAFNet / DenoisingSDEModel / add_noise
                       codes/utils/sde_utils.py:373-593, codes/config/denoising-sde/models/{modules/DenoisingUNet_arch.py,
                       modules/DenoisingNAFNet_arch.py, denoising_model.py}, codes/utils/deg_utils.py:13-15
    DenoisingModel     codes/config/deraining/models/denoising_model.py (inference surface)
    latent.UNet / latent.ConditionalNAFNet / latent.CNAFNetLocal (also exported as CNAFNetLocal) / LatentDenoisingModel
                       codes/config/latent-dehazing/models/{modules/UNet_arch.py, modules/DenoisingNAFNet_arch.py,
                       latent_denoising_model.py} (encode once, sample in the latent, decode once)
    stereo_sr.ConditionalNAFNet
                       codes/config/stereo-sr/models/modules/DenoisingNAFNet_arch.py (NAFBlocks + SCAM on stereo pairs)
    stereo_sr.ConditionalUNet
                       codes/config/stereo-sr/models/modules/DenoisingUNet_arch.py (the IR-SDE UNet with a full-resolution SCAM on every level)
    metrics            codes/utils/img_utils.py:136-234 + codes/data/util.py:177-198 (tensor2img / PSNR / SSIM / Y channel)
    LPIPS (metrics.LPIPS)
                       lpips.LPIPS(net='alex') of codes/config/deraining/test.py:74, 149-154 (an AlexNet feature tower + the distance, fp32)
    degradations       codes/utils/deg_utils.py (upscale: bicubic by an integer factor; mask_to: the inpainting composite; add_noise) +
                       codes/data/util.py:221-387 (imresize: the MATLAB-style antialiased cubic downscale that makes LQ from GT; modcrop)
"""
from ._lib import IrsdeError, IrsdeLibraryError, build_library  # noqa: F401
from .denoising_model import DenoisingModel, ReverseSDEDenoisingModel, create_model, define_G  # noqa: F401
from .dist import gather_batch, sample_shard, sample_sharded, shard_bounds  # noqa: F401
from .sde import IRSDE  # noqa: F401
from .unet import ConditionalUNet  # noqa: F401
from .nafnet import ConditionalNAFNet  # noqa: F401
from . import denoising_sde  # noqa: F401
from .denoising_sde import DenoisingSDE  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import LPIPS  # noqa: F401
from . import degradations  # noqa: F401
from . import latent  # noqa: F401
from . import latent_bokeh  # noqa: F401
from . import stereo_sr  # noqa: F401
from .latent import CNAFNetLocal, LatentDenoisingModel  # noqa: F401

__all__ = ["IRSDE", "DenoisingSDE", "denoising_sde", "metrics", "LPIPS", "degradations", "latent", "latent_bokeh", "stereo_sr", "LatentDenoisingModel", "CNAFNetLocal", "ConditionalUNet", "ConditionalNAFNet", "DenoisingModel", "ReverseSDEDenoisingModel", "create_model", "define_G", "build_library",
           "IrsdeError", "IrsdeLibraryError", "shard_bounds", "gather_batch", "sample_shard", "sample_sharded"]
