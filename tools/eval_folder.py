"""eval_folder.py — the dataset evaluation loop of the reference's test scripts on the MI355X sampler.

Reproduces /root/reference/codes/config/deraining/test.py:93-217 on the product API: walk an LQ (and optional GT)
image folder -> `sde.noise_state(LQ)` -> `model.feed_data / model.test(sde, mode) / get_current_visuals` semantics
(here: batched `sde.reverse_*` calls) -> `tensor2img` -> save PNG -> PSNR / SSIM on RGB and on the Y channel ->
dataset averages.  This is the one command for the Rain100H gate of BASELINE.json (PSNR within 0.05 dB of the
reference's 31.65 dB, /root/reference/README.md:42-46) once `rain100h_sde.pth` and the dataset are supplied:

    python tools/eval_folder.py --lq Rain100H/LQ --gt Rain100H/GT --weights rain100h_sde.pth \
        --max-sigma 10 --T 100 --mode posterior --scale 4 --out results/Rain100H [--gpus 8]

(`--scale 4` is the default: the reference crops `crop_border or scale` = 4 pixels before PSNR / SSIM, test.py:134.)

Differences from the reference loop, all stated: images of equal size are sampled as one batch (`--batch`); with
`--gpus N` the image list is sharded over N ranks (one process per GPU, no collective except the final metric
all_reduce); image I/O is PIL instead of cv2 (PNG decoding is lossless, so the tensors are identical; JPEG decoders
may differ in the last bit); LPIPS is computed when --lpips-weights is given (the AlexNet and lin weights are external
downloads: `metrics.LPIPS`, csrc/lpips.hip); the noise of `noise_state` is drawn per image from a generator seeded by (--seed, image index) so a run is
reproducible and independent of batching / sharding.

`--task denoising` is the loop of codes/config/denoising-sde/test.py:91-142 instead (Gaussian denoising, options/test/refusion.yml and
ir-sde.yml): walk a clean GT folder -> `add_noise(GT, sigma)` -> `model.feed_data(LQ, GT)` / `model.test(sde, sigma=sigma)`
(`DenoisingSDE.reverse_ode` from `get_optimal_timestep(sigma)`) -> <name>.png (restored), <name>_noisy.png, <name>_clean.png -> PSNR / SSIM per
image (no border crop, as there) and averaged:

    python tools/eval_folder.py --task denoising --gt CBSD68 --sigma 15 --max-sigma 70 --T 1000 --weights refusion.pth \
        [--arch nafnet|unet] --out results/CBSD68_sigma15 [--gpus 8]

Its stated differences: equal-sized images are batched; the restored image is written as .png where test.py writes .tif without a suffix; the
noise is the library's keyed Philox draw (`denoising_sde.add_noise`, key = (--seed, global image index)), so the result does not depend on
batching or on the rank count; LPIPS is computed when --lpips-weights is given.

`--task sisr | inpainting | stereo-sr` are the loops of codes/config/{sisr,inpainting,stereo-sr}/test.py, which put a degradation step of
codes/utils/deg_utils.py in front of `sde.noise_state(LQ)`; here that step runs on the device (`degradations.upscale` / `mask_to`,
csrc/degrade.hip), and the rest is the LQ / GT loop above:

    python tools/eval_folder.py --task sisr --lq DIV2K/LR_x4 --gt DIV2K/HR --scale 4 --max-sigma 30 --weights sisr.pth --out results/sisr
    python tools/eval_folder.py --task inpainting --gt celebaHQ/testHQ --mask-root gt_keep_masks/thin --max-sigma 30 --weights inp.pth
    python tools/eval_folder.py --task stereo-sr --lq Flickr1024/LR_x4 --gt Flickr1024/HR --max-sigma 30 --weights stereo.pth \
        --naf-width 64 --naf-enc 1,1,1,28 [--model unet --nf 64 --depth 4] [--wide-rows]

    sisr       sisr/test.py:102        LQ = util.upscale(LQ, scale): bicubic by --scale; PSNR / SSIM on RGB and Y, cropped as above
    inpainting inpainting/test.py:103  LQ = util.mask_to(GT, mask_root, mask_id=i), i the global image index -> '%06d.png' % i
    stereo-sr  stereo-sr/test.py:105-126  --lq (and --gt) hold L / R files, paired in sorted order as StereoLQ_dataset.py:66-67 pairs them
               (2i, 2i + 1); each view is upscaled x4 (the factor is hard-coded there), the pair [L | R] is sampled by the stereo network,
               and the output is chunked into L / R for the images and for PSNR / SSIM per view (RGB only, no border crop, as there)
The sampler defaults to `--mode sde`: these task directories' `denoising_model.test` hard-codes `reverse_sde` (stereo-sr: or `reverse_ode` with
perform_ode = `--mode ode`).  Their stated differences, beyond those of the LQ / GT loop (batching, sharding, PIL, LPIPS only with --lpips-weights, the per-image
seeded `noise_state` draw): the degraded LQ lives on the device, so the noise is drawn on the CPU as before and added there; inpainting does not
write the intermediate states (`save_states=True` in inpainting/test.py:108); stereo-sr names the right view's files after the right view's own
file instead of `img_name.replace('L', 'R')`, and also writes <name>_LQ.png / <name>_HQ.png per view.

`--task sisr --lq-from-gt` needs no LQ folder: like LQGT_dataset with no dataroot_LQ (codes/data/LQGT_dataset.py:94-96, 106-130) every GT image
is cropped to a multiple of --scale (`degradations.modcrop`) and the low-resolution image is made from it on the device with the MATLAB-style
antialiased cubic resize `degradations.imresize(GT, 1 / scale, True)` (codes/data/util.py:238-387, csrc/degrade.hip) — the filter the usual x2 /
x3 / x4 LR test sets were made with; then the sisr loop as above, with PSNR / SSIM against the cropped GT:

    python tools/eval_folder.py --task sisr --gt DIV2K/HR --lq-from-gt --scale 4 --max-sigma 30 --weights sisr.pth --out results/sisr

Stated difference: the low-resolution image stays float32 (LQGT_dataset makes it from the float GT in the same way; a stored LR set has been
rounded to 8 bits on the way to disk).
"""
import argparse
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".tif")  # codes/data/util.py:12


def list_images(folder):
    """Sorted image paths of a folder tree (codes/data/util.py:17-28 `_get_paths_from_images`)."""
    out = []
    for dirpath, _, fnames in sorted(os.walk(folder)):
        for f in sorted(fnames):
            if f.lower().endswith(IMG_EXTENSIONS):
                out.append(os.path.join(dirpath, f))
    if not out:
        raise FileNotFoundError("%s has no valid image file" % folder)
    return out


def pair_paths(lq_dir, gt_dir):
    """[(lq_path, gt_path | None)] in sorted order; like LQGTDataset the i-th LQ file goes with the i-th GT file
    (codes/data/LQGT_dataset.py:48-54), and the counts must agree."""
    lq = list_images(lq_dir)
    if gt_dir is None:
        return [(p, None) for p in lq]
    gt = list_images(gt_dir)
    if len(gt) != len(lq):
        raise ValueError("GT and LQ datasets have different number of images - %d, %d" % (len(gt), len(lq)))
    return list(zip(lq, gt))


def read_img(path):
    """codes/data/util.py:65-81 `read_img` + the BGR->RGB / HWC->CHW of LQGT_dataset.py:177-186: float32 CHW RGB
    in [0, 1]."""
    import numpy as np
    from PIL import Image
    im = Image.open(path)
    a = np.asarray(im.convert("RGB") if im.mode != "L" else im, dtype=np.float32) / np.float32(255.0)
    if a.ndim == 2:
        a = a[:, :, None]
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def save_img(img_bgr, path):
    """util.save_img (cv2.imwrite of a BGR / gray uint8 image) through PIL."""
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(img_bgr[..., ::-1] if img_bgr.ndim == 3 else img_bgr).save(path)


def batches_of_equal_size(items, sizes, max_batch):
    """Consecutive-in-order grouping: indices into `items` batched while the (H, W) stays the same."""
    out, cur = [], []
    for i in range(len(items)):
        if cur and (sizes[i] != sizes[cur[0]] or len(cur) >= max_batch):
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def build_model(a, P, torch):
    if a.model == "nafnet":
        m = P.ConditionalNAFNet(img_channel=3, width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
    else:
        m = P.ConditionalUNet(3, 3, a.nf, depth=a.depth)
    sd = torch.load(a.weights, map_location="cpu")
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}  # base_model.py:92-105
    m.load_state_dict(sd, strict=True)
    return m


def load_lpips(a, P):
    """lpips.LPIPS(net='alex') of test.py:74 from the user's weight files, or None without --lpips-weights."""
    return P.metrics.LPIPS.from_files(*a.lpips_weights) if a.lpips_weights else None


def _with_lpips(line, lp_value):
    """A per-image log line with `LPIPS: x` behind its SSIM entry, where test.py:181 has it."""
    head, sep, tail = line.partition("; PSNR_Y")
    if sep:
        return "%s; LPIPS: %.6f%s%s" % (head, lp_value, sep, tail)
    return "%s; LPIPS: %.6f." % (line[:-1], lp_value)


def _ints(s):
    return [int(v) for v in s.split(",") if v != ""]


def run_denoising(a, P, torch, np, dev, world, rank, log):
    """denoising-sde/test.py:91-142 on `create_model(opt, task="denoising-sde")`, `DenoisingSDE` and `add_noise`."""
    if a.arch == "nafnet":
        net = {"which_model_G": "ConditionalNAFNet",
               "setting": dict(width=a.naf_width, enc_blk_nums=_ints(a.naf_enc), middle_blk_num=a.naf_mid, dec_blk_nums=_ints(a.naf_dec))}
    else:
        net = {"which_model_G": "ConditionalUNet", "setting": dict(in_nc=3, out_nc=3, nf=a.nf, depth=a.depth)}
    opt = {"model": "denoising", "network_G": net, "path": {"pretrain_model_G": a.weights, "strict_load": True}}
    with torch.cuda.device(dev):
        model = P.create_model(opt, task="denoising-sde")
    if a.dtype != "fp32":
        model.model.set_compute_dtype(a.dtype)
    sde = P.DenoisingSDE(max_sigma=a.max_sigma, T=a.T, schedule=a.schedule, device=dev)
    sde.set_model(model.model)
    sde.seed = a.seed
    paths = list_images(a.gt)
    lo, hi = P.shard_bounds(len(paths), world, rank)
    mine = list(range(lo, hi))
    gt_np = [read_img(paths[i]) for i in mine]
    res = {"psnr": [], "ssim": []}
    lp = load_lpips(a, P)
    if lp is not None:
        res["lpips"] = []
    times = []
    for grp in batches_of_equal_size(mine, [x.shape for x in gt_np], a.batch):
        GT = torch.from_numpy(np.stack([gt_np[j] for j in grp])).to(dev)
        LQ = P.denoising_sde.add_noise(GT, a.sigma, seed=a.seed, image_offset=mine[grp[0]])   # util.add_noise(GT, degrad_sigma), test.py:104
        sde.image_offset = mine[grp[0]]
        model.feed_data(LQ, GT)
        torch.cuda.synchronize()
        tic = time.time()
        model.test(sde, sigma=a.sigma, save_states=False)
        torch.cuda.synchronize()
        times.append((time.time() - tic) / len(grp))
        m = P.metrics.evaluate_batch(model.output, GT, crop_border=0, lpips=lp)   # calculate_psnr / calculate_ssim(output, GT): no crop (test.py:128-129)
        names = [os.path.splitext(os.path.basename(paths[mine[j]]))[0] for j in grp]
        for n, name in enumerate(names):
            res["psnr"].append(float(m["psnr"][n]))
            res["ssim"].append(float(m["ssim"][n]))
            line = "img%3d:%-15s - PSNR: %.6f dB; SSIM: %.6f." % (mine[grp[n]], name, m["psnr"][n], m["ssim"][n])
            if lp is not None:
                res["lpips"].append(float(m["lpips"][n]))
                line = _with_lpips(line, m["lpips"][n])
            log(line)
        if a.out:
            imgs, lqi, gti = (P.metrics.tensor2img_batch(t) for t in (model.output, LQ, GT))
            for n, name in enumerate(names):
                save_img(imgs[n], os.path.join(a.out, name + ".png"))
                save_img(lqi[n], os.path.join(a.out, name + "_noisy.png"))
                save_img(gti[n], os.path.join(a.out, name + "_clean.png"))
    summary = None
    local = {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}
    if world > 1 or len(local["psnr"]):
        summary = P.metrics.reduce_metrics(local)
    if rank == 0 and summary is not None:
        log("----Average PSNR/SSIM results for %s_sigma%g----\n\tPSNR: %.6f dB; SSIM: %.6f\n" %
            (os.path.basename(os.path.normpath(a.gt)), a.sigma, summary["psnr"], summary["ssim"]))
        if "lpips" in summary:
            log("----average LPIPS\t: %.6f\n" % summary["lpips"])
    if rank == 0 and times:
        log("average test time per image: %.4f s (rank 0, %d images over %d rank(s))" % (float(np.mean(times)), len(paths), world))
    return summary


DEGRADED_TASKS = ("sisr", "inpainting", "stereo-sr")


def run_degraded(a, P, torch, np, dev, world, rank, log, crop_border, on_batch=None):
    """The sisr / inpainting / stereo-sr loops: the degradation step of `P.degradations` on the device, then the LQ / GT loop's noise,
    sampler, images and metrics.  `on_batch(global_indices, LQ, output)` receives every batch's device tensors."""
    stereo = a.task == "stereo-sr"
    if stereo:
        if a.model == "nafnet":
            net = {"which_model_G": "ConditionalNAFNet",
                   "setting": dict(img_channel=3, width=a.naf_width, enc_blk_nums=_ints(a.naf_enc), middle_blk_num=a.naf_mid, dec_blk_nums=_ints(a.naf_dec))}
        else:
            net = {"which_model_G": "ConditionalUNet", "setting": dict(in_nc=3, out_nc=3, nf=a.nf, depth=a.depth)}
        opt = {"model": "denoising", "network_G": net, "path": {"pretrain_model_G": a.weights, "strict_load": True}}
        with torch.cuda.device(dev):
            wrapper = P.create_model(opt, task="stereo-sr")
        model = wrapper.model.eval()
        if a.wide_rows:
            model.set_wide_rows()
    else:
        model = build_model(a, P, torch).to(dev).eval()
    if a.dtype != "fp32":
        model.set_compute_dtype(a.dtype)
    sde = P.IRSDE(max_sigma=a.max_sigma, T=a.T, schedule=a.schedule, eps=a.eps, device=dev)
    sde.set_model(model)
    sde.seed = a.seed

    per = 2 if stereo else 1   # files per dataset item: stereo-sr pairs files 2i, 2i + 1 of the sorted list (StereoLQ_dataset.py:66-67)
    from_gt = a.lq_from_gt   # sisr: LQ made from the modcropped GT (LQGT_dataset.py:94-96, 106-130)
    src = list_images(a.gt if a.task == "inpainting" or from_gt else a.lq)
    gts = list_images(a.gt) if a.gt is not None else None
    if gts is not None and len(gts) != len(src):
        raise ValueError("GT and LQ datasets have different number of images - %d, %d" % (len(gts), len(src)))
    if len(src) % per:
        raise ValueError("stereo-sr needs an even number of images (L / R pairs in sorted order), not %d" % len(src))
    n_items = len(src) // per
    lo, hi = P.shard_bounds(n_items, world, rank)
    mine = list(range(lo, hi))

    def item(paths, i):   # [C, H, W]; stereo: cat([L, R], 0) (StereoLQ_dataset.py:87)
        return np.concatenate([read_img(paths[per * i + v]) for v in range(per)], axis=0)

    src_np = [item(src, i) for i in mine]
    if from_gt:
        src_np = [P.degradations.modcrop(torch.from_numpy(x), a.scale).contiguous().numpy() for x in src_np]
    res = {"psnr": [], "ssim": []} if stereo else {"psnr": [], "ssim": [], "psnr_y": [], "ssim_y": []}
    lp = load_lpips(a, P)
    if lp is not None:
        res["lpips"] = []
    times = []
    fn = {"sde": sde.reverse_sde, "ode": sde.reverse_ode, "posterior": sde.reverse_posterior}[a.mode]
    for grp in batches_of_equal_size(mine, [x.shape for x in src_np], a.batch):
        idx = [mine[j] for j in grp]
        x = torch.from_numpy(np.stack([src_np[j] for j in grp])).to(dev)
        GT = None
        if from_gt:
            GT = x
            LQ = P.degradations.upscale(P.degradations.imresize(x, 1 / a.scale, True), a.scale)   # util.imresize(img_GT, 1 / scale, True), then as below
        elif a.task == "sisr":
            LQ = P.degradations.upscale(x, a.scale)                        # util.upscale(LQ, scale), sisr/test.py:102
        elif stereo:
            LQ = torch.cat([P.degradations.upscale(v, 4) for v in x.chunk(2, dim=1)], dim=1)   # stereo-sr/test.py:105-108
        else:
            GT = x
            LQ = torch.cat([P.degradations.mask_to(x[n:n + 1], a.mask_root, mask_id=i) for n, i in enumerate(idx)])  # mask_id = i, inpainting/test.py:103
        if GT is None and gts is not None:
            GT = torch.from_numpy(np.stack([item(gts, i) for i in idx])).to(dev)
        noise = torch.stack([torch.randn(LQ.shape[1:], generator=torch.Generator().manual_seed(a.seed * 1000003 + i)) for i in idx])
        noisy_state = LQ + (noise * sde.max_sigma).to(dev)                 # IRSDE.noise_state (sde_utils.py:360-361)
        sde.image_offset = idx[0]
        sde.set_mu(LQ)
        torch.cuda.synchronize()
        tic = time.time()
        out = fn(noisy_state)
        torch.cuda.synchronize()
        times.append((time.time() - tic) / len(grp))
        if on_batch is not None:
            on_batch(idx, LQ, out)
        # views of a batch as images: stereo-sr chunks the pair into L / R (stereo-sr/test.py:119-126)
        views = (lambda t: torch.cat(t.chunk(2, dim=1), dim=0)) if stereo else (lambda t: t)
        nb = len(grp)
        names = [[os.path.splitext(os.path.basename((gts or src)[per * i + v]))[0] for i in idx] for v in range(per)]
        if GT is not None:
            m = P.metrics.evaluate_batch(views(out), views(GT), crop_border=0 if stereo else crop_border, lpips=lp)   # stereo-sr/test.py:139-140: no crop
            for n in range(nb):
                for v in range(per):
                    k = v * nb + n
                    for key in res:
                        res[key].append(float(m[key][k]))
                    if stereo:
                        line = "img:%-15s - PSNR: %.6f dB; SSIM: %.6f." % (names[v][n], m["psnr"][k], m["ssim"][k])
                    else:
                        line = ("img%3d:%-15s - PSNR: %.6f dB; SSIM: %.6f; PSNR_Y: %.6f dB; SSIM_Y: %.6f." %
                                (idx[n], names[v][n], m["psnr"][k], m["ssim"][k], m["psnr_y"][k], m["ssim_y"][k]))
                    log(line if lp is None else _with_lpips(line, m["lpips"][k]))
        if a.out:
            imgs = P.metrics.tensor2img_batch(views(out))
            lqi = P.metrics.tensor2img_batch(views(LQ))
            gti = P.metrics.tensor2img_batch(views(GT)) if GT is not None else None
            for n in range(nb):
                for v in range(per):
                    k = v * nb + n
                    save_img(imgs[k], os.path.join(a.out, names[v][n] + ".png"))
                    save_img(lqi[k], os.path.join(a.out, names[v][n] + "_LQ.png"))
                    if gti is not None:
                        save_img(gti[k], os.path.join(a.out, names[v][n] + "_HQ.png"))
    summary = None
    if res["psnr"] or (world > 1 and (gts is not None or a.task == "inpainting")):
        summary = P.metrics.reduce_metrics({k: np.asarray(v, dtype=np.float64) for k, v in res.items()})
    if rank == 0 and summary is not None:
        log("----Average PSNR/SSIM results for %s----\n\tPSNR: %.6f dB; SSIM: %.6f\n" %
            (os.path.basename(os.path.normpath(a.gt if a.task == "inpainting" or from_gt else a.lq)), summary["psnr"], summary["ssim"]))
        if not stereo:
            log("----Y channel, average PSNR/SSIM----\n\tPSNR_Y: %.6f dB; SSIM_Y: %.6f\n" % (summary["psnr_y"], summary["ssim_y"]))
        if "lpips" in summary:
            log("----average LPIPS\t: %.6f\n" % summary["lpips"])
    if rank == 0 and times:
        log("average test time per image: %.4f s (rank 0, %d images over %d rank(s))" % (float(np.mean(times)), n_items, world))
    return summary


def main(argv=None, on_batch=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--task", default=None, choices=["denoising", "sisr", "inpainting", "stereo-sr"],
                    help="denoising: the denoising-sde loop (clean --gt folder + --sigma, DenoisingSDE, "
                    "reverse_ode from the optimal timestep; PSNR / SSIM; LPIPS computed when --lpips-weights is given).  sisr: --lq is the low-resolution "
                    "folder (or --lq-from-gt), bicubic upscale by --scale on the device, then the LQ / GT loop with the reverse-SDE sampler.  inpainting: --gt + --mask-root, "
                    "mask_to with the image index as mask id.  stereo-sr: --lq holds L / R files paired in sorted order, x4 upscale per view, the stereo "
                    "ConditionalNAFNet (--naf-*) or, with --model unet, the stereo ConditionalUNet.  Absent: the LQ / GT loop")
    ap.add_argument("--lq", default=None, help="degraded images (required unless --task denoising / inpainting)")
    ap.add_argument("--gt", default=None)
    ap.add_argument("--lq-from-gt", action="store_true", help="--task sisr without --lq: every --gt image is cropped to a multiple of --scale (modcrop) and "
                    "its low-resolution image is made on the device by imresize(GT, 1 / scale), the MATLAB-style antialiased cubic resize of LQGT_dataset")
    ap.add_argument("--mask-root", default=None, help="--task inpainting: folder of the '%%06d.png' keep-masks (opt['degradation']['mask_root'])")
    ap.add_argument("--wide-rows", action="store_true", help="--task stereo-sr: set_wide_rows(), views wider than the SCAM strip kernels hold")
    ap.add_argument("--sigma", type=float, default=15, help="--task denoising: opt['degradation']['sigma'] (/ 255 when > 1)")
    ap.add_argument("--arch", default="nafnet", choices=["nafnet", "unet"], help="--task denoising: denoising_sde.ConditionalNAFNet (refusion.yml) "
                    "or denoising_sde.ConditionalUNet (ir-sde.yml; --nf / --depth)")
    ap.add_argument("--naf-width", type=int, default=64)
    ap.add_argument("--naf-enc", default="1,1,1,28")
    ap.add_argument("--naf-mid", type=int, default=1)
    ap.add_argument("--naf-dec", default="1,1,1,1")
    ap.add_argument("--weights", required=True, help="reference checkpoint (state_dict .pth, optional 'module.' prefixes)")
    ap.add_argument("--lpips-weights", nargs="+", default=None, metavar="FILE",
                    help="LPIPS (lpips.LPIPS(net='alex'), test.py:74) for every task that has a GT: one saved state_dict of it, or the two published files "
                    "(torchvision's AlexNet checkpoint and lpips' alex.pth).  Adds `LPIPS: x` to the per-image lines and the `average LPIPS` line; absent: not computed")
    ap.add_argument("--out", default=None, help="results folder: <name>.png, <name>_LQ.png, <name>_HQ.png as test.py:118-128")
    ap.add_argument("--model", default=None, choices=["unet", "nafnet"], help="default unet; --task stereo-sr: default nafnet (the stereo ConditionalNAFNet, --naf-*)")
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--max-sigma", type=float, default=10)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--schedule", default="cosine")
    ap.add_argument("--eps", type=float, default=0.005)
    ap.add_argument("--mode", default=None, choices=["sde", "ode", "posterior"], help="default posterior; --task sisr / inpainting / stereo-sr: default sde "
                    "(their denoising_model.test runs reverse_sde)")
    ap.add_argument("--crop-border", type=int, default=None, help="opt['crop_border']; unset / 0 falls back to --scale exactly as test.py:134 does")
    ap.add_argument("--scale", type=int, default=4, help="opt['degradation']['scale'] (deraining options/test/ir-sde.yml:20 sets 4 and no crop_border, "
                    "so the published Rain100H PSNR / SSIM are computed on images cropped by 4 px)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "bf16_act", "fp16", "fp16_act"],
                    help="compute mode (set_compute_dtype): bf16 / fp16 = 16-bit MFMA operands with fp32 storage; bf16_act = bf16 operands + bf16 activation "
                    "storage, for both UNets (deraining --arch unet and --task denoising --arch unet, whose bottleneck attention then runs on the bf16 MFMA); "
                    "the NAFNets take fp32 / bf16 / fp16, and the image-space ones fp16_act (fp16 operands + fp16 activation storage)")
    a = ap.parse_args(argv)
    if a.task is None and a.lq is None:
        ap.error("the following arguments are required: --lq")
    if a.task == "denoising" and a.gt is None:
        ap.error("--task denoising needs the clean images: --gt")
    if a.lq_from_gt and a.task != "sisr":
        ap.error("--lq-from-gt goes with --task sisr only")
    if a.lq_from_gt and a.lq is not None:
        ap.error("--lq-from-gt makes the low-resolution images from --gt: --lq must be absent")
    if a.lq_from_gt and a.gt is None:
        ap.error("--lq-from-gt needs the high-resolution images: --gt")
    if a.task in ("sisr", "stereo-sr") and a.lq is None and not a.lq_from_gt:
        ap.error("--task %s needs the low-resolution images: --lq" % a.task)
    if a.task == "inpainting" and (a.gt is None or a.mask_root is None):
        ap.error("--task inpainting needs the clean images and the masks: --gt, --mask-root")
    if a.task == "stereo-sr" and a.mode == "posterior":
        ap.error("--task stereo-sr samples with --mode sde or ode (stereo-sr/models/denoising_model.py: reverse_sde, or reverse_ode with perform_ode)")
    if a.mode is None:
        a.mode = "sde" if a.task in DEGRADED_TASKS else "posterior"
    if a.model is None:
        a.model = "nafnet" if a.task == "stereo-sr" else "unet"
    crop_border = a.crop_border if a.crop_border else a.scale   # test.py:134: `opt["crop_border"] if opt["crop_border"] else scale`

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
        return subprocess.call(cmd)

    import numpy as np
    import torch
    import torch.distributed as dist
    import image_restoration_sde_amd as P

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        sys.exit("eval_folder.py: --gpus %d does not match WORLD_SIZE=%d" % (a.gpus, world))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    if a.task == "denoising":
        summary = run_denoising(a, P, torch, np, dev, world, rank, (lambda *s: print(*s, flush=True)))
        if world > 1:
            dist.destroy_process_group()
        return summary
    if a.task in DEGRADED_TASKS:
        summary = run_degraded(a, P, torch, np, dev, world, rank, (lambda *s: print(*s, flush=True)), crop_border, on_batch)
        if world > 1:
            dist.destroy_process_group()
        return summary
    pairs = pair_paths(a.lq, a.gt)
    lo, hi = P.shard_bounds(len(pairs), world, rank)   # this rank's images; noise keyed by the global index
    model = build_model(a, P, torch).to(dev).eval()
    if a.dtype != "fp32":
        model.set_compute_dtype(a.dtype)
    sde = P.IRSDE(max_sigma=a.max_sigma, T=a.T, schedule=a.schedule, eps=a.eps, device=dev)
    sde.set_model(model)
    sde.seed = a.seed

    mine = list(range(lo, hi))
    lq_np = [read_img(pairs[i][0]) for i in mine]
    sizes = [x.shape for x in lq_np]
    res = {"psnr": [], "ssim": [], "psnr_y": [], "ssim_y": []}
    lp = load_lpips(a, P) if a.gt is not None else None
    if lp is not None:
        res["lpips"] = []
    times = []
    log = (lambda *s: print(*s, flush=True))
    for grp in batches_of_equal_size(mine, sizes, a.batch):
        LQ = torch.from_numpy(np.stack([lq_np[j] for j in grp]))
        noise = torch.stack([torch.randn(LQ.shape[1:], generator=torch.Generator().manual_seed(a.seed * 1000003 + mine[j]))
                             for j in grp])
        noisy_state = LQ + noise * sde.max_sigma           # IRSDE.noise_state (sde_utils.py:360-361), on the CPU as test.py:104
        sde.image_offset = mine[grp[0]]
        sde.set_mu(LQ.to(dev))
        torch.cuda.synchronize()
        tic = time.time()
        fn = {"sde": sde.reverse_sde, "ode": sde.reverse_ode, "posterior": sde.reverse_posterior}[a.mode]
        out = fn(noisy_state.to(dev))
        torch.cuda.synchronize()
        times.append((time.time() - tic) / len(grp))
        names = [os.path.splitext(os.path.basename(pairs[mine[j]][1] or pairs[mine[j]][0]))[0] for j in grp]
        GT = None
        if a.gt is not None:
            GT = torch.from_numpy(np.stack([read_img(pairs[mine[j]][1]) for j in grp])).to(dev)
            m = P.metrics.evaluate_batch(out, GT, crop_border=crop_border, lpips=lp)
            for k in res:
                res[k].extend(m[k].tolist())
            for n, name in enumerate(names):
                line = ("img%3d:%-15s - PSNR: %.6f dB; SSIM: %.6f; PSNR_Y: %.6f dB; SSIM_Y: %.6f." %
                        (mine[grp[n]], name, m["psnr"][n], m["ssim"][n], m["psnr_y"][n], m["ssim_y"][n]))
                log(line if lp is None else _with_lpips(line, m["lpips"][n]))
        if a.out:
            imgs = P.metrics.tensor2img_batch(out)
            lqi = P.metrics.tensor2img_batch(LQ.to(dev))
            gti = P.metrics.tensor2img_batch(GT) if GT is not None else None
            for n, name in enumerate(names):
                save_img(imgs[n], os.path.join(a.out, name + ".png"))
                save_img(lqi[n], os.path.join(a.out, name + "_LQ.png"))
                if gti is not None:
                    save_img(gti[n], os.path.join(a.out, name + "_HQ.png"))
    summary = None
    if a.gt is not None:
        local = {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}
        if world > 1 or len(local["psnr"]):
            summary = P.metrics.reduce_metrics(local)
    if rank == 0 and summary is not None:
        log("----Average PSNR/SSIM results for %s----\n\tPSNR: %.6f dB; SSIM: %.6f\n" % (os.path.basename(os.path.normpath(a.lq)), summary["psnr"], summary["ssim"]))
        log("----Y channel, average PSNR/SSIM----\n\tPSNR_Y: %.6f dB; SSIM_Y: %.6f\n" % (summary["psnr_y"], summary["ssim_y"]))
        if "lpips" in summary:
            log("----average LPIPS\t: %.6f\n" % summary["lpips"])
    if rank == 0 and times:
        log("average test time per image: %.4f s (rank 0, %d images over %d rank(s))" % (float(np.mean(times)), len(pairs), world))
    if world > 1:
        dist.destroy_process_group()
    return summary


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
