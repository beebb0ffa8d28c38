"""denoising-sde ConditionalNAFNet (IRSDE_FLAG_NAF_UNCOND) on the GPU (run with -m gpu on an MI355X): the unconditional Refusion
network against the real reference's goldens (tests/golden/dsde_naf.npz) and the float64 restatement (tests/dsde_naf_oracle.py),
the DenoisingSDE samplers on it, and the task's public surface (create_model / add_noise / tools/eval_folder.py --task denoising).

Bars are the sibling rows' of tests/test_gpu_parity.py: one network evaluation vs the reference golden 1e-4, every tap vs the
float64 restatement 5e-5, a sampler vs the reference golden 2e-3 (all relative to max |ref|); batch vs single images 5e-5
(tests/test_gpu_fullres.py: test_nafnet_batch8_512_equals_single_images); fp16 operand mode vs the fp32 engine 3e-3
(test_naf_chain_vs_per_layer_path)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O
import dsde_naf_oracle as DN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NETS = {}


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def net(name, flags=0, cfg=None, cond=False):
    """The unconditional network with the synthetic weights (cond=True: the deraining class with `oracle.naf_synth_params`)."""
    key = (name, flags, cond)
    if key not in _NETS:
        cfg = cfg or DN.CFGS[name]
        kw = dict(img_channel=3, width=cfg["width"], enc_blk_nums=list(cfg["enc_blk_nums"]), middle_blk_num=cfg["middle_blk_num"],
                  dec_blk_nums=list(cfg["dec_blk_nums"]))
        params = O.naf_synth_params(seed=0, img_channel=3, **cfg) if cond else DN.synth_params(seed=0, **cfg)
        m = (P.ConditionalNAFNet if cond else P.denoising_sde.ConditionalNAFNet)(**kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m.engine_flags = flags
        _NETS[key] = (m.to(DEV).eval(), params, cfg)
    return _NETS[key]


def describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 18)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine(torch.device(DEV)).h, B, H, W, buf, len(buf)))
    return buf.value.decode()


@pytest.mark.parametrize("tag", sorted(DN.FORWARD))
def test_forward_vs_reference_golden(golden, tag):
    """forward(x, time) at t in {1, 7, T_opt}; both shapes are zero-padded (22 x 19 -> 24 x 20: ragged on both axes, null cond)."""
    g = golden.dsde_naf
    name, B, H, W = DN.FORWARD[tag]
    m, _, _ = net(name)
    _, noisy = DN.inputs(B, H, W, 25 if name == "w32_e12" else 15)
    x = torch.from_numpy(noisy).to(DEV)
    for t in g[tag + "/ts"]:
        for tt in (int(t), float(t)):
            e = relerr(m(x, tt).cpu().numpy(), g[tag + "/t%d" % t])
            print("%s t=%d: %.3g" % (tag, t, e))
            assert e < 1e-4, (tag, int(t), e)


def test_layers_vs_restatement_and_per_sample_timesteps():
    m, params, cfg = net("w32_e12", flags=_lib.FLAG_KEEP_ACTIVATIONS)
    B, H, W = 2, 22, 19
    _, noisy = DN.inputs(B, H, W, 25)
    taps = {}
    ref = DN.forward(params, noisy, 7, cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"], taps=taps)
    x = torch.from_numpy(noisy).to(DEV)
    y = m(x, 7).cpu().numpy()
    bad = {}
    for name, want in taps.items():
        got = m.debug_tap(name).numpy()
        assert got.shape == want.shape, name
        e = relerr(got, want)
        if not e < 5e-5:
            bad[name] = e
    assert not bad, bad
    assert "intro" in taps and taps["intro"].shape == (B, 32, 24, 20)
    assert relerr(y, ref) < 5e-5
    y2 = m(x, torch.tensor([5, 60])).cpu().numpy()
    r2 = DN.forward(params, noisy, np.array([5, 60]), cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"])
    assert relerr(y2, r2) < 5e-5
    assert relerr(y2[0], y[0]) > 1e-4   # the time really enters


@pytest.mark.parametrize("tag", sorted(DN.SAMPLER))
def test_sampler_vs_reference_golden(golden, tag):
    """DenoisingSDE.reverse_ode (and reverse_sde with injected noise on the small case) from the optimal timestep vs the reference;
    refusion_1x32x32 is the shipped config's schedule: DenoisingSDE(70, T = 1000), sigma 15 -> 158 network evaluations."""
    g = golden.dsde_naf
    name, B, H, W, max_sigma, T, sigma = DN.SAMPLER[tag]
    m, _, _ = net(name)
    k = tag + "/sampler"
    noisy = g[k + "/noisy"]
    sde = P.DenoisingSDE(max_sigma=max_sigma, T=T, device=DEV)
    sde.set_model(m)
    Topt = sde.get_optimal_timestep(sigma)
    assert int(Topt) == int(g[k + "/T"])
    x = torch.from_numpy(noisy).to(DEV)
    modes = [("ode", sde.reverse_ode)]
    if k + "/sde" in g.files:
        sde.injected_noise = torch.from_numpy(O.synth_noise(7, T, noisy.shape)).to(DEV)
        modes.append(("sde", sde.reverse_sde))
    for mode, fn in modes:
        got = fn(x, T=Topt).cpu().numpy()
        e = relerr(got, g[k + "/" + mode])
        print("%s %s T_opt=%d: %.3g" % (tag, mode, int(Topt), e))
        assert e < 2e-3, (tag, mode, e)
        sde.use_graph = False
        assert np.array_equal(fn(x, T=Topt).cpu().numpy(), got)   # graph replay == eager launches
        sde.use_graph = True


def test_batch_of_four_equals_single_images():
    m, _, _ = net("refusion")
    _, noisy = DN.inputs(4, 120, 88, 15, seed=79)
    x = torch.from_numpy(noisy).to(DEV)
    yb = m(x, 60).cpu().numpy()
    scale = np.abs(yb).max()
    worst = 0.0
    for b in range(4):
        worst = max(worst, float(np.abs(m(x[b:b + 1], 60).cpu().numpy() - yb[b:b + 1]).max() / scale))
    print("unconditional NAFNet B=4 vs 4 x B=1 at 120x88: %.3g" % worst)
    assert worst < 5e-5
    assert relerr(yb[0], yb[3]) > 1e-2


def test_fp16_sampler_and_chain():
    """fp16 operand mode: the 512-channel levels on an 8 x 8 map run as the fused NAFBlock chain exactly where the conditional network's plan
    runs it, and the sampler stays within the mode's bar of the fp32 engine."""
    cfg = dict(width=64, enc_blk_nums=(1, 1, 1, 3), middle_blk_num=1, dec_blk_nums=(1, 1, 1, 1))
    B, H, W = 2, 64, 64
    outs, chains = {}, {}
    _, noisy = DN.inputs(B, H, W, 25)
    x = torch.from_numpy(noisy).to(DEV)
    for tag, flags in (("fp32", 0), ("fp16", _lib.FLAG_FP16)):
        m, _, _ = net("w64_e1113", flags=flags, cfg=cfg)
        chains[tag] = describe(m, B, H, W).count("naf_chain(fp16)")
        sde = P.DenoisingSDE(max_sigma=50, T=100, device=DEV)
        sde.set_model(m)
        outs[tag] = sde.reverse_ode(x, T=sde.get_optimal_timestep(25)).cpu().numpy()
    mc, _, _ = net("w64_e1113", flags=_lib.FLAG_FP16, cfg=cfg, cond=True)
    n_cond = describe(mc, B, H, W).count("naf_chain(fp16)")
    assert chains["fp32"] == 0 and chains["fp16"] == n_cond == 2, (chains, n_cond)
    e = relerr(outs["fp16"], outs["fp32"])
    print("unconditional NAFNet fp16 reverse_ode vs fp32: %.3g" % e)
    assert np.isfinite(outs["fp16"]).all() and 0 < e < 3e-3
    m16, _, _ = net("w64_e1113", flags=_lib.FLAG_FP16, cfg=cfg)
    m32, _, _ = net("w64_e1113", flags=0, cfg=cfg)
    ef = relerr(m16(x, 29).cpu().numpy(), m32(x, 29).cpu().numpy())
    print("unconditional NAFNet fp16 forward vs fp32: %.3g" % ef)
    assert ef < 3e-3


@pytest.mark.parametrize("flags", [0, _lib.FLAG_FP16])
def test_plan_is_the_conditional_networks_kernel_list(flags):
    """Kernel reuse pinned: the unconditional refusion engine's plan lists the conditional one's rows in the same order; only the intro row
    may differ, and only in its K / FLOPs (both intros issue one 32-wide K chunk per row tap -- 3 x 4 resp. 3 x 8 real values -- so the printed
    rows are in fact equal).  The algorithmic FLOP account (irsde_work_model) differs by exactly the intro's missing half:
    9 x img_channel instead of 9 x 2 img_channel MACs per output value."""
    mu, _, _ = net("refusion", flags=flags)
    mc, _, _ = net("refusion", flags=flags, cond=True)
    ru, rc = describe(mu, 2, 64, 64).splitlines(), describe(mc, 2, 64, 64).splitlines()
    assert len(ru) == len(rc) >= 40   # (fp16: the 28-block level is one chain row)
    diff = [i for i in range(len(ru)) if ru[i] != rc[i]]
    assert diff in ([], [1]), [(ru[i], rc[i]) for i in diff[:4]]    # row 0: input prep, row 1: intro
    assert "conv" in ru[1] and "Cout=64" in ru[1], ru[1]
    strip = lambda s: re.sub(r"\b(flops|exec|Cin|K)=\S+", "", s)
    assert strip(ru[1]) == strip(rc[1]), (ru[1], rc[1])
    wu, wc = (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
    _lib.check(_lib.lib().irsde_work_model(mu.engine().h, 2, 64, 64, wu))
    _lib.check(_lib.lib().irsde_work_model(mc.engine().h, 2, 64, 64, wc))
    assert abs((wc[0] - wu[0]) - 2.0 * 2 * 64 * 64 * 64 * 9.0 * 3) < 1.0, (wu[0], wc[0])   # 2 B Hp Wp Cout 9 img_channel
    if flags:
        assert sum("naf_chain(fp16)" in r for r in ru) == sum("naf_chain(fp16)" in r for r in rc) > 0


def test_cabi_refusals():
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    mu_, _, _ = net("w32_e12")
    mc, _, _ = net("w32_e12", cond=True)
    sde = P.DenoisingSDE(max_sigma=50, T=100, device=DEV)
    x = torch.from_numpy(DN.inputs(1, 16, 16, 25)[1]).to(DEV)
    out = torch.empty_like(x)
    for m in (mu_, mc):
        _lib.check(L.irsde_set_schedule(m.engine(torch.device(DEV)).h, sde.T, ctypes.c_void_p(sde._coef.data_ptr())))
    hu, hc = mu_.engine().h, mc.engine().h
    msg = b"DenoisingSDE modes (3,4) go with the unconditional network and vice versa"
    for mode in (0, 1, 2):       # the IR-SDE modes need mu: refused on the unconditional engine, with or without one
        for mu in (None, p(x)):
            assert L.irsde_sample(hu, mode, p(x), mu, None, 0, 0, 1, 16, 16, 3, 0, p(out), None, 0) == -1
            assert msg in L.irsde_last_error()
    for mode in (3, 4):
        assert L.irsde_sample(hu, mode, p(x), None, None, 0, 0, 1, 16, 16, 3, 0, p(out), None, 0) == 0   # mu == NULL allowed
        assert L.irsde_sample(hc, mode, p(x), p(x), None, 0, 0, 1, 16, 16, 3, 0, p(out), None, 0) == -1    # unchanged message
        assert msg in L.irsde_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert L.irsde_sample(hc, 1, p(x), None, None, 0, 0, 1, 16, 16, 3, 0, p(out), None, 0) == -1   # the conditional engine needs mu
    assert b"null argument" in L.irsde_last_error()
    t = (ctypes.c_int64 * 1)(5)
    assert L.irsde_unet_forward(hc, p(x), None, t, 1, 1, 16, 16, p(out), None) == -1                # ... and cond
    assert b"null argument" in L.irsde_last_error()
    assert L.irsde_unet_forward(hu, p(x), None, t, 1, 1, 16, 16, p(out), None) == 0
    torch.cuda.synchronize()

    def naf(flags):
        cfg = _lib.NafConfig()
        cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, 32, 1, 2, 2
        for i in range(2):
            cfg.enc_blk_nums[i] = cfg.dec_blk_nums[i] = 1
        cfg.device, cfg.flags = 0, flags
        h = ctypes.c_void_p()
        rc = L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            L.irsde_destroy(h)
        return rc

    for f in (_lib.FLAG_NAF_STEREO, _lib.FLAG_NAF_LENS, _lib.FLAG_NAF_INTRO_SKIP):
        assert naf(_lib.FLAG_NAF_UNCOND | f) == -1
        assert b"IRSDE_FLAG_NAF_UNCOND cannot be combined" in L.irsde_last_error()


def test_add_noise_is_the_keyed_philox_draw():
    clean = torch.from_numpy(DN.inputs(3, 17, 13, 25)[0]).to(DEV)
    seed = 0x1234567890ABCDEF
    y = P.denoising_sde.add_noise(clean, 25, seed=seed, image_offset=5)
    z = ((y - clean) / (25 / 255)).cpu().numpy().reshape(3, -1)
    for b in range(3):
        np.testing.assert_allclose(z[b], O.device_normal(seed, 0, 5 + b, 3 * 17 * 13), rtol=0, atol=1e-4)
    # image 6 as "image 1 of a batch starting at 5" == "image 0 of a batch starting at 6": no dependence on batching / rank count
    assert torch.equal(P.denoising_sde.add_noise(clean[1:2], 25, seed=seed, image_offset=6), y[1:2])
    assert torch.equal(P.denoising_sde.add_noise(clean[1], 25, seed=seed, image_offset=6), y[1])
    cpu = P.denoising_sde.add_noise(clean.cpu(), 25, seed=seed, image_offset=5)
    assert cpu.device.type == "cpu" and torch.equal(cpu, y.cpu())
    small = P.denoising_sde.add_noise(clean, 0.5, seed=seed, image_offset=5)      # sigma <= 1 is taken as is
    assert relerr(((small - clean) / 0.5).cpu().numpy(), z.reshape(clean.shape)) < 1e-4


def test_wrapper_end_to_end():
    cfg = DN.CFGS["w32_e12"]
    opt = {"model": "denoising", "network_G": {"which_model_G": "ConditionalNAFNet", "setting": dict(
        width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1])}}
    mdl = P.create_model(opt, task="denoising-sde")
    assert type(mdl.model) is P.denoising_sde.ConditionalNAFNet
    mdl.model.load_state_dict({k: torch.from_numpy(v) for k, v in DN.synth_params(seed=0, **cfg).items()}, strict=True)
    sde = P.DenoisingSDE(max_sigma=50, T=100, device=mdl.device)
    sde.set_model(mdl.model)
    GT = torch.from_numpy(DN.inputs(2, 22, 19, 25)[0])
    outs = {}
    for seed in (3, 3, 4):
        LQ = P.denoising_sde.add_noise(GT, 25, seed=seed)
        mdl.feed_data(LQ, GT)
        mdl.test(sde, sigma=25, save_states=False)
        vis = mdl.get_current_visuals()
        assert list(vis) == ["Input", "Output", "GT"] and vis["Output"].shape == (3, 22, 19)
        assert torch.equal(vis["Input"], LQ[0]) and torch.equal(vis["GT"], GT[0])
        assert torch.isfinite(mdl.output).all() and mdl.output.shape == (2, 3, 22, 19)
        outs.setdefault(seed, []).append(mdl.output.cpu().numpy())
    assert np.array_equal(outs[3][0], outs[3][1])
    assert relerr(outs[4][0], outs[3][0]) > 1e-3
    # the wrapper's result is the sampler's: reverse_ode from the optimal timestep
    want = sde.reverse_ode(P.denoising_sde.add_noise(GT, 25, seed=4).to(mdl.device), T=sde.get_optimal_timestep(25)).cpu().numpy()
    assert np.array_equal(outs[4][0], want)


def test_eval_folder_denoising_task(tmp_path):
    """tools/eval_folder.py --task denoising (the loop of denoising-sde/test.py:91-142) on three tiny PNGs with synthetic weights."""
    from PIL import Image
    rs = np.random.RandomState(2)
    gt_dir, out_dir = tmp_path / "GT", tmp_path / "res"
    gt_dir.mkdir()
    names = []
    for i, (h, w) in enumerate([(24, 20), (24, 20), (22, 19)]):
        base = rs.randint(0, 256, size=(h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR))
        Image.fromarray(img).save(str(gt_dir / ("im%d.png" % i)))
        names.append("im%d" % i)
    cfg = DN.CFGS["w32_e12"]
    ckpt = tmp_path / "G.pth"
    torch.save({"module." + k: torch.from_numpy(v) for k, v in DN.synth_params(seed=0, **cfg).items()}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--task", "denoising", "--gt", str(gt_dir), "--sigma", "25",
           "--max-sigma", "50", "--T", "100", "--weights", str(ckpt), "--arch", "nafnet", "--naf-width", "32", "--naf-enc", "1,2",
           "--naf-dec", "1,1", "--out", str(out_dir), "--batch", "2", "--seed", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for n in names:
        for suffix in ("", "_noisy", "_clean"):
            assert (out_dir / (n + suffix + ".png")).exists(), (n, suffix)
        assert np.array_equal(np.asarray(Image.open(str(out_dir / (n + "_clean.png")))), np.asarray(Image.open(str(gt_dir / (n + ".png")))))
        assert not np.array_equal(np.asarray(Image.open(str(out_dir / (n + "_noisy.png")))), np.asarray(Image.open(str(gt_dir / (n + ".png")))))
        assert re.search(r"img\s*\d+:%s\s+- PSNR: [-\d.]+ dB; SSIM: [-\d.]+\." % n, r.stdout), r.stdout
    # the printed PSNR of an image is the reference metric of the written restored PNG against the clean one
    o = np.asarray(Image.open(str(out_dir / "im2.png")), dtype=np.float64)[..., ::-1]
    gtv = np.asarray(Image.open(str(gt_dir / "im2.png")), dtype=np.float64)[..., ::-1]
    got = float(re.search(r"im2\s+- PSNR: ([-\d.]+) dB", r.stdout).group(1))
    assert abs(got - O.calculate_psnr(o, gtv)) < 1e-5
    assert "Average PSNR/SSIM" in r.stdout
