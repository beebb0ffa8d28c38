"""Generate tests/golden/*.npz from the REAL reference code (test infrastructure only).

Runs in the build container only (needs /root/reference, which is read-only and absent on
the GPU box).  It imports the reference's `IRSDE` (codes/utils/sde_utils.py) and
`ConditionalUNet` (codes/config/deraining/models/modules/DenoisingUNet_arch.py) on CPU,
feeds them the deterministic synthetic weights / inputs / injected noise from
`oracle.irsde_oracle`, and stores the reference's outputs as small fixtures.

Import recipe: stub `torchvision.utils`, load sde_utils.py by path, put
codes/config/deraining on sys.path for `models.modules`.

Usage:  python oracle/gen_golden.py [--ref /root/reference] [--only NAME]
"""
import argparse
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import irsde_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def load_reference(ref_root):
    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")
    tvu.save_image = lambda *a, **k: None
    tv.utils = tvu
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.utils", tvu)
    spec = importlib.util.spec_from_file_location(
        "ref_sde_utils", os.path.join(ref_root, "codes/utils/sde_utils.py"))
    sde_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sde_utils)
    sys.path.insert(0, os.path.join(ref_root, "codes/config/deraining"))
    from models.modules.DenoisingUNet_arch import ConditionalUNet
    return sde_utils, ConditionalUNet


def load_reference_again(ref_root):
    """After gen_dsde / gen_latent replaced `models.modules` with another task's package: drop it and re-import the
    deraining one."""
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    while os.path.join(ref_root, "codes/config/denoising-sde") in sys.path:
        sys.path.remove(os.path.join(ref_root, "codes/config/denoising-sde"))
    return load_reference(ref_root)


class InjectedIRSDE:
    """Mixin factory: reference IRSDE with torch.randn_like replaced by a pre-drawn tensor
    (the reference has no hook; we override the two methods that draw:
    dispersion sde_utils.py:181-182 and reverse_posterior_step :219-223)."""

    @staticmethod
    def make(sde_utils):
        class _Inj(sde_utils.IRSDE):
            noise = None
            cur_t = None

            def dispersion(self, x, t):
                import math
                z = self.noise[t]
                return self.sigmas[t] * (z * math.sqrt(self.dt)).to(self.device)

            def reverse_posterior_step(self, xt, noise, t):
                x0 = self.get_init_state_from_noise(xt, noise, t)
                mean = self.reverse_optimum_step(xt, x0, t)
                std = self.reverse_optimum_std(t)
                return mean + std * self.noise[t]
        return _Inj


def build_ref_net(ConditionalUNet, params, nf, depth):
    net = ConditionalUNet(in_nc=3, out_nc=3, nf=nf, depth=depth).eval()
    sd = net.state_dict()
    shapes = O.unet_param_shapes(3, 3, nf, depth)
    assert set(sd.keys()) == set(shapes.keys()), (set(sd) ^ set(shapes))
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, v.shape, shapes[k])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return net


def gen_schedule(sde_utils):
    out = {}
    for tag, (ms, T, sched, eps) in {
        "s10_T100": (10, 100, "cosine", 0.005),
        "s50_T100": (50, 100, "cosine", 0.005),
        "s50_T200": (50, 200, "cosine", 0.005),
        "s25_T100_lin": (25, 100, "linear", 0.005),
        "s0p1_T50_const": (0.1, 50, "constant", 0.01),
    }.items():
        sde = sde_utils.IRSDE(max_sigma=ms, T=T, schedule=sched, eps=eps, device="cpu")
        out[tag + "/cfg"] = np.array([ms, T, eps], dtype=np.float64)
        out[tag + "/sched"] = np.array(sched)
        out[tag + "/dt"] = np.float32(sde.dt.item())
        for n in ("thetas", "sigmas", "thetas_cumsum", "sigma_bars"):
            out[tag + "/" + n] = getattr(sde, n).numpy()
        std = np.zeros(T + 1, dtype=np.float32)
        t1 = np.zeros(T + 1, dtype=np.float32)
        t2 = np.zeros(T + 1, dtype=np.float32)
        g = np.zeros(T + 1, dtype=np.float32)
        sde.set_mu(torch.zeros(1))
        for t in range(1, T + 1):
            std[t] = sde.reverse_optimum_std(t).item()
            # term1/term2 via reverse_optimum_step on basis inputs (mu=0)
            t1[t] = sde.reverse_optimum_step(torch.ones(1), torch.zeros(1), t).item()
            t2[t] = sde.reverse_optimum_step(torch.zeros(1), torch.ones(1), t).item()
            g[t] = sde.get_init_state_from_noise(torch.ones(1), torch.zeros(1), t).item()
        out[tag + "/post_std"] = std
        out[tag + "/post_term1"] = t1
        out[tag + "/post_term2"] = t2
        out[tag + "/x0_gain"] = g
    np.savez_compressed(os.path.join(GOLD, "schedule.npz"), **out)
    print("schedule.npz", len(out))


def gen_forward(sde_utils, ConditionalUNet):
    """Single-forward goldens (nf=64, depth=4 = the deraining config) + a small net."""
    out = {}
    cases = {
        # tag: (nf, depth, B, H, W, ts)
        "nf64d4_1x64x64": (64, 4, 1, 64, 64, [1, 50, 100]),
        "nf64d4_2x40x56": (64, 4, 2, 40, 56, [37]),      # reflect-pad path (40->48, 56->64)
        "nf32d2_2x24x20": (32, 2, 2, 24, 20, [3, 77]),    # small net used by quick tests
    }
    for tag, (nf, depth, B, H, W, ts) in cases.items():
        params = O.synth_params(seed=0, nf=nf, depth=depth)
        net = build_ref_net(ConditionalUNet, params, nf, depth)
        lq, xT = O.synth_inputs(1234, B, H, W)
        out[tag + "/cfg"] = np.array([nf, depth, B, H, W], dtype=np.int64)
        out[tag + "/ts"] = np.array(ts, dtype=np.int64)
        for t in ts:
            with torch.no_grad():
                y = net(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
            out[tag + "/t%d" % t] = y
            print(tag, t, float(np.abs(y).max()))
        if tag == "nf32d2_2x24x20":
            # training-style per-sample timesteps [B] (denoising_model.py:135)
            tt = torch.tensor([5, 60])
            with torch.no_grad():
                y = net(torch.from_numpy(xT), torch.from_numpy(lq), tt).numpy()
            out[tag + "/tvec"] = y
    np.savez_compressed(os.path.join(GOLD, "forward.npz"), **out)
    print("forward.npz")


def gen_forward_attn(sde_utils, ConditionalUNet):
    """r05: forwards of the REAL reference with attention-sensitive weights (O.attn_sensitive_params: to_out.0.weight of every LinearAttention block scaled by the
    pixel count of its level, so that softmax / context / output product carry the block instead of to_out's bias), plus the input and output of two
    Residual(PreNorm(LinearAttention)) modules captured by forward hooks: pins the oracle's attention restatement and the engine's attention kernels to the reference."""
    out = {}
    cases = {"nf64d4_1x64x64": (64, 4, 1, 64, 64, 50), "nf64d4_2x40x56": (64, 4, 2, 40, 56, 37), "nf64d4_1x32x32": (64, 4, 1, 32, 32, 77)}
    for tag, (nf, depth, B, H, W, t) in cases.items():
        params = O.attn_sensitive_params(O.synth_params(seed=0, nf=nf, depth=depth), H, W, depth)
        net = build_ref_net(ConditionalUNet, params, nf, depth)
        lq, xT = O.synth_inputs(1234, B, H, W)
        caught = {}

        def hook(name):
            def f(mod, inp, outp):
                caught[name + "/in"] = inp[0].detach().numpy().copy()
                caught[name + "/out"] = outp.detach().numpy().copy()
            return f
        hs = []
        if tag == "nf64d4_1x32x32":   # (the small case only: the fixtures stay small)
            hs = [net.downs[0][2].register_forward_hook(hook("downs.0.2")), net.downs[2][2].register_forward_hook(hook("downs.2.2")),
                  net.mid_attn.register_forward_hook(hook("mid_attn"))]
        with torch.no_grad():
            y = net(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
        for h in hs:
            h.remove()
        out[tag + "/cfg"] = np.array([nf, depth, B, H, W, t], dtype=np.int64)
        out[tag + "/y"] = y
        for k, v in caught.items():
            out[tag + "/" + k] = v
        print(tag, float(np.abs(y).max()), {k: v.shape for k, v in caught.items()})
    np.savez_compressed(os.path.join(GOLD, "forward_attn.npz"), **out)
    print("forward_attn.npz")


def gen_forward_attn256(sde_utils, ConditionalUNet):
    """r06 (VERDICT r05 weak #1a): the attention-sensitive forward of the REAL reference at the BENCHMARKED image size, 1x3x256x256 (N = 65 536 pixels at level 0:
    512 tiles of 128 pixels per image, the grid shape of the bench plan's fused LinearAttention kernels; `module_util.py:150-178`).  `sub3` sample of the output plus
    one full corner; its own file, so that forward_attn.npz (bit-reproduced by the r05 judge) is not regenerated."""
    out = {}
    nf, depth, B, H, W, t = 64, 4, 1, 256, 256, 50
    tag = "nf64d4_1x256x256"
    params = O.attn_sensitive_params(O.synth_params(seed=0, nf=nf, depth=depth), H, W, depth)
    net = build_ref_net(ConditionalUNet, params, nf, depth)
    lq, xT = O.synth_inputs(1234, B, H, W)
    with torch.no_grad():
        y = net(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
    out[tag + "/cfg"] = np.array([nf, depth, B, H, W, t], dtype=np.int64)
    out[tag + "/y_sub3"] = sub3(y)
    out[tag + "/y_corner"] = np.ascontiguousarray(y[:, :, -48:, -48:])
    out[tag + "/y_absmax"] = np.float64(np.abs(y).max())
    # the same inputs with the DEFAULT synthetic weights: how far the attention-sensitive scaling moves the output (the test asserts the fixture is sensitive)
    net0 = build_ref_net(ConditionalUNet, O.synth_params(seed=0, nf=nf, depth=depth), nf, depth)
    with torch.no_grad():
        y0 = net0(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
    out[tag + "/moved_by"] = np.float64(np.abs(y - y0).max() / np.abs(y).max())
    print(tag, float(np.abs(y).max()), "moved by", float(out[tag + "/moved_by"]))
    np.savez_compressed(os.path.join(GOLD, "forward_attn256.npz"), **out)
    print("forward_attn256.npz")


def gen_steps(sde_utils):
    """Teacher-forced single reverse steps (elementwise part only) for the 3 samplers."""
    Inj = InjectedIRSDE.make(sde_utils)
    out = {}
    rs = np.random.RandomState(99)
    shape = (2, 3, 8, 8)
    x = rs.standard_normal(shape).astype(np.float32)
    mu = rs.uniform(0, 1, shape).astype(np.float32)
    eps_hat = rs.standard_normal(shape).astype(np.float32)
    for tag, (ms, T) in {"s10_T100": (10, 100), "s50_T200": (50, 200)}.items():
        sde = Inj(max_sigma=ms, T=T, schedule="cosine", eps=0.005, device="cpu")
        z = O.synth_noise(5, T, shape)
        sde.noise = torch.from_numpy(z)
        sde.set_mu(torch.from_numpy(mu))
        out[tag + "/x"] = x
        out[tag + "/mu"] = mu
        out[tag + "/eps_hat"] = eps_hat
        for t in (1, 2, T // 2, T):
            xt = torch.from_numpy(x)
            n = torch.from_numpy(eps_hat)
            score = sde.get_score_from_noise(n, t)
            out[tag + "/sde_t%d" % t] = sde.reverse_sde_step(xt, score, t).numpy()
            out[tag + "/ode_t%d" % t] = sde.reverse_ode_step(xt, score, t).numpy()
            out[tag + "/post_t%d" % t] = sde.reverse_posterior_step(xt, n, t).numpy()
    np.savez_compressed(os.path.join(GOLD, "steps.npz"), **out)
    print("steps.npz")


def gen_sampler(sde_utils, ConditionalUNet, big=True):
    """End-to-end reverse samplers with injected noise."""
    Inj = InjectedIRSDE.make(sde_utils)
    out = {}
    cases = {
        # tag: (nf, depth, B, H, W, T, modes)
        "nf32d2_2x16x16_T20": (32, 2, 2, 16, 16, 20, ["sde", "ode", "posterior"]),
        "nf64d4_1x32x32_T100": (64, 4, 1, 32, 32, 100, ["sde", "ode", "posterior"]),
    }
    if big:
        # BASELINE.json configs[0]: the reference's own CPU-runnable case
        cases["nf64d4_1x128x128_T100"] = (64, 4, 1, 128, 128, 100, ["sde", "posterior"])
    for tag, (nf, depth, B, H, W, T, modes) in cases.items():
        params = O.synth_params(seed=0, nf=nf, depth=depth)
        net = build_ref_net(ConditionalUNet, params, nf, depth)
        lq, xT = O.synth_inputs(1234, B, H, W)
        z = O.synth_noise(7, T, (B, 3, H, W))
        sde = Inj(max_sigma=10, T=T, schedule="cosine", eps=0.005, device="cpu")
        sde.noise = torch.from_numpy(z)
        sde.set_model(net)
        sde.set_mu(torch.from_numpy(lq))
        out[tag + "/cfg"] = np.array([nf, depth, B, H, W, T], dtype=np.int64)
        for mode in modes:
            t0 = time.time()
            with torch.no_grad():
                fn = {"sde": sde.reverse_sde, "ode": sde.reverse_ode, "posterior": sde.reverse_posterior}[mode]
                y = fn(torch.from_numpy(xT)).numpy()
            out[tag + "/" + mode] = y
            out[tag + "/" + mode + "_wall_s"] = np.float64(time.time() - t0)
            print(tag, mode, "max|x0|=%.4f" % np.abs(y).max(), "%.1fs" % (time.time() - t0))
    np.savez_compressed(os.path.join(GOLD, "sampler.npz"), **out)
    print("sampler.npz")


def gen_nafnet(sde_utils):
    """ConditionalNAFNet (Refusion) forward + sampler goldens from the real reference."""
    from models.modules.DenoisingNAFNet_arch import ConditionalNAFNet
    Inj = InjectedIRSDE.make(sde_utils)
    out = {}
    cases = {
        # tag: (cfg, B, H, W, ts)
        "refusion_1x64x64": (dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1]), 1, 64, 64, [1, 60]),
        "refusion_2x40x56": (dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1]), 2, 40, 56, [37]),
        "w32_e12_2x24x20": (dict(width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1]), 2, 24, 20, [3, 77]),
    }
    nets = {}
    for tag, (cfg, B, H, W, ts) in cases.items():
        params = O.naf_synth_params(seed=0, img_channel=3, width=cfg["width"], middle_blk_num=cfg["middle_blk_num"],
                                    enc_blk_nums=tuple(cfg["enc_blk_nums"]), dec_blk_nums=tuple(cfg["dec_blk_nums"]))
        net = ConditionalNAFNet(img_channel=3, **cfg).eval()
        sd = net.state_dict()
        assert set(sd) == set(params), set(sd) ^ set(params)
        for k in sd:
            assert tuple(sd[k].shape) == params[k].shape, (k, sd[k].shape, params[k].shape)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        nets[tag] = (net, cfg)
        lq, xT = O.synth_inputs(1234, B, H, W, max_sigma=50)
        out[tag + "/shape"] = np.array([B, H, W], dtype=np.int64)
        out[tag + "/ts"] = np.array(ts, dtype=np.int64)
        for t in ts:
            with torch.no_grad():
                y = net(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
            out[tag + "/t%d" % t] = y
            print(tag, t, float(np.abs(y).max()))
    # samplers (refusion.yml: max_sigma 50, T 100, cosine, eps 0.005; deraining test.py default mode posterior)
    for tag, (B, H, W, T) in {"w32_e12_2x24x20": (2, 24, 20, 20), "refusion_1x64x64": (1, 32, 32, 100)}.items():
        net, cfg = nets[tag]
        lq, xT = O.synth_inputs(1234, B, H, W, max_sigma=50)
        z = O.synth_noise(7, T, (B, 3, H, W))
        sde = Inj(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
        sde.noise = torch.from_numpy(z)
        sde.set_model(net)
        sde.set_mu(torch.from_numpy(lq))
        key = "%s/sampler_%dx%dx%d_T%d" % (tag, B, H, W, T)
        for mode in ("sde", "posterior"):
            with torch.no_grad():
                fn = {"sde": sde.reverse_sde, "posterior": sde.reverse_posterior}[mode]
                y = fn(torch.from_numpy(xT)).numpy()
            out[key + "/" + mode] = y
            print(key, mode, float(np.abs(y).max()))
    np.savez_compressed(os.path.join(GOLD, "nafnet.npz"), **out)
    print("nafnet.npz")


def gen_dsde(sde_utils, ref_root):
    """denoising-sde variant: DenoisingSDE + unconditional UNet (full attention at mid) from the real reference."""
    import importlib
    # the denoising-sde task dir has its own models.modules (same package name): load it under a private name
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(ref_root, "codes/config/denoising-sde"))
    arch = importlib.import_module("models.modules.DenoisingUNet_arch")
    assert "denoising-sde" in arch.__file__, arch.__file__
    Net = arch.ConditionalUNet
    out = {}
    cases = {"nf32d2_2x24x20": (32, 2, 2, 24, 20, [3, 77]), "nf64d4_1x64x64": (64, 4, 1, 64, 64, [50]),
             "nf64d4_2x88x80": (64, 4, 2, 88, 80, [20])}   # 88x80 -> 96x80 padded; bottleneck 12x10 = 120 tokens (not a multiple of 32)
    nets = {}
    for tag, (nf, depth, B, H, W, ts) in cases.items():
        params = O.uncond_synth_params(seed=0, nf=nf, depth=depth)
        net = Net(in_nc=3, out_nc=3, nf=nf, depth=depth).eval()
        sd = net.state_dict()
        assert set(sd) == set(params), set(sd) ^ set(params)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        nets[tag] = net
        lq, xT = O.synth_inputs(1234, B, H, W, max_sigma=25)
        out[tag + "/cfg"] = np.array([nf, depth, B, H, W], dtype=np.int64)
        out[tag + "/ts"] = np.array(ts, dtype=np.int64)
        for t in ts:
            with torch.no_grad():
                y = net(torch.from_numpy(xT), t).numpy()
            out[tag + "/t%d" % t] = y
            print(tag, t, float(np.abs(y).max()))
    # DenoisingSDE(max_sigma=75, T=100) as in denoising-sde/options/test/ir-sde.yml
    sde = sde_utils.DenoisingSDE(max_sigma=75, T=100, device="cpu")
    out["sde/dt"] = np.float32(sde.dt.item())
    for n in ("thetas", "sigmas", "thetas_cumsum", "sigma_bars"):
        out["sde/" + n] = getattr(sde, n).numpy()
    out["sde/opt_t"] = np.array([int(sde.get_optimal_timestep(s)) for s in (15, 25, 50)], dtype=np.int64)

    class Inj(sde_utils.DenoisingSDE):
        noise = None

        def dispersion(self, x, t):
            import math
            return self.sigmas[t] * (self.noise[t] * math.sqrt(self.dt)).to(self.device)
    for tag, (B, H, W) in {"nf32d2_2x24x20": (2, 16, 16), "nf64d4_1x64x64": (1, 32, 32)}.items():
        net = nets[tag]
        isde = Inj(max_sigma=75, T=100, device="cpu")
        lq, _ = O.synth_inputs(1234, B, H, W)
        rs = np.random.RandomState(5)
        noisy = (lq + rs.standard_normal(lq.shape).astype(np.float32) * np.float32(25 / 255)).astype(np.float32)
        z = O.synth_noise(7, 100, (B, 3, H, W))
        isde.noise = torch.from_numpy(z)
        isde.set_model(net)
        Topt = int(isde.get_optimal_timestep(25))
        key = "%s/sampler_%dx%dx%d" % (tag, B, H, W)
        out[key + "/T"] = np.int64(Topt)
        out[key + "/noisy"] = noisy
        with torch.no_grad():
            out[key + "/ode"] = isde.reverse_ode(torch.from_numpy(noisy), T=Topt).numpy()
            out[key + "/sde"] = isde.reverse_sde(torch.from_numpy(noisy), T=Topt).numpy()
        print(key, Topt, float(np.abs(out[key + "/ode"]).max()), float(np.abs(out[key + "/sde"]).max()))
    np.savez_compressed(os.path.join(GOLD, "dsde.npz"), **out)
    print("dsde.npz")


def load_task_modules(task_dir, names):
    """Import models/modules/<name>.py of one task directory without running its package __init__ (latent-dehazing's
    pulls DiT -> timm, absent here): stand-in `models` / `models.modules` packages with the task's search path."""
    import importlib
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    pk, pm = types.ModuleType("models"), types.ModuleType("models.modules")
    pk.__path__ = [os.path.join(task_dir, "models")]
    pm.__path__ = [os.path.join(task_dir, "models", "modules")]
    sys.modules["models"], sys.modules["models.modules"] = pk, pm
    return [importlib.import_module("models.modules." + n) for n in names]


def gen_latent(sde_utils, ref_root):
    """Latent wrapper: the reference's latent UNet (encode / decode) and latent-task ConditionalNAFNet,
    plus the whole latent pipeline of latent-dehazing/test.py:90-100 with injected noise."""
    ua, na = load_task_modules(os.path.join(ref_root, "codes/config/latent-dehazing"), ["UNet_arch", "DenoisingNAFNet_arch"])
    assert "latent-dehazing" in ua.__file__ and "latent-dehazing" in na.__file__
    out = {}
    ucases = {"nasde_1x3x40x52": (dict(in_ch=3, out_ch=3, ch=8, ch_mult=[4, 8, 8, 16], embed_dim=8), 1, 40, 52),
              "bokeh_2x3x24x32": (dict(in_ch=3, out_ch=3, ch=16, ch_mult=[1, 2, 4], embed_dim=4), 2, 24, 32)}
    unets = {}
    for tag, (cfg, B, H, W) in ucases.items():
        params = O.latent_unet_synth_params(seed=0, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()})
        net = ua.UNet(**cfg).eval()
        sd = net.state_dict()
        assert set(sd) == set(params), set(sd) ^ set(params)
        for k in sd:
            assert tuple(sd[k].shape) == params[k].shape, k
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        unets[tag] = (net, cfg)
        lq, _ = O.synth_inputs(1234, B, H, W)
        with torch.no_grad():
            lat, hid = net.encode(torch.from_numpy(lq))
            rec = net.decode(lat, hid)
            lat2 = lat + 0.1 * torch.from_numpy(np.random.RandomState(5).standard_normal(tuple(lat.shape)).astype(np.float32))
            rec2 = net.decode(lat2, hid)
        out[tag + "/shape"] = np.array([B, H, W], dtype=np.int64)
        out[tag + "/latent"] = lat.numpy()
        for i, h in enumerate(hid):
            out[tag + "/hidden%d" % i] = h.numpy()
        out[tag + "/decode"] = rec.numpy()
        out[tag + "/latent2"] = lat2.numpy()
        out[tag + "/decode2"] = rec2.numpy()
        print("latent", tag, tuple(lat.shape), float(np.abs(rec.numpy()).max()))
    # latent-task ConditionalNAFNet (ending(x + intro(x))) on an 8-channel latent
    ncfg = dict(width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1])
    nparams = O.naf_synth_params(seed=0, img_channel=8, width=32, middle_blk_num=1, enc_blk_nums=(1, 2), dec_blk_nums=(1, 1))
    nnet = na.ConditionalNAFNet(img_channel=8, **ncfg).eval()
    assert set(nnet.state_dict()) == set(nparams)
    nnet.load_state_dict({k: torch.from_numpy(v) for k, v in nparams.items()}, strict=True)
    rs = np.random.RandomState(11)
    cond = rs.standard_normal((2, 8, 12, 10)).astype(np.float32)
    xt = (cond + 0.2 * rs.standard_normal(cond.shape)).astype(np.float32)
    out["naf/cond"], out["naf/xt"] = cond, xt
    for t in (4, 61):
        with torch.no_grad():
            out["naf/t%d" % t] = nnet(torch.from_numpy(xt), torch.from_numpy(cond), t).numpy()
    # whole pipeline (test.py:90-100): encode -> noise_state -> reverse_sde in the latent -> decode
    Inj = InjectedIRSDE.make(sde_utils)
    unet, _ = unets["nasde_1x3x40x52"]
    lq, _ = O.synth_inputs(1234, 1, 40, 52)
    T = 12
    with torch.no_grad():
        lat, hid = unet.encode(torch.from_numpy(lq))
        z = O.synth_noise(7, T, tuple(lat.shape))
        z0 = np.random.RandomState(3).standard_normal(tuple(lat.shape)).astype(np.float32)
        sde = Inj(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
        sde.noise = torch.from_numpy(z)
        sde.set_model(nnet)
        sde.set_mu(lat)
        noisy = lat + torch.from_numpy(z0) * sde.max_sigma          # IRSDE.noise_state (sde_utils.py:360-361)
        for mode in ("sde", "ode"):
            x0 = (sde.reverse_sde if mode == "sde" else sde.reverse_ode)(noisy)
            out["pipe/latent_" + mode] = x0.numpy()
            out["pipe/out_" + mode] = unet.decode(x0, hid).numpy()
    out["pipe/z0"], out["pipe/T"] = z0, np.array(T)
    # latent-bokeh score network: lens-conditioned ConditionalNAFNet (4 latent channels), forward + reverse_sde with kwargs
    (nb,) = load_task_modules(os.path.join(ref_root, "codes/config/latent-bokeh"), ["DenoisingNAFNet_arch"])
    assert "latent-bokeh" in nb.__file__
    bcfg = dict(width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1])
    bparams = O.naf_synth_params(seed=3, img_channel=4, width=32, middle_blk_num=1, enc_blk_nums=(1, 2), dec_blk_nums=(1, 1), lens=True)
    bnet = nb.ConditionalNAFNet(img_channel=4, **bcfg).eval()
    assert set(bnet.state_dict()) == set(bparams), set(bnet.state_dict()) ^ set(bparams)
    bnet.load_state_dict({k: torch.from_numpy(v) for k, v in bparams.items()}, strict=True)
    rs = np.random.RandomState(12)
    cond = rs.standard_normal((2, 4, 12, 10)).astype(np.float32)
    xt = (cond + 0.2 * rs.standard_normal(cond.shape)).astype(np.float32)
    lens = np.array([[1.8, 16.0, 30.0], [2.0, 8.0, 75.5]], dtype=np.float32)   # per image: src_lens, tgt_lens, disparity
    out["bokeh/cond"], out["bokeh/xt"], out["bokeh/lens"] = cond, xt, lens
    with torch.no_grad():
        li = [torch.from_numpy(lens[:, i].copy()) for i in range(3)]
        out["bokeh/tvec"] = bnet(torch.from_numpy(xt), torch.from_numpy(cond), torch.tensor([5, 60]), lens_info=li).numpy()
        li1 = [torch.from_numpy(lens[:1, i].copy()) for i in range(3)]                     # test.py path: int time, one image
        out["bokeh/t33"] = bnet(torch.from_numpy(xt[:1]), torch.from_numpy(cond[:1]), 33, lens_info=li1).numpy()
        Tb = 10
        zb = O.synth_noise(9, Tb, (1, 4, 12, 10))
        sde = Inj(max_sigma=50, T=Tb, schedule="cosine", eps=0.005, device="cpu")
        sde.noise = torch.from_numpy(zb)
        sde.set_model(bnet)
        sde.set_mu(torch.from_numpy(cond[:1]))
        out["bokeh/sde"] = sde.reverse_sde(torch.from_numpy(xt[:1]), lens_info=li1).numpy()
    out["bokeh/T"] = np.array(Tb)
    np.savez_compressed(os.path.join(GOLD, "latent.npz"), **out)
    print("latent.npz")


def gen_metrics(ref_root):
    """Evaluation tail: the reference's own tensor2img / calculate_psnr / calculate_ssim
    (codes/utils/img_utils.py) and bgr2ycbcr (codes/data/util.py) run on synthetic output/GT pairs, following
    deraining/test.py:110-178.  cv2 is absent in this image; the two cv2 calls ssim() makes are stubbed with their
    published definitions — getGaussianKernel(k, s): g_i = exp(-(i-(k-1)/2)^2 / (2 s^2)) / sum, float64; filter2D(img,
    -1, w): per-channel correlation with the anchor at the window centre (only its 'valid' interior is used, :203-208,
    so the border mode does not matter) — everything else is reference code."""
    import scipy.ndimage as ndi
    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(k, sigma):
        i = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (g / g.sum()).reshape(k, 1)

    def filter2D(img, ddepth, window):
        if img.ndim == 2:
            return ndi.correlate(img, window, mode="mirror")
        return np.stack([ndi.correlate(img[..., c], window, mode="mirror") for c in range(img.shape[2])], axis=-1)

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    sys.modules["cv2"] = cv2
    sys.modules["torchvision.utils"].make_grid = lambda *a, **k: None

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    iu = load("ref_img_utils", "codes/utils/img_utils.py")
    du = load("ref_data_util", "codes/data/util.py")
    out = {}
    cases = {"rgb_1x3x40x52_cb0": (1, 3, 40, 52, 0), "rgb_2x3x64x48_cb4": (2, 3, 64, 48, 4), "gray_1x1x33x37_cb0": (1, 1, 33, 37, 0)}
    for tag, (B, C, H, W, cb) in cases.items():
        rs = np.random.RandomState(len(tag))
        gt = rs.rand(B, C, H, W).astype(np.float32)
        # restored image = GT + small error, with values outside [0,1] so the clamp matters
        o = (gt + 0.05 * rs.standard_normal(gt.shape)).astype(np.float32)
        res = np.zeros((B, 4))
        imgs = []
        for b in range(B):
            output = iu.tensor2img(torch.from_numpy(o[b:b + 1]).squeeze())      # deraining/test.py:112
            GT_ = iu.tensor2img(torch.from_numpy(gt[b:b + 1]).squeeze())        # :114
            imgs.append(output)
            gt_img, sr_img = GT_ / 255.0, output / 255.0                        # :137-138
            crop = (lambda im: im if cb == 0 else im[cb:-cb, cb:-cb])           # :140-150
            res[b, 0] = iu.calculate_psnr(crop(sr_img) * 255, crop(gt_img) * 255)
            res[b, 1] = iu.calculate_ssim(crop(sr_img) * 255, crop(gt_img) * 255)
            if C == 3:                                                          # :161-178
                sr_y, gt_y = du.bgr2ycbcr(sr_img, only_y=True), du.bgr2ycbcr(gt_img, only_y=True)
                res[b, 2] = iu.calculate_psnr(crop(sr_y) * 255, crop(gt_y) * 255)
                res[b, 3] = iu.calculate_ssim(crop(sr_y) * 255, crop(gt_y) * 255)
            else:
                res[b, 2:] = np.nan
        out[tag + "/cfg"] = np.array([B, C, H, W, cb])
        out[tag + "/out"], out[tag + "/gt"] = o, gt
        out[tag + "/metrics"] = res
        out[tag + "/img0"] = imgs[0]
        print("metrics", tag, res[0])
    np.savez_compressed(os.path.join(GOLD, "metrics.npz"), **out)


def sub3(y):
    """Fixture-size reduction for the full-resolution goldens: every third pixel in both directions (offsets 1, 2).
    3 is coprime with every tile size of the product (4x4 / 2x2 Winograd tiles, 16x16 halo tiles, 128-pixel GEMM row
    tiles), so over the image every in-tile position is sampled."""
    return np.ascontiguousarray(y[..., 1::3, 2::3])


def gen_fullres(sde_utils, ConditionalUNet, ref_root):
    """Reference goldens at the shapes that are benchmarked (VERDICT r01 'weak' #1 / SURVEY 8c): 256x256 forward and
    T=100 samplers, the Rain100H-sized 2x3x321x481 reflect-pad case, Refusion NAFNet at 512x512, a T=200 / max_sigma 50
    Refusion sampler, and the latent pipeline at 256x256 -> 64x64x4.  Full tensors where small, else `sub3` samples plus
    full border strips (the pad / crop region)."""
    Inj = InjectedIRSDE.make(sde_utils)
    out = {}
    params = O.synth_params(seed=0, nf=64, depth=4)
    net = build_ref_net(ConditionalUNet, params, 64, 4)
    # --- ConditionalUNet forward, 1x3x256x256 (BASELINE configs[1] image size)
    lq, xT = O.synth_inputs(1234, 1, 256, 256)
    for t in (1, 50, 100):
        with torch.no_grad():
            y = net(torch.from_numpy(xT), torch.from_numpy(lq), t).numpy()
        out["unet_1x256x256/t%d" % t] = y if t == 50 else sub3(y)
        print("unet 256", t, float(np.abs(y).max()))
    # --- ConditionalUNet forward, 2x3x321x481 (Rain100H size: reflect pad 321 -> 336, 481 -> 496)
    lq2, xT2 = O.synth_inputs(1234, 2, 321, 481)
    with torch.no_grad():
        y = net(torch.from_numpy(xT2), torch.from_numpy(lq2), 37).numpy()
    out["unet_2x321x481/t37_sub3"] = sub3(y)
    out["unet_2x321x481/t37_bottom"] = np.ascontiguousarray(y[:, :, -20:, :])
    out["unet_2x321x481/t37_right"] = np.ascontiguousarray(y[:, :, :, -20:])
    print("unet 321x481", float(np.abs(y).max()))
    # --- full T=100 samplers at 1x3x256x256 with injected noise
    z = O.synth_noise(7, 100, (1, 3, 256, 256))
    sde = Inj(max_sigma=10, T=100, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(z)
    sde.set_model(net)
    sde.set_mu(torch.from_numpy(lq))
    for mode in ("sde", "posterior"):
        t0 = time.time()
        with torch.no_grad():
            y = (sde.reverse_sde if mode == "sde" else sde.reverse_posterior)(torch.from_numpy(xT)).numpy()
        out["unet_1x256x256/sampler_" + mode] = y if mode == "sde" else sub3(y)
        print("unet 256 sampler", mode, float(np.abs(y).max()), "%.0fs" % (time.time() - t0))
    # --- Refusion ConditionalNAFNet forward at 1x3x512x512 (BASELINE configs[3] image size) + T=200 sampler (small image)
    from models.modules.DenoisingNAFNet_arch import ConditionalNAFNet
    cfg = dict(width=64, enc_blk_nums=[1, 1, 1, 28], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
    nparams = O.naf_synth_params(seed=0, img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 28), dec_blk_nums=(1, 1, 1, 1))
    nnet = ConditionalNAFNet(img_channel=3, **cfg).eval()
    nnet.load_state_dict({k: torch.from_numpy(v) for k, v in nparams.items()}, strict=True)
    lq5, xT5 = O.synth_inputs(1234, 1, 512, 512, max_sigma=50)
    with torch.no_grad():
        y = nnet(torch.from_numpy(xT5), torch.from_numpy(lq5), 60).numpy()
    out["naf_1x512x512/t60_sub3"] = sub3(y)
    out["naf_1x512x512/t60_corner"] = np.ascontiguousarray(y[:, :, -64:, -64:])
    print("nafnet 512", float(np.abs(y).max()))
    lqs, xTs = O.synth_inputs(1234, 1, 32, 32, max_sigma=50)
    zs = O.synth_noise(7, 200, (1, 3, 32, 32))
    sde = Inj(max_sigma=50, T=200, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(zs)
    sde.set_model(nnet)
    sde.set_mu(torch.from_numpy(lqs))
    for mode in ("sde", "posterior"):
        with torch.no_grad():
            y = (sde.reverse_sde if mode == "sde" else sde.reverse_posterior)(torch.from_numpy(xTs)).numpy()
        out["naf_1x32x32_T200/" + mode] = y
        print("nafnet T200", mode, float(np.abs(y).max()))
    # --- latent pipeline at 1x3x256x256 -> 64x64x4 (BASELINE configs[4] shape; latent-bokeh/options/bokeh/test/refusion.yml networks)
    ua, = load_task_modules(os.path.join(ref_root, "codes/config/latent-dehazing"), ["UNet_arch"])
    (nb,) = load_task_modules(os.path.join(ref_root, "codes/config/latent-bokeh"), ["DenoisingNAFNet_arch"])
    ucfg = dict(in_ch=3, out_ch=3, ch=64, ch_mult=[1, 2, 4], embed_dim=4)
    uparams = O.latent_unet_synth_params(seed=0, in_ch=3, out_ch=3, ch=64, ch_mult=(1, 2, 4), embed_dim=4)
    unet = ua.UNet(**ucfg).eval()
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in uparams.items()}, strict=True)
    bparams = O.naf_synth_params(seed=3, img_channel=4, width=64, middle_blk_num=1, enc_blk_nums=(1, 1, 1, 28), dec_blk_nums=(1, 1, 1, 1), lens=True)
    bnet = nb.ConditionalNAFNet(img_channel=4, **cfg).eval()
    assert set(bnet.state_dict()) == set(bparams), set(bnet.state_dict()) ^ set(bparams)
    bnet.load_state_dict({k: torch.from_numpy(v) for k, v in bparams.items()}, strict=True)
    T = 100
    lens = np.array([[1.8, 16.0, 30.0]], dtype=np.float32)
    li = [torch.from_numpy(lens[:, i].copy()) for i in range(3)]
    with torch.no_grad():
        lat, hid = unet.encode(torch.from_numpy(lq))
        assert tuple(lat.shape) == (1, 4, 64, 64), lat.shape
        zl = O.synth_noise(7, T, tuple(lat.shape))
        z0 = np.random.RandomState(3).standard_normal(tuple(lat.shape)).astype(np.float32)
        sde = Inj(max_sigma=50, T=T, schedule="cosine", eps=0.005, device="cpu")
        sde.noise = torch.from_numpy(zl)
        sde.set_model(bnet)
        sde.set_mu(lat)
        noisy = lat + torch.from_numpy(z0) * sde.max_sigma
        x0 = sde.reverse_sde(noisy, lens_info=li)
        rec = unet.decode(x0, hid).numpy()
    out["latent_1x256x256/lens"] = lens
    out["latent_1x256x256/z0"] = z0
    out["latent_1x256x256/latent"] = lat.numpy()
    out["latent_1x256x256/latent_sde"] = x0.numpy()
    out["latent_1x256x256/out_sde_sub3"] = sub3(rec)
    print("latent 256", float(np.abs(rec).max()))
    np.savez_compressed(os.path.join(GOLD, "fullres.npz"), **out)
    print("fullres.npz")


def gen_fullres2(sde_utils, ConditionalUNet, ref_root):
    """r03 additions (VERDICT r02 'missing' #3): the two benchmarked shapes that had no reference golden —
    `reverse_ode` T=100 at 1x3x256x256 (`sde_utils.py:268-282`; BASELINE configs[2] IS the ODE) and
    `ConditionalUNet.forward` at 1x3x512x512 (`DenoisingUNet_arch.py:85-134`).  Written to its own file so that
    fullres.npz (bit-reproduced by the r02 judge) is not regenerated."""
    Inj = InjectedIRSDE.make(sde_utils)
    out = {}
    params = O.synth_params(seed=0, nf=64, depth=4)
    net = build_ref_net(ConditionalUNet, params, 64, 4)
    lq, xT = O.synth_inputs(1234, 1, 256, 256)
    sde = Inj(max_sigma=10, T=100, schedule="cosine", eps=0.005, device="cpu")
    sde.noise = torch.from_numpy(O.synth_noise(7, 100, (1, 3, 256, 256)))   # unused by the ODE; kept for symmetry
    sde.set_model(net)
    sde.set_mu(torch.from_numpy(lq))
    t0 = time.time()
    with torch.no_grad():
        y = sde.reverse_ode(torch.from_numpy(xT)).numpy()
    out["unet_1x256x256/sampler_ode"] = y
    print("unet 256 sampler ode", float(np.abs(y).max()), "%.0fs" % (time.time() - t0))
    lq5, xT5 = O.synth_inputs(1234, 1, 512, 512)
    for t in (100, 23):
        with torch.no_grad():
            y = net(torch.from_numpy(xT5), torch.from_numpy(lq5), t).numpy()
        out["unet_1x512x512/t%d_sub3" % t] = sub3(y)
        out["unet_1x512x512/t%d_corner" % t] = np.ascontiguousarray(y[:, :, -48:, -48:])
        print("unet 512", t, float(np.abs(y).max()))
    np.savez_compressed(os.path.join(GOLD, "fullres2.npz"), **out)
    print("fullres2.npz")


def gen_seam(sde_utils, ConditionalUNet):
    """The reference's own `IRSDE.reverse_ode` (`sde_utils.py:268-282`, no noise drawn) around its own `ConditionalUNet`
    at 1x3x32x32, T=6: the pin of tests/test_gpu_fullres.py's seam test, which used to import the reference at run time."""
    params = O.synth_params(seed=0, nf=64, depth=4)
    net = build_ref_net(ConditionalUNet, params, 64, 4)
    lq, xT = O.synth_inputs(2, 1, 32, 32)
    sde = sde_utils.IRSDE(max_sigma=10, T=6, schedule="cosine", eps=0.005, device="cpu")
    sde.set_model(net)
    sde.set_mu(torch.from_numpy(lq))
    with torch.no_grad():
        y = sde.reverse_ode(torch.from_numpy(xT)).numpy()
    np.savez_compressed(os.path.join(GOLD, "seam.npz"), **{"nf64d4_1x32x32_T6/ode": y})
    print("seam.npz", float(np.abs(y).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="")
    ap.add_argument("--no-big", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    os.makedirs(GOLD, exist_ok=True)
    sde_utils, ConditionalUNet = load_reference(a.ref)
    if a.only in ("", "schedule"):
        gen_schedule(sde_utils)
    if a.only in ("", "forward"):
        gen_forward(sde_utils, ConditionalUNet)
    if a.only in ("", "forward_attn"):
        gen_forward_attn(sde_utils, ConditionalUNet)
    if a.only in ("", "forward_attn256"):
        gen_forward_attn256(sde_utils, ConditionalUNet)
    if a.only in ("", "steps"):
        gen_steps(sde_utils)
    if a.only in ("", "sampler"):
        gen_sampler(sde_utils, ConditionalUNet, big=not a.no_big)
    if a.only in ("", "nafnet"):
        gen_nafnet(sde_utils)
    if a.only in ("", "dsde"):
        gen_dsde(sde_utils, a.ref)
    if a.only in ("", "latent"):
        gen_latent(sde_utils, a.ref)
    if a.only in ("", "metrics"):
        gen_metrics(a.ref)
    if a.only in ("", "fullres"):   # last: it re-imports task-local `models.modules` packages
        sde_utils, ConditionalUNet = (sde_utils, ConditionalUNet) if a.only == "fullres" else load_reference_again(a.ref)
        gen_fullres(sde_utils, ConditionalUNet, a.ref)
    if a.only in ("", "fullres2"):
        if a.only == "":
            sde_utils, ConditionalUNet = load_reference_again(a.ref)
        gen_fullres2(sde_utils, ConditionalUNet, a.ref)
    if a.only in ("", "seam"):
        if a.only == "":
            sde_utils, ConditionalUNet = load_reference_again(a.ref)
        gen_seam(sde_utils, ConditionalUNet)


if __name__ == "__main__":
    main()
