"""denoising-sde ConditionalNAFNet (the unconditional Refusion network), host side (no GPU): the drop-in module's parameter
inventory against the reference's (tests/golden/dsde_naf.npz, tools/gen_dsde_naf_golden.py), the float64 restatement
(tests/dsde_naf_oracle.py) against the reference goldens, the task wrapper's dispatch and `test(sigma)` wiring, `add_noise`'s
sigma rule, the C ABI flag and the evaluation tool's help."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def module(name):
    cfg = DN.CFGS[name]
    return P.denoising_sde.ConditionalNAFNet(img_channel=3, width=cfg["width"], enc_blk_nums=list(cfg["enc_blk_nums"]),
                                             middle_blk_num=cfg["middle_blk_num"], dec_blk_nums=list(cfg["dec_blk_nums"]))


@pytest.mark.parametrize("name", ["refusion", "w32_e12"])
def test_state_dict_inventory_equals_reference(golden, name):
    g = golden.dsde_naf
    names = [str(n) for n in g[name + "/names"]]
    sd = module(name).state_dict()
    assert sorted(sd) == names
    for k, shp in zip(names, g[name + "/shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp[:sd[k].dim()]), k
    assert tuple(sd["intro.weight"].shape) == (DN.CFGS[name]["width"], 3, 3, 3)
    if name == "refusion":
        assert len(names) == 668


def test_strict_load_and_deraining_intro_is_rejected():
    cfg = DN.CFGS["w32_e12"]
    m = module("w32_e12")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DN.synth_params(seed=0, **cfg).items()}, strict=True)
    derain = O.naf_synth_params(seed=0, img_channel=3, **cfg)   # intro.weight [32, 6, 3, 3]
    with pytest.raises(RuntimeError, match="intro.weight"):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in derain.items()}, strict=True)
    # and the other way round: the conditional class does not take this task's checkpoint
    with pytest.raises(RuntimeError, match="intro.weight"):
        P.ConditionalNAFNet(img_channel=3, width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1]).load_state_dict(
            {k: torch.from_numpy(v) for k, v in DN.synth_params(seed=0, **cfg).items()}, strict=True)


@pytest.mark.parametrize("tag", sorted(DN.FORWARD))
def test_restatement_forward_matches_reference_golden(golden, tag):
    """Bar: the one tests/test_oracle_golden.py::test_nafnet_forward uses for the conditional network's restatement (2e-5)."""
    g = golden.dsde_naf
    name, B, H, W = DN.FORWARD[tag]
    cfg = DN.CFGS[name]
    params = DN.synth_params(seed=0, **cfg)
    _, noisy = DN.inputs(B, H, W, 25 if name == "w32_e12" else 15)
    ts = [int(t) for t in g[tag + "/ts"]]
    assert ts[:2] == [1, 7] and ts[2] == int(g[{"w32_e12": "w32_e12_2x22x19", "refusion": "refusion_1x32x32"}[name] + "/sampler/T"])
    for t in ts:
        y = DN.forward(params, noisy, t, cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"])
        e = rel(y, g[tag + "/t%d" % t])
        print(tag, t, "%.3g" % e)
        assert e < 2e-5, (tag, t, e)


def test_restatement_small_sampler_matches_reference_golden(golden):
    """DenoisingSDE(50, 100), sigma 25 -> T_opt steps of reverse_ode / reverse_sde (injected noise) around the restated network;
    bar: tests/test_oracle_golden.py::test_dsde_sampler_small's (1e-3)."""
    g = golden.dsde_naf
    tag = "w32_e12_2x22x19"
    name, B, H, W, max_sigma, T, sigma = DN.SAMPLER[tag]
    cfg = DN.CFGS[name]
    params = DN.synth_params(seed=0, **cfg)
    sde = P.DenoisingSDE(max_sigma=max_sigma, T=T)
    Topt = int(sde.get_optimal_timestep(sigma))
    assert Topt == int(g[tag + "/sampler/T"]) == 29
    sch = O.dsde_schedule(max_sigma, T)
    assert O.dsde_optimal_timestep(sch, sigma) == Topt
    _, noisy = DN.inputs(B, H, W, sigma)
    assert np.array_equal(noisy, g[tag + "/sampler/noisy"])
    z = O.synth_noise(7, T, (B, 3, H, W))
    for mode in ("ode", "sde"):
        y = DN.sample(params, sch, noisy, mode == "ode", Topt, cfg, noise=z)
        e = rel(y, g[tag + "/sampler/" + mode])
        print(mode, "%.3g" % e)
        assert e < 1e-3, (mode, e)


def test_shipped_schedule_optimal_timestep(golden):
    """denoising-sde/options/test/refusion.yml: DenoisingSDE(max_sigma 70, T 1000), sigma 15 -> the reference's T_opt (158)."""
    sde = P.DenoisingSDE(max_sigma=70, T=1000)
    assert int(sde.get_optimal_timestep(15)) == int(golden.dsde_naf["refusion_1x32x32/sampler/T"]) == 158


def test_define_g_and_create_model_dispatch(monkeypatch):
    setting = dict(width=32, enc_blk_nums=[1, 2], middle_blk_num=1, dec_blk_nums=[1, 1])
    opt = {"model": "denoising", "network_G": {"which_model_G": "ConditionalNAFNet", "setting": setting}}
    m = P.define_G(opt, "denoising-sde")
    assert type(m) is P.denoising_sde.ConditionalNAFNet and tuple(m.intro.weight.shape) == (32, 3, 3, 3)
    assert type(P.define_G(opt)) is P.ConditionalNAFNet                     # the deraining lookup is unchanged
    u = P.define_G({"network_G": {"which_model_G": "ConditionalUNet", "setting": dict(in_nc=3, out_nc=3, nf=32, depth=2)}}, "denoising-sde")
    assert type(u) is P.denoising_sde.ConditionalUNet
    with pytest.raises(NotImplementedError):
        P.define_G({"network_G": {"which_model_G": "Other", "setting": {}}}, "denoising-sde")
    # the wrapper, without a device: keep the module where it is
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    mdl = P.create_model(opt, task="denoising-sde")
    assert type(mdl) is P.denoising_sde.DenoisingSDEModel and type(mdl.model) is P.denoising_sde.ConditionalNAFNet
    assert type(P.create_model(opt)) is P.DenoisingModel


def test_wrapper_test_wires_sigma_to_the_optimal_timestep(monkeypatch):
    """denoising-sde/models/denoising_model.py:162-170: T = sde.T if sigma < 0 else sde.get_optimal_timestep(sigma); reverse_ode(LQ, T)."""
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    opt = {"model": "denoising", "network_G": {"which_model_G": "ConditionalNAFNet",
                                               "setting": dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])}}
    mdl = P.create_model(opt, task="denoising-sde")
    mdl.device = torch.device("cpu")   # feed_data moves its tensors there

    class Stub:
        T = 1000
        calls = []

        def get_optimal_timestep(self, sigma):
            self.calls.append(("opt", sigma))
            return 158

        def reverse_ode(self, xt, T=-1, save_states=False):
            self.calls.append(("ode", T, save_states, xt))
            return xt * 0.5

        def reverse_sde(self, *a, **k):
            raise AssertionError("denoising-sde tests with reverse_ode")

    sde = Stub()
    lq, gt = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    mdl.feed_data(lq, gt)
    mdl.test(sde, sigma=15, save_states=False)
    assert sde.calls[0] == ("opt", 15) and sde.calls[1][:3] == ("ode", 158, False) and sde.calls[1][3] is mdl.LQ
    vis = mdl.get_current_visuals()
    assert list(vis) == ["Input", "Output", "GT"]
    assert torch.equal(vis["Input"], lq[0]) and torch.equal(vis["Output"], lq[0] * 0.5) and torch.equal(vis["GT"], gt[0])
    sde.calls.clear()
    mdl.test(sde)   # sigma = -1: the whole schedule
    assert sde.calls[0][:2] == ("ode", 1000)
    mdl2 = P.create_model(opt, task="denoising-sde")
    mdl2.device = torch.device("cpu")
    mdl2.feed_data(lq)
    mdl2.test(sde, sigma=-1)
    assert list(mdl2.get_current_visuals()) == ["Input", "Output"]


def test_add_noise_sigma_rule(monkeypatch):
    """codes/utils/deg_utils.py:13-15: sigma / 255 if sigma > 1 (so 1 itself is taken as is).  The draw is stubbed here (it is the
    device's Philox; tests/test_gpu_dsde_naf.py covers it): the scale is what this test pins."""
    ds = P.denoising_sde
    seen = {}

    class FakeLib:
        def irsde_philox_normal(self, out, B, CHW, t, seed, off, stream):
            seen.update(B=B, CHW=CHW, t=t, seed=seed, off=off)
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: FakeLib())
    monkeypatch.setattr(_lib, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(torch, "empty", lambda shape, device=None, dtype=None: torch.ones(shape, dtype=dtype))
    x = torch.zeros(2, 3, 4, 5)
    for sigma, want in ((15, 15 / 255), (1, 1.0), (0.1, 0.1), (25.0, 25 / 255)):
        y = ds.add_noise(x, sigma, seed=9, image_offset=4)
        assert y.shape == x.shape and torch.allclose(y, torch.full_like(x, want), rtol=1e-6, atol=0), sigma
    assert seen == dict(B=2, CHW=60, t=0, seed=9, off=4)
    assert ds.add_noise(x[0], 15).shape == (3, 4, 5)


def test_flag_is_declared_in_the_header_and_mirrored():
    with open(os.path.join(ROOT, "include", "irsde_hip.h")) as f:
        h = f.read()
    m = re.search(r"IRSDE_FLAG_NAF_UNCOND\s*=\s*(\d+)", h)
    assert m and int(m.group(1)) == 131072 == _lib.FLAG_NAF_UNCOND
    flags = {k: int(v) for k, v in re.findall(r"(IRSDE_FLAG_\w+)\s*=\s*(\d+)", h)}
    assert sorted(flags.values()) == sorted(set(flags.values()))        # a bit of its own
    assert _lib.lib().irsde_version() == 107                            # additive: same ABI version


def test_engine_inventory_and_flag_refusals(golden):
    """Engine creation and its weight inventory are host-side: the names / shapes are the reference state_dict; the flag does not combine
    with the stereo / lens / intro-skip variants, and irsde_create (the UNet) refuses it."""
    L = _lib.lib()

    def naf(flags, enc=(1, 1, 1, 28), dec=(1, 1, 1, 1), width=64, keep=False):
        cfg = _lib.NafConfig()
        cfg.img_channel, cfg.width, cfg.middle_blk_num, cfg.n_enc, cfg.n_dec = 3, width, 1, len(enc), len(dec)
        for i, (a, b) in enumerate(zip(enc, dec)):
            cfg.enc_blk_nums[i], cfg.dec_blk_nums[i] = a, b
        cfg.device, cfg.flags = 0, flags
        h = ctypes.c_void_p()
        rc = L.irsde_create_nafnet(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0 and not keep:
            L.irsde_destroy(h)
        return (rc, h) if keep else rc

    U = _lib.FLAG_NAF_UNCOND
    rc, h = naf(U, keep=True)
    assert rc == 0
    try:
        n = L.irsde_num_weights(h)
        names = [L.irsde_weight_name(h, i).decode() for i in range(n)]
        assert sorted(names) == [str(v) for v in golden.dsde_naf["refusion/names"]] and n == 668
        shape, nd = (ctypes.c_int64 * 4)(), ctypes.c_int()
        assert L.irsde_weight_shape(h, names.index("intro.weight"), shape, ctypes.byref(nd)) == 0
        assert nd.value == 4 and list(shape) == [64, 3, 3, 3]
        bad = np.zeros((64, 6, 3, 3), np.float32)
        assert L.irsde_load_weight(h, b"intro.weight", bad.ctypes.data_as(ctypes.c_void_p), (ctypes.c_int64 * 4)(64, 6, 3, 3), 4) != 0
        assert b"shape mismatch" in L.irsde_last_error()
    finally:
        L.irsde_destroy(h)
    for mode in (_lib.FLAG_FP16, _lib.FLAG_BF16, _lib.FLAG_SPLIT_BF16X2, _lib.FLAG_SPLIT_F16X2, _lib.FLAG_NO_NAF_CHAIN):
        assert naf(U | mode, enc=(1, 1), dec=(1, 1), width=32) == 0, mode
    for f in (_lib.FLAG_NAF_STEREO, _lib.FLAG_NAF_LENS, _lib.FLAG_NAF_INTRO_SKIP):
        assert naf(U | f, enc=(1, 1), dec=(1, 1), width=32) == -1, f   # IRSDE_ERR_INVALID
        assert b"IRSDE_FLAG_NAF_UNCOND cannot be combined" in L.irsde_last_error()
    cfg = _lib.Config(3, 3, 32, 2, 0, U)
    h = ctypes.c_void_p()
    assert L.irsde_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"IRSDE_FLAG_NAF_UNCOND" in L.irsde_last_error()


def test_eval_folder_help_mentions_the_task():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--task" in r.stdout and "denoising" in r.stdout and "--sigma" in r.stdout and "LPIPS" in r.stdout
    # without --task the tool is the LQ / GT loop it was: --lq stays required
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_folder.py"), "--weights", "x.pth"], capture_output=True, text=True)
    assert r.returncode == 2 and "required: --lq" in r.stderr
