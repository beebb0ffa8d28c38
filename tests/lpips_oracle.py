"""Oracle of LPIPS v0.1 / net='alex' (what `lpips.LPIPS(net='alex')(in0, in1)` computes), written with torch CPU ops, float64 by
default.  Independent of the package under test.  The pip package `lpips` and torchvision are not dependencies of this
project; the definition is:
  x = (x - shift) / scale;  AlexNet `features` tapped after each ReLU;
  per tap: n = f / (sqrt(sum_c f^2) + 1e-10), d = (n0 - n1)^2, term = mean over pixels of sum_c w[c] d[c];  lpips = sum of the terms.
Real-weight values (the reference README's LPIPS column) are unpinned and blocked on assets, like the Rain100H PSNR gate: the
published AlexNet / lpips weight files are not available here, so every test runs on `synth_weights`."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (Cout, Cin, k, stride, pad); a 3x3 stride-2 max-pool (floor mode) in front of layers 2 and 3
LAYERS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))


def synth_weights(seed=0):
    """15 float32 arrays under the engine's names: conv weights N(0, 2 / (Cin k^2)), biases N(0, 0.1^2), lin weights
    uniform[0, 1) * 4 / C (non-negative like the published ones)."""
    rng = np.random.default_rng(seed)
    w = {}
    for i, (co, ci, k, _, _) in enumerate(LAYERS, 1):
        w["conv%d.weight" % i] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        w["conv%d.bias" % i] = (rng.standard_normal(co) * 0.1).astype(np.float32)
        w["lin%d.weight" % i] = (rng.random((1, co, 1, 1)) * 4.0 / co).astype(np.float32)
    return w


def feature_shapes(H, W):
    """[(C, h, w)] of the five taps for an H x W input."""
    out = []
    h, w = H, W
    for i, (co, _, k, s, p) in enumerate(LAYERS):
        if i in (1, 2):
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((co, h, w))
    return out


def features(weights, x, dtype=torch.float64):
    """x: (B, 3, H, W) in [-1, 1] -> the five ReLU'd feature maps, NCHW tensors of `dtype`."""
    x = torch.as_tensor(x).to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = (x - shift) / scale
    maps = []
    for i, (_, _, _, s, p) in enumerate(LAYERS, 1):
        if i in (2, 3):
            h = F.max_pool2d(h, kernel_size=3, stride=2)
        h = F.relu(F.conv2d(h, torch.as_tensor(weights["conv%d.weight" % i]).to(dtype), torch.as_tensor(weights["conv%d.bias" % i]).to(dtype),
                            stride=s, padding=p))
        maps.append(h)
    return maps


def lpips_terms(weights, in0, in1, dtype=torch.float64):
    """-> (terms [B, 5] as a numpy array of `dtype`, the five feature maps of in0)."""
    f0, f1 = features(weights, in0, dtype), features(weights, in1, dtype)
    terms = []
    for i, (a, b) in enumerate(zip(f0, f1), 1):
        na = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b * b).sum(1, keepdim=True)) + 1e-10)
        d = (na - nb) ** 2
        w = torch.as_tensor(weights["lin%d.weight" % i]).to(dtype)
        terms.append((d * w).sum(1, keepdim=True).mean((2, 3)).reshape(-1))
    return torch.stack(terms, 1).numpy(), f0


# ---- the two checkpoint layouts metrics.LPIPS accepts, made from `synth_weights` (the key names are written from memory of lpips 0.1.4 / torchvision) ----
TV_IDX = {1: 0, 2: 3, 3: 6, 4: 8, 5: 10}   # conv number -> index inside torchvision's AlexNet.features


def lpips_layout(w):
    """The keys of lpips.LPIPS(net='alex').state_dict() (lin layers registered twice, the scaling layer's buffers)."""
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    for n, idx in TV_IDX.items():
        for p in ("weight", "bias"):
            sd["net.slice%d.%d.%s" % (n, idx, p)] = torch.from_numpy(w["conv%d.%s" % (n, p)])
        sd["lin%d.model.1.weight" % (n - 1)] = torch.from_numpy(w["lin%d.weight" % n])
        sd["lins.%d.model.1.weight" % (n - 1)] = torch.from_numpy(w["lin%d.weight" % n])
    return sd


def files_layout(w):
    """The two published files merged: torchvision's AlexNet checkpoint (features + classifier) and lpips' alex.pth."""
    sd = {}
    for n, idx in TV_IDX.items():
        for p in ("weight", "bias"):
            sd["features.%d.%s" % (idx, p)] = torch.from_numpy(w["conv%d.%s" % (n, p)])
        sd["lin%d.model.1.weight" % (n - 1)] = torch.from_numpy(w["lin%d.weight" % n])
    sd["classifier.1.weight"] = torch.zeros(8, 8)
    sd["classifier.1.bias"] = torch.zeros(8)
    return sd
