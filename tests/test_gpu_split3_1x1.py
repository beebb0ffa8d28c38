"""GPU tests of the plain 1x1 convolutions on three bf16 pieces (csrc/gemm_split.hip, gemm_split3a_kernel: the weights as the triples of split_triples_kernel,
the f32 activations split inside the GEMM; plan rule split3_1x1_choose, knob IRSDE_SPLIT3_1X1, hooks irsde_debug_split3_1x1 / irsde_debug_force_split3_1x1,
irsde_debug_conv selector 49).

Kernel: per output element the kernel runs the six products of a 16-k sub-step in gemm_split3i_kernel's order over the same K order with the same k -> lane
assignment, on A pieces made by split_triples_kernel's chain, so it must equal split_triples_kernel + gemm_split3i_kernel (irsde_debug_split_gemm, nplanes 43) on
the concatenated A BIT FOR BIT; its one-item-per-block and drain twins (modes 1 / 2) must equal the production walk bit for bit.  float64 bar: split3_oracle.bar,
three times the error of numpy's float32 product on the same inputs; tests/test_split3_host.py shows that a lost plane or product lands above it on
split3_oracle.inputs.  Layer bar: 2e-5 against the float64 convolution, the bar of the direct kernels (tests/test_gpu_parity.py).  Network bar: 1e-4 against the
reference golden.  Every test prints its figures before it asserts; the measured columns are in profiles/split3_1x1.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

import split3_oracle as S3
from test_gpu_parity import DEV, _sample, oracle_conv, relerr, run_conv

pytestmark = pytest.mark.gpu

MARK = "kernel=split3a bf16x3"

# (M, N, C0, C1, out_stride, block cap)
SHAPES = [(300, 160, 64, 0, 160, -1),       # ragged rows and columns, two K-steps
          (256, 128, 32, 0, 128, -1),       # a single K-step: the ring's prologue is its epilogue
          (130, 96, 32, 64, 128, -1),       # the source switch behind an odd step, N below one column tile, out_stride > N
          (512, 256, 1024, 512, 256, -1),   # long accumulation, 48 steps
          (2304, 384, 64, 0, 384, 8)]       # 27 items on 8 blocks: several items per block, a ragged last round


@pytest.fixture()
def hooks():
    """The process-wide hooks back at their defaults afterwards."""
    L = _lib.lib()
    yield L
    L.irsde_debug_force_split3_blocks(-1)
    L.irsde_debug_force_split3_1x1(-1)
    L.irsde_debug_force_split3_attn(-1)
    L.irsde_debug_force_split3(-1)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _run(d0, d1, dw, dbias, M, N, C0, C1, ostr, mode):
    """out [M][ostr] of the hook on a NaN-filled buffer with one guard row behind it"""
    out = torch.full((M + 1, ostr), float("nan"), device=DEV)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_split3_1x1(_ptr(d0), C0, C0, _ptr(d1), C1, C1, _ptr(dw), _ptr(dbias), _ptr(out), M, N, ostr, mode, None))
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_twins_two_launch_form_bias_and_float64(shape, hooks):
    M, N, C0, C1, ostr, cap = shape
    K = C0 + C1
    A, W = S3.inputs(M, N, K)
    A, W = A[0], W[0]
    bias = np.random.RandomState(M + N).standard_normal(N).astype(np.float32)
    d0 = torch.from_numpy(np.ascontiguousarray(A[:, :C0])).to(DEV)
    d1 = torch.from_numpy(np.ascontiguousarray(A[:, C0:])).to(DEV) if C1 else None
    dA, dw, db = torch.from_numpy(A).to(DEV), torch.from_numpy(W).to(DEV), torch.from_numpy(bias).to(DEV)
    if cap > 0:
        _lib.check(hooks.irsde_debug_force_split3_blocks(cap))
    # (a) the three launch forms agree bit for bit, (e) columns beyond N of a strided output and the guard row stay NaN
    full = [_run(d0, d1, dw, None, M, N, C0, C1, ostr, mode) for mode in (0, 1, 2)]
    for y in full:
        assert np.isfinite(y[:M, :N]).all() and np.isnan(y[:M, N:]).all() and np.isnan(y[M]).all()
    y = full[0][:M, :N]
    assert np.array_equal(y, full[1][:M, :N]) and np.array_equal(y, full[2][:M, :N])
    # (b) = split_triples_kernel on the concatenated A, then gemm_split3i_kernel
    two = torch.full((M, N), float("nan"), device=DEV)
    torch.cuda.synchronize()
    _lib.check(hooks.irsde_debug_split_gemm(_ptr(dA), _ptr(dw), _ptr(two), M, N, K, 1, 43, None))
    two = two.cpu().numpy()
    print("M=%d N=%d C0=%d C1=%d: elements differing from the two-launch form: %d of %d" % (M, N, C0, C1, int((y != two).sum()), y.size))
    assert np.array_equal(y, two)
    # (c) the bias is added in float32 behind the last product
    yb = _run(d0, d1, dw, db, M, N, C0, C1, ostr, 0)
    assert np.isnan(yb[:M, N:]).all() and np.isnan(yb[M]).all()
    assert np.array_equal(yb[:M, :N], y + bias[None, :])
    # (d) float64
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    wc = np.ascontiguousarray(W.reshape(N, K, 1, 1))
    x0 = np.ascontiguousarray(A.T.reshape(1, K, 1, M))
    native = run_conv(x0, None, wc, None, 1, 0, 0, None, 0, None, naive=0)[0, :, 0, :].T
    e, en, bar = S3.err(y, ref), S3.err(native, ref), S3.bar(A, W, ref)
    print("M=%d N=%d K=%d: three pieces %.3g, native f32 kernel %.3g, bar %.3g" % (M, N, K, e, en, bar))
    assert e < bar


def test_pixel_strides_wider_than_the_channel_counts():
    """the two sources as channel slices of wider tensors (pix0 = C0 + 32, pix1 = C1 + 96): bit-identical to the same values stored densely"""
    M, N, C0, C1 = 300, 160, 64, 32
    A, W = S3.inputs(M, N, C0 + C1)
    A, W = A[0], W[0]
    wide0 = np.full((M, C0 + 32), np.nan, np.float32)
    wide1 = np.full((M, C1 + 96), np.nan, np.float32)
    wide0[:, :C0], wide1[:, :C1] = A[:, :C0], A[:, C0:]
    dw = torch.from_numpy(W).to(DEV)
    d0, d1 = torch.from_numpy(np.ascontiguousarray(A[:, :C0])).to(DEV), torch.from_numpy(np.ascontiguousarray(A[:, C0:])).to(DEV)
    w0, w1 = torch.from_numpy(wide0).to(DEV), torch.from_numpy(wide1).to(DEV)
    dense = _run(d0, d1, dw, None, M, N, C0, C1, N, 0)
    out = torch.full((M + 1, N), float("nan"), device=DEV)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_split3_1x1(_ptr(w0), C0, C0 + 32, _ptr(w1), C1, C1 + 96, _ptr(dw), None, _ptr(out), M, N, N, 0, None))
    out = out.cpu().numpy()
    assert np.isfinite(out[:M]).all() and np.isnan(out[M]).all()
    assert np.array_equal(out, dense, equal_nan=True)


def test_layer_selector_vs_float64():
    """irsde_debug_conv selector 49 (the layer through launch_gemm_split3a): 64 + 32 -> 64, B = 2, 12 x 20 (M = 480: two row tiles, the second ragged), with bias"""
    rs = np.random.RandomState(3)
    B, H, W, C0, C1, Cout = 2, 12, 20, 64, 32, 64
    x0 = rs.standard_normal((B, C0, H, W)).astype(np.float32)
    x1 = rs.standard_normal((B, C1, H, W)).astype(np.float32)
    w = (rs.uniform(-1, 1, (Cout, C0 + C1, 1, 1)) / np.sqrt(C0 + C1)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    ref = oracle_conv(x0, x1, w, bias, 1, 0, 0, None, 0, None)
    e3 = relerr(run_conv(x0, x1, w, bias, 1, 0, 0, None, 0, None, naive=49), ref)
    ef = relerr(run_conv(x0, x1, w, bias, 1, 0, 0, None, 0, None, naive=0), ref)
    print("layer 64+32 -> 64, M = 480: selector 49 %.3g, native selector 0 %.3g" % (e3, ef))
    assert e3 < 2e-5


# ---- the network: nf = 32, depth = 2, 2 x 24 x 20 ----
NF, DEPTH, NB, NH, NW = 32, 2, 2, 24, 20


def _model(params, flags=0):
    m = P.ConditionalUNet(3, 3, NF, depth=DEPTH)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    m.engine_flags |= flags
    return m.to(DEV).eval()


def _describe(m, B, H, W):
    buf = ctypes.create_string_buffer(1 << 17)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return buf.value.decode()


def _rows_1x1(d):
    return [l.strip() for l in d.splitlines() if l.strip().startswith("conv M=") and " k=1x1 " in l]


def _shape(row):
    return tuple(int(row.split(k)[1].split()[0]) for k in ("M=", "Cout=", "Cin="))


# (M, Cout, Cin) of the network's 1x1 conv rows: the q projection 32 -> 128 and to_out 128 -> 32 of the level-0 LinearAttention blocks (C = 32 has no fused
# instance), the res_conv 64 -> 32 at level 0 (960 pixels), the up path's res_conv 192 -> 128 at level 1 (240 pixels, x2) and 96 -> 64 at level 0 (x2)
FORCED_ROWS = [(960, 128, 32), (960, 32, 128), (240, 128, 192), (240, 128, 192), (960, 64, 96), (960, 64, 96), (960, 32, 64)]


def test_network_forced_marker_golden_and_graph(golden, hooks):
    g = golden.forward
    tag = "nf32d2_2x24x20"
    params = O.synth_params(seed=0, nf=NF, depth=DEPTH)
    hooks.irsde_debug_force_split3_1x1(0)
    rows_off = _rows_1x1(_describe(_model(params), NB, NH, NW))
    hooks.irsde_debug_force_split3_1x1(2)
    m = _model(params)
    rows = _rows_1x1(_describe(m, NB, NH, NW))
    for r in rows:
        print(r)
    assert len(rows) == len(rows_off) > 0
    # The knob-0 plan of this network has exactly these seven 1x1 conv rows, all with at most a bias, stride 1, one launch, channels multiples of 32 (the
    # to_out row's LayerNorm is a launch of its own).  Every one is eligible (tests/test_split3_1x1_host.py feeds these shapes to the choice function), so
    # every one must carry the marker.
    assert sorted(_shape(r) for r in rows_off) == sorted(FORCED_ROWS)
    assert sorted(_shape(r) for r in rows if MARK in r) == sorted(FORCED_ROWS)
    for o, f in zip(rows_off, rows):   # a marked row is the row knob 0 shows, on another kernel and grid
        assert MARK not in o and o.split(" blocks=")[0] == f.split(" blocks=")[0]
    lq, xT = O.synth_inputs(1234, NB, NH, NW)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    for t in g[tag + "/ts"]:
        e = relerr(m(x, c, int(t)).cpu().numpy(), g[tag + "/t%d" % t])
        print("forward %s t=%d, every eligible 1x1 layer on three pieces, vs the reference: %.3g" % (tag, int(t), e))
        assert e < 1e-4
    T = 2
    lq, xT = O.synth_inputs(5, NB, NH, NW)
    z = O.synth_noise(7, T, (NB, 3, NH, NW))
    eager = _sample(m, "sde", T, lq, xT, z, graph=False)
    graph = _sample(m, "sde", T, lq, xT, z, graph=True)
    assert np.isfinite(eager).all() and np.array_equal(eager, graph)


def test_network_switches(hooks):
    """IRSDE_FLAG_NO_SPLIT3 = the master mode 0 = knob 0, bit for bit; all three differ from the forced mode; the rule adopts no layer of this network"""
    params = O.synth_params(seed=0, nf=NF, depth=DEPTH)
    lq, xT = O.synth_inputs(1234, NB, NH, NW)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)

    def run(m):
        return _describe(m, NB, NH, NW), m(x, c, 50).cpu().numpy()

    hooks.irsde_debug_force_split3_attn(0)   # (the fused attention blocks on their f32 kernels throughout: the 1x1 layers are the only three-piece launches)
    hooks.irsde_debug_force_split3_1x1(2)
    d_on, y_on = run(_model(params))
    d_flag, y_flag = run(_model(params, _lib.FLAG_NO_SPLIT3))
    hooks.irsde_debug_force_split3(0)
    d_master, y_master = run(_model(params))
    hooks.irsde_debug_force_split3(-1)
    hooks.irsde_debug_force_split3_1x1(0)
    d_off, y_off = run(_model(params))
    assert MARK in d_on
    for d in (d_flag, d_master, d_off):
        assert "split3a" not in d
    assert "bf16x3" not in d_flag and "bf16x3" not in d_master
    assert _rows_1x1(d_flag) == _rows_1x1(d_master) == _rows_1x1(d_off)
    assert np.array_equal(y_flag, y_master) and np.array_equal(y_flag, y_off)
    assert np.isfinite(y_on).all() and not np.array_equal(y_on, y_off)
    # the master's mode 2 does not force it
    hooks.irsde_debug_force_split3(2)
    assert "split3a" not in _describe(_model(params), NB, NH, NW)
    hooks.irsde_debug_force_split3(-1)
    # the rule (knob 1, the default)
    hooks.irsde_debug_force_split3_1x1(-1)
    assert "split3a" not in _describe(_model(params), NB, NH, NW)


# the rows the rule adopts on the benchmarked plan (profiles/split3_1x1.md, section 3): (M, Cout, Cin)
# the eight res_conv of the up path from 192 -> 128 up and the three to_qkv with at least 1e10 FLOP: 11 rows; the ninth res_conv (128 -> 64 at level 0), the
# to_qkv 512 -> 384 at 32 x 32 and the four to_out (128 -> C) stay on the f32 kernels
ADOPTED_16x256 = [(16384, 1024, 1536)] * 2 + [(65536, 512, 768)] * 2 + [(262144, 256, 384)] * 2 + [(1048576, 128, 192)] * 2 + \
                 [(16384, 384, 1024), (16384, 384, 1024), (65536, 384, 512)]


def test_plan_pin_16x256(hooks):
    """irsde_plan_describe at 16 x 256 x 256 (plan only, nothing runs): the rows the rule adopts carry the marker, no other row does"""
    m = _model_full()
    rows = _rows_1x1(_describe(m, 16, 256, 256))
    marked = sorted(_shape(r) for r in rows if MARK in r)
    print(marked)
    assert marked == sorted(ADOPTED_16x256)
    assert not any(MARK in r for r in rows if "Cout=64 Cin=128" in r)


def _model_full():
    m = P.ConditionalUNet(3, 3, 64, depth=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0).items()})
    return m.to(DEV).eval()
