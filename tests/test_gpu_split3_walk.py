"""GPU tests of the three-piece GEMM's persistent launch (csrc/gemm_split.hip, gemm_split3i_kernel<ABL, WALK = true>): at most one block per compute unit, each
walking several (component, row tile, column tile) items as one pipelined loop, the next item's first LDS stage in flight while the finished accumulators go out.

Twin: irsde_debug_split_gemm selector 43 is the production launch (the walk), selector 45 the one-item-per-block launch of the same kernel (selector 44, which the
issue named for it, has long been the fp16 pair kernel of tests/test_gpu_split.py, so the twin took the next free number).  Per output element both run the
same six products in the same order over the same K order, so the two must agree bit for bit.  irsde_debug_force_split3_blocks caps the walk's grid so that a
small problem makes every block walk several items.

float64 bar: tests/split3_oracle.py's, three times the error of numpy's float32 product on the same inputs, as in tests/test_gpu_split3.py; it pins selector 43
on its own (a walk that was wrong in both selectors would need selector 45 to have changed too).

Writer: the polyphase Upsample input transform stores its triples as whole 384-byte row-pair blocks through LDS (irsde_debug_conv selector 27); selector 28 runs
the same layer with the per-thread writer.  Same loads, same transform order, same splitting per thread: the layer outputs must agree bit for bit, and both
stay inside the 5e-5 bar of tests/test_gpu_split3.py against the float64 direct convolution.

Plan: the F(4x4,3x3) layers with exactly 512 input channels and at least 512 output channels now have their weights' triples.  The smallest network whose default
rule admits one is nf = 32, depth = 4 at 8 x 256 x 256: its 512 -> 512 layers on the 32 x 32 map have T = 8 * 8 * 8 = 512 tiles (>= the 256-row floor), 512
output channels and 36 * 2 * 512 * 512 * 512 = 9.66e9 executed FLOP (>= 9e9); with fewer than 1024 tiles the fused kernels do not take them, so they are
three-launch layers on either arithmetic.  Network bar: 1e-4 of max |output| between the two engines, the bar of tests/test_gpu_split3.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_restoration_sde_amd as P
from image_restoration_sde_amd import _lib
from oracle import irsde_oracle as O

import split3_oracle as S3
import wino_poly_oracle as WP
from test_gpu_parity import DEV, _sample, relerr, run_conv

pytestmark = pytest.mark.gpu

# (M, N, K, ncomp, block cap); cap -1 = the default, one block per compute unit.  Tiles are 256 x 128, an item = (component, row tile, column tile).
WALK = [(300, 160, 32, 5, 8),        # one K-step per item: the prefetch crosses an item boundary at every step; ragged rows and columns; 20 items on 8 blocks
        (256, 256, 64, 3, 8),        # two steps; six items on eight blocks: some blocks get none
        (130, 512, 96, 36, 8),       # odd step count; 36 units do not divide by 8 XCDs; 4 - 5 units = 16 - 20 items per block
        (512, 128, 64, 25, 24),      # 50 items on three blocks per XCD
        (512, 128, 64, 25, 20),      # a cap that is no multiple of 8: XCDs 0 - 3 hold three blocks, 4 - 7 two
        (512, 256, 64, 100, -1)]     # 400 items on a full grid: one or two per block


@pytest.fixture()
def cap():
    """Sets the process-wide grid cap; back at the default (-1) afterwards."""
    L = _lib.lib()
    yield lambda n: _lib.check(L.irsde_debug_force_split3_blocks(n))
    L.irsde_debug_force_split3_blocks(-1)


def _run(A, B, sel):
    """C of selector `sel` on a NaN-filled buffer with one guard row behind [ncomp][M][N]; returns (C, guard row)"""
    ncomp, M, K = A.shape
    N = B.shape[1]
    dA, dB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    dC = torch.full((ncomp * M + 1, N), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    _lib.check(_lib.lib().irsde_debug_split_gemm(p(dA), p(dB), p(dC), M, N, K, ncomp, sel, None))
    C = dC.cpu().numpy()
    return C[:-1].reshape(ncomp, M, N), C[-1]


@pytest.mark.parametrize("shape", WALK)
def test_walk_equals_one_item_per_block_bit_for_bit(shape, cap):
    M, N, K, ncomp, blocks = shape
    A, B = S3.inputs(M, N, K, ncomp)
    cap(blocks)
    walk, guard = _run(A, B, 43)
    twin, guard_t = _run(A, B, 45)
    assert np.isfinite(walk).all() and np.isfinite(twin).all()         # every element of [M][N] written ...
    assert np.isnan(guard).all() and np.isnan(guard_t).all()           # ... and nothing behind the last row
    assert np.array_equal(walk, twin)


@pytest.mark.parametrize("shape", WALK[:3])
def test_walk_vs_float64(shape, cap):
    M, N, K, ncomp, blocks = shape
    A, B = S3.inputs(M, N, K, ncomp)
    ref = np.einsum("zmk,znk->zmn", A.astype(np.float64), B.astype(np.float64))
    bar = S3.bar(A, B, ref)
    cap(blocks)
    C, _ = _run(A, B, 43)
    e = S3.err(C, ref)
    print("three-piece gemm, walk on %d blocks, %s: %.3g (bar %.3g = 3 x numpy float32)" % (blocks, shape[:4], e, bar))
    assert np.isfinite(C).all() and e < bar


def test_cap_below_one_block_per_xcd_is_refused(cap):
    L = _lib.lib()
    assert L.irsde_debug_force_split3_blocks(3) != 0 and L.irsde_debug_force_split3_blocks(0) != 0
    cap(-1)


# ---------------------------------------------------------------------------------------------
# the whole-line triple writer of the polyphase Upsample against its per-thread twin
# ---------------------------------------------------------------------------------------------
# (B, C, H, W, Cout)
WRITER = [(1, 64, 8, 8, 32),        # the case of tests/test_gpu_split3.py: T = 4, two 32-k blocks
          (1, 96, 12, 12, 32),      # T = 9: an odd tile count, so the pad row; three 32-k blocks
          (3, 32, 6, 10, 64)]       # ragged tiles on both axes, one 32-k block, several images: 18 tiles = 36 groups, the third work-group a quarter full


@pytest.mark.parametrize("case", WRITER)
def test_whole_line_writer_equals_per_thread_writer_bit_for_bit(case):
    Bn, C, Hh, Ww, Cout = case
    rs = np.random.RandomState(C + Hh)
    x0 = rs.standard_normal((Bn, C, Hh, Ww)).astype(np.float32)
    w = (rs.standard_normal((Cout, C, 3, 3)) / np.sqrt(C * 9)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    args = (x0, None, w, bias, 1, 1, 1, None, 0, None)
    ref = WP.direct_up(x0, w, bias)
    lines, threads = run_conv(*args, naive=27), run_conv(*args, naive=28)
    e = relerr(lines, ref)
    print("polyphase up %s on triples: whole-line writer %.3g, per-thread writer %.3g" % (case, e, relerr(threads, ref)))
    assert lines.shape == ref.shape and np.isfinite(lines).all() and e < 5e-5
    assert np.array_equal(lines, threads)


# ---------------------------------------------------------------------------------------------
# plan: the Cin = 512 layers on the three-piece GEMM
# ---------------------------------------------------------------------------------------------
NF, DEPTH, B, H, W = 32, 4, 8, 256, 256


def _fresh(flags=0):
    m = P.ConditionalUNet(3, 3, NF, depth=DEPTH)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.synth_params(seed=0, nf=NF, depth=DEPTH).items()}, strict=True)
    m.engine_flags = flags
    return m.to(DEV).eval()


def _rows512(m):
    buf = ctypes.create_string_buffer(1 << 17)
    _lib.check(_lib.lib().irsde_plan_describe(m.engine().h, B, H, W, buf, len(buf)))
    return [l.split("ms", 1)[-1].strip() for l in buf.value.decode().splitlines() if "conv(winograd F4 gemm x36) T=512 Cout=512 Cin=512 " in l]


@pytest.fixture(scope="module")
def engines():
    return _fresh(), _fresh(_lib.FLAG_NO_SPLIT3)


def test_cin512_layers_plan_marker_and_forward(engines):
    on, off = engines
    r_on, r_off = _rows512(on), _rows512(off)
    print("\n".join(r_on[:1] + r_off[:1]))
    assert len(r_on) >= 2 and all(r.endswith(" bf16x3") for r in r_on), r_on
    assert r_off == [r[:-len(" bf16x3")] for r in r_on], r_off          # the flag: the same rows on the f32 GEMM
    lq, xT = O.synth_inputs(1234, B, H, W)
    x, c = torch.from_numpy(xT).to(DEV), torch.from_numpy(lq).to(DEV)
    y_on, y_off = on(x, c, 50).cpu().numpy(), off(x, c, 50).cpu().numpy()
    e = float(np.abs(y_on - y_off).max() / np.abs(y_off).max())
    print("nf=%d depth=%d %dx%dx%d, three-piece against f32 GEMMs: %.3g of max |output|" % (NF, DEPTH, B, H, W, e))
    assert np.isfinite(y_on).all() and e < 1e-4
    assert not np.array_equal(y_on, y_off)


def test_cin512_plan_graph_replay_is_bit_identical_to_eager(engines):
    m, T = engines[0], 2
    lq, xT = O.synth_inputs(5, B, H, W)
    z = O.synth_noise(7, T, (B, 3, H, W))
    eager = _sample(m, "sde", T, lq, xT, z, graph=False)
    graph = _sample(m, "sde", T, lq, xT, z, graph=True)
    assert np.isfinite(eager).all() and np.array_equal(eager, graph)
