"""naf_chain_kernel (csrc/naf_chain.hip) on its own against the float64 restatement of tests/naf_chain_oracle.py (run with -m gpu on an MI355X): the hook
irsde_debug_naf_chain packs the caller's reference-layout weights with the engine's packer and runs the production launcher once, with 1, 2 or 4 work-groups
per image.  64 pixels x 512 channels per image is the only shape the kernel has; each case of naf_chain_oracle.CASES is named for one code path.  The metric
is max |err| / max |ref| on the branch sum out - x; the bar of a case is 4 x the error of the restated kernel arithmetic against float64 on that case's
inputs, capped at 2^-8 (profiles/naf_chain_parity.md; tests/test_naf_chain_host.py shows on the CPU that a wrong pooled mean, image or block row, FiLM
half, pad, gate pairing, scale placement or variance formula misses these bars at least tenfold).

Every call runs once: no retries; a non-zero return fails the test with the library's message.  The output sits between two guards of sentinel floats
and starts as NaN (tests/test_gpu_naf_glue.py's Guarded); FiLM / lens buffers hold NaN outside the rows a correct kernel reads.

One MI355X run: 12 tests in 3.25 s, measured errors 0.90 - 1.00 x the restated arithmetic's own (profiles/naf_chain_parity.md).
"""
import functools

import numpy as np
import pytest
import torch

from image_restoration_sde_amd import _lib
import naf_chain_oracle as N
from test_gpu_naf_glue import DEV, Guarded, dev, ptr

pytestmark = pytest.mark.gpu


def run_chain(name, groups, out=None):
    """One call of the hook on the inputs of case `name` with `groups` work-groups per image -> out [B, 64, 512] (guards and finiteness checked)."""
    _, B, nb, per_image, lens, film_off, cam_off, _ = N.CASES[name]
    inp = N.inputs(name)
    x = dev(inp["x"])
    fbuf, fstride = N.row_buffer(inp["film"], film_off)
    film = dev(fbuf)
    cam, cstride = None, 0
    if lens:
        cbuf, cstride = N.row_buffer(inp["cam"], cam_off)
        cam = dev(cbuf)
    out = out or Guarded(B, N.PX, N.C)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().irsde_debug_naf_chain(ptr(x), out.ptr(), B, nb, *[ptr(inp[k]) for k in N.WEIGHTS], ptr(film), fstride, film_off, ptr(cam), cstride,
                                                    cam_off if lens else 0, groups, _lib.stream_ptr()))
    assert torch.equal(x, dev(inp["x"])), name + ": the input was written"
    return out.result("%s, %d groups" % (name, groups))


@functools.lru_cache(maxsize=None)
def one_group(name):
    return run_chain(name, 1)


@pytest.mark.parametrize("name", list(N.CASES))
def test_chain_vs_float64(name):
    groups = N.CASES[name][0]
    inp = N.inputs(name)
    ref, bar, self_err, _ = N.reference(name)
    got = one_group(name) if groups == 1 else run_chain(name, groups)
    e = N.branch_err(got, inp["x"], ref)
    print("naf_chain %-22s float32 flavour %.3g, bar %.3g, measured %.3g" % (name, self_err, bar, e))
    assert e <= bar, (name, e, bar)
    if groups > 1:   # the groups trade slices, not arithmetic: the one-group kernel's bits
        assert np.array_equal(got, one_group(name)), name


@pytest.mark.parametrize("name", ["g1_b3_lens", "g2_b2_n2", "g4_b9_n3"])
def test_chain_ignores_what_out_held_and_repeats(name):
    """`out` pre-filled (with more than one group per image it doubles as the exchange buffer of the residual stream), then a second call in a row into the
    same tensor: both equal the first result.  The hook itself fails a call that leaves a barrier counter or the error word set."""
    groups, B = N.CASES[name][:2]
    want = one_group(name)
    out = Guarded(B, N.PX, N.C)
    out.view.copy_(torch.linspace(-3e4, 3e4, out.n, device=DEV))
    first = run_chain(name, groups, out).copy()
    second = run_chain(name, groups, out)
    assert np.array_equal(first, want) and np.array_equal(second, want)


def test_hook_refuses_what_a_launcher_cannot_run():
    """Refused on the host, before any launch: the call fails with an error string and writes nothing."""
    L = _lib.lib()
    name = "g1_b1_shared_nolens"
    inp = N.inputs(name)
    x, film = dev(inp["x"]), dev(N.row_buffer(inp["film"], 0)[0])
    out = torch.zeros(N.PX * N.C, device=DEV)
    w = [ptr(inp[k]) for k in N.WEIGHTS]
    s = _lib.stream_ptr()

    def call(B=1, nb=1, fstride=0, foff=0, groups=1, xp=ptr(x)):
        return L.irsde_debug_naf_chain(xp, ptr(out), B, nb, *w, ptr(film), fstride, foff, None, 0, 0, groups, s)

    assert call(groups=3) != 0 and b"groups must be 1, 2 or 4" in L.irsde_last_error()
    assert call(groups=0) != 0
    assert call(nb=0) != 0 and b"debug_naf_chain" in L.irsde_last_error()
    assert call(B=0) != 0
    assert call(fstride=2) != 0 and call(foff=6) != 0
    assert call(xp=None) != 0
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    B = 8 * (ncu // 32) + 1   # 8 ceil(B / 8) * 4 work-groups: one slot of eight images more than the compute units hold
    assert call(B=B, groups=4) != 0 and b"co-resident" in L.irsde_last_error()
    assert float(out.abs().sum()) == 0.0
