"""The reference-only figures behind the bounds of tests/test_gpu_conv_rows.py, measured on the CPU (no device): for every case of
tests/conv_rows_oracle.py a float32 numpy restatement of the layer (`reference(..., dtype=np.float32)`: float32 products and sums in numpy's order) against the
float64 oracle, on the table's own inputs.

    16-bit tensors    share of elements whose stored value differs between the two (the test caps the kernel's share at 2 %), and the worst excess over the
                      elementwise bound 2^-7 / 2^-10 |ref| + 1e-6 (<= 0: inside)
    16-bit operands   the operand-rounded oracle against the full one: where the kernel's own error must land inside the mode's band
    everything        float32 against float64 relative to max|ref|: what a correct fp32-accumulating kernel may differ by

The halo family's table (tests/conv_halo_cases.py, the figures behind tests/test_gpu_conv_halo.py) follows, one line per layer: the same figures; for the bf16-tensor
layers the share of differing elements is what the 2 % cap of the GPU test asks of the inputs (at most 0.2 %: profiles/conv_halo.md).

Usage: python tools/conv_rows_cpu_figures.py  (prints one line per case and the maxima per class; profiles/conv_rows.md and profiles/conv_halo.md quote them)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import conv_halo_cases as H  # noqa: E402
import conv_rows_oracle as R  # noqa: E402
from oracle import irsde_oracle as O  # noqa: E402

OPERANDS = {0: None, 1: "bf16", 2: "f16"}
ULPS = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}
ROUND = {"bf16": O.round_bf16, "f16": O.round_f16}


def main():
    table(R.CASES, R.tensors, "")
    layers = {c["inputs"]: c for c in H.CASES}   # one line per layer: the tuning codes of a layer share its inputs
    table([dict(c, name=stem) for stem, c in layers.items()], H.case_tensors, "halo ")


def table(cases, tensors, tag):
    worst = {}
    for c in cases:
        if tag == "" and c["row"] is None:
            continue
        operand, storage, pair = c["mode"]
        ops, st = (None if pair else OPERANDS[operand]), OPERANDS[storage]
        t = tensors(c)
        ref = R.reference(c, t, operands=ops, storage=st)
        r32 = R.reference(c, t, operands=ops, storage=st, dtype=np.float32).astype(np.float64)
        line = "%-24s" % c["name"]
        feature = "ln" if c["feat"] & R.LN_G else "gate" if c["feat"] & R.GATE else "plain"
        if st:
            err = np.abs(r32 - ref)
            share, excess = float((err > 0).mean()), float((err - (np.abs(ref) * ULPS[st] + 1e-6)).max())
            line += " share_differing=%.4f%% worst_excess=%.3g" % (100 * share, excess)
            worst[st + " tensors: share differing"] = max(worst.get(st + " tensors: share differing", 0), share)
            worst[st + " tensors: worst excess"] = max(worst.get(st + " tensors: worst excess", -1), excess)
        else:
            e = R.relerr(r32, ref)
            line += " f32_vs_f64=%.3g" % e
            worst["f32 vs f64, " + feature] = max(worst.get("f32 vs f64, " + feature, 0), e)
            if ops:
                b = R.relerr(ref, R.reference(c, t))
                line += " rounded_vs_full=%.3g" % b
                worst[ops + " operands: rounded vs full, max"] = max(worst.get(ops + " operands: rounded vs full, max", 0), b)
                worst[ops + " operands: rounded vs full, min"] = min(worst.get(ops + " operands: rounded vs full, min", 1), b)
        print(tag + line)
    for k in sorted(worst):
        print("%sMAX %-40s %.4g" % (tag, k, worst[k]))


if __name__ == "__main__":
    main()
