"""Decode attention parity table: every case of tests/attn_probe.py (the table tests/test_attn_probe_gpu.py asserts on) through
ops.attention_decode / ops.attention_decode_q8, with the kernel the launcher picks and the worst error against the fp64
reference as a multiple of the tolerance (rtol 2^-6, atol 2e-2; <= 1 passes).  int8 cases: also the fp64 restatement of the kernels'
documented roundings (fp16 q, fp16 P x V scale) against the plain reference -- no kernel involved -- and the kernel against it.

    python tools/attn_probe_parity.py > profiles/attn_probe_parity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import attn_probe as ap                                    # noqa: E402
from phi_3_vision_mlx_amd import ops                       # noqa: E402


def main():
    ops.L.lib()
    print(f"{'case':64s} {'kernel':44s} {'tiles/split':>11s} {'live splits':>11s} {'max|ref|':>8s} {'max err':>8s} {'err/tol':>7s} {'restated/tol':>12s} {'vs restated':>11s}")
    worst = 0.0
    for c in ap.CASES:
        pr = ap.Probe(c)
        out = ap.launch(ops, pr)["out"]
        ratio = ap.worst_ratio(out, pr.ref)
        worst = max(worst, ratio)
        live = len({s for b in range(c.B) for s in pr.live[b]})
        extra = ""
        if c.kind == "q8":
            rs = ap.restated(pr)
            extra = f" {ap.worst_ratio(rs, pr.ref):12.3f} {ap.worst_ratio(out, rs):11.3f}"
        print(f"{c.id:64s} {c.kernel:44s} {c.chunk // 64:11d} {live:5d} /{c.n_split:4d} {float(pr.ref.abs().max()):8.3f} "
              f"{float((out.double() - pr.ref).abs().max()):8.5f} {ratio:7.3f}{extra}")
    print(f"{len(ap.CASES)} cases, worst error / tolerance {worst:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
