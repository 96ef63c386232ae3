"""Prompt attention parity table: every case of tests/prefill_probe.py (the table tests/test_attn_prefill_probe_gpu.py asserts on)
through ops.attention on each of the four pinned paths, with the kernel launched, the number of 64-key tiles and the worst error
against the fp64 reference as a multiple of the tolerance (rtol 2^-6, atol 2e-2; <= 1 passes).

    python tools/prefill_probe_parity.py > profiles/prefill_probe_parity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch                                               # noqa: E402

import prefill_probe as pp                                 # noqa: E402
from phi_3_vision_mlx_amd import ops                       # noqa: E402


def main():
    ops.L.lib()
    print(f"{'case':32s} {'path':5s} {'kernel':32s} {'tiles':>5s} {'head_group':>10s} {'rows':>5s} {'max|ref|':>8s} {'max err':>8s} {'err/tol':>7s} {'2nd launch':>10s}")
    worst = 0.0
    for c in pp.CASES:
        pr = pp.Probe(c)
        for path in pp.PATHS:
            res = pp.launch(ops, pr, path)
            got = res["out"][:, pr.rows].double()
            ratio = pp.worst_ratio(got[pr.live], pr.ref[pr.live]) if bool(torch.isfinite(got).all()) else float("inf")
            worst = max(worst, ratio)
            same = torch.equal(res["out2"].view(torch.int16), res["out"].view(torch.int16))
            print(f"{c.id:32s} {path:5s} {pp.KERNELS[path].format(hd=c.hd):32s} {c.n_tiles:5d} {c.head_group:4d} /{c.nh:3d}  {len(pr.rows):5d} "
                  f"{float(pr.ref.abs().max()):8.3f} {float((got - pr.ref)[pr.live].abs().max()):8.5f} {ratio:7.3f} {'same bits' if same else 'DIFFERS':>10s}")
    print(f"{len(pp.CASES)} cases x {len(pp.PATHS)} paths, worst error / tolerance {worst:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
