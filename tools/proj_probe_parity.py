"""Projection parity table: the lines tests/test_proj_kernels_gpu.py and tests/test_qproj_kernels_gpu.py print per case and family -- `id [family]: kernel: result` -- as
columns.  The test is the only thing that runs the kernels; this reads its output.

    python -m pytest -m gpu -s -q tests/test_proj_kernels_gpu.py | python tools/proj_probe_parity.py > profiles/proj_probe_parity.txt
    python -m pytest -m gpu -s -q tests/test_qproj_kernels_gpu.py | python tools/proj_probe_parity.py > profiles/qproj_probe_parity.txt"""
import re
import sys


def main():
    rows = [m.groups() for m in (re.match(r"^\.*(\S+) \[([a-z-]+)\]: ([^:]+): (.*)$", line.rstrip()) for line in sys.stdin) if m]
    if not rows:
        print("no result lines on stdin (run the test with -s)", file=sys.stderr)
        return 1
    w0, w1, w2 = (max(len(r[i]) for r in rows) for i in range(3))
    print(f"{'case':<{w0}}  {'family':<{w1}}  {'kernel':<{w2}}  result (smallest multiple of E that accepts; memory outside [M, N])")
    for case, family, kernel, result in rows:
        print(f"{case:<{w0}}  {family:<{w1}}  {kernel:<{w2}}  {result}")
    exact = sum("bit-exact" in r[3] and "outside E" not in r[3] for r in rows)
    print(f"{len(rows)} runs, {exact} bit-exact against the rounded fp64 reference")
    return 0


if __name__ == "__main__":
    sys.exit(main())
