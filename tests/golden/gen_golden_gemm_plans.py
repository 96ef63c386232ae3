"""Records the two host queries of the bf16 prefill GEMM -- p3v_gemm_ws_bytes and p3v_gemm_rows_slices -- over a grid of shapes,
epilogues and knob settings: the fixture of tests/test_gemm_route_cpu.py (tests/golden/gemm_plans.json).  No GPU.

    python tests/golden/gen_golden_gemm_plans.py          # rewrites tests/golden/gemm_plans.json

Recorded on the tree BEFORE the route existed, through the two exported queries alone; the file must come out byte-identical from any
later tree.  Per (variant, M, N, K, epilogue), in `grid()`'s order, one symbol of the table of distinct outcomes [S, rows_slices]:
p3v_gemm_ws_bytes == S * M * (2 N for SiLU, else N) * 4 for S > 1 and 0 for S <= 1 (checked here), rows_slices as answered.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")
MS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300, 1023, 1024, 1025, 2531)
NS = (64, 96, 192, 1024, 3072, 4096, 8192, 9216, 32064)
KS = (64, 384, 512, 768, 1024, 3072, 8192)
EPIS = tuple(range(9))
SILU = 6
VARIANTS = ((), ("gemm_skinny_tm128", 1), ("gemm_skinny_s", 1), ("gemm_skinny_s", 2), ("gemm_no_skinny", 1), ("gemm_no_splitk", 1),
            ("gemm_big_rows", 0), ("gemm_big_rows", 256), ("gemm_big_rows", 1000000), ("gemm_128", 1), ("gemm_persistent", 0),
            ("gemm_no_qkv_fuse", 1))
SYMBOLS = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")


def grid():
    return itertools.product(MS, NS, KS, EPIS)


def variant_name(v):
    return "default" if not v else "%s=%d" % v


def record():
    from phi_3_vision_mlx_amd import _lib
    lib = _lib.lib()
    table, cases = [], {}
    for v in VARIANTS:
        old = ctypes.c_int(0)
        if v:
            assert lib.p3v_get_tuning(v[0].encode(), ctypes.byref(old)) == 0 and lib.p3v_set_tuning(v[0].encode(), v[1]) == 0
        row = []
        for M, N, K, epi in grid():
            ws, rs = lib.p3v_gemm_ws_bytes(M, N, K, epi), lib.p3v_gemm_rows_slices(M, N, K, epi)
            unit = M * (2 * N if epi == SILU else N) * 4
            assert ws % unit == 0 and ws // unit != 1, (M, N, K, epi, ws)
            outcome = [ws // unit or 1, rs]
            if outcome not in table:
                table.append(outcome)
            row.append(SYMBOLS[table.index(outcome)])
        if v:
            assert lib.p3v_set_tuning(v[0].encode(), old.value) == 0
        cases[variant_name(v)] = "".join(row)
    return {"axes": {"M": MS, "N": NS, "K": KS, "epilogue": EPIS}, "outcome": ["S", "rows_slices"],
            "outcomes": dict(zip(SYMBOLS, table)), "cases": cases}


def dumps(rec):
    lines = [json.dumps([k, rec[k]], separators=(",", ":")) for k in ("axes", "outcome", "outcomes")]
    lines += [json.dumps(["case", k, v], separators=(",", ":")) for k, v in rec["cases"].items()]
    return "[\n" + ",\n".join(lines) + "\n]\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    text = dumps(record())
    with open(PATH, "w") as f:
        f.write(text)
    print(f"wrote {PATH}: {len(text)} bytes")
