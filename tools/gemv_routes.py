"""Which kernel the library launches for a decode projection call -- the recording behind tests/golden/gemv_routes.json and
profiles/gemv_routes.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o routes -- python tools/gemv_routes.py DIR/cases.json
    python tools/gemv_routes.py --join DIR/cases.json DIR/..._kernel_trace.csv [tests/golden/gemv_routes.json [table.txt]]

The first form calls ops.gemv / gemv_fp8 / gemv_q4 / gemv_b13 / gemv_step_begin / gemv_step_end once per case of `cases()` on zero
tensors (a refused call is recorded by its error code), with one k_stage_rope launch in front of every case as a separator, and writes
the case list.  It asks the library nothing but the call itself, so it runs on any commit that has the entries.  The second form joins
the trace with the list: per case the kernel names in order, each with its grid (in workgroups) and block.  The cases are the smallest
calls that reach every branch and both sides of every threshold, plus the model's own shapes for the streaming kernel's plan.
"""
import csv
import json
import os
import re
import sys

NONE, BIAS, RESID, SILU, F32 = 0, 1, 5, 6, 8
BF16, FP8, Q4, B13 = "bf16", "fp8", "q4", "b13"
MODEL = ((9216, 3072, NONE), (8192, 3072, SILU), (3072, 3072, RESID), (3072, 8192, RESID), (32064, 3072, NONE))   # qkv, gate_up, o, down, head
BANDS = (1, 2, 4, 5, 8, 9, 16, 17)


def cases():
    """dicts of fmt, step ("none" / "begin" / "end"), M, N, K, epilogue, has_norm, exp_base, knobs."""
    out = []

    def add(fmt, M, N, K, epi=NONE, step="none", norm=0, base=0, **knobs):
        c = dict(fmt=fmt, step=step, M=M, N=N, K=K, epilogue=epi, has_norm=norm, exp_base=base or (97 if fmt == B13 else 0), knobs=knobs)
        if c not in out:                                       # (two of the sweeps below cross at a point)
            out.append(c)

    # ---- bf16: the M bands at both streaming K; every K at one, five and nine rows
    for M in BANDS:
        add(BF16, M, 264, 3072)
        add(BF16, M, 24, 8192)
    for K in (520, 1024, 2048, 4096, 5120):
        for M in (1, 5, 9):
            add(BF16, M, 100, K)
    for N in (16, 24, 100, 264, 272):                          # the MFMA kernels' row sets, with the SiLU halves
        for epi in (NONE, SILU):
            add(BF16, 8, N, 3072, epi)
            add(BF16, 9, N, 1024, epi)
    for M in (1, 2, 5, 9):                                     # the epilogues (the bands above ran NONE)
        for epi in (RESID, SILU, F32, BIAS):
            add(BF16, M, 264, 3072, epi)
    add(BF16, 1, 264, 3072, norm=1)
    add(BF16, 5, 264, 3072, norm=1)
    for M in (1, 2, 5):                                        # N odd: no streaming kernel
        add(BF16, M, 101, 3072)
    add(BF16, 1, 264, 3072, gemv_variant=1)                    # each knob flipped
    add(BF16, 2, 264, 3072, gemv_variant=1, gemv8_min=5)
    for M in (2, 3, 4, 5):
        for K in (3072, 8192):
            add(BF16, M, 264, K, gemv8_min=5)
    add(BF16, 2, 264, 3072, F32, gemv8_min=5)                  # the rows stream has no fp32 output
    add(BF16, 2, 101, 3072, gemv8_min=5)
    add(BF16, 2, 264, 1024, gemv8_min=5)
    add(BF16, 2, 264, 3072, gemv8_min=5, gemv_rows=0)
    add(BF16, 4, 264, 3072, gemv8_min=4)
    for M in (2, 5, 8):
        add(BF16, M, 264, 3072, gemv_mfma8=0)
    for M in (1, 2, 3, 5, 9):
        add(BF16, M, 264, 1024, gemv_mfma8=0, gemv_no_mfma=1)
    add(BF16, 9, 264, 3072, gemv_no_mfma=1)
    add(BF16, 8, 4112, 1024)                                   # 257 row sets: two per workgroup
    add(BF16, 8, 4096, 1024)
    add(BF16, 8, 2064, 1024, gemv8_wgs=64)
    add(BF16, 8, 2064, 1024, SILU, gemv8_wgs=64)
    add(BF16, 1, 16400, 520)                                   # k_gemv: 2050 workgroups asked for, 2048 launched
    add(BF16, 1, 16384, 520)
    add(BF16, 8, 16, 10216)                                    # k_gemv: the last K whose eight rows fit LDS, and the first that does not
    add(BF16, 8, 16, 10224)
    add(BF16, 1, 9216, 3072, gemv_wpc=4)
    add(BF16, 1, 9216, 3072, gemv_wpw=3)
    add(BF16, 1, 9216, 3072, gemv_wpw=4)
    add(BF16, 1, 3072, 8192, gemv_wpc=16)
    # ---- e4m3
    for M in BANDS:
        add(FP8, M, 24, 3072)
    for M in (1, 5, 9):
        add(FP8, M, 24, 8192)
        add(FP8, M, 100, 3072, SILU)
    for epi in (RESID, F32, BIAS):
        add(FP8, 1, 24, 3072, epi)
    add(FP8, 5, 24, 3072, gemv_no_mfma8=1)
    add(FP8, 1, 24, 4096)
    add(FP8, 1, 25, 3072)
    add(FP8, 1, 9216, 3072, gemv_f8_wpc=8)
    # ---- 4-bit
    for M in BANDS:
        add(Q4, M, 272, 3072)
    for M in (1, 2, 9):
        add(Q4, M, 272, 8192)
        add(Q4, M, 264, 3072, SILU)                            # N % 8 serves the SiLU halves ...
        add(Q4, M, 264, 3072)                                  # ... N % 16 everything else
    for epi in (RESID, F32, BIAS):
        add(Q4, 1, 272, 3072, epi)
        add(Q4, 2, 272, 3072, epi)
    add(Q4, 2, 100, 3072)
    add(Q4, 1, 101, 3072)
    add(Q4, 2, 272, 4096)
    for M in (1, 8, 9):
        add(Q4, M, 272, 3072, norm=1)
    add(Q4, 2, 272, 3072, gemv_q4_rows8=0)
    add(Q4, 2, 272, 3072, norm=1, gemv_q4_rows8=0)
    add(Q4, 8, 4112, 3072)
    add(Q4, 8, 2064, 3072, gemv_q4_rows_wgs=64)
    add(Q4, 9, 2064, 3072, gemv_q4_rows_wgs=64)
    add(Q4, 1, 9216, 3072, gemv_q4_wpc=4)
    # ---- 13-bit codes: one row; the scaled form by exponent base, K and knob
    for K in (3072, 8192):
        for base in (97, 98):
            for xs in (1, 0):
                add(B13, 1, 264, K, base=base, gemv_b13_xscale=xs)
    for epi in (RESID, SILU, F32, BIAS):
        add(B13, 1, 264, 3072, epi)
    add(B13, 2, 264, 3072)
    add(B13, 1, 101, 3072)
    add(B13, 1, 264, 4096)
    add(B13, 1, 264, 3072, base=225)
    add(B13, 1, 264, 3072, norm=1)
    add(B13, 1, 9216, 3072, gemv_b13_wpc=8)
    # ---- the streaming kernel on the model's own matrices, one row: the 3- and the 4-wave form of the plan
    for fmt in (BF16, FP8, Q4, B13):
        for N, K, epi in MODEL:
            add(fmt, 1, N, K, epi)
    # ---- both ends of the folded step
    for fmt in (BF16, FP8, Q4, B13):
        for K in (3072, 8192):
            add(fmt, 1, 1024, K, step="begin", norm=1)
            add(fmt, 1, 4102, K, step="end", norm=1)
        add(fmt, 1, 9216, 3072, step="begin", norm=1)
        add(fmt, 1, 32064, 3072, step="end", norm=1)
        add(fmt, 1, 6200, 3072, step="begin", norm=1)          # 3100 row pairs: at 16 waves a CU more workgroups than the fold's workspace holds
        add(fmt, 1, 6200, 3072, step="end", norm=1)
        add(fmt, 2, 4102, 3072, step="end", norm=1)
        add(fmt, 1, 4101, 3072, step="end", norm=1)
        add(fmt, 1, 1024, 4096, step="begin", norm=1)
    add(BF16, 1, 1024, 3072, step="begin", norm=1, gemv_variant=1)
    add(BF16, 1, 4102, 3072, step="end", norm=1, gemv_variant=1)
    add(BF16, 1, 6200, 3072, step="end", norm=1, gemv_wpc=16)
    add(FP8, 1, 8192, 3072, step="end", norm=1, gemv_wpw=3)
    add(FP8, 1, 8192, 3072, step="end", norm=1, gemv_wpw=4)
    add(B13, 1, 6200, 3072, step="end", norm=1, gemv_b13_wpc_end=16)
    add(B13, 1, 6200, 3072, step="begin", norm=1, gemv_b13_wpc=8)
    add(B13, 1, 4102, 3072, step="end", norm=1, base=98)
    add(B13, 1, 4102, 3072, step="end", norm=1, gemv_b13_xscale=0)
    for c in out:
        c["id"] = "%s%s,M=%d,N=%d,K=%d,epi=%d%s%s%s" % (c["fmt"], "" if c["step"] == "none" else "_" + c["step"], c["M"], c["N"], c["K"],
                                                     c["epilogue"], ",norm" if c["has_norm"] else "",
                                                     ",base=%d" % c["exp_base"] if c["fmt"] == B13 else "",
                                                     "".join(",%s=%d" % kv for kv in c["knobs"].items()))
    assert len({c["id"] for c in out}) == len(out)
    return out


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from phi_3_vision_mlx_amd import ops
    bf16, f32, i32, dev = torch.bfloat16, torch.float32, torch.int32, "cuda"
    tab = torch.zeros((2, 4, 48), device=dev)
    tab_o = torch.empty((2, 1, 48), device=dev)

    def zeros(rows, cols, dtype=bf16, slack=32):               # with `slack` rows behind it: a row set read past a ragged edge stays inside
        return torch.zeros((rows + slack) * cols, dtype=dtype, device=dev)[:rows * cols].view(rows, cols)

    def handle(c, rows):
        K = c["K"]
        if c["fmt"] == BF16:
            return zeros(rows, K)
        if c["fmt"] == FP8:
            return (zeros(rows, K, torch.uint8), torch.zeros(rows + 32, dtype=f32, device=dev)[:rows])
        if c["fmt"] == Q4:
            return (zeros(rows, K // 8, i32), zeros(rows, K // 64, i32))
        return ops.PackedB13(zeros(rows, K * 13 // 8, torch.uint8), c["exp_base"], rows, K, c["epilogue"] == SILU)

    done = []
    for c in cases():
        M, N, K, epi = c["M"], c["N"], c["K"], c["epilogue"]
        w = handle(c, 2 * N if epi == SILU else N)
        x = zeros(M, K, slack=16)
        out = zeros(M, N, f32 if epi == F32 else bf16, slack=16)
        resid = zeros(M, N, slack=16) if epi == RESID else None
        nw = torch.zeros(K, dtype=bf16, device=dev) if c["has_norm"] else None
        old = [(name, ops.set_tuning(name, v)) for name, v in c["knobs"].items()]
        torch.cuda.synchronize()
        ops.stage_rope(tab, tab, tab_o, tab_o, 2, 1, 4)            # the separator
        try:
            if c["step"] == "begin":
                table, d_past = zeros(64, K), torch.zeros(1, dtype=i32, device=dev)
                cos, co = torch.zeros((M, 8, 48), device=dev), torch.zeros((M, 1, 48), device=dev)
                ok = ops.gemv_step_begin(torch.zeros(M, dtype=i32, device=dev), table, x, cos, cos, d_past, co, torch.zeros_like(co), w, nw, 1e-5, out)
                status = 0 if ok else ops.L.ERR_UNSUPPORTED
            elif c["step"] == "end":
                z = lambda *s: torch.zeros(s, dtype=i32, device=dev)
                ws = torch.zeros(ops.L.GEMV_STEP_WS_BYTES // 4, dtype=f32, device=dev)
                ok = ops.gemv_step_end(x, w, nw, 1e-5, out, z(M), z(M), z(M, 4), z(1), z(1), z(1), ws)
                status = 0 if ok else ops.L.ERR_UNSUPPORTED
            else:
                f = {BF16: ops.gemv, FP8: ops.gemv_fp8, Q4: ops.gemv_q4, B13: ops.gemv_b13}[c["fmt"]]
                f(x, *(w if isinstance(w, tuple) else (w,)), epilogue=epi, resid=resid, norm_w=nw, norm_eps=1e-5, out=out)
                status = 0
        except RuntimeError as e:
            status = int(re.search(r"failed: (-?\d+)", str(e)).group(1))
        torch.cuda.synchronize()
        for name, v in old:
            ops.set_tuning(name, v)
        done.append(dict(c, status=status))
        print(c["id"], status, flush=True)
    with open(path, "w") as f:
        json.dump({"device": {"cu_count": ops.device_props(0)["cu_count"]}, "cases": done}, f)


def join(cases_path, trace_path, out_path=None, table_path=None):
    with open(cases_path) as f:
        rec = json.load(f)
    with open(trace_path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    groups = []
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"]).removesuffix(".kd")
        name = name[:name.rindex("(")] if name.endswith(")") else name
        if name == "k_stage_rope":
            groups.append([])
        elif groups and re.match(r"k_gemv|k_gemm_rows_q4", name):
            block = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
            groups[-1].append([name, [int(r["Grid_Size_" + a]) // b for a, b in zip("XYZ", block)], block])
    assert len(groups) == len(rec["cases"]), (len(groups), len(rec["cases"]))
    for c, launches in zip(rec["cases"], groups):
        assert len(launches) == (c["status"] == 0), c
        c["launches"] = launches
    lines = [json.dumps(["device", rec["device"]], separators=(",", ":"))] + [json.dumps(["case", c], separators=(",", ":")) for c in rec["cases"]]
    if out_path:
        with open(out_path, "w") as f:
            f.write("[\n" + ",\n".join(lines) + "\n]\n")
    table = ["decode GEMV: what p3v_gemv / _fp8 / _q4 / _b13 and their _step entries launch (tools/gemv_routes.py, rocprofv3 --kernel-trace)",
             "device: " + json.dumps(rec["device"]), "", "%-72s %s" % ("case", "status, or kernel grid block")]
    for c in rec["cases"]:
        what = "  +  ".join("%s %s %s" % (n, "x".join(map(str, g)), "x".join(map(str, b))) for n, g, b in c["launches"]) or "refused: %d" % c["status"]
        table.append("%-72s %s" % (c["id"], what))
    if table_path:
        with open(table_path, "w") as f:
            f.write("\n".join(table) + "\n")
    else:
        print("\n".join(table))


if __name__ == "__main__":
    if sys.argv[1] == "--join":
        join(*sys.argv[2:6])
    else:
        run(sys.argv[1])
