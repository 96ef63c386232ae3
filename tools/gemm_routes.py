"""Which kernels the library launches for a bf16 prefill GEMM call -- the recording behind tests/golden/gemm_routes.json and
profiles/gemm_routes.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o routes -- python tools/gemm_routes.py DIR/cases.json
    python tools/gemm_routes.py --join DIR/cases.json DIR/..._kernel_trace.csv [tests/golden/gemm_routes.json [table.txt]]

The first form calls p3v_gemm / p3v_gemm_resid_norm / p3v_gemm_qkv (the C ABI: the recording predates the route function and must run
on a tree without it) once per case of `cases()`, with one k_stage_rope launch in front of every case as a separator, and writes the
case list with each call's status.  The second form joins the trace with the list: per case the kernel names in order, each with its
grid (in workgroups) and block.  The cases are the smallest shapes that reach every branch of the dispatch, not the model's shapes.
"""
import csv
import ctypes as C
import json
import os
import re
import sys

NONE, BIAS, QGELU, GELU, BIAS_RESID_F32, RESID, SILU, PATCH = range(8)
GEMM, RESID_NORM, QKV = "gemm", "resid_norm", "qkv"
PPI = 256                                                       # patches per image of the PATCH cases


def cases():
    out = []

    def add(entry, M, N, K, epi=NONE, ws=1, knobs=(), **qkv):
        out.append(dict(entry=entry, M=M, N=N, K=K, epilogue=epi, ws=ws, knobs=dict(knobs), **qkv))

    # ---- the rows kernel: one pass (MT 1 and 2), four slices with and without a workspace, the SiLU shape whose split no kernel runs
    for M in (9, 16, 17):
        add(GEMM, M, 8192, 3072)
        add(GEMM, M, 4096, 3072, SILU)
    for M, ws in ((16, 1), (17, 1), (16, 0)):
        add(GEMM, M, 3072, 3072, RESID, ws)
        add(GEMM, M, 3072, 8192, RESID, ws)
    add(GEMM, 16, 1024, 3072, SILU)
    # ---- the weight-streaming tiles: 64- and 128-row tiles, one pass and K slices
    for M in (33, 64, 65, 256):
        for epi in (RESID, NONE, SILU):
            add(GEMM, M, 64, 384, epi)
            add(GEMM, M, 192, 768, epi)
    for M in (33, 65):
        for epi in (RESID, NONE, SILU):
            add(GEMM, M, 64, 3072, epi)
    add(GEMM, 33, 64, 3072, RESID, 0)
    add(GEMM, 33, 64, 384, knobs=(("gemm_skinny_tm128", 1),))
    for s in (1, 2):
        add(GEMM, 33, 64, 3072, RESID, knobs=(("gemm_skinny_s", s),))
    # ---- K slices on the 128 x 128 kernel
    for ws in (1, 0):
        add(GEMM, 129, 1024, 1024, ws=ws, knobs=(("gemm_no_skinny", 1),))
        add(GEMM, 300, 3072, 8192, RESID, ws)
    add(GEMM, 300, 3072, 8192, RESID, knobs=(("gemm_no_splitk", 1),))
    # ---- whole rounds of 256 x 256 and 128 x 128 tiles
    for M in (1024, 1280):
        for N in (256, 512):
            for K in (512, 2048):
                add(GEMM, M, N, K)
    add(GEMM, 1024, 256, 512, SILU)
    for v in (-1, 0, 256, 1000000):
        add(GEMM, 1280, 256, 2048, knobs=(("gemm_big_rows", v),))
    add(GEMM, 1280, 512, 2048, knobs=(("gemm_128", 1),))
    add(GEMM, 2560, 8192, 512, knobs=(("gemm_big_rows", 1000000),))       # more 256 x 256 tiles than CUs: the persistent grid
    add(GEMM, 2560, 8192, 512, knobs=(("gemm_big_rows", 1000000), ("gemm_persistent", 0)))
    for epi in (BIAS, QGELU, GELU, BIAS_RESID_F32, PATCH):
        add(GEMM, 1024, 256, 512, epi)
    add(GEMM, 2049, 8192, 512)                                  # (the short K's surcharge: no big tiles)
    add(GEMM, 2049, 8192, 2048)                                 # the smallest M whose cost model mixes 256 + 128 tiles: 1792 + 257 rows
    # ---- p3v_gemm_resid_norm
    for M, N, K in ((16, 3072, 8192), (17, 3072, 3072), (129, 1024, 1024), (250, 192, 768), (300, 3072, 3072), (17, 4096, 3072)):
        add(RESID_NORM, M, N, K, RESID)
    add(RESID_NORM, 17, 3072, 3072, RESID, 0)
    # ---- p3v_gemm_qkv: 256-column regions (whole 256-column tiles) and 128-column regions (whole 128-column tiles only)
    for M in (17, 256, 300, 1024, 1280):
        add(QKV, M, 768, 128, n_heads=4, n_kv=4, hd=64, past=0)
    for M in (1024, 1280):
        add(QKV, M, 384, 128, n_heads=2, n_kv=2, hd=64, past=0)
    add(QKV, 1280, 768, 128, knobs=(("gemm_big_rows", 1024),), n_heads=4, n_kv=4, hd=64, past=0)
    add(QKV, 1024, 768, 128, knobs=(("gemm_no_qkv_fuse", 1),), n_heads=4, n_kv=4, hd=64, past=0)
    add(QKV, 256, 768, 128, n_heads=4, n_kv=4, hd=64, past=3)   # an unaligned append offset
    for c in out:
        c["id"] = "%s,M=%d,N=%d,K=%d,epi=%d,ws=%d%s%s" % (c["entry"], c["M"], c["N"], c["K"], c["epilogue"], c["ws"],
                                                         ",nh=%d,past=%d" % (c["n_heads"], c["past"]) if c["entry"] == QKV else "",
                                                         "".join(",%s=%d" % kv for kv in c["knobs"].items()))
    assert len({c["id"] for c in out}) == len(out)
    return out


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from phi_3_vision_mlx_amd import ops
    L, lib = ops.L, ops.L.lib()
    BF16, dev = torch.bfloat16, "cuda"
    tab = torch.rand((2, 4, 48), device=dev)
    tab_o = torch.empty((2, 1, 48), device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    done = []
    for c in cases():
        M, N, K, epi = c["M"], c["N"], c["K"], c["epilogue"]
        a = torch.zeros((M, K), dtype=BF16, device=dev)
        w = torch.zeros((2 * N if epi == SILU else N, K), dtype=BF16, device=dev)
        f32 = epi in (BIAS_RESID_F32, PATCH)
        rows = (M + PPI - 1) // PPI * (PPI + 1) if epi == PATCH else M
        out = torch.zeros((rows, N), dtype=torch.float32 if f32 else BF16, device=dev)
        resid = torch.zeros_like(out) if epi in (BIAS_RESID_F32, RESID) else None
        bias = torch.zeros((N,), dtype=BF16, device=dev) if epi in (BIAS, QGELU, GELU, BIAS_RESID_F32, PATCH) else None
        pos = torch.zeros((1 + PPI, N), dtype=BF16, device=dev) if epi == PATCH else None
        old = [(name, ops.set_tuning(name, v)) for name, v in c["knobs"].items()]
        need = lib.p3v_gemm_ws_bytes(M, N, K, epi) if c["ws"] else 0
        ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        g = L.GemmArgs(p(a), p(w), p(out), p(bias), p(resid), p(pos), M, N, K, K, K, N, epi, PPI if epi == PATCH else 0, p(ws), need)
        torch.cuda.synchronize()
        ops.stage_rope(tab, tab, tab_o, tab_o, 2, 1, 4)            # the separator
        stream = torch.cuda.current_stream().cuda_stream
        if c["entry"] == GEMM:
            status = lib.p3v_gemm(C.byref(g), stream)
        elif c["entry"] == RESID_NORM:
            nw, normed = torch.zeros((N,), dtype=BF16, device=dev), torch.zeros((M, N), dtype=BF16, device=dev)
            status = lib.p3v_gemm_resid_norm(C.byref(g), p(nw), C.c_float(1e-5), p(normed), stream)
        else:
            nh, nkv, hd, past = c["n_heads"], c["n_kv"], c["hd"], c["past"]
            Tp = (past + M + 127) // 128 * 128
            c["dst_t"], c["dst_off"] = Tp, past
            q = torch.zeros((1, nh, M, hd), dtype=BF16, device=dev)
            k, v = torch.zeros((1, nkv, Tp, hd), dtype=BF16, device=dev), torch.zeros((1, nkv, hd, Tp), dtype=BF16, device=dev)
            g.out = None
            cos = torch.rand((1, past + M + 5, hd // 2), device=dev)
            sp = L.QkvSplit(p(cos), p(cos), p(q), p(k), p(v), 1, M, nh, nkv, hd, past, Tp, 1, past + M + 5, 1, 1.0)
            status = lib.p3v_gemm_qkv(C.byref(g), C.byref(sp), stream)
        torch.cuda.synchronize()
        for name, v in old:
            ops.set_tuning(name, v)
        c["status"] = status
        done.append(c)
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
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("(")[0].removesuffix(".kd")
        if name == "k_stage_rope":
            groups.append([])
        elif groups and re.match(r"k_gemm|k_splitk_reduce", name):
            block = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
            groups[-1].append([name, [int(r["Grid_Size_" + a]) // b for a, b in zip("XYZ", block)], block])
    assert len(groups) == len(rec["cases"]), (len(groups), len(rec["cases"]))
    for c, launches in zip(rec["cases"], groups):
        assert bool(launches) == (c["status"] == 0), c
        c["launches"] = launches
    lines = [json.dumps(["device", rec["device"]], separators=(",", ":"))] + [json.dumps(["case", c], separators=(",", ":")) for c in rec["cases"]]
    if out_path:
        with open(out_path, "w") as f:
            f.write("[\n" + ",\n".join(lines) + "\n]\n")
    table = ["prefill GEMM: what p3v_gemm / p3v_gemm_resid_norm / p3v_gemm_qkv launch (tools/gemm_routes.py, rocprofv3 --kernel-trace)",
             "device: " + json.dumps(rec["device"]), "", "%-64s %s" % ("case", "status, or kernel grid block ...")]
    for c in rec["cases"]:
        what = "  +  ".join("%s %s %s" % (n, "x".join(map(str, g)), "x".join(map(str, b))) for n, g, b in c["launches"]) or "refused: %d" % c["status"]
        table.append("%-64s %s" % (c["id"], what))
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
