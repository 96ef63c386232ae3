"""Which kernels the library launches for a decode attention call -- the recording behind tests/golden/attn_decode_routes.json and
profiles/attn_decode_routes.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o routes -- python tools/attn_decode_routes.py DIR/cases.json
    python tools/attn_decode_routes.py --join DIR/cases.json DIR/..._kernel_trace.csv [tests/golden/attn_decode_routes.json [table.txt]]

The first form calls ops.attention_decode / ops.attention_decode_q8 once per case of `cases()` (a refused call is recorded by its
error code), with one k_stage_rope launch in front of every case as a separator, and writes the case list; it also asks the two
can_fuse functions for the largest n_split they take on this device, which names the fused kernels' workgroups per CU.  The second
form joins the trace with the list: per case the kernel names in order, each with its grid (in workgroups) and block.
"""
import csv
import json
import math
import os
import re
import sys

NH, HD, H = 32, 96, 3072
# (n_split, cache_t): the smallest shapes that reach every branch of the two launchers
PLAIN = ((1, 64), (4, 256), (2, 256), (1, 256), (3, 320), (17, 1088), (16, 1024), (48, 6144))
FUSED = ((13, 1664), (24, 3072), (12, 1536), (4, 256), (48, 6144))


def cases():
    """(id, kind, B, heads, kv heads, n_split, cache_t, merge_in_launch, o_proj format or None, knobs)."""
    out = []
    for kind in ("bf16", "q8"):
        for (n_split, T), merge in ((c, m) for c in PLAIN for m in (1, 0)):
            out.append((kind, 1, 4, 1, n_split, T, merge, None, ()))
        for fmt in (("bf16", "q4") if kind == "bf16" else ("e4m3",)):
            for (n_split, T), merge in ((c, m) for c in FUSED for m in (1, 0)):
                out.append((kind, 1, NH, NH, n_split, T, merge, fmt, ()))
            out.append((kind, 2, NH, NH, 13, 1664, 1, fmt, ()))
            out.append((kind, 2, NH, NH, 13, 1664, 0, fmt, ()))
    for n_split, T in ((16, 1024), (2, 256), (4, 256)):
        out.append(("q8", 1, 4, 1, n_split, T, 1, None, (("q8_old", 1),)))
    out.append(("q8", 1, NH, NH, 13, 1664, 1, "e4m3", (("q8_old", 1),)))
    out.append(("q8", 1, NH, NH, 13, 1664, 0, "e4m3", (("q8_old", 1),)))
    out.append(("q8", 1, NH, NH, 13, 1664, 1, "e4m3", (("attn_fo_map_q8", 1),)))
    for fmt in ("bf16", "q4"):
        for v in (0, 1, 2):
            out.append(("bf16", 1, NH, NH, 13, 1664, 1, fmt, (("attn_fo_map", v),)))
    ids = ["%s,B=%d,nh=%d,n_split=%d,T=%d,merge=%d,o=%s%s" % (k, B, nh, n, T, m, fmt, "".join(",%s=%d" % kn for kn in knobs))
           for k, B, nh, nkv, n, T, m, fmt, knobs in out]
    assert len(set(ids)) == len(ids)
    return [(i,) + c for i, c in zip(ids, out)]


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from phi_3_vision_mlx_amd import ops
    BF16, dev = torch.bfloat16, "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    tab = torch.rand((2, 4, HD // 2), device=dev, generator=gen)
    tab_o = torch.empty((2, 1, HD // 2), device=dev)
    o_w = {"bf16": dict(o_proj_w=torch.zeros((H, H), dtype=BF16, device=dev)),
           "q4": dict(o_proj_w=torch.zeros((H, H // 8), dtype=torch.int32, device=dev), o_proj_sb=torch.zeros((H, H // 64), dtype=torch.int32, device=dev)),
           "e4m3": dict(o_proj_w8=torch.zeros((H, H), dtype=torch.uint8, device=dev), o_proj_scale=torch.ones((H,), device=dev))}
    done = []
    for cid, kind, B, nh, nkv, n_split, T, merge, fmt, knobs in cases():
        qkv = torch.randn((B, (nh + 2 * nkv) * HD), device=dev, generator=gen).to(BF16)
        cos, sin = tab[:B, :1].contiguous(), tab[:B, 1:2].contiguous()
        out = torch.full((B, 1, nh * HD), -1, dtype=torch.int16, device=dev).view(BF16)
        ws = ops.attention_ws(B, 1, nh, HD, n_split, dev)
        kw = dict(merge_in_launch=bool(merge))
        if fmt:
            kw.update(o_w[fmt], o_proj_x=torch.zeros((1, H), dtype=BF16, device=dev), o_rearm=torch.zeros((1, 1, H), dtype=BF16, device=dev))
        if kind == "bf16":
            cache = (torch.zeros((B, nkv, T, HD), dtype=BF16, device=dev), torch.zeros((B, nkv, HD, T), dtype=BF16, device=dev))
            call = ops.attention_decode
        else:
            cache = (torch.full((B, nkv, T, HD), 128, dtype=torch.uint8, device=dev), torch.full((B, nkv, HD, T), 128, dtype=torch.uint8, device=dev),
                     torch.ones((B, nkv, T), device=dev), torch.ones((B, nkv, T), device=dev))
            call = ops.attention_decode_q8
        old = [(name, ops.set_tuning(name, v)) for name, v in knobs]
        torch.cuda.synchronize()
        ops.stage_rope(tab, tab, tab_o, tab_o, 2, 1, 4)            # the separator
        try:
            call(qkv, cos, sin, 1, *cache, out, B, 1, nh, nkv, HD, HD ** -0.5, T - 8, T, ws, n_split, **kw)
            status = 0
        except RuntimeError as e:
            status = int(re.search(r"failed: (-?\d+)", str(e)).group(1))
        torch.cuda.synchronize()
        for name, v in old:
            ops.set_tuning(name, v)
        done.append({"id": cid, "kind": kind, "B": B, "heads": nh, "kv_heads": nkv, "n_split": n_split, "cache_t": T, "merge_in_launch": merge,
                     "o_proj": fmt, "knobs": dict(knobs), "status": status})
        print(cid, status, flush=True)
    cus = ops.device_props(0)["cu_count"]
    device = {"cu_count": cus}
    for kind, can in (("bf16", ops.attention_decode_can_fuse_oproj), ("q8", ops.attention_decode_q8_can_fuse_oproj)):
        n_max = max([n for n in range(13, 129) if can(1, 1, NH, HD, n, n * 128, H, True)], default=0)
        per_cu = math.ceil(NH * n_max / (cus - 8))               # the capacity is per_cu * (CUs - 8), a whole grid of 32 * n_split fits it
        device[kind] = {"largest_n_split": n_max, "workgroups_per_cu": per_cu, "capacity": per_cu * (cus - 8)}
    with open(path, "w") as f:
        json.dump({"device": device, "cases": done}, f)
    print(json.dumps(device))


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
        elif groups and name.startswith("k_attn"):
            block = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
            groups[-1].append([name, [int(r["Grid_Size_" + a]) // b for a, b in zip("XYZ", block)], block])
    assert len(groups) == len(rec["cases"]), (len(groups), len(rec["cases"]))
    for c, launches in zip(rec["cases"], groups):
        assert bool(launches) == (c["status"] == 0), c
        c["launches"] = launches
    lines = [json.dumps(["device", rec["device"]], separators=(",", ":"))] + [json.dumps(["case", c], separators=(",", ":")) for c in rec["cases"]]
    text = "[\n" + ",\n".join(lines) + "\n]\n"
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    table = ["decode attention: what p3v_attention_decode / p3v_attention_decode_q8 launch (tools/attn_decode_routes.py, rocprofv3 --kernel-trace)",
             "device: " + json.dumps(rec["device"]), "", "%-72s %s" % ("case", "status, or kernel grid block ...")]
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
