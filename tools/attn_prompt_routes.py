"""Which kernels the library launches for a p3v_attention call -- the recording behind tests/golden/attn_prompt_routes.json and
profiles/attn_prompt_routes.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o routes -- python tools/attn_prompt_routes.py DIR/cases.json
    python tools/attn_prompt_routes.py --join DIR/cases.json DIR/..._kernel_trace.csv [tests/golden/attn_prompt_routes.json [table.txt]]

The first form calls ops.attention once per case of `cases()` on zero tensors (a refused call is recorded by its error code), with one
k_stage_rope launch in front of every case as a separator, and writes the case list.  It asks the library nothing but the call itself,
so it runs on any commit that has p3v_attention.  The second form joins the trace with the list: per case the kernel names in order,
each with its grid (in workgroups) and block.
"""
import csv
import json
import os
import re
import sys

KNOBS = ("attn_old", "attn_no_dma", "attn_pp", "attn_il", "attn_il_waves")


def cases():
    """The smallest calls that reach every branch of the launcher: dicts of B, L, heads, kv_heads, hd, past, past_t, n_split, has_ws,
    new_is_cache, q_prescaled, knobs."""
    out = []

    def add(B, L, hd=96, nh=1, nkv=1, past=0, past_t=None, n_split=0, has_ws=0, new_is_cache=1, pre=1, **knobs):
        assert set(knobs) <= set(KNOBS)
        out.append(dict(B=B, L=L, heads=nh, kv_heads=nkv, hd=hd, past=past, past_t=(past + L + 63) // 64 * 64 if past_t is None else past_t,
                        n_split=n_split, has_ws=has_ws, new_is_cache=new_is_cache, q_prescaled=pre, knobs=knobs))

    for L in (16, 17):                                         # the split-KV threshold: split, workspace
        for n_split in (1, 4):
            for has_ws in (1, 0):
                add(1, L, nh=2, past=48, n_split=n_split, has_ws=has_ws, pre=0)
    for L in (767, 768, 2815, 2816, 3071, 3072, 6143, 6144):   # pre-scaled Q, one row
        add(1, L)
    for L in (3583, 3584, 6143, 6144):                         # ... two rows
        add(2, L)
    for hd in (96, 64):                                        # plain Q
        for L in (3071, 3072):
            add(1, L, hd=hd, pre=0)
    for hd in (96, 64):                                        # pre-scaled, the other head dim: short, interleaved 4 / 8 waves
        for L in (100, 768, 3072):
            if (hd, L) != (96, 768) and (hd, L) != (96, 3072):
                add(1, L, hd=hd)
    add(1, 100, nh=2, new_is_cache=0, pre=0)                   # keys of the call in their own tensors
    add(1, 100, hd=64, new_is_cache=0, pre=0)
    add(1, 100, past_t=104)                                    # a cache whose capacity is no multiple of 64
    add(1, 40, nh=2, past=200, past_t=256)                     # a cached call with several new rows
    add(1, 6144, attn_pp=0)                                    # attn_pp = 0 pins dma: the automatic il choice is off ...
    add(1, 6144, attn_pp=0, attn_il=1)                         # ... a pinned il is not
    add(1, 6144, attn_pp=1)                                    # attn_pp = 1 leaves the automatic il choice on
    add(1, 100, attn_pp=1)
    add(1, 100, attn_pp=1, pre=0)
    add(1, 100, hd=64, attn_pp=1, pre=0)
    add(1, 6144, attn_il=0)                                    # il off: pp from 3072 tokens (pre-scaled)
    add(1, 3071, attn_il=0)
    add(1, 3072, hd=64, attn_il=0)
    add(1, 100, attn_il=1)
    add(1, 100, attn_il=1, pre=0)                              # plain Q never takes il
    add(1, 6144, attn_il=1, pre=0)
    add(1, 6144, attn_il_waves=4)
    add(1, 768, attn_il_waves=8)
    add(1, 768, hd=64, attn_il_waves=8)
    add(2, 100, attn_il_waves=8)                               # the wave count applies inside il only
    add(1, 768, attn_il=0, attn_il_waves=4)
    add(1, 100, nh=2, attn_old=1)
    add(1, 100, hd=64, attn_old=1, pre=0)
    add(1, 16, nh=2, past=48, n_split=4, has_ws=1, pre=0, attn_old=1)
    add(1, 6144, attn_no_dma=1)
    add(1, 100, hd=64, attn_no_dma=1, pre=0)
    add(1, 100, hd=80)                                         # refused
    add(1, 0, past_t=64)                                       # nothing to do
    add(0, 100)
    ids = ["B=%d,L=%d,nh=%d,hd=%d,past=%d,past_t=%d,n_split=%d,ws=%d,cache=%d,pre=%d%s" % (
        c["B"], c["L"], c["heads"], c["hd"], c["past"], c["past_t"], c["n_split"], c["has_ws"], c["new_is_cache"], c["q_prescaled"],
        "".join(",%s=%d" % kv for kv in c["knobs"].items())) for c in out]
    assert len(set(ids)) == len(ids)
    return [dict(id=i, **c) for i, c in zip(ids, out)]


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from phi_3_vision_mlx_amd import ops
    BF16, dev = torch.bfloat16, "cuda"
    tab = torch.zeros((2, 4, 48), device=dev)
    tab_o = torch.empty((2, 1, 48), device=dev)

    def zeros(*shape):                                         # with slack behind it: a chunk read past a ragged capacity stays inside
        n = 1
        for s in shape:
            n *= s
        return torch.zeros(n + 8192, dtype=BF16, device=dev)[:n].view(*shape)

    done = []
    for c in cases():
        B, L, nh, nkv, hd, T = c["B"], c["L"], c["heads"], c["kv_heads"], c["hd"], c["past_t"]
        q, out = zeros(max(B, 1), nh, max(L, 1), hd), zeros(max(B, 1), max(L, 1), nh * hd)
        k, vt = zeros(max(B, 1), nkv, T, hd), zeros(max(B, 1), nkv, hd, T)
        kw = dict(k_past=k, v_past=vt, past_t=T) if c["new_is_cache"] else dict(k_new=k, v_new=vt, new_t=T)
        ws = ops.attention_ws(B, min(L, ops.L.DECODE_MAX_L), nh, hd, max(c["n_split"], 1), dev) if c["has_ws"] else None
        old = [(name, ops.set_tuning(name, v)) for name, v in c["knobs"].items()]
        torch.cuda.synchronize()
        ops.stage_rope(tab, tab, tab_o, tab_o, 2, 1, 4)            # the separator
        try:
            ops.attention(q, out, B, L, nh, nkv, hd, hd ** -0.5, True, past=c["past"], ws=ws, n_split=c["n_split"],
                          new_is_cache=bool(c["new_is_cache"]), q_prescaled=bool(c["q_prescaled"]), **kw)
            status = 0
        except RuntimeError as e:
            status = int(re.search(r"failed: (-?\d+)", str(e)).group(1))
        torch.cuda.synchronize()
        for name, v in old:
            ops.set_tuning(name, v)
        done.append(dict(c, status=status))
        print(c["id"], status, flush=True)
    with open(path, "w") as f:
        json.dump({"cases": done}, f)


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
        assert not (launches and c["status"]), c
        c["launches"] = launches
    text = "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in rec["cases"]) + "\n]\n"
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    table = ["prompt attention: what p3v_attention launches (tools/attn_prompt_routes.py, rocprofv3 --kernel-trace)", "",
             "%-96s %s" % ("case", "status, or kernel grid block ...")]
    for c in rec["cases"]:
        what = "  +  ".join("%s %s %s" % (n, "x".join(map(str, g)), "x".join(map(str, b))) for n, g, b in c["launches"])
        table.append("%-96s %s" % (c["id"], what or ("refused: %d" % c["status"] if c["status"] else "nothing to launch")))
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
