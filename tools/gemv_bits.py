"""sha256 of what the streaming M = 1 GEMV (gemv_stream_body, csrc/p3v_gemv3_body.h) writes, one line per case, for comparing two
builds of the library bit for bit:

    P3V_LIB=/path/to/other/libp3v.so python tools/gemv_bits.py > a.txt;  python tools/gemv_bits.py > b.txt;  diff a.txt b.txt

Cases (bf16, e4m3 and 4-bit weights; K = 3072 and 8192; inputs from fixed seeds on the CPU):
  * M = 1, every epilogue (none, resid, silu, f32) with and without the fused RMSNorm, at N = 2, 3072, 4102, 6144, 8198, 9216, 32064
    (with the default knobs on 256 CUs: 1, 2, 3 and >= 4 pipeline stages per wave, a last wave with fewer row pairs, idle waves);
  * bf16 at M = 2, 3, 4 with the gemv8_min knob at 5: the MT = 2 / 4 streaming instantiations no default path reaches;
  * both step folds (p3v_gemv*_step begin and end) over three steps, with a tie that wins the arg-max and a NaN row: every side output.
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from phi_3_vision_mlx_amd import ops
from phi_3_vision_mlx_amd.weights import mlx_quantize, q4_repack

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
V = 32064
NS = (2, 3072, 4102, 6144, 8198, 9216, 32064)
EPIS = {"none": ops.EPI_NONE, "resid": ops.EPI_RESID_BF16, "silu": ops.EPI_SILU_MUL, "f32": ops.EPI_F32}


def g(shape, seed, std=1.0, dtype=BF16):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * std).to(dtype)


def sha(*tensors):
    torch.cuda.synchronize()
    return " ".join(hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32] for t in tensors)


def formats(w):
    """bf16 rows [R, K] on the device -> {format: (the projection on its first n rows, the weight argument of the step folds)}"""
    w8, sc = ops.quantize_fp8_rows(w)
    w4, sb = (t.contiguous() for t in q4_repack(*mlx_quantize(w)))
    return {
        "bf16": (lambda x, n, *a, **k: ops.gemv(x, w[:n], *a, **k), w),
        "e4m3": (lambda x, n, *a, **k: ops.gemv_fp8(x, w8[:n], sc[:n], *a, **k), (w8, sc)),
        "q4": (lambda x, n, *a, **k: ops.gemv_q4(x, w4[:n], sb[:n], *a, **k), (w4, sb)),
    }


def main():
    for K in (3072, 8192):
        base = g((V, K), 500 + K, 0.03)
        x1 = g((1, K), 501).cuda()
        nw = (g((K,), 502) * 0.1 + 1).cuda()
        # the vocabulary head of the step folds: rows 300 and 20000 are equal and point along step 1's normalised activations, so the
        # arg-max of that step is a tie between them (the first one wins); step 2's activations hold a NaN (the row reports -1)
        xs = [g((1, K), 510 + s).cuda() for s in range(3)]
        xs[2][0, 5] = float("nan")
        base[300] = base[20000] = 0.05 * torch.sign(xs[1][0].float().cpu() * nw.float().cpu()).to(BF16)
        wide = torch.cat([base, base.flip(0)]).cuda()              # silu at N = 32064 reads 2 N rows
        fm = formats(wide)
        for fmt, (proj, w_step) in fm.items():
            for N in NS:
                res = g((1, N), 503).cuda()
                for epi, e in EPIS.items():
                    for norm in (False, True):
                        kw = dict(norm_w=nw, norm_eps=1e-5) if norm else {}
                        out = proj(x1, 2 * N if epi == "silu" else N, e, resid=res if epi == "resid" else None, **kw)
                        print(f"{fmt} K={K} M=1 N={N} {epi} norm={int(norm)}: {sha(out)}")
            if fmt == "bf16":                                      # the MT = 2 / 4 streaming instantiations
                old = ops.set_tuning("gemv8_min", 5)
                try:
                    for M in (2, 3, 4):
                        xm = g((M, K), 520 + M).cuda()
                        for N in (3072, 4102):
                            res = g((M, N), 504).cuda()
                            for epi in ("none", "resid", "silu"):
                                for norm in (False, True):
                                    kw = dict(norm_w=nw, norm_eps=1e-5) if norm else {}
                                    out = proj(xm, 2 * N if epi == "silu" else N, EPIS[epi], resid=res if epi == "resid" else None, **kw)
                                    print(f"{fmt} K={K} M={M} N={N} {epi} norm={int(norm)}: {sha(out)}")
                finally:
                    ops.set_tuning("gemv8_min", old)
            # ---- the step folds: the table is the same V rows; the first projection has 1024 rows
            w_first = tuple(t[:1024] for t in w_step) if isinstance(w_step, tuple) else w_step[:1024]
            w_head = tuple(t[:V] for t in w_step) if isinstance(w_step, tuple) else w_step[:V]
            table = wide[:V]
            T, half, steps = 40, 48, 3
            gen = torch.Generator().manual_seed(530)
            cos, sin = torch.rand((1, T, half), generator=gen).cuda(), torch.rand((1, T, half), generator=gen).cuda()
            d_past = torch.tensor([11], dtype=I32).cuda()
            for tok in (7004, V + 5, -3):                          # (out of range: clamped)
                t = torch.tensor([tok], dtype=I32).cuda()
                x_out = torch.zeros((1, K), dtype=BF16).cuda()
                co, so = torch.zeros((1, 1, half), dtype=F32).cuda(), torch.zeros((1, 1, half), dtype=F32).cuda()
                out = torch.zeros((1, 1024), dtype=BF16).cuda()
                assert ops.gemv_step_begin(t, table, x_out, cos, sin, d_past, co, so, w_first, nw, 1e-5, out)
                print(f"{fmt} K={K} step-begin tok={tok}: {sha(out, x_out, co, so)}")
            amax_ws = torch.zeros((ops.L.GEMV_STEP_WS_BYTES // 4,), dtype=F32).cuda()
            hist = torch.zeros((1, steps), dtype=I32).cuda()
            d_step, ticket = torch.zeros(1, dtype=I32).cuda(), torch.zeros(1, dtype=I32).cuda()
            nxt, tko = torch.zeros(1, dtype=I32).cuda(), torch.zeros(1, dtype=I32).cuda()
            for s in range(steps):
                lg = torch.zeros((1, V), dtype=BF16).cuda()
                assert ops.gemv_step_end(xs[s], w_head, nw, 1e-5, lg, nxt, tko, hist, d_step, d_past, ticket, amax_ws)
                print(f"{fmt} K={K} step-end s={s} token={nxt.item()}: {sha(lg, nxt, tko, hist, d_step, d_past, ticket, amax_ws)}")
        del fm, wide


if __name__ == "__main__":
    main()
