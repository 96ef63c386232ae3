"""Minimal eager launches of the dominant decode kernel for PMC collection (no graphs, no weight generation).
`pmc_kernel.py b13` (or P3V_PMC_FMT=b13, as tools/pmc_gemv.sh passes it): the same launches on 13-bit packed weights (ops.gemv_b13)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from phi_3_vision_mlx_amd import ops
I, H = 8192, 3072
Ws = [torch.zeros((2 * I, H), dtype=torch.bfloat16, device="cuda") for _ in range(4)]      # 4 x 100 MB > 256 MiB Infinity Cache
x = torch.ones((1, H), dtype=torch.bfloat16, device="cuda")
nw = torch.ones((H,), dtype=torch.bfloat16, device="cuda")
out = torch.empty((1, I), dtype=torch.bfloat16, device="cuda")
B13 = sys.argv[1:] == ["b13"] or os.environ.get("P3V_PMC_FMT") == "b13"
if B13:                                                                                    # 4 x 82 MB, still beyond the cache
    Ws[0].view(torch.int16).random_(100 << 7, 127 << 7)                                      # values inside one window
    Ws = [ops.pack_b13(Ws[0], silu_pairs=True) for _ in range(4)]
for i in range(12):
    if B13:
        ops.gemv_b13(x, Ws[i % 4], ops.EPI_SILU_MUL, norm_w=nw, norm_eps=1e-5, out=out)
    else:
        ops.gemv(x, Ws[i % 4], ops.EPI_SILU_MUL, norm_w=nw, norm_eps=1e-5, out=out)
torch.cuda.synchronize()
print("done")
