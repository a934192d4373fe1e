"""qk_norm kernels at the Stable Audio Open shapes (24 heads of 64, K = 1536; B 2 x N 1025 and B 2 x N 6145), GPU:
the heads GEMM with and without the norm epilogue (sat_gemm_qkv_norm_bf16 vs sat_gemm_qkv_bf16), and the standalone forward / backward
kernels (sat_qk_norm_fwd / sat_qk_norm_bwd on the q and k heads of the fused projection, bf16 and fp32) next to sat_layernorm_fwd /
sat_layernorm_bwd on a (B, N, 3072) tensor — the same byte count.  GB/s counts one read and one write of the rows (forward) and
the reads of dy and x plus the write of dx (backward).
    python tools/qk_norm_bench.py"""
import json
import sys

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd.ops import get_ops

o = get_ops()
torch.manual_seed(0)


def timeit(f, n=30):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


H = 24
inv = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
tabs = [torch.randn(64, device='cuda') for _ in range(4)]
for (nb, ntok) in [(2, 1025), (2, 6145)]:
    m = nb * ntok
    x = torch.randn(m, 1536, device='cuda').bfloat16()
    w = (torch.randn(3 * H * 64, 1536, device='cuda') / 39).bfloat16()
    cs = o.rope_tables(inv.cuda(), ntok)
    row = {"nb": nb, "ntok": ntok, "tile": o._pick_tile(m, 3 * H * 64, 1, 1536),
           "heads_us": round(timeit(lambda: o.gemm_heads_bf16(x, w, cs, H, nb, ntok, 0, 3, reuse="self")), 1)}
    for mode in ("ln", "l2"):
        row[f"heads_{mode}_us"] = round(timeit(lambda: o.gemm_heads_bf16(x, w, cs, H, nb, ntok, 0, 3, reuse="self", qk_norm=mode, norm_tables=tabs)), 1)
    print(json.dumps(row), flush=True)
    for dtype in (torch.bfloat16, torch.float32):
        es = 2 if dtype == torch.bfloat16 else 4
        qkv = torch.randn(nb, ntok, 3 * H * 64, device='cuda').to(dtype)
        out = torch.empty(nb, ntok, 2 * H * 64, device='cuda', dtype=dtype)
        dy = torch.randn(nb, ntok, 3 * H * 64, device='cuda').to(dtype)
        nbytes = m * 2 * H * 64 * es
        row = {"nb": nb, "ntok": ntok, "dtype": str(dtype).split(".")[1], "MB": round(nbytes / 1e6, 1)}
        for mode in ("ln", "l2"):
            _, stat = o.qk_norm(qkv, 2 * H, H, mode, tabs, cs, out=out, save_stats=True)
            tf = timeit(lambda: o.qk_norm(qkv, 2 * H, H, mode, tabs, cs, out=out, save_stats=True))
            tb = timeit(lambda: o.qk_norm_bwd_(dy, qkv, stat, 2 * H, H, mode, tabs, cs))
            row.update({f"{mode}_fwd_us": round(tf, 1), f"{mode}_fwd_GBs": round(2 * nbytes / tf / 1e3), f"{mode}_bwd_us": round(tb, 1),
                        f"{mode}_bwd_GBs": round(3 * nbytes / tb / 1e3)})
        xl = torch.randn(nb, ntok, 2 * H * 64, device='cuda').to(dtype)
        gl = torch.randn(2 * H * 64, device='cuda')
        y, mean, rstd = o.layernorm(xl, gl, None, save_stats=True)
        tf = timeit(lambda: o.layernorm(xl, gl, None, save_stats=True))
        tb = timeit(lambda: o.layernorm_bwd(y, xl, gl, None, None, mean, rstd))
        row.update({"layernorm_fwd_us": round(tf, 1), "layernorm_fwd_GBs": round(2 * nbytes / tf / 1e3), "layernorm_bwd_us": round(tb, 1),
                    "layernorm_bwd_GBs": round(3 * nbytes / tb / 1e3)})
        print(json.dumps(row), flush=True)
