"""The k = 7 convs' weight gradient (csrc/conv_wgrad7_bf16x3_pipe.h) at four Oobleck level shapes: microseconds per launch with and without the
SnakeBeta recompute of x, fraction of the bf16x3 peak; and the same gradient from bf16 planes (csrc/conv_wgrad7_planes.h: planes_us,
planes_frac — the planes themselves are built outside the timed region, as in the training step).  MI355X only.
    python tools/wgrad7_bench.py"""
import ctypes
import json
import sys

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd.ops import get_ops

o = get_ops()


def timeit(f, n=10):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for (c, t, dil) in [(128, 2097152, 1), (128, 2097152, 9), (256, 262144, 3), (512, 65536, 9)]:
    x = torch.randn(1, c, t, device='cuda') * 0.5
    dy = torch.randn(1, c, t, device='cuda')
    la = torch.randn(c, device='cuda') * 0.1
    lb = torch.randn(c, device='cuda') * 0.1
    us = timeit(lambda: o.conv_wgrad7_bf16x3(dy, x, dil, 3 * dil, snake=(la, lb), dy_rowsum=True, raw=True))
    usn = timeit(lambda: o.conv_wgrad7_bf16x3(dy, x, dil, 3 * dil, raw=True))
    planes = []
    for src, sn in ((dy, None), (x, (la, lb))):
        rows = o.lib.sat_conv1d_k7_plane_rows(t, t, 0)
        hi, lo = torch.zeros(2, (c // 8) * rows * 8, dtype=torch.int16, device='cuda').unbind(0)
        sa, sib = o.snake_consts(*sn) if sn is not None else (None, None)
        ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
        assert o.lib.sat_conv1d_k7_planes(ptr(src), ptr(sa), ptr(sib), ptr(hi), ptr(lo), 1, c, t, rows, None) == 0
        planes.append((hi, lo, rows))
    usp = timeit(lambda: o.conv_wgrad7_planes(planes[0], planes[1], 1, c, c, t, dil, 3 * dil, raw=True))
    print(json.dumps({"C": c, "T": t, "dil": dil, "us": round(us, 1), "nosnake_us": round(usn, 1),
                      "frac": round(2.0 * c * c * 7 * t / us * 1e-6 / 833.3, 3), "planes_us": round(usp, 1),
                      "planes_frac": round(2.0 * c * c * 7 * t / usp * 1e-6 / 833.3, 3)}), flush=True)
