"""The k = 7 convs' weight gradient from bf16 planes (csrc/conv_wgrad7_planes.h) at four Oobleck level shapes: microseconds per launch of
each kernel variant (sat_conv_wgrad7_planes_v: 2 = 16x16x32 MFMAs, the shipped form; 0 = 32x32x16) and the fraction of the bf16x3
peak.  The variants are timed interleaved in one process on random data, each after at least `--heat` seconds of its own
back-to-back launches (the chip lowers its clock under load: a cold first round flatters whatever runs first); median and minimum over
`--rounds` rounds.  The planes themselves are built outside the timed region, as in the training step.  `--pipe` adds the pipelined
fp32-input kernel (csrc/conv_wgrad7_bf16x3_pipe.h) with and without the SnakeBeta recompute of x.  MI355X only.
    python tools/wgrad7_bench.py [--variants 0,2] [--rounds 10] [--heat 2.0] [--pipe]"""
import argparse
import ctypes
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd.ops import get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--variants", default="0,2")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--heat", type=float, default=2.0)
ap.add_argument("--pipe", action="store_true")
args = ap.parse_args()
variants = [int(v) for v in args.variants.split(",")]
o = get_ops()
PEAK = 833.3                                                        # bf16x3 TFLOP/s: a third of the bf16 peak


def timeit(f, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def heat(f, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50):
            f()
        torch.cuda.synchronize()


for (c, t, dil) in [(128, 2097152, 1), (128, 2097152, 9), (256, 262144, 3), (512, 65536, 9)]:
    x = torch.randn(1, c, t, device='cuda') * 0.5
    dy = torch.randn(1, c, t, device='cuda')
    la = torch.randn(c, device='cuda') * 0.1
    lb = torch.randn(c, device='cuda') * 0.1
    frac = lambda us: round(2.0 * c * c * 7 * t / us * 1e-6 / PEAK, 3)
    row = {"C": c, "T": t, "dil": dil}
    if args.pipe:
        for key, f in (("us", lambda: o.conv_wgrad7_bf16x3(dy, x, dil, 3 * dil, snake=(la, lb), dy_rowsum=True, raw=True)),
                       ("nosnake_us", lambda: o.conv_wgrad7_bf16x3(dy, x, dil, 3 * dil, raw=True))):
            heat(f, 0.5)
            row[key] = round(timeit(f), 1)
        row["frac"] = frac(row["us"])
    planes = []
    for src, sn in ((dy, None), (x, (la, lb))):
        rows = o.lib.sat_conv1d_k7_plane_rows(t, t, 0)
        hi, lo = torch.zeros(2, (c // 8) * rows * 8, dtype=torch.int16, device='cuda').unbind(0)
        sa, sib = o.snake_consts(*sn) if sn is not None else (None, None)
        ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
        assert o.lib.sat_conv1d_k7_planes(ptr(src), ptr(sa), ptr(sib), ptr(hi), ptr(lo), 1, c, t, rows, None) == 0
        planes.append((hi, lo, rows))

    def run(v):
        o.wgrad7_planes_variant = v
        o.conv_wgrad7_planes(planes[0], planes[1], 1, c, c, t, dil, 3 * dil, raw=True)

    for v in variants:
        heat(lambda: run(v), args.heat)
    times = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            times[v].append(timeit(lambda: run(v)))
    for v in variants:
        med = statistics.median(times[v])
        row[f"v{v}"] = {"median_us": round(med, 1), "min_us": round(min(times[v]), 1), "frac": frac(med)}
    print(json.dumps(row), flush=True)
