"""Self-attention forward (bf16 planes, the sampler's / train step's path): microseconds and achieved TFLOP/s per launch for the two
kernel shapes of sat_attention_fwd (32 / 64 queries per wave, round 6), and what the library picks by itself.
    python tools/attn_bench.py                     one JSON line per (shape, kernel), head dim 64
    python tools/attn_bench.py --head-dim 128      the head dim 128 forward (bf16 at N = 1025 / 6145, fp32 at N = 1025), each next to the
                                                   head dim 64 32-query kernel at EQUAL FLOPs (twice the heads, same N) in the same
                                                   process; median of 5 timings (HIP events around graph replays), plus the plane
                                                   preparation of q / k / v at 128
    python tools/attn_bench.py --window 63 64      the sliding-window launch (sat_attention_fwd_window) beside the dense ones at the same
                                                   shape: bf16, N = 1025 and 6145, head dims 64 and 128, one process, six alternated
                                                   rounds of (windowed, dense basic, dense auto); median of 5 timings each"""
import argparse
import json
import sys

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd.ops import _ptr, get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--head-dim", type=int, default=64, choices=(64, 128))
ap.add_argument("--window", type=int, nargs=2, metavar=("L", "R"), default=None)
args = ap.parse_args()

o = get_ops()
torch.manual_seed(0)


def timeit(f, n=100):
    """microseconds per call of f: 20 calls captured into ONE HIP graph, the graph replayed n / 20 times — a launch of a few microseconds
    is otherwise timed together with the host's ~10 us of Python / ctypes dispatch per call (the first version of this tool did)."""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        f()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            for _ in range(20):
                f()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    reps = max(1, n // 20)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (20 * reps) * 1e3


def head_dim_64():
    for (b, h, hkv, nq, nk) in [(2, 24, 24, 1025, 1025), (4, 24, 24, 1025, 1025), (8, 24, 24, 1025, 1025), (16, 24, 24, 1025, 1025), (2, 24, 24, 6145, 6145)]:
        q = torch.randn(b, h, nq, 64, device='cuda').bfloat16()
        k = torch.randn(b, hkv, nk, 64, device='cuda').bfloat16()
        v = torch.randn(b, hkv, nk, 64, device='cuda').bfloat16()
        ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float(), scale=0.125).permute(0, 2, 1, 3).reshape(b, nq, h * 64)
        for q64 in (False, True, None):
            o.attn_q64 = q64
            out, lse, planes = o.attention(q, k, v, 0.125, return_planes=True)
            err = float((out.float() - ref).abs().max() / ref.abs().max())
            us = timeit(lambda: o.attention_planes(planes["q"]["rm"][0], planes["k"]["rm"][0], planes["v"]["tr"][0], nq, nk, 0.125),
                        n=100 if nq < 4000 else 30)
            tf = 4.0 * b * h * nq * nk * 64 / us * 1e-6
            print(json.dumps({"shape": [b, h, hkv, nq, nk], "queries_per_wave": {False: 32, True: 64, None: "auto"}[q64], "us": round(us, 2),
                              "tflops": round(tf, 1), "frac_of_2500": round(tf / 2500, 4), "err": round(err, 5)}), flush=True)
    o.attn_q64 = None


def kernel_only(b, h, n, d, dtype, auto=False, window=None):
    """(callable launching sat_attention_fwd — with `window`, sat_attention_fwd_window — alone on prepared planes, callable preparing the
    three operands, max rel error against torch's attention under the same band)"""
    q, k, v = (torch.randn(b, n, h, d, device='cuda').to(dtype).permute(0, 2, 1, 3) for _ in range(3))      # the model's (B, N, H, D) storage
    scale = d ** -0.5
    qp, kp, vp = o.attn_planes(q), o.attn_planes(k), o.attn_planes(v, row_major=False, transposed=True)
    out = torch.empty(b, n, h * d, dtype=dtype, device='cuda')
    # bf16: 2 = the basic shape forced (head dim 64: 32 queries per wave, the kernel head dim 128 is modelled on; 128: 4 waves per
    # workgroup), 1 = what the library picks (128: 8 waves per workgroup once 256-query workgroups give every CU one)
    dt = 0 if dtype == torch.float32 else (1 if auto else 2)

    def launch():
        common = (_ptr(qp["rm"][0]), _ptr(qp["rm"][1]), _ptr(kp["rm"][0]), _ptr(kp["rm"][1]), _ptr(vp["tr"][0]), _ptr(vp["tr"][1]),
                  _ptr(out), None, b, h, h, n, n, qp["np"], kp["np"], d, scale, dt, torch.cuda.current_stream().cuda_stream)
        rc = o.lib.sat_attention_fwd(*common) if window is None else o.lib.sat_attention_fwd_window(*common, *window)
        assert rc == 0, o.lib.sat_last_error()

    def prepare():
        o.attn_planes(q), o.attn_planes(k), o.attn_planes(v, row_major=False, transposed=True)
    launch()
    mask = None
    if window is not None:
        i, j = torch.arange(n, device='cuda')[:, None], torch.arange(n, device='cuda')[None, :]
        mask = ((j >= i - window[0]) if window[0] >= 0 else (j >= 0)) & ((j <= i + window[1]) if window[1] >= 0 else (j >= 0))
    ref = torch.nn.functional.scaled_dot_product_attention(q[:1].float(), k[:1].float(), v[:1].float(), attn_mask=mask, scale=scale).permute(0, 2, 1, 3).reshape(1, n, h * d)
    err = float((out[:1].float() - ref).abs().max() / ref.abs().max())
    return launch, prepare, err


def median_us(f, n):
    t = sorted(timeit(f, n=n) for _ in range(5))
    return t[2], t[0], t[4]


def head_dim_128():
    peak = {torch.bfloat16: 2500.0}      # dense bf16 MFMA peak, TFLOP/s; the fp32 mode issues 3 bf16 MFMAs per product
    for dtype, n, bh in ((torch.bfloat16, 1025, 16), (torch.bfloat16, 6145, 16), (torch.float32, 1025, 16)):
        rows = []
        variants = [(128, bh, False), (64, 2 * bh, False)] + ([(128, bh, True)] if dtype == torch.bfloat16 else [])
        for d, heads, auto in variants + variants:      # alternate the kernels: same process, same box
            launch, prepare, err = kernel_only(2, heads // 2, n, d, dtype, auto)
            med, lo, hi = median_us(launch, 100 if n < 4000 else 40)
            pmed, _, _ = median_us(prepare, 100 if n < 4000 else 40)
            flops = 4.0 * heads * n * n * d
            mf = flops * (3 if dtype == torch.float32 else 1)
            rows.append({"head_dim": d, "kernel": "auto" if auto else "basic", "dtype": str(dtype).split(".")[1], "B*H": heads, "N": n, "us_median": round(med, 2), "us_min": round(lo, 2),
                         "us_max": round(hi, 2), "tflops": round(flops / med * 1e-6, 1), "mfma_frac_of_bf16_peak": round(mf / med * 1e-6 / peak[torch.bfloat16], 4),
                         "prepare_qkv_us": round(pmed, 2), "err": round(err, 6)})
            print(json.dumps(rows[-1]), flush=True)
        t128 = min(r["us_median"] for r in rows if r["head_dim"] == 128 and r["kernel"] == ("auto" if dtype == torch.bfloat16 else "basic"))
        t64 = min(r["us_median"] for r in rows if r["head_dim"] == 64)
        print(json.dumps({"N": n, "dtype": rows[0]["dtype"], "hd128_over_hd64_time_at_equal_flops": round(t128 / t64, 4)}), flush=True)


def windowed(window):
    for d, heads in ((64, 48), (128, 24)):
        for n in (1025, 6145):
            reps = 100 if n < 4000 else 40
            kinds = {"windowed": kernel_only(2, heads // 2, n, d, torch.bfloat16, False, tuple(window)),
                     "dense_basic": kernel_only(2, heads // 2, n, d, torch.bfloat16, False),
                     "dense_auto": kernel_only(2, heads // 2, n, d, torch.bfloat16, True)}
            runs = {name: [] for name in kinds}
            for _ in range(6):      # alternate the launches: same process, same box
                for name, (launch, _, _) in kinds.items():
                    runs[name].append(round(median_us(launch, reps)[0], 2))
            for name in kinds:
                print(json.dumps({"head_dim": d, "N": n, "B*H": heads, "dtype": "bfloat16", "launch": name, "window": list(window) if name == "windowed" else None,
                                  "us_runs": runs[name], "us_min": min(runs[name]), "us_max": max(runs[name]), "err": round(kinds[name][2], 6)}), flush=True)
            dense = min(min(runs["dense_basic"]), min(runs["dense_auto"]))
            print(json.dumps({"head_dim": d, "N": n, "windowed_over_dense_time": round(max(runs["windowed"]) / dense, 4)}), flush=True)


if args.window is not None:
    windowed(args.window)
elif args.head_dim == 64:
    head_dim_64()
else:
    head_dim_128()
