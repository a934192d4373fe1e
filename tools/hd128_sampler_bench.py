"""A Stable-Audio-Open-Small-shaped DiT at head dim 128 (embed_dim 1024, depth 16, 8 heads of 128, qk_norm "ln", adaLN, cross-attention
on 64 context tokens of width 768 projected to 1024, N = 1025, bf16, CFG 6.0: a denoiser batch of 2), GPU:
  * one sampler step = one guided denoiser evaluation: milliseconds per step (median of 5 timings of 20 evaluations replayed from a HIP
    graph, HIP events) and steps/s; sample_v_ddim(use_graph=True) over 50 steps end to end next to it;
  * the share of a step spent in what head dim 128 does NOT yet fuse into the projection epilogue: plane preparation (ops.attn_planes) and
    the standalone norm / rotary (ops.qk_norm): every such call of one evaluation is recorded with its arguments and re-timed alone
    (graph replays), the attention kernel itself (ops.attention minus its three preparations) the same way.
    python tools/hd128_sampler_bench.py [--batch 1] [--length 1025]"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd import ops as ops_mod
from stable_audio_tools_amd.dit import DiffusionTransformer
from stable_audio_tools_amd.sampling import sample_v_ddim

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--length", type=int, default=1025)
ap.add_argument("--depth", type=int, default=16)
args = ap.parse_args()
torch.manual_seed(0)
real = ops_mod.get_ops()


def graph_us(f, calls=20, reps=3):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        f()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            for _ in range(calls):
                f()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / (calls * reps) * 1e3)
    return sorted(times)[2]


class Recording:
    """Forwards to the ops object; keeps the arguments of every qk_norm / attention call."""

    def __init__(self, ops):
        self.__dict__["_ops"], self.__dict__["calls"] = ops, []

    def __getattr__(self, name):
        val = getattr(self._ops, name)
        if name not in ("qk_norm", "attention"):
            return val

        def wrapped(*a, **k):
            self.calls.append((name, a, k))
            return val(*a, **k)
        return wrapped

    def __setattr__(self, name, val):
        setattr(self._ops, name, val)


model = DiffusionTransformer(io_channels=64, embed_dim=1024, depth=args.depth, num_heads=8, cond_token_dim=768, global_cond_dim=768,
                             project_cond_tokens=True, global_cond_type="adaLN", attn_kwargs={"qk_norm": "ln"})      # context projected to 1024: 8 kv heads
for p in model.parameters():      # the output projections are zero-initialised: give every layer work that reaches the output
    if p.dim() > 1 and float(p.abs().max()) == 0.0:
        torch.nn.init.normal_(p, std=0.02)
model = model.to(device="cuda", dtype=torch.bfloat16).train(False)
assert model.transformer.layers[0].self_attn.dim_heads == 128
b, n = args.batch, args.length
x = torch.randn(b, 64, n, device="cuda")
t = torch.full((b,), 0.5, device="cuda")
kw = dict(cross_attn_cond=torch.randn(b, 64, 768, device="cuda"), global_embed=torch.randn(b, 768, device="cuda"), cfg_scale=6.0, scale_phi=0.75)


def step():
    with torch.no_grad():
        return model(x, t, **kw)


rec = Recording(real)
original = ops_mod.get_ops
ops_mod.get_ops = lambda: rec
try:
    step()
    rec.calls.clear()
    step()
    recorded = list(rec.calls)
finally:
    ops_mod.get_ops = original
step_us = graph_us(step, calls=20, reps=2)
parts = {"attn_planes": 0.0, "qk_norm": 0.0, "attention": 0.0}
with torch.no_grad():
    for name, a, k in recorded:
        parts[name] += graph_us(lambda: getattr(real, name)(*a, **k), calls=20, reps=3)
        if name == "attention":      # its three plane preparations, alone
            q_, k_, v_ = a[:3]
            parts["attn_planes"] += graph_us(lambda: (real.attn_planes(q_), real.attn_planes(k_), real.attn_planes(v_, row_major=False, transposed=True)),
                                             calls=20, reps=3)
kernel_us = parts["attention"] - parts["attn_planes"]      # ops.attention = three preparations + the forward kernel
count = {nm: sum(1 for c in recorded if c[0] == nm) for nm in ("qk_norm", "attention")}
torch.cuda.synchronize()
sample_v_ddim(model, x, 4, use_graph=True, **kw)
torch.cuda.synchronize()
t0 = time.perf_counter()
sample_v_ddim(model, x, 50, use_graph=True, **kw)
torch.cuda.synchronize()
wall = time.perf_counter() - t0
print(json.dumps({"batch": b, "N": n, "depth": args.depth, "step_ms": round(step_us / 1e3, 3), "steps_per_s": round(1e6 / step_us, 1),
                  "sample_v_ddim_50_steps_s": round(wall, 3), "sample_v_ddim_steps_per_s": round(50 / wall, 1),
                  "calls_per_step": count, "attn_planes_us": round(parts["attn_planes"], 1), "qk_norm_us": round(parts["qk_norm"], 1),
                  "attention_kernels_us": round(kernel_us, 1),
                  "share_planes_plus_norm": round((parts["attn_planes"] + parts["qk_norm"]) / step_us, 4),
                  "share_attention_kernels": round(kernel_us / step_us, 4)}))
