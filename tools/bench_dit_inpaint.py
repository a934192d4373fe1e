#!/usr/bin/env python
"""A / B / A / B of the inpainting train step's front at the `bench.py --workload dit_train` shape (Stable Audio Open DiT, B = 4,
C = 64, T = 1024, bf16-mixed), with the model widened to an inpainting model (input_concat_dim = io_channels + 1) and
DiTTrainStep(inpainting_config={}): arm "fused" is ops.dit_step_fused = True (one sat_diffusion_noise_inpaint launch), arm "torch"
is dit_step_fused = False (the table expanded, torch.where, cat).  Prints one JSON line:
  step_ms: per arm, the time of each of its rounds (the spread between rounds of the same arm is the A/A spread);
  front_us: HIP-event time of the step front alone (DiTTrainStep._inpaint_front), median over --front-reps calls, per arm;
  front_launches / step_launches: GPU kernel launches of one front call / one whole step per arm (torch.profiler);
  host_syncs_per_step: 0 when one step per arm, with the timesteps handed in as a device tensor, runs under
  torch.cuda.set_sync_debug_mode("error") without raising; host_syncs_default_sampler: the same check with the step drawing its own
  timesteps ("uniform": Sobol points drawn on the CPU as the reference draws them, then a blocking copy of B floats from pageable
  memory, which the debug mode reports — a host-to-device copy, not a read of the device).
    python tools/bench_dit_inpaint.py --steps 5 --warmup 2 --rounds 2"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def count_launches(fn):
    """GPU kernels launched by fn(), or None when the profiler is not usable here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:      # noqa: BLE001
        print(f"profiler unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--depth", type=int, default=None, help="transformer depth (default: the config's)")
    ap.add_argument("--front-reps", type=int, default=50)
    ap.add_argument("--no-launch-counts", action="store_true")
    args = ap.parse_args()
    from stable_audio_tools_amd import ops as ops_mod
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.training import DiTTrainStep, random_inpaint_segments
    dev = torch.device("cuda", 0)
    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_open_dit.json")))
    dcfg = dict(cfg["diffusion"]["config"])
    dcfg["input_concat_dim"] = dcfg["io_channels"] + 1
    if args.depth is not None:
        dcfg["depth"] = args.depth
    torch.manual_seed(1234)
    model = DiffusionTransformer(**dcfg)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("to_out.weight") or ".ff.ff.2." in n_ or "process_conv" in n_:
                p.normal_(0.0, 0.02)
    model = model.to(dev).train(True)
    stepper = DiTTrainStep(model, lr=5e-5, cfg_dropout_prob=0.1, autocast_dtype=torch.bfloat16, inpainting_config={})
    o = ops_mod.get_ops()
    b, tlat, m = args.batch, cfg["latent_length"], cfg["context_length"]
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(b, dcfg["io_channels"], tlat, generator=g).to(dev)
    cross = torch.randn(b, m, dcfg["cond_token_dim"], generator=g).to(dev)
    glob = torch.randn(b, dcfg["global_cond_dim"], generator=g).to(dev)

    def step(**kw):
        return stepper(lat, cross_attn_cond=cross, global_embed=glob, **kw)

    def raises_on_sync(**kw):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            step(**kw)
            return 0
        except RuntimeError as e:
            return repr(e)[:200]
        finally:
            torch.cuda.set_sync_debug_mode("default")

    arms = {"fused": True, "torch": False}
    step_ms = {k: [] for k in arms}
    try:
        for name, flag in arms.items():
            o.dit_step_fused = flag
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, flag in arms.items():
                o.dit_step_fused = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = step()
                torch.cuda.synchronize()
                step_ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        # the front alone
        noise, t = torch.randn_like(lat), torch.rand(b, device=dev)
        seg = random_inpaint_segments([tlat] * b, tlat).to(dev)
        front_us, front_launches, step_launches, syncs, syncs_default = {}, {}, {}, {}, {}
        for name, flag in arms.items():
            o.dit_step_fused = flag
            times = []
            for _ in range(args.front_reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                stepper._inpaint_front(lat, noise, t, seg)
                e1.record()
                e1.synchronize()
                times.append(1e3 * e0.elapsed_time(e1))
            front_us[name] = statistics.median(times[5:])
            syncs[name] = raises_on_sync(t=t)
            syncs_default[name] = raises_on_sync()
            if not args.no_launch_counts:
                front_launches[name] = count_launches(lambda: stepper._inpaint_front(lat, noise, t, seg))
                step_launches[name] = count_launches(step)
    finally:
        o.dit_step_fused = True
    print(json.dumps({"tool": "bench_dit_inpaint", "batch": b, "channels": dcfg["io_channels"], "latent_frames": tlat, "depth": dcfg["depth"],
                      "steps_per_round": args.steps, "warmup": args.warmup, "step_ms": step_ms, "front_us": front_us,
                      "front_launches": front_launches, "step_launches": step_launches, "host_syncs_per_step": syncs,
                      "host_syncs_default_sampler": syncs_default,
                      "final_loss": float(out["loss"])}))


if __name__ == "__main__":
    main()
