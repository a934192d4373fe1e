#!/usr/bin/env python
"""bench.py — train-step throughput of the hot path on MI355X.

Workload (BASELINE.json configs[1], named in `config.workload`): one *generator optimisation step* of
the Oobleck audio VAE on 47.55 s stereo 44.1 kHz items (sample_size 2097152): encode -> VAE sample ->
decode -> multi-resolution STFT loss (sum/diff + L + R, 7 resolutions, A-weighted) + KL -> backward ->
data-parallel gradient all-reduce -> fused AdamW (+EMA).  fp32, synthetic audio, random-init weights of
the stable_audio_2_0_vae architecture.  `value` times that generator step (comparable across rounds and
across N).

A plain run does what that figure needs and no more: set-up, the warm-up and timed steps (eager launches,
then the same steps replayed from a HIP graph), `--dump-outputs`, the line.  Its `roofline` (dominant
kernel) comes from HIP events recorded in the timed eager steps and from committed counter profiles, so
it costs no run of its own.

`--full` adds everything else the line can carry, each leg a run of its own after the headline's steps:
the reference's REAL step, which alternates the generator step with the MS-STFT discriminator update
(training/autoencoders.py:440-515) on the same items — top-level
`real_step_samples_per_s` / `real_step_ms`, details in `config.real_step`; `config.batch_sweep`;
`cpu_baseline` (ONE un-scaled generator step of the REFERENCE's own modules on the host cores, from the
tree oracle/stage_ref.py staged); `parity` (the bench item against the CPU oracle); `secondary` (the
metric's second half: DiT sampling steps/s, configs[2]); `long_context` (configs[4] on one GPU) and
`dit_train`.  The other workloads keep their CPU baselines and parity evaluations behind `--full` too.

Contract: `python bench.py --gpus N --steps K --warmup W [--full]`; for N>1 launched by torch.distributed.run
(one rank per GPU, RCCL).  Rank 0 prints ONE JSON line.  `--ddp-single-rank` runs the N=1 step inside a
1-rank RCCL process group with the overlapped gradient exchange forced on (the P1 path on a 1-GPU box).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on these hosts: RCCL across processes needs it (set before HIP starts)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SAMPLE_SIZE = 2097152
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak (= fp32 vector peak)


# the legs of the line that only `--full` runs (each has a --no-<leg> option that drops it from a full run)
FULL_ONLY_LEGS = ("cpu_baseline", "real_step", "secondary", "long_context", "dit_train", "batch_sweep", "parity")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 3 vae_train, 50 dit_sample, 5 dit_train)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default: 1 / 5 / 2)")
    ap.add_argument("--batch", type=int, default=None,
                    help="items per GPU per step (default: 1 for vae_train and dit_sample, 4 for dit_train)")
    ap.add_argument("--sample-size", type=int, default=SAMPLE_SIZE)
    ap.add_argument("--full", action="store_true",
                    help="after the headline's steps, also run everything else the line can carry: the batch sweep, the CPU baselines, the "
                         "oracle parity checks, the alternating discriminator / generator step, the DiT sampling, long-context and DiT "
                         "training measurements (minutes; the --no-* options below drop single legs of it).  Without it a run sets up, "
                         "warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines (and the DiT parity evaluations that ride on them)")
    ap.add_argument("--no-real-step", action="store_true", help="--full: skip the timing of the alternating discriminator / generator step")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the DiT sampling measurement appended to the full line")
    ap.add_argument("--no-long-context", action="store_true", help="--full: skip the N = 6145 fp8 sampling measurement (BASELINE.json configs[4])")
    ap.add_argument("--no-dit-train", action="store_true", help="--full: skip the DiT training-step measurement appended to the full line (configs[2]/[3])")
    ap.add_argument("--no-batch-sweep", action="store_true", help="--full: skip the generator step at per-GPU batch 2 and 4 (config.batch_sweep)")
    ap.add_argument("--no-parity", action="store_true", help="--full: skip the oracle parity check of the bench item (about one CPU-minute)")
    ap.add_argument("--no-parity-gradients", action="store_true",
                    help="--full parity: forward quantities only (skip the oracle's autograd pass over the full item: ~1.5 CPU-minutes, +41 GiB host memory)")
    ap.add_argument("--cpu-baseline-samples", type=int, default=32768, help="length of the probe crop that picks the thread count")
    ap.add_argument("--cpu-baseline-budget-s", type=float, default=100.0,
                    help="time budget of the ONE un-scaled CPU reference step (the full item when it fits, else the largest 1/2^k of it)")
    ap.add_argument("--workload", choices=["vae_train", "dit_sample", "dit_train", "long_context"], default="vae_train",
                    help="vae_train: BASELINE.json configs[1] (default, the metric's first half); "
                         "dit_sample: configs[2] DiT sampling steps/s (the metric's second half)")
    ap.add_argument("--dit-dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--ddp-single-rank", action="store_true",
                    help="N = 1 inside a 1-rank RCCL ('nccl') process group with the gradient exchange forced on (hooks, side stream, "
                         "per-bucket events, collectives on a 1-rank communicator): the data-parallel code path on a single-GPU box")
    ap.add_argument("--ddp-mode", choices=["all_reduce", "reduce_scatter"], default="all_reduce")
    ap.add_argument("--ddp-comm-dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--ops-set", action="append", default=[], metavar="ATTR=VALUE",
                    help="A/B knob: set an attribute of the SatOps object before the run (e.g. ru_k1_fused=0); recorded in config.ops_set")
    ap.add_argument("--no-grad-steal", action="store_true",
                    help="A/B knob: gradients accumulate into the flat views through autograd's per-parameter adds (rounds 1-4) instead of "
                         "being adopted and gathered in one launch (training.FlatParameters.steal)")
    ap.add_argument("--no-graph", action="store_true", help="time the eager launches only (skip the HIP-graph replay of the train step)")
    ap.add_argument("--graph-ddp", action="store_true",
                    help="also try the HIP-graph step when a process group is active (the RCCL collectives are then captured too)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="vae_train: after the timed steps, write what the last timed step of each launch mode returned (its losses, "
                         "float64) and the parameters it wrote (float32, a fixed seeded sample) to DIR/<mode>_<name>.npy "
                         "(bench_outputs/ is git-ignored)")
    args = ap.parse_args(argv)
    if args.dump_outputs is not None and args.workload != "vae_train":
        ap.error("--dump-outputs is implemented for --workload vae_train")
    if not args.full:       # a plain run is the headline alone: every leg beside it is off, whatever the --no-* options say
        for leg in FULL_ONLY_LEGS:
            setattr(args, "no_" + leg, True)
    if args.batch is None:
        args.batch = 4 if args.workload == "dit_train" else 1
    dsteps, dwarm = {"vae_train": (3, 1), "dit_sample": (50, 5), "dit_train": (5, 2), "long_context": (6, 2)}[args.workload]
    if args.steps is None:
        args.steps = dsteps
    if args.warmup is None:
        args.warmup = dwarm
    return args


PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak


class AttnProfiler:
    """HIP-event timing + algorithmic flops (4*Nq*Nk*64*H*B) of every sat_attn_fwd_kernel launch, self-attention
    (Nk == Nq) and cross-attention (Nk = context length) kept apart."""

    def __init__(self, ops, max_launches=192):
        self.records = {"self": [], "cross": [], "bwd_self": [], "bwd_cross": []}
        self.enabled = False
        self.budget = max_launches     # only the first launches of the timed region carry events: a sampler step is
        orig = ops.lib.sat_attention_fwd   # host-bound, and two event objects per launch would slow the measured loop

        def timed(*a):
            if not self.enabled or self.budget <= 0:
                return orig(*a)
            self.budget -= 1
            b, h, _hkv, nq, nk = a[8:13]
            d = a[15]
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig(*a)
            e.record()
            self.records["self" if nq == nk else "cross"].append((s, e, 4.0 * b * h * nq * nk * d))
            return rc

        self._lib, self._orig = ops.lib, orig
        ops.lib.sat_attention_fwd = timed
        # backward (training): one entry point = the dQ kernel + the dK / dV kernel; algorithmic flops = the five matmuls of the attention
        # backward (S, dP, dV, dK, dQ: 10 * Nq * Nk * 64 * H * B; both kernels recompute S and dP, which is not counted)
        self.bwd_budget = max_launches
        orig_bwd = ops.lib.sat_attention_bwd

        def timed_bwd(*a):
            if not self.enabled or self.bwd_budget <= 0:
                return orig_bwd(*a)
            self.bwd_budget -= 1
            b, h, _hkv, nq, nk = a[6:11]
            d = a[13]
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig_bwd(*a)
            e.record()
            self.records["bwd_self" if nq == nk else "bwd_cross"].append((s, e, 10.0 * b * h * nq * nk * d))
            return rc

        self._orig_bwd = orig_bwd
        ops.lib.sat_attention_bwd = timed_bwd
        # round 6: the short-key (cross-attention) entry points, csrc/attention_cross.h — own budgets, so that the self-attention
        # launches keep theirs; the same records ("cross" / "bwd_cross"; a self-attention with <= 256 keys would land in "self")
        self.cross_budget, self.cross_bwd_budget = max_launches, max_launches
        orig_x, orig_xb = ops.lib.sat_attention_cross_fwd, ops.lib.sat_attention_cross_bwd

        def timed_x(*a):      # (q_rm, k_rm, v_tr, o, lse, B, H, Hkv, Nq, Nk, Nqp, Nkp, head_dim, scale, stream)
            if not self.enabled or self.cross_budget <= 0:
                return orig_x(*a)
            self.cross_budget -= 1
            b, h, _hkv, nq, nk = a[5:10]
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig_x(*a)
            e.record()
            self.records["self" if nq == nk else "cross"].append((s, e, 4.0 * b * h * nq * nk * a[12]))
            return rc

        def timed_xb(*a):     # (planes, lse, dsum, dq, dk, dv, ws, ws_bytes, B, H, Hkv, Nq, Nk, Nqp, Nkp, head_dim, scale, stream)
            if not self.enabled or self.cross_bwd_budget <= 0:
                return orig_xb(*a)
            self.cross_bwd_budget -= 1
            b, h, _hkv, nq, nk = a[8:13]
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig_xb(*a)
            e.record()
            self.records["bwd_self" if nq == nk else "bwd_cross"].append((s, e, 10.0 * b * h * nq * nk * a[15]))
            return rc

        self._orig_x, self._orig_xb = orig_x, orig_xb
        ops.lib.sat_attention_cross_fwd = timed_x
        ops.lib.sat_attention_cross_bwd = timed_xb
        # the projection GEMMs (80 % of a sampler step's GPU time): same budgeted event timing, algorithmic flops 2*M*N*K
        self.gemm = []
        self.gemm_budget = 2 * max_launches     # (about two model evaluations: events cost host time in the measured loop)
        self._gemm_orig = {}
        specs = {"sat_gemm_bf16": lambda a: 2.0 * a[15] * a[16] * a[17],
                 "sat_gemm_qkv_bf16": lambda a: 2.0 * (a[10] * a[11]) * (a[16] * a[13] * 64) * a[14],
                 # fp8 (e4m3, MX MFMA) forward projections of the long-context configuration
                 "sat_gemm_fp8": lambda a: 2.0 * a[18] * a[19] * a[20],
                 "sat_gemm_qkv_fp8": lambda a: 2.0 * (a[13] * a[14]) * (a[19] * a[16] * 64) * a[17],
                 # activation quantisation passes in front of the fp8 GEMMs: time only (per-row quantiser; round 3's per-tensor pair)
                 "sat_quant_fp8_rows": lambda a: 0.0, "sat_quant_fp8": lambda a: 0.0, "sat_absmax_scale": lambda a: 0.0}
        self.kinds = {}
        for name, fl in specs.items():
            self._wrap_gemm(ops.lib, name, fl)

    def _wrap_gemm(self, lib, name, flops):
        orig = getattr(lib, name)
        self._gemm_orig[name] = orig

        def timed(*a):
            if not self.enabled or self.gemm_budget <= 0:
                return orig(*a)
            self.gemm_budget -= 1
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig(*a)
            e.record()
            self.gemm.append((s, e, flops(a), name, self._shape_key(name, a)))
            return rc

        setattr(lib, name, timed)

    @staticmethod
    def _shape_key(name, a):
        """(entry point, M, N, K, epilogue, fp32 out, splits, tile) of a projection launch — SAT_BENCH_GEMM_SHAPES=1 lists the time per shape"""
        if name == "sat_gemm_bf16":
            return (name, a[15], a[16], a[17], a[18], a[19], a[20], a[21])
        if name == "sat_gemm_qkv_bf16":
            return (name, a[10] * a[11], a[16] * a[13] * 64, a[14], 4, 0, 1, a[17])
        if name == "sat_gemm_fp8":
            return (name, a[18], a[19], a[20], a[21], a[22], 1, a[23])
        if name == "sat_gemm_qkv_fp8":
            return (name, a[13] * a[14], a[19] * a[16] * 64, a[17], 4, 0, 1, a[20])
        return (name,)

    def gemm_shapes(self):
        torch.cuda.synchronize()
        agg = {}
        for s, e, _f, _n, key in self.gemm:
            d = agg.setdefault(key, [0, 0.0])
            d[0] += 1
            d[1] += s.elapsed_time(e)
        rows = [{"key": list(k), "launches": v[0], "avg_us": round(1e3 * v[1] / v[0], 1), "total_ms": round(v[1], 3)} for k, v in agg.items()]
        rows.sort(key=lambda r: -r["total_ms"])
        return rows

    def restore(self):
        self._lib.sat_attention_fwd = self._orig
        self._lib.sat_attention_bwd = self._orig_bwd
        self._lib.sat_attention_cross_fwd = self._orig_x
        self._lib.sat_attention_cross_bwd = self._orig_xb
        for name, orig in self._gemm_orig.items():
            setattr(self._lib, name, orig)

    def gemm_summary(self, peak, fp8=False):
        """bf16 (or, fp8=True, fp8) projection launches: achieved TFLOP/s over HIP-event time; the fp8 summary also carries the
        time of the sat_quant_fp8 passes that feed them."""
        torch.cuda.synchronize()
        want = ("sat_gemm_fp8", "sat_gemm_qkv_fp8") if fp8 else ("sat_gemm_bf16", "sat_gemm_qkv_bf16")
        recs = [r for r in self.gemm if r[3] in want]
        ms = sum(r[0].elapsed_time(r[1]) for r in recs)
        fl = sum(r[2] for r in recs)
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        out_extra = {}
        if fp8:
            q = [r for r in self.gemm if r[3] in ("sat_quant_fp8_rows", "sat_quant_fp8", "sat_absmax_scale")]
            out_extra = {"quant_launches": len(q), "quant_total_ms": round(sum(r[0].elapsed_time(r[1]) for r in q), 3)}
        if os.environ.get("SAT_BENCH_GEMM_SHAPES") == "1":
            out_extra["shapes"] = self.gemm_shapes()
        return {"kernel": "sat_gemm_kernel" + ("<fp8>" if fp8 else ""), "launches": len(recs), "total_ms": round(ms, 3), "achieved": round(ach, 1),
                "peak": peak, "frac": round(ach / peak, 4), **out_extra,
                "note": "every projection launch (sat_gemm_bf16 / sat_gemm_qkv_bf16) of the first model evaluations of the timed region: "
                        "2*M*N*K over HIP-event time, epilogues (SwiGLU, residual, head split + rotary + plane layout) included"}

    def summary(self, which="self"):
        torch.cuda.synchronize()
        recs = self.records[which]
        ms = sum(s.elapsed_time(e) for s, e, _ in recs)
        return len(recs), ms, sum(f for _, _, f in recs)

    def roofline(self, peak):
        """roofline object of the self-attention launches (the dominant ones); cross-attention listed beside it."""
        nl, ms, fl = self.summary("self")
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        nc, msc, flc = self.summary("cross")
        bwd = {}
        for which in ("bwd_self", "bwd_cross"):
            nb, msb, flb = self.summary(which)
            if nb:
                achb = flb / (msb * 1e-3) / 1e12
                kn = ("sat_attn_cross_dq_kernel + sat_attn_cross_dkv_kernel + sat_attn_cross_reduce_kernel (short-key kernels, csrc/attention_cross.h; cross_kernels off or fp32: the general ones)"
                      if which == "bwd_cross" else "sat_attn_bwd_dq_bf16_kernel + sat_attn_bwd_dkv_bf16_kernel (fp32 mode: the general sat_attn_bwd_{dq,dkv}_kernel)")
                bwd[which] = {"kernels": kn, "launches": nb, "avg_launch_ms": msb / nb,
                              "achieved": round(achb, 1), "frac": round(achb / peak, 4)}
        extra = {"backward": bwd} if bwd else {}
        return {**extra, "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
                "kernel": "sat_attn_fwd_kernel", "launches": nl, "avg_launch_ms": ms / nl if nl else None,
                "cross_attention": {"kernel": "sat_attn_cross_fwd_kernel (csrc/attention_cross.h; sat_attn_fwd_kernel when ops.cross_kernels is off)",
                                    "launches": nc, "avg_launch_ms": msc / nc if nc else None,
                                    "achieved": flc / (msc * 1e-3) / 1e12 if msc > 0 else 0.0,
                                    "frac": (flc / (msc * 1e-3) / 1e12 / peak) if msc > 0 else 0.0},
                "projections": self.gemm_summary(peak),
                "note": "self-attention launches (the first ~4 model evaluations of the timed region): algorithmic flops 4*N*N*64*H*B over HIP-event time on the launch stream; "
                        "peak = dense bf16 MFMA (fp32 mode: /3 for the bf16x3 split); cross-attention (GQA, M=130 keys) apart"}



_REF_DIT = {}


def _ref_dit(dcfg, train=False):
    """The reference's DiffusionTransformer (fp32, host) for `dcfg`, built ONCE per configuration and shared by every CPU leg of the line
    (sampler baseline, the two parity evaluations, the training baseline): its default initialisation alone takes ~8 s of host time.
    Callers load the weights they compare against; the training leg's gradients are dropped by the next call."""
    import contextlib
    import refimport
    key = json.dumps(dcfg, sort_keys=True)
    ref = _REF_DIT.get(key)
    if ref is None:
        with contextlib.redirect_stdout(sys.stderr):
            refimport.import_reference()
            from stable_audio_tools.models.dit import DiffusionTransformer as RefDiT
            ref = _REF_DIT[key] = RefDiT(**dcfg).float()
    ref.zero_grad(set_to_none=True)
    return ref.train(train)

def dit_cpu_baseline(dcfg, latent_len, ctx_len):
    """One sampler step's model evaluation (fp32, CFG batch of 2) on this box's host cores: the reference's own
    DiffusionTransformer when /root/reference is importable (kind "reference"), the oracle port otherwise.  Thread count =
    the faster of 16 / 32 (one probe each after a warm-up), then the median of 3."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import dit_oracle
    from stable_audio_tools_amd.dit import DiffusionTransformer
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, dcfg["io_channels"], latent_len, generator=g)
    cross = torch.randn(1, ctx_len, dcfg["cond_token_dim"], generator=g)
    glob = torch.randn(1, dcfg["global_cond_dim"], generator=g)
    t = torch.tensor([0.5])
    kind = "port"
    if _reference_importable():
        ref = _ref_dit(dcfg)
        kind = "reference"

        def step():
            with torch.no_grad():
                ref(x, t, cross_attn_cond=cross, global_embed=glob, cfg_scale=6.0, scale_phi=0.75)
    else:
        with torch.device("meta"):
            shapes = {k: (tuple(v.shape), v.dtype) for k, v in DiffusionTransformer(**dcfg).state_dict().items()}
        sd = {k: (torch.randn(sh) * 0.02 if dt.is_floating_point else torch.zeros(sh, dtype=dt)) for k, (sh, dt) in shapes.items()}
        half = 32
        sd["transformer.rotary_pos_emb.inv_freq"] = 1.0 / (10000 ** (torch.arange(0, half, 2).float() / half))

        def step():
            with torch.no_grad():
                dit_oracle.dit_forward(sd, dcfg, x, t, cross, glob, cfg_scale=6.0, scale_phi=0.75)
    ncpu = os.cpu_count() or 1
    probes = {}
    for cores in sorted({min(ncpu, c) for c in (16, 32)}):
        torch.set_num_threads(cores)
        probes[cores] = _median_time(step, reps=1)
    cores = min(probes, key=probes.get)
    torch.set_num_threads(cores)
    dt = _median_time(step, reps=3)
    return {"value": 1.0 / dt, "unit": "steps/s", "cores": cores, "kind": kind,
            "sample": f"1 sampler step = 1 model evaluation (fp32, CFG batch 2, N={latent_len + 1}): median of 3 after warm-up = {dt:.2f} s "
                      f"at {cores} threads (probes: {', '.join(f'{c}: {v:.2f} s' for c, v in probes.items())})"}


def dit_train_cpu_baseline(dcfg, latent_len, ctx_len):
    """One DiT training evaluation on the host cores (fp32 forward + autograd backward of the v-objective MSE, ONE sample, no optimizer
    step): the reference's own DiffusionTransformer (models/dit.py:231-431; its per-layer checkpointing, transformer.py:840-845, is what
    the reference trains with) when its tree is importable (kind "reference"), else the oracle port."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, dcfg["io_channels"], latent_len, generator=g)
    cross = torch.randn(1, ctx_len, dcfg["cond_token_dim"], generator=g)
    glob = torch.randn(1, dcfg["global_cond_dim"], generator=g)
    target = torch.randn(1, dcfg["io_channels"], latent_len, generator=g)
    t = torch.tensor([0.5])
    if _reference_importable():
        ref = _ref_dit(dcfg, train=True)
        t0 = time.perf_counter()
        out = ref(x, t, cross_attn_cond=cross, global_embed=glob, cfg_dropout_prob=0.1)
        (out - target).square().mean().backward()
        dt = time.perf_counter() - t0
        ref.zero_grad(set_to_none=True)
        return {"value": 1.0 / dt, "unit": "samples/s", "cores": cores, "kind": "reference",
                "sample": f"1 sample: the reference's DiffusionTransformer forward (per-layer checkpointing as it trains) + autograd backward "
                          f"(fp32, N={latent_len + 1}, no optimizer step), single evaluation = {dt:.2f} s at {cores} threads"}
    import dit_oracle
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**dcfg)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    t0 = time.perf_counter()
    out = dit_oracle.dit_forward(sd, dcfg, x, t, cross, glob, cfg_scale=1.0)
    (out - target).square().mean().backward()
    dt = time.perf_counter() - t0
    return {"value": 1.0 / dt, "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": f"1 sample: oracle DiT forward + autograd backward (fp32, N={latent_len + 1}, no optimizer step) in {dt:.2f} s at {cores} threads"}


def dit_train_object(batches=(4, 16), steps=5, warmup=2, with_cpu_baseline=True):
    """BASELINE.json configs[2]/[3] inside the DEFAULT line: the Stable-Audio-Open-1.0 DiT training step (training/diffusion.py:332-487
    restated by training.DiTTrainStep: v-objective MSE, cfg_dropout 0.1, bf16-mixed, fused AdamW + EMA; every activation resident, no
    checkpoint recompute) on ONE GPU at per-GPU batch 4 and at the larger batch the 288 GB hold — samples/s, model TFLOP/s, the
    attention kernels' rooflines (forward and backward) by HIP events, the reference's CPU step beside it."""
    dev = torch.device("cuda", 0)
    from stable_audio_tools_amd import ops as O
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.training import DiTTrainStep
    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_open_dit.json")))
    dcfg = cfg["diffusion"]["config"]
    torch.manual_seed(1234)
    model = DiffusionTransformer(**dcfg)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("to_out.weight") or ".ff.ff.2." in n_ or "process_conv" in n_:
                p.normal_(0.0, 0.02)
    model = model.to(dev).train(True)
    stepper = DiTTrainStep(model, lr=5e-5, cfg_dropout_prob=0.1, autocast_dtype=torch.bfloat16)
    tlat, m = cfg["latent_length"], cfg["context_length"]
    n, d, depth = tlat + 1, dcfg["embed_dim"], dcfg["depth"]
    fwd = depth * (2 * n * d * 3 * d + 4 * n * n * d + 2 * n * d * d + 2 * n * d * d + 2 * m * 768 * 2 * 768
                   + 4 * n * m * d + 2 * n * d * d + 2 * n * d * 8 * d + 2 * n * 4 * d * d)
    obj = {"workload": "stable_audio_open_1_0 DiT train step (v-objective MSE, cfg_dropout 0.1, fwd+bwd, fused_adamw_ema), bf16-mixed, pre-encoded latents "
                       "(1024 frames = 47.55 s), synthetic conditioning tensors, random init, no activation checkpointing; ONE GPU "
                       "(`bench.py --workload dit_train --gpus N` is the data-parallel form)",
           "unit": "samples/s", "dtype": "bf16", "model_tflop_per_sample_fwd_bwd": 3 * fwd / 1e12, "batches": {}}
    g = torch.Generator().manual_seed(0)
    for b in batches:
        prof = None
        try:
            lat = torch.randn(b, dcfg["io_channels"], tlat, generator=g).to(dev)
            cross = torch.randn(b, m, dcfg["cond_token_dim"], generator=g).to(dev)
            glob = torch.randn(b, dcfg["global_cond_dim"], generator=g).to(dev)
            for _ in range(warmup):
                stepper(lat, cross_attn_cond=cross, global_embed=glob)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            prof = AttnProfiler(O.get_ops())
            prof.enabled = True
            t0 = time.perf_counter()
            for _ in range(steps):
                out = stepper(lat, cross_attn_cond=cross, global_embed=glob)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            prof.enabled = False
            r = prof.roofline(PEAK_BF16_MFMA_TFLOPS)
            obj["batches"][str(b)] = {"samples_per_s": b / dt, "ms_per_step": 1e3 * dt, "steps": steps, "warmup": warmup,
                                      "achieved_model_tflops": 3 * fwd * b / dt / 1e12, "frac_of_bf16_peak": 3 * fwd * b / dt / 1e12 / PEAK_BF16_MFMA_TFLOPS,
                                      "peak_hbm_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "final_loss": float(out["loss"]),
                                      "roofline": {k: r[k] for k in ("backward", "achieved", "peak", "frac", "kernel", "launches", "avg_launch_ms",
                                                                     "cross_attention", "projections") if k in r}}
        except torch.cuda.OutOfMemoryError:
            obj["batches"][str(b)] = {"out_of_memory": True}
        finally:
            if prof is not None:
                prof.restore()
            lat = cross = glob = None
            torch.cuda.empty_cache()
    done = [(k, v) for k, v in obj["batches"].items() if "samples_per_s" in v]
    if done:
        best = max(done, key=lambda kv: kv[1]["samples_per_s"])
        obj["value"], obj["per_gpu_batch"], obj["ms_per_step"] = best[1]["samples_per_s"], int(best[0]), best[1]["ms_per_step"]
    del stepper, model
    torch.cuda.empty_cache()
    if with_cpu_baseline:
        obj["cpu_baseline"] = dit_train_cpu_baseline(dcfg, tlat, m)
    return obj


def apply_ops_set(args, ops=None):
    """--ops-set NAME=VALUE: attributes of the SatOps object for A/B runs (every workload; recorded in config.ops_set)."""
    if not args.ops_set:
        return
    if ops is None:
        from stable_audio_tools_amd import ops as O
        ops = O.get_ops()
    for kv in args.ops_set:
        name, val = kv.split("=", 1)
        if not hasattr(ops, name):
            raise SystemExit(f"--ops-set: SatOps has no attribute {name!r}")
        cur = getattr(type(ops), name)
        setattr(ops, name, (type(cur)(int(val)) if isinstance(cur, (bool, int)) else (bool(int(val)) if cur is None else val)))


def run_dit_sample(args):
    apply_ops_set(args)
    line = dit_sample_line(args.dit_dtype, args.batch, args.steps, args.warmup, not args.no_cpu_baseline)
    emit(line)


def dit_sample_line(dit_dtype, batch, steps, warmup, with_cpu_baseline):
    """BASELINE.json configs[2]: Stable-Audio-Open-1.0 DiT, text-conditioned, v-DDIM sampling with CFG
    (batch doubled inside the model, dit.py:324-410).  One 'step' = one sampler step = one DiT evaluation
    at batch 2*B plus the DDIM update."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from stable_audio_tools_amd import ops as O
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.sampling import sample_v_ddim
    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_open_dit.json")))
    dcfg = cfg["diffusion"]["config"]
    dtype = torch.bfloat16 if dit_dtype == "bf16" else torch.float32
    torch.manual_seed(1234)
    model = DiffusionTransformer(**dcfg)
    with torch.no_grad():   # de-zero the branch outputs the reference zero-initialises
        for n_, p in model.named_parameters():
            if n_.endswith("to_out.weight") or ".ff.ff.2." in n_ or "process_conv" in n_:
                p.normal_(0.0, 0.02)
    model = model.to(device=dev, dtype=dtype).train(False)
    ops = O.get_ops()
    prof = AttnProfiler(ops)
    b, tlat, m = batch, cfg["latent_length"], cfg["context_length"]
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(b, dcfg["io_channels"], tlat, generator=g).to(dev, dtype)
    cross = torch.randn(b, m, dcfg["cond_token_dim"], generator=g).to(dev, dtype)
    glob = torch.randn(b, dcfg["global_cond_dim"], generator=g).to(dev, dtype)
    kw = dict(cross_attn_cond=cross, global_embed=glob, cfg_scale=6.0, scale_phi=0.75)
    # (i) eager launches — every kernel issued from Python; the per-kernel HIP events of the roofline object are taken here
    sample_v_ddim(model, noise, max(warmup, 1), **kw)
    torch.cuda.synchronize()
    prof.enabled = True
    t0 = time.perf_counter()
    out = sample_v_ddim(model, noise, steps, **kw)
    torch.cuda.synchronize()
    elapsed_eager = time.perf_counter() - t0
    prof.enabled = False
    prof.restore()
    # (ii) the same loop with the denoiser evaluation + fused update replayed from ONE captured HIP graph per step
    # (sampling.GraphedDenoiser): identical kernels and arithmetic, no per-launch host cost.  Capture is outside the timed region
    # (a serving process captures once per shape); `value` is the faster of the two modes on this box, both are reported.
    from stable_audio_tools_amd.sampling import GraphedDenoiser
    import math
    with torch.no_grad():
        gd = GraphedDenoiser(model, noise, noise.new_ones([b]), **kw)
    tt = torch.linspace(1.0, 0, steps + 1)[:-1]
    al, sg = torch.cos(tt * math.pi / 2), torch.sin(tt * math.pi / 2)
    an, sn = torch.cat([al[1:], al.new_ones(1)]), torch.cat([sg[1:], sg.new_zeros(1)])
    zc = torch.zeros_like(al)
    table = torch.stack([an * al + sn * sg, -an * sg + sn * al, zc, zc, al, -sg, zc, zc], dim=1).float().to(dev)   # c0x c0v c0p c0u c1x c1v c1p c1u
    tsteps = (noise.new_ones([b])[:, None] * tt.to(dev)[None, :]).t().contiguous()

    @torch.no_grad()
    def graph_loop(nsteps):
        x = noise
        for i in range(nsteps):
            x, pred = gd(x, tsteps[i], fused_update=table[i])
        return pred.clone()
    graph_loop(max(warmup, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out_g = graph_loop(steps)
    torch.cuda.synchronize()
    elapsed_graph = time.perf_counter() - t0
    graph_matches = bool(torch.equal(out_g, out))
    elapsed = min(elapsed_eager, elapsed_graph)
    mode = "hip_graph" if elapsed_graph <= elapsed_eager else "eager"
    peak = PEAK_BF16_MFMA_TFLOPS if dit_dtype == "bf16" else PEAK_BF16_MFMA_TFLOPS / 3.0
    n = tlat + 1
    line = {
        "metric": "DiT sampling steps/sec", "value": steps / elapsed, "unit": "steps/s", "n_gpus": 1,
        "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": dit_dtype, "data": "synthetic",
        "config": {"workload": "stable_audio_open_1_0 DiT (d=1536, 24 layers, 24x64 heads, GQA cross-attn to 130x768 context), "
                               "v-DDIM loop (the arithmetic of inference/sampling.py:254-307 `sample`, eta 0; stable_audio_tools_amd.sampling.sample_v_ddim: "
                               "the per-step update of x rides in the native guidance kernel through the model's `fused_update=` extension) "
                               "with CFG scale 6 + rescale 0.75 (model batch 2B), random init",
                   "latent_frames": tlat, "tokens": n, "context": m, "per_gpu_batch": b, "finite": bool(torch.isfinite(out.float()).all()),
                   "launch_mode": mode, "steps_per_s": {"eager": steps / elapsed_eager, "hip_graph": steps / elapsed_graph},
                   "graph_output_equals_eager": graph_matches},
        "roofline": prof.roofline(peak),
    }
    if with_cpu_baseline:
        line["cpu_baseline"] = dit_cpu_baseline(dcfg, tlat, m)
        line["config"]["parity"] = dit_eval_parity(model, dcfg, noise, cross, glob, kw)
    del model
    torch.cuda.empty_cache()
    return line


def _capture_halves(module):
    """Shadow `module._forward` (the doubled-batch evaluation inside DiffusionTransformer.forward under CFG: dit.py:385-398 in the reference,
    the same method name in the native class) so that its raw output — [conditioned half; unconditioned half] — is kept."""
    box, orig = {}, module._forward

    def wrapped(*a, **k):
        out = orig(*a, **k)
        box["halves"] = (out[0] if isinstance(out, tuple) else out).detach().float().cpu()
        return out
    module._forward = wrapped
    return box, lambda: module.__dict__.pop("_forward", None)


def dit_eval_parity(model, dcfg, x, cross, glob, kw, bound=4e-2, ref_cache=None):
    """ONE guided evaluation (t = 0.5, CFG scale and rescale of the timed loop, model batch 2) of the TIMED native model — bf16 storage /
    fp8 projections as configured, full depth, full length — against the fp32 CPU path on the same weights widened to fp32: the
    reference's own DiffusionTransformer (models/dit.py:231-431) when a reference tree is importable, else the oracle port.  Compared
    tensors (relative L2 and max), all FINAL outputs of the full stack:
      plain   the conditioned half of the doubled batch  == the model output at cfg_scale 1   — bounded by `bound`
      uncond  the unconditioned half (null conditioning)                                      — bounded by `bound`
      guided_pre_rescale  u + s (c - u) (dit.py:402), the native combine kernel at scale_phi 0 — bounded by the triangle inequality on
              the two measured half errors: (s |dc| + (s - 1) |du|) / |g_ref| + one bf16 output rounding (2^-8): CFG at scale 6 multiplies the halves'
              rounding errors by up to 11, the bound says by how much at most for THIS evaluation
      guided  the output the sampler consumes (with the channel-std rescale, scale_phi) — reported; the rescale is a ratio of two
              statistics of the tensors above.
    Returns the parity object; `cpu_seconds` is the wall time of the ONE reference evaluation (batch 2) — long_context uses it as its
    un-scaled CPU baseline."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    xc, cc, gc = x.float().cpu(), cross.float().cpu(), glob.float().cpu()
    t = torch.full((x.shape[0],), 0.5)
    s_, phi = float(kw["cfg_scale"]), float(kw["scale_phi"])
    got = {}
    box, undo = _capture_halves(model)
    try:
        with torch.no_grad():
            tn = t.to(x.device, x.dtype)
            got["guided"] = model(x, tn, cross_attn_cond=kw["cross_attn_cond"], global_embed=kw["global_embed"], cfg_scale=s_, scale_phi=phi).float().cpu()
            got["plain"], got["uncond"] = box["halves"].chunk(2, dim=0)
            got["guided_pre_rescale"] = model(x, tn, cross_attn_cond=kw["cross_attn_cond"], global_embed=kw["global_embed"], cfg_scale=s_, scale_phi=0.0).float().cpu()
    finally:
        undo()
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    want = {}
    if ref_cache is not None and "want" in ref_cache:      # a second native configuration against the SAME reference evaluation
        want, kind, secs = ref_cache["want"], ref_cache["kind"], ref_cache["secs"]
    elif _reference_importable():
        ref = _ref_dit(dcfg)
        ref.load_state_dict(sd, strict=False)
        kind = "reference"
        rbox, rundo = _capture_halves(ref)
        t0 = time.perf_counter()
        with torch.no_grad():
            want["guided"] = ref(xc, t, cross_attn_cond=cc, global_embed=gc, cfg_scale=s_, scale_phi=phi)
        secs = time.perf_counter() - t0
        rundo()
        want["plain"], want["uncond"] = rbox["halves"].chunk(2, dim=0)
        del ref
    else:
        import dit_oracle
        kind = "port"
        t0 = time.perf_counter()
        with torch.no_grad():
            want["plain"] = dit_oracle.dit_forward(sd, dcfg, xc, t, cc, gc)
            want["uncond"] = dit_oracle.dit_forward(sd, dcfg, xc, t, torch.zeros_like(cc), gc)
        secs = time.perf_counter() - t0
        cu, uu = want["plain"], want["uncond"]
        g = uu + (cu - uu) * s_
        want["guided"] = phi * (g * (cu.std(dim=1, keepdim=True) / g.std(dim=1, keepdim=True))) + (1 - phi) * g if phi != 0.0 else g
    want["guided_pre_rescale"] = want["uncond"] + (want["plain"] - want["uncond"]) * s_        # dit.py:402 on the reference's own halves
    if ref_cache is not None:
        ref_cache.update(want=want, kind=kind, secs=secs)
    out = {}
    for name in ("plain", "uncond", "guided_pre_rescale", "guided"):
        d = got[name] - want[name]
        out[name] = {"rel_l2": float(f"{float(d.norm() / want[name].norm()):.3e}"), "rel_max": float(f"{float(d.abs().max() / want[name].abs().max()):.3e}")}
    dc, du = float((got["plain"] - want["plain"]).norm()), float((got["uncond"] - want["uncond"]).norm())
    gb = (s_ * dc + (s_ - 1.0) * du) / float(want["guided_pre_rescale"].norm()) + 2.0 ** -8
    out["plain"]["bound_rel_l2"] = out["uncond"]["bound_rel_l2"] = bound
    out["guided_pre_rescale"]["bound_rel_l2"] = float(f"{gb:.3e}")
    ok = out["plain"]["rel_l2"] < bound and out["uncond"]["rel_l2"] < bound and out["guided_pre_rescale"]["rel_l2"] <= gb
    out.update({"bound_rel_l2": bound, "bounded": ["plain", "uncond", "guided_pre_rescale"], "ok": bool(ok), "against": kind + " fp32 on CPU",
                "cpu_seconds": round(secs, 1), "cpu_threads": cores, "depth": dcfg["depth"], "tokens": int(x.shape[-1]) + 1,
                "what": f"FINAL output (B, {dcfg['io_channels']}, {int(x.shape[-1])}) of the timed depth-{dcfg['depth']} model at t = 0.5 vs fp32 on the same (16-bit-rounded) weights: "
                        f"conditioned half (= cfg_scale 1 output) and unconditioned half bounded by {bound:g}; guided output before the rescale (u + {s_:g} (c - u)) "
                        "bounded by the triangle inequality on the measured half errors; guided output after the channel-std rescale reported"})
    return out


PEAK_FP8_MFMA_TFLOPS = 5000.0   # MI355X_MICROARCH.md: dense fp8 (MX) MFMA peak
FP8_DEPTH24_BOUND = 0.2         # tests/test_long_context.py FP8_DEPTH24: derivation there
FP8_ATTN_DEPTH24_BOUND = 0.08   # tests/test_long_context.py FP8_ATTN_DEPTH24: fp8 on the attention projections only (policy "attn")


def long_context_line(steps=6, warmup=2, with_cpu_baseline=True):
    """BASELINE.json configs[4] on ONE GPU: the Stable-Audio-2.0-length DiT (sample_size 12582912 -> 6144 latent frames, N = 6145
    tokens; reference configs/model_configs/txt2audio/stable_audio_2_0.json:3, :79-86) sampled with CFG (model batch 2), every
    projection with >= 256 features in fp8 e4m3 on the MX MFMA (linear.set_fp8: dynamic scales — weights per output channel (round 6), activations per row: sat_quant_fp8_rows per GEMM
    input), attention in bf16 with fp32 softmax.  Reports sampler steps/s (eager and HIP-graph), the self-attention kernel against the
    2.5 PF bf16 peak, the fp8 projections against the 5 PF fp8 peak (with the quantisation passes' time beside them), and a CPU
    baseline = ONE un-scaled evaluation of the reference's fp32 model at this configuration, which is also the parity partner of the
    timed model's final output."""
    dev = torch.device("cuda", 0)
    from stable_audio_tools_amd import ops as O
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.linear import set_fp8
    from stable_audio_tools_amd.sampling import GraphedDenoiser, sample_v_ddim
    import math
    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_open_dit.json")))
    dcfg = cfg["diffusion"]["config"]
    tlat, m, b = 6144, cfg["context_length"], 1
    torch.manual_seed(1234)
    model = DiffusionTransformer(**dcfg)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("to_out.weight") or ".ff.ff.2." in n_ or "process_conv" in n_:
                p_.normal_(0.0, 0.02)
    model = model.to(device=dev, dtype=torch.bfloat16).train(False)
    nfp8 = set_fp8(model, True)
    ops = O.get_ops()
    prof = AttnProfiler(ops, max_launches=96)
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(b, dcfg["io_channels"], tlat, generator=g).to(dev, torch.bfloat16)
    cross = torch.randn(b, m, dcfg["cond_token_dim"], generator=g).to(dev, torch.bfloat16)
    glob = torch.randn(b, dcfg["global_cond_dim"], generator=g).to(dev, torch.bfloat16)
    kw = dict(cross_attn_cond=cross, global_embed=glob, cfg_scale=6.0, scale_phi=0.75)
    sample_v_ddim(model, noise, warmup, **kw)
    torch.cuda.synchronize()
    prof.enabled = True
    t0 = time.perf_counter()
    out = sample_v_ddim(model, noise, steps, **kw)
    torch.cuda.synchronize()
    el_eager = time.perf_counter() - t0
    prof.enabled = False
    prof.restore()
    peak_mem = torch.cuda.max_memory_allocated() / 2 ** 30
    with torch.no_grad():
        gd = GraphedDenoiser(model, noise, noise.new_ones([b]), **kw)
    tt = torch.linspace(1.0, 0, steps + 1)[:-1]
    al, sg = torch.cos(tt * math.pi / 2), torch.sin(tt * math.pi / 2)
    an, sn = torch.cat([al[1:], al.new_ones(1)]), torch.cat([sg[1:], sg.new_zeros(1)])
    zc = torch.zeros_like(al)
    table = torch.stack([an * al + sn * sg, -an * sg + sn * al, zc, zc, al, -sg, zc, zc], dim=1).float().to(dev)   # c0x c0v c0p c0u c1x c1v c1p c1u
    tsteps = (noise.new_ones([b])[:, None] * tt.to(dev)[None, :]).t().contiguous()

    @torch.no_grad()
    def graph_loop(ns):
        x = noise
        for i in range(ns):
            x, pred = gd(x, tsteps[i], fused_update=table[i])
        return pred
    graph_loop(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graph_loop(steps)
    torch.cuda.synchronize()
    el_graph = time.perf_counter() - t0
    elapsed = min(el_eager, el_graph)
    n = tlat + 1
    d, depth = dcfg["embed_dim"], dcfg["depth"]
    fwd = depth * (2 * n * d * 3 * d + 4 * n * n * d + 2 * n * d * d + 2 * n * d * d + 2 * m * 768 * 2 * 768
                   + 4 * n * m * d + 2 * n * d * d + 2 * n * d * 8 * d + 2 * n * 4 * d * d)
    nl, ms, fl = prof.summary("self")
    attn_tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    line = {"workload": "stable_audio_2_0-length DiT sampling step (d=1536, 24 layers, N=6145 tokens = 285 s of audio, context 130), CFG scale 6 "
                        "(model batch 2), fp8 e4m3 projections (MX MFMA; dynamic scales: weights per output channel, activations per token row in one pass), bf16 attention, random init; ONE GPU "
                        "(BASELINE.json configs[4] names 8: sampling is replicas-only, no collective)",
            "value": steps / elapsed, "unit": "steps/s", "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps,
            "steps_per_s": {"eager": steps / el_eager, "hip_graph": steps / el_graph}, "fp8_linears": nfp8,
            "finite": bool(torch.isfinite(out.float()).all()), "peak_hbm_gib": round(peak_mem, 2),
            "model_tflop_per_step": 2 * fwd / 1e12, "achieved_model_tflops": 2 * fwd * steps / elapsed / 1e12,
            "attention": {"kernel": "sat_attn_fwd_kernel", "launches": nl, "avg_launch_ms": ms / nl if nl else None, "achieved": round(attn_tf, 1),
                          "peak": PEAK_BF16_MFMA_TFLOPS, "frac": round(attn_tf / PEAK_BF16_MFMA_TFLOPS, 4)},
            "fp8_projections": prof.gemm_summary(PEAK_FP8_MFMA_TFLOPS, fp8=True),
            "bf16_projections": prof.gemm_summary(PEAK_BF16_MFMA_TFLOPS)}
    del gd
    if with_cpu_baseline:
        # ONE un-scaled evaluation of the reference's fp32 DiffusionTransformer at the timed configuration (depth 24, N = 6145, CFG batch 2) on
        # the host cores: it is both the parity partner of the timed fp8 model's FINAL output and the CPU baseline (no extrapolation).
        # bound: tests/test_long_context.py FP8_DEPTH24 (derived there)
        rc = {}
        par = dit_eval_parity(model, dcfg, noise, cross, glob, kw, bound=FP8_DEPTH24_BOUND, ref_cache=rc)
        # trajectory level (round 6): 10 v-DDIM steps from the timed noise, final latents of the fp8 model and of a bf16 copy against the
        # float32 trajectory of the same weights on the native fp32 path (bounds: tests/test_long_context.py FP8_TRAJECTORY / FP8_OVER_BF16)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from golden_util import dit_trajectory_distances
        tr = dit_trajectory_distances(model, dcfg, noise, kw, steps=10)
        par["trajectory"] = {"steps": 10, "sampler": "v-DDIM, eta 0, CFG 6, rescale 0.75", "fp8_vs_fp32_rel_l2": float(f"{tr['lowp']:.3e}"),
                             "bf16_vs_fp32_rel_l2": float(f"{tr['bf16']:.3e}"), "fp8_over_bf16": round(tr["lowp"] / max(tr["bf16"], 1e-30), 2),
                             "bound_rel_l2": 0.5, "bound_fp8_over_bf16": 8.0, "ok": bool(tr["finite"] and tr["lowp"] < 0.5 and tr["lowp"] < 8.0 * tr["bf16"]),
                             "against": "native fp32 path (bf16x3 products; 3e-6 from the reference's fp32 DiffusionTransformer at depth 24: tests/test_full_width.py)",
                             "what": "final latents after 10 sampler steps from the timed noise, relative L2 to the float32 trajectory of the same weights; "
                                     "bounds stated in tests/test_long_context.py before the first measurement (coherent accumulation of the per-evaluation "
                                     "guided error over ten steps of sin(pi/20); fp8 no more than 8 x bf16's distance)"}
        # the accuracy-first policy (round 6): fp8 on the attention projections only, the feed-forward pair in bf16 — timed the same way, held
        # to the same reference evaluation; bound 0.08 (the round-5 verdict's criterion for the plain output; the ablation that picked
        # the policy measured 0.043 against the native fp32 path: profiles/r06_experiments/fp8_policy/)
        set_fp8(model, True, policy="attn")
        sample_v_ddim(model, noise, 1, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample_v_ddim(model, noise, steps, **kw)
        torch.cuda.synchronize()
        el_af = time.perf_counter() - t0
        par_af = dit_eval_parity(model, dcfg, noise, cross, glob, kw, bound=FP8_ATTN_DEPTH24_BOUND, ref_cache=rc)
        tr_af = dit_trajectory_distances(model, dcfg, noise, kw, steps=10, variants=())
        line["accuracy_first"] = {"policy": "linear.set_fp8(model, True, policy='attn'): fp8 e4m3 on to_qkv / to_out / to_q / to_kv (39 % of a layer's projection "
                                            "flops), the feed-forward pair in bf16 — the feed-forward input projection (SwiGLU) carries most of the fp8 distance",
                                  "steps_per_s_eager": steps / el_af, "ms_per_step": 1e3 * el_af / steps,
                                  "parity": {k: par_af[k] for k in ("plain", "uncond", "guided_pre_rescale", "guided", "bound_rel_l2", "ok")},
                                  "trajectory_fp8_vs_fp32_rel_l2": float(f"{tr_af['lowp']:.3e}")}
        set_fp8(model, True)
        line["parity"] = par
        line["cpu_baseline"] = {"value": 1.0 / par["cpu_seconds"], "unit": "steps/s", "cores": par["cpu_threads"],
                                "kind": "reference" if par["against"].startswith("reference") else "port", "scaled": False,
                                "sample": f"ONE sampler step's model evaluation, un-scaled: the {par['against'].split()[0]}'s fp32 DiffusionTransformer at depth {depth}, N={n}, CFG batch 2 "
                                          f"(the parity partner above), single evaluation without warm-up = {par['cpu_seconds']:.1f} s at {par['cpu_threads']} threads"
                                          + ("" if par["against"].startswith("reference") else " (no reference tree: two batch-1 evaluations of the oracle port)")}
    del model
    torch.cuda.empty_cache()
    return line


class ConvProfiler:
    """Times every launch of the conv-family kernels with HIP events on the launch stream (torch's current stream ==
    the stream handed to the C-ABI) and tallies their ALGORITHMIC flops (2 * Cin * Cout * K * Tout * B per launch;
    wgrad: 2 * M * N * K * T * B — DESIGN.md §4).  Each C-ABI entry point issues exactly one launch of its kernel."""

    # entry point -> (kernel name (or args -> name), peak TFLOP/s, flops(args))
    #   fp32 kernels: peak = fp32 MFMA dense (157.3); bf16x3 kernels: peak = dense bf16 MFMA / 3 (three MFMAs per product)
    X3 = 2500.0 / 3
    SPECS = {
        "sat_conv1d": ("sat_conv1d_kernel", PEAK_F32_MFMA_TFLOPS, lambda a: 2.0 * a[12] * a[13] * a[14] * a[17] * a[16]),
        "sat_conv1d_bf16x3": (lambda a: "sat_conv1d_bf16x3_k7_kernel" if (a[18] >= 5 and a[19] == 1) else "sat_conv1d_bf16x3_kernel",
                              X3, lambda a: 2.0 * a[13] * a[14] * a[15] * a[18] * a[17]),
        "sat_conv1d_k7_planes": ("sat_k7_planes_kernel", X3, lambda a: 0.0),     # the planes kernel's pre-pass: time, no flops of its own
        "sat_conv1d_bf16x3_planesq": ("sat_conv1d_bf16x3_k7q_kernel", X3, lambda a: 2.0 * a[13] * a[14] * a[15] * a[18] * a[17]),
        # the fused backward of a unit's 1x1 conv (csrc/ru_k1_bwd.hip): data gradient + weight gradient = 4 * C * C * T * B flop, HBM-bound
        "sat_ru_k1_bwd": ("sat_ru_k1_bwd_kernel", X3, lambda a: 4.0 * a[13] * a[13] * a[14] * a[12]),
        # the fused ResidualUnit forward (C <= 128): conv7 + conv1 in one launch of the k7q kernel
        "sat_residual_unit_fwd": ("sat_conv1d_bf16x3_k7q_kernel", X3, lambda a: 2.0 * a[14] * a[15] * a[15] * (a[17] + 1) * a[16]),
        # the k1 / strided convs that also write their consumer's activation planes (generic kernel, plane emission)
        "sat_conv1d_bf16x3_emit": ("sat_conv1d_bf16x3_kernel", X3, lambda a: 2.0 * a[13] * a[14] * a[15] * a[18] * a[17]),
        "sat_convtr1d_bf16x3": ("sat_conv1d_bf16x3_kernel", X3, lambda a: 2.0 * a[13] * a[14] * a[15] * a[18] * a[16]),
        "sat_convtr1d": ("sat_convtr1d_kernel", PEAK_F32_MFMA_TFLOPS, lambda a: 2.0 * a[12] * a[13] * a[14] * 2 * a[16]),
        "sat_conv_wgrad": ("sat_conv_wgrad_kernel", PEAK_F32_MFMA_TFLOPS, lambda a: 2.0 * a[9] * a[10] * a[11] * a[14] * a[12]),
        # N >= 64 input channels and T % 4 == 0 -> the 8-wave pipelined kernel (conv_wgrad_bf16x3.hip sat_wgrad7 plan)
        "sat_conv_wgrad7_bf16x3": (lambda a: "sat_wgrad7_bf16x3_pipe_kernel" if (a[10] >= 64 and a[11] % 4 == 0) else "sat_wgrad7_bf16x3_kernel",
                                   X3, lambda a: 2.0 * a[8] * a[9] * a[10] * 7 * a[11]),
        "sat_conv_wgrad_bf16x3": ("sat_wgrad_small_bf16x3_kernel", X3, lambda a: 2.0 * a[9] * a[10] * a[11] * a[14] * a[12]),
        # the discriminator's Conv2d layers (csrc/disc_conv.hip): 2 * B * Cin * Cout * kh * kw * frames * W per launch (forward and
        # data-gradient: the same kernel), the same count for the weight-gradient
        "sat_disc_conv": ("sat_disc_conv_kernel", X3, lambda a: 2.0 * a[7] * a[8] * a[9] * a[12] * a[13] * a[10] * a[11]),
        "sat_disc_wgrad": ("sat_disc_wgrad_kernel", X3, lambda a: 2.0 * a[3] * a[4] * a[5] * a[8] * a[9] * a[6] * a[7]),
        "sat_disc_planes": ("sat_disc_planes_kernel", X3, lambda a: 0.0),
    }

    def __init__(self, ops):
        self.records = {}            # kernel name -> [(start, end, flops)]
        self.peaks = {}
        self.enabled = False
        for name, (kern, peak, flops) in self.SPECS.items():
            self._wrap(ops.lib, name, kern, peak, flops)

    def _wrap(self, lib, name, kern, peak, flops):
        orig = getattr(lib, name)

        def timed(*a):
            if not self.enabled:
                return orig(*a)
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = orig(*a)
            e.record()
            k = kern(a) if callable(kern) else kern
            self.peaks[k] = peak
            self.records.setdefault(k, []).append((s, e, flops(a)))
            return rc

        setattr(lib, name, timed)

    def summary(self):
        """Per kernel: launches, total ms, total flops; returns (dominant kernel dict, all dicts)."""
        torch.cuda.synchronize()
        out = []
        for kern, recs in self.records.items():
            if not recs:
                continue
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            fl = sum(f for _, _, f in recs)
            peak = self.peaks[kern]
            ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            out.append({"kernel": kern, "launches": len(recs), "total_ms": ms, "avg_launch_ms": ms / len(recs),
                        "achieved": ach, "peak": peak, "frac": ach / peak})
        out.sort(key=lambda d: -d["total_ms"])
        return (out[0] if out else None), out


def k7_family(allk):
    """The k = 7 convs of the ResidualUnits run on two kernels since round 2 (direct staging below C = 256, pre-split planes above):
    their combined algorithmic flops / combined HIP-event time (the planes pre-pass included), for continuity with the single-kernel
    figure of round 1."""
    fam = [d for d in allk if d["kernel"].startswith("sat_conv1d_bf16x3_k7") or d["kernel"] == "sat_k7_planes_kernel"]     # k7, k7p, k7q + pre-pass
    if not fam:
        return None
    ms = sum(d["total_ms"] for d in fam)
    fl = sum(d["achieved"] * d["total_ms"] for d in fam)        # TFLOP/s * ms
    ach = fl / ms if ms > 0 else 0.0
    return {"kernels": [d["kernel"] for d in fam], "launches": sum(d["launches"] for d in fam), "total_ms": round(ms, 3),
            "achieved": round(ach, 2), "peak": fam[0]["peak"], "frac": round(ach / fam[0]["peak"], 4)}


def pmc_traffic(kernel, args):
    """HBM bytes per launch of `kernel` from the committed PMC profile of the DEFAULT workload (rocprofv3 cannot collect
    counters from inside this process: tools/collect_profiles.sh runs the separate --pmc passes on this same command)."""
    if args.sample_size != 2097152 or args.batch != 1:
        return None
    try:
        for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01g_pmc_traffic.json"):        # the newest committed profile that has this kernel
            path = os.path.join(ROOT, "profiles", name)
            if os.path.exists(path):
                doc = json.load(open(path))
                if kernel in doc["kernels"]:
                    return doc["kernels"][kernel]["hbm_bytes_per_launch"]
        return None
    except (OSError, KeyError, ValueError):
        return None


def pmc_mfma(kernel, args, profile="vae"):
    """MFMA utilisation of `kernel` from the committed SQ-counter pass of this same command (profiles/r06_pmc_mfma_<profile>.json,
    tools/collect_profiles.sh + tools/pmc_mfma_busy.py): SQ_VALU_MFMA_BUSY_CYCLES / (4 x SQ_BUSY_CU_CYCLES) summed over every dispatch of
    the kernel, with VALU instructions per MFMA and the issue-stall fraction of wave cycles — the north-star's "rocprof-reported MFMA
    utilisation" next to the roofline fraction.  Instances of one template (the dilations of the weight gradient ...) are pooled."""
    if profile == "vae" and (args.sample_size != 2097152 or args.batch != 1):
        return None
    path = os.path.join(ROOT, "profiles", f"r06_pmc_mfma_{profile}.json")
    try:
        doc = json.load(open(path))
        rows = [v for k, v in doc["kernels"].items() if k.split("<")[0].split("(")[0] == kernel]
        cu = sum(r["busy_cu_cycles"] for r in rows)
        if not rows or cu <= 0:
            return None
        out = {"mfma_busy": round(sum(r["mfma_busy"] * r["busy_cu_cycles"] for r in rows) / cu, 4), "dispatches": sum(r["dispatches"] for r in rows),
               "source": os.path.basename(path)}
        if all("valu_per_mfma" in r for r in rows):
            out["valu_per_mfma"] = round(sum(r["valu_per_mfma"] * r["busy_cu_cycles"] for r in rows) / cu, 2)
        if all("wait_inst_frac" in r for r in rows):
            out["wait_inst_frac"] = round(sum(r["wait_inst_frac"] * r["busy_cu_cycles"] for r in rows) / cu, 3)
        return out
    except (OSError, KeyError, ValueError):
        return None


def hbm_roofline(args, ms_per_step):
    """The north-star's HBM view of the whole step (BASELINE.json: >= 60 % of the HBM roofline on the conv stack): HBM bytes per step
    summed over every kernel of the committed rocprofv3 --pmc passes of this same command (profiles/r05_pmc_traffic.json, else the previous round's: 2 x
    FETCH_SIZE + WRITE_SIZE per launch, gfx950 correction; the passes profile `--steps 1 --warmup 1` = 2 steps) against the
    algorithmic bytes of SURVEY.md 8(d)'s fusion-unit convention (16.4 GB per direction per sample forward; x3 for forward +
    backward) and the 8 TB/s peak, at this run's step time."""
    if args.sample_size != 2097152 or args.batch != 1:
        return None
    path = None
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json"):      # the newest committed profile
        if os.path.exists(os.path.join(ROOT, "profiles", name)):
            path = os.path.join(ROOT, "profiles", name)
            break
    if path is None:
        return None
    try:
        doc = json.load(open(path))
        steps = float(doc.get("steps_profiled", 2))
        counter = sum(v["hbm_bytes_per_launch"] * v.get("launches", 0) for v in doc["kernels"].values()) / steps
    except (OSError, KeyError, ValueError):
        return None
    algorithmic = 3 * 2 * 16.4e9
    t = ms_per_step * 1e-3
    return {"counter_bytes_per_step": counter, "algorithmic_bytes_per_step": algorithmic, "peak_bytes_per_s": 8.0e12,
            "counter_rate_frac_of_8TBs": counter / t / 8.0e12, "frac_of_8TBs": algorithmic / t / 8.0e12,
            "traffic_over_algorithmic": counter / algorithmic,
            "source": os.path.basename(path),
            "note": "counter bytes: every sat_* kernel of the committed --pmc passes (`source`); algorithmic: 3 x (16.4 + 16.4) GB "
                    "(fusion-unit convention, forward + backward); frac_of_8TBs = algorithmic bytes / this run's step time / 8 TB/s — the "
                    "step is matrix-pipe-bound (roofline.bound), this is the north-star's second view of it"}


def _reference_importable():
    """/root/reference in the build container; on the GPU box the tree oracle/stage_ref.py staged into oracle/_ref/ (git-ignored,
    shipped with the working tree)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refimport
    return refimport.available()


def _median_time(fn, reps=3):
    fn()                                   # warm-up (allocator, thread pool, code paths)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


class _PeakRSS:
    """Peak resident set of this process while a CPU step runs (20 ms sampling thread): sizes the un-scaled baseline step so that
    it cannot drive the box out of host memory."""

    def __enter__(self):
        import threading
        import psutil
        self._proc = psutil.Process()
        self.base = self.peak = self._proc.memory_info().rss
        self._stop = threading.Event()

        def watch():
            while not self._stop.wait(0.02):
                self.peak = max(self.peak, self._proc.memory_info().rss)
        self._thr = threading.Thread(target=watch, daemon=True)
        self._thr.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thr.join()
        self.peak = max(self.peak, self._proc.memory_info().rss)

    @property
    def delta(self):
        return max(self.peak - self.base, 0)


def cpu_baseline(cfg, probe_samples, budget_s=100.0, full_samples=SAMPLE_SIZE):
    """CPU baseline of the SAME workload on this box's host cores: ONE generator step (forward + autograd backward
    + torch AdamW) of the REFERENCE's own modules (stable_audio_tools.models.autoencoders + training/losses/auraloss.py, staged
    for the GPU box by oracle/stage_ref.py; kind "reference") — or of the oracle restatement (kind "port") if no reference tree is
    importable.  Protocol: (1) probe on a `probe_samples` crop — 1 warm-up + 1 timed step at 8 / 16 / 32 threads, peak RSS sampled —
    picks the thread count and predicts time and memory (the model is fully convolutional: both are linear in length);
    (2) ONE timed step at the LARGEST of {1, 1/2, 1/4, 1/8, ...} x the full 2 097 152-sample item whose prediction fits `budget_s`
    seconds and half of the free host memory — un-scaled when that is the full item, which is what a default run does on the GPU
    box; `sample` says what ran."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import psutil
    import stft_oracle
    import vae_oracle
    sc = cfg["training"]["loss_configs"]["spectral"]["config"]
    lat, ratio = cfg["model"]["latent_dim"], cfg["model"]["downsampling_ratio"]

    def make_inputs(n):
        g = torch.Generator().manual_seed(0)
        return 0.1 * torch.randn(1, 2, n, generator=g), torch.randn(1, lat, n // ratio, generator=g)

    kind = "port"
    if _reference_importable():
        import contextlib
        import refimport
        with contextlib.redirect_stdout(sys.stderr):       # the reference prints its optional-import notices to stdout
            refimport.import_reference()
            al = refimport.import_auraloss()
        from stable_audio_tools.models.autoencoders import create_autoencoder_from_config as ref_create
        torch.manual_seed(1234)
        model = ref_create(cfg).float().train(True)
        opt = torch.optim.AdamW(model.parameters(), lr=1.5e-4, betas=(0.8, 0.99), weight_decay=1e-3)
        sd_loss = al.SumAndDifferenceSTFTLoss(sample_rate=cfg["sample_rate"], **sc)
        lr_loss = al.MultiResolutionSTFTLoss(sample_rate=cfg["sample_rate"], **sc)
        kind = "reference"

        def step(audio, noise):
            # AutoencoderTrainingWrapper.training_step, generator branch (training/autoencoders.py:398-515), on the reference's modules
            opt.zero_grad(set_to_none=True)
            pre = model.encoder(audio)
            mean, scale = pre.chunk(2, dim=1)
            stdev = torch.nn.functional.softplus(scale) + 1e-4
            z = noise * stdev + mean
            kl = (mean * mean + stdev * stdev - torch.log(stdev * stdev) - 1).sum(1).mean()
            dec = model.decode(z)
            loss = sd_loss(audio, dec) + 0.5 * lr_loss(audio[:, 0:1], dec[:, 0:1]) + 0.5 * lr_loss(audio[:, 1:2], dec[:, 1:2]) + 1e-4 * kl
            loss.backward()
            opt.step()
    else:
        from stable_audio_tools_amd.autoencoders import create_autoencoder_from_config
        torch.manual_seed(1234)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in create_autoencoder_from_config(cfg).state_dict().items()}
        opt = torch.optim.AdamW(list(sd.values()), lr=1.5e-4, betas=(0.8, 0.99), weight_decay=1e-3)

        def step(audio, noise):
            opt.zero_grad(set_to_none=True)
            z, kl, _ = vae_oracle.autoencoder_encode(sd, cfg["model"], audio, noise)
            dec = vae_oracle.autoencoder_decode(sd, cfg["model"], z)
            loss = stft_oracle.autoencoder_spectral_loss(audio, dec, sc, cfg["sample_rate"]) + 1e-4 * kl
            loss.backward()
            opt.step()
    # (1) probe.  torch's CPU conv path degrades when oversubscribed (256 hardware threads on the GPU box's host took 700 s for what 8
    # do in ~25 s): try a few pool sizes, keep the fastest, report the threads actually used
    ncpu = os.cpu_count() or 1
    pa, pn = make_inputs(probe_samples)
    probes = {}
    for cores in sorted({min(ncpu, c) for c in (8, 16, 32)}):
        torch.set_num_threads(cores)
        step(pa, pn)
        with _PeakRSS() as rss:
            t0 = time.perf_counter()
            step(pa, pn)
            probes[cores] = (time.perf_counter() - t0, rss.delta)
    cores = min(probes, key=lambda c: probes[c][0])
    torch.set_num_threads(cores)
    dt_probe, rss_probe = probes[cores]
    rss_probe = max(rss_probe, 64 << 20)
    free = psutil.virtual_memory().available
    # (2) the largest fraction of the full item that fits the time and memory budget
    n = full_samples
    while n > probe_samples and (dt_probe * n / probe_samples > budget_s or 1.5 * rss_probe * n / probe_samples > 0.5 * free):
        n //= 2
    if n <= probe_samples:
        n, dt, peak = probe_samples, dt_probe, rss_probe
    else:
        fa, fn = make_inputs(n)
        with _PeakRSS() as rss:
            t0 = time.perf_counter()
            step(fa, fn)
            dt = time.perf_counter() - t0
        peak = rss.delta
        del fa, fn
    scale = full_samples / n
    what = (f"ONE generator step (fwd + autograd bwd + AdamW) of the {'reference modules' if kind == 'reference' else 'oracle port'} on "
            f"{'the full ' if n == full_samples else 'a '}{n}-sample stereo item: {dt:.1f} s at {cores} threads, peak host memory +{peak / 2 ** 30:.1f} GiB"
            + ("" if n == full_samples else f", scaled x{scale:.0f} to {full_samples} samples (time / memory budget: {budget_s:.0f} s, "
                                             f"{free / 2 ** 30:.0f} GiB free)")
            + f"; thread count from a {probe_samples}-sample probe ("
            + ", ".join(f"{c}: {v[0]:.2f} s" for c, v in probes.items()) + ")")
    return {"value": 1.0 / (dt * scale), "unit": "samples/s", "cores": cores, "kind": kind, "sample": what,
            "sample_samples": n, "seconds": dt, "scaled": n != full_samples}


def headline_parity(model, cfg, stepper, audio, with_gradients=True):
    """Parity ON the bench item, outside the timed region: the native forward of the first full-length item of the timed
    batches (encode with an explicit VAE draw -> decode -> MR-STFT generator loss), with the weights as the timed steps left them,
    against the CPU oracle (oracle/vae_oracle.py, oracle/stft_oracle.py — the restatement pinned to the reference by
    tests/test_full_width.py) run on this box's host cores.  rel err = max|a-b| / max|b| (the 1e-3 bar of BASELINE.json).
    Round 6 — `gradients`: the same oracle pass keeps its autograd graph and differentiates a linear functional of the decoded audio
    (seeded projection, + 0.1 KL): EVERY parameter gradient of the conv stack at T = 2 097 152 against the native backward (data
    gradients, split-K weight gradients, weight-norm / SnakeBeta / bias sums) — well conditioned, unlike the composite MR-STFT
    gradient (tests/test_full_width.py), whose two chain-rule factors are held separately by the tests."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import stft_oracle
    import vae_oracle

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    mc = cfg["model"]
    x = audio[:1]
    g = torch.Generator().manual_seed(4321)
    noise = torch.randn(1, mc["latent_dim"], x.shape[-1] // mc["downsampling_ratio"], generator=g)
    proj = torch.randn(x.shape, generator=g)
    with torch.no_grad():
        z, info = model.encode(x, return_info=True, noise=noise.to(x.device))
        dec = model.decode(z)
        loss = stepper.spectral(x, dec)
    grads_native = None
    if with_gradients:
        zg, infog = model.encode(x, return_info=True, noise=noise.to(x.device))
        decg = model.decode(zg)
        pr = proj.to(x.device)
        loss_lin = (decg * pr).sum() / pr.numel() ** 0.5 + 0.1 * infog["kl"]
        names = [n for n, _ in model.named_parameters()]
        grads_native = {n: t.detach().cpu() for n, t in zip(names, torch.autograd.grad(loss_lin, list(model.parameters())))}
        loss_lin_native = float(loss_lin)
        del zg, infog, decg, pr, loss_lin
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cores = min(os.cpu_count() or 1, 48 if with_gradients else 16)      # (not a timed baseline: the autograd pass over 2 M samples scales past 16 threads)
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    grad_obj = "skipped (--no-parity-gradients)"
    if with_gradients:
        sdg = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
        z_o, kl_o, pre_o = vae_oracle.autoencoder_encode(sdg, mc, x.cpu(), noise)
        dec_o = vae_oracle.autoencoder_decode(sdg, mc, z_o)
        lin_o = (dec_o * proj).sum() / proj.numel() ** 0.5 + 0.1 * kl_o
        want = [n for n in grads_native if n in sdg]
        g_o = dict(zip(want, torch.autograd.grad(lin_o, [sdg[n] for n in want])))
        z_o, kl_o, pre_o, dec_o = z_o.detach(), kl_o.detach(), pre_o.detach(), dec_o.detach()
        errs = {n: rel(grads_native[n], g_o[n]) for n in want}
        l2 = {n: float((grads_native[n].double() - g_o[n].double()).norm() / g_o[n].double().norm().clamp_min(1e-30)) for n in want}
        wn = max(errs, key=errs.get)
        grad_obj = {"worst": float(f"{errs[wn]:.3e}"), "worst_parameter": wn, "worst_l2": float(f"{max(l2.values()):.3e}"), "parameters": len(want),
                    "parameters_over_tolerance": int(sum(e >= 1e-3 for e in errs.values())), "tolerance": 1e-3,
                    "ok": bool(len(want) == len(grads_native) and max(errs.values()) < 1e-3),
                    "functional_rel_err": abs(loss_lin_native - float(lin_o)) / max(abs(float(lin_o)), 1.0),
                    "what": "every parameter gradient of L = <decoded, P> / sqrt(|P|) + 0.1 KL (P seeded normal) at the full 2 097 152-sample item: native "
                            "backward vs the oracle's autograd on this box; max|a-b|/max|b| per parameter, worst reported (worst_l2: relative L2)"}
        del sdg, g_o, lin_o
    else:
        with torch.no_grad():
            z_o, kl_o, pre_o = vae_oracle.autoencoder_encode(sd, mc, x.cpu(), noise)
            dec_o = vae_oracle.autoencoder_decode(sd, mc, z_o)
    with torch.no_grad():
        loss_o = stft_oracle.autoencoder_spectral_loss(x.cpu(), dec_o, cfg["training"]["loss_configs"]["spectral"]["config"], cfg["sample_rate"],
                                                       weight=cfg["training"]["loss_configs"]["spectral"]["weights"]["mrstft"])
    secs = time.perf_counter() - t0
    out = {"pre_latents": rel(info["pre_bottleneck_latents"], pre_o), "z": rel(z, z_o), "kl": rel(info["kl"], kl_o), "decoded": rel(dec, dec_o),
           "mrstft_loss": abs(float(loss) - float(loss_o)) / abs(float(loss_o))}
    ok = max(out.values()) < 1e-3 and (not isinstance(grad_obj, dict) or grad_obj["ok"])
    return {"rel_err": {k: float(f"{v:.3e}") for k, v in out.items()}, "tolerance": 1e-3, "ok": bool(ok),
            "samples": int(x.shape[-1]), "batch_item": 0, "oracle_seconds": round(secs, 1), "oracle_threads": cores,
            "what": "native forward (encode, VAE sample with a given draw, decode, MR-STFT generator loss) of the bench item itself vs the CPU "
                    "oracle (fp32) on this box, weights as left by the timed steps; max|a-b|/max|b|; outside the timed region "
                    "(tests/test_headline_parity.py holds the same comparisons plus dL/d(decoded) of the MR-STFT loss and the B = 2 offsets)",
            "gradients": grad_obj}


def run_dit_train(args):
    """BASELINE.json configs[2]/[3]: Stable-Audio-Open-1.0 DiT training step (v-objective MSE on 1024 latent frames =
    47.55 s of audio, pre-encoded latents), bf16-mixed, data-parallel over RCCL.  samples/s = items/s."""
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(local_rank)
    if world > 1 or args.ddp_single_rank:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group("nccl", rank=rank, world_size=world)
    dev = torch.device("cuda", local_rank)
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.training import DiTTrainStep
    apply_ops_set(args)
    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_open_dit.json")))
    dcfg = cfg["diffusion"]["config"]
    torch.manual_seed(1234)
    model = DiffusionTransformer(**dcfg)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("to_out.weight") or ".ff.ff.2." in n_ or "process_conv" in n_:
                p.normal_(0.0, 0.02)
    model = model.to(dev).train(True)
    mixed = args.dit_dtype == "bf16"
    stepper = DiTTrainStep(model, lr=5e-5, cfg_dropout_prob=0.1, autocast_dtype=torch.bfloat16 if mixed else None,
                           ddp_single_rank=True if args.ddp_single_rank else None, ddp_mode=args.ddp_mode,
                           ddp_comm_dtype=torch.bfloat16 if args.ddp_comm_dtype == "bf16" else None)
    stepper.comm.timing = stepper.comm.active
    from stable_audio_tools_amd import ops as O
    prof = AttnProfiler(O.get_ops())
    b, tlat, m = args.batch, cfg["latent_length"], cfg["context_length"]
    g = torch.Generator().manual_seed(rank)
    lat = torch.randn(b, dcfg["io_channels"], tlat, generator=g).to(dev)
    cross = torch.randn(b, m, dcfg["cond_token_dim"], generator=g).to(dev)
    glob = torch.randn(b, dcfg["global_cond_dim"], generator=g).to(dev)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        stepper(lat, cross_attn_cond=cross, global_embed=glob)
    sync()
    prof.enabled = True
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = stepper(lat, cross_attn_cond=cross, global_embed=glob)
    sync()
    elapsed = time.perf_counter() - t0
    prof.enabled = False
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if dist.is_initialized():
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)
    if rank == 0:
        n = tlat + 1
        d, depth, mm = dcfg["embed_dim"], dcfg["depth"], m
        fwd = depth * (2 * n * d * 3 * d + 4 * n * n * d + 2 * n * d * d + 2 * n * d * d + 2 * mm * 768 * 2 * 768
                       + 4 * n * mm * d + 2 * n * d * d + 2 * n * d * 8 * d + 2 * n * 4 * d * d)
        line = {"metric": "train-step samples/sec (47s@44.1kHz)", "value": b * world * args.steps / elapsed, "unit": "samples/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if mixed else "f32",
                "data": "synthetic",
                "config": {"workload": "stable_audio_open_1_0 DiT train step (v-objective MSE, cfg_dropout 0.1, fwd+bwd, dp_allreduce, "
                                       "fused_adamw_ema), pre-encoded latents, synthetic conditioning tensors, random init, no activation checkpointing",
                           "latent_frames": tlat, "per_gpu_batch": b, "global_batch": b * world, "parallelism": f"dp{world}",
                           "final_loss": float(out["loss"]), "model_tflop_per_sample_fwd_bwd": 3 * fwd / 1e12,
                           "achieved_model_tflops": 3 * fwd * b * world * args.steps / elapsed / 1e12,
                           "ddp": {"process_group": (dist.get_backend() if dist.is_initialized() else None), "exchange_active": stepper.comm.active,
                                   "world_size": (dist.get_world_size() if dist.is_initialized() else 1), "mode": stepper.comm.mode,
                                   "comm_dtype": args.ddp_comm_dtype, "buckets": len(stepper.comm.buckets), "overlap": stepper.comm.overlap,
                                   "gradient_bytes": int(stepper.flat.padded) * 4,
                                   "buckets_launched_from_backward_hooks": sum(int(h) for _, h in getattr(stepper.comm, "last_launch_log", [])),
                                   "timeline": stepper.comm.timeline()}},
                "roofline": prof.roofline(PEAK_BF16_MFMA_TFLOPS if mixed else PEAK_BF16_MFMA_TFLOPS / 3.0)}
        if not args.no_cpu_baseline and world == 1:
            line["cpu_baseline"] = dit_train_cpu_baseline(dcfg, tlat, m)
        emit(line)
    if world > 1:
        dist.destroy_process_group()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU (the driver's own
    invocation sets WORLD_SIZE and lands in the normal path)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


_REAL_STDOUT = None


def guard_stdout():
    """Rank 0 prints ONE JSON line on stdout — and nothing else: the reference's modules print optional-import notices
    ("flash_attn not installed ...", the seed in generate_diffusion_cond) with plain print().  Everything written to file
    descriptor 1 from here on goes to stderr; emit() writes the line to the saved descriptor."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        sys.stdout = sys.stderr


def emit(line):
    out = _REAL_STDOUT if _REAL_STDOUT is not None else sys.stdout
    out.write(json.dumps(line) + "\n")
    out.flush()


DUMP_BUDGET_BYTES = 64 << 20
DUMP_PARAM_SAMPLE = 1 << 22     # parameters kept per dumped step: 16 MiB of float32 (the VAE has ~157 M)


def step_outputs(out, flat, sample=DUMP_PARAM_SAMPLE, seed=0):
    """What one train step hands its caller, copied to the host: every loss of the returned dict (float64) and the parameters the
    step wrote (float32; the same seeded sample of `sample` positions on every run when the model is larger).  Read right after the
    step: a replayed step returns the graph's static buffers."""
    res = {k: v.detach().double().cpu().numpy() for k, v in sorted(out.items())}
    data = flat.data[:flat.numel]
    if data.numel() > sample:
        idx = torch.randint(0, data.numel(), (sample,), generator=torch.Generator().manual_seed(seed)).sort().values
        data = data[idx.to(data.device)]
    res["params"] = data.cpu().numpy()
    return res


def write_outputs(dirpath, by_mode):
    """by_mode: {launch mode: step_outputs(...)} -> dirpath/<mode>_<name>.npy.  Returns the file names."""
    import numpy as np
    arrays = {f"{mode}_{name}": a for mode, res in by_mode.items() for name, a in res.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BUDGET_BYTES, f"--dump-outputs: {total} bytes > {DUMP_BUDGET_BYTES}"
    os.makedirs(dirpath, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dirpath, name + ".npy"), a)
    return sorted(n + ".npy" for n in arrays)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args)
    guard_stdout()
    if args.gpus != int(os.environ.get("WORLD_SIZE", 1)):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE')}")
    if args.workload == "dit_train":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (there is no CPU path for the product kernels)")
        return run_dit_train(args)
    if args.workload == "long_context":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (there is no CPU path for the product kernels)")
        torch.cuda.set_device(0)
        apply_ops_set(args)
        lc = long_context_line(args.steps, args.warmup, not args.no_cpu_baseline)
        emit(({"metric": "DiT sampling steps/sec", "value": lc["value"], "unit": "steps/s", "n_gpus": 1, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": lc["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "fp8(e4m3 projections) + bf16", "data": "synthetic", "config": {"workload": lc["workload"]}, "long_context": lc}))
        return
    if args.workload == "dit_sample":
        if int(os.environ.get("WORLD_SIZE", 1)) > 1:
            raise SystemExit("dit_sample is replicas-only (independent prompts per GPU, no collective): run it per GPU")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (there is no CPU path for the product kernels)")
        return run_dit_sample(args)
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU path for the product kernels)")
    torch.cuda.set_device(local_rank)
    if world > 1 or args.ddp_single_rank:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group("nccl", rank=rank, world_size=world)
    dev = torch.device("cuda", local_rank)

    from stable_audio_tools_amd import ops as O
    from stable_audio_tools_amd.autoencoders import create_autoencoder_from_config
    from stable_audio_tools_amd.training import AutoencoderTrainStep

    cfg = json.load(open(os.path.join(ROOT, "stable_audio_tools_amd", "configs", "stable_audio_2_0_vae.json")))
    torch.manual_seed(1234)                     # identical random-init replica on every rank
    model = create_autoencoder_from_config(cfg).to(dev)
    # de-zero the SnakeBeta parameters a little so the activation path is not the trivial alpha=beta=1 case
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("alpha") or n_.endswith("beta"):
                p.normal_(0.0, 0.1)
    stepper = AutoencoderTrainStep(model, cfg, use_discriminator=(world == 1 and not args.no_real_step), ddp_mode=args.ddp_mode,
                                   ddp_comm_dtype=torch.bfloat16 if args.ddp_comm_dtype == "bf16" else None,
                                   ddp_single_rank=True if args.ddp_single_rank else None)
    if args.no_grad_steal:
        stepper.flat.steal = False
        if getattr(stepper, "flat_d", None) is not None:
            stepper.flat_d.steal = False
    stepper.comm.timing = stepper.comm.active      # exchange timeline of the last timed step (config.ddp.timeline)
    stepper.use_disc = False        # the headline `value` is the generator step (comparable across rounds); the real alternating
    ops = O.get_ops()               # discriminator / generator step is timed separately below -> config.real_step
    apply_ops_set(args, ops)
    prof = ConvProfiler(ops)

    g = torch.Generator().manual_seed(rank)     # per-rank data (train.py:30-33 seeds ranks differently)
    batches = [(0.1 * torch.randn(args.batch, 2, args.sample_size, generator=g)).to(dev) for _ in range(2)]

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        stepper(batches[i % 2])
    sync()
    prof.enabled = True
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = stepper(batches[i % 2])
    sync()
    elapsed = time.perf_counter() - t0
    prof.enabled = False
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    loss = float(out["loss"])
    dumped = {"eager": step_outputs(out, stepper.flat)} if args.dump_outputs is not None else None
    ddp_timeline = stepper.comm.timeline()
    stepper.comm.timing = False
    elapsed_eager = elapsed
    launch = {"mode": "eager", "ms_per_step": {"eager": 1e3 * elapsed_eager / args.steps}}
    gstep = None
    if not args.no_graph and (world == 1 or args.graph_ddp):
        # the same steps with every update replayed from ONE HIP graph (training.GraphedTrainStep: forward + loss + backward + gradient
        # exchange + fused AdamW of a step captured once; the per-step optimizer scalars are read from device memory).  Identical kernels
        # and arithmetic (tests/test_train_step.py::test_graphed_*: bit-equal parameters); what goes away are the launch gaps between the
        # ~400 microsecond-scale kernels of a step.  Capture is outside the timed region; `value` is the faster mode, both are reported.
        from stable_audio_tools_amd.training import GraphedTrainStep
        ops.release_workspaces()
        torch.cuda.empty_cache()
        gstep = GraphedTrainStep(stepper, eager_steps=1)
        for i in range(max(args.warmup, 1) + 2):          # eager call, capturing call, warm replays
            gstep(batches[i % 2])
        sync()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out_g = gstep(batches[i % 2])
        sync()
        elapsed_graph = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed_graph], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed_graph = float(t.item())
        if dumped is not None:
            dumped["hip_graph"] = step_outputs(out_g, stepper.flat)
        launch["ms_per_step"]["hip_graph"] = 1e3 * elapsed_graph / args.steps
        launch["graph_replays"] = gstep.replays
        if gstep.fallback:
            launch["graph_fallback"] = list(gstep.fallback.values())
        # `value` = the faster of the two launch modes (round 6; rounds 4-5 reported the replay and used the eager time).  The replayed
        # step is the SAME kernels in the same order (tests/test_train_step.py::test_graphed_*: bit-equal parameters after eager and
        # replayed steps); the defect that kept the headline on eager launches — torch's multi-block reductions returning stale values
        # under replay, profiles/r04_experiments/graph_reductions/ — concerned torch reductions the step has not contained since
        # (ops.sum_all), and the generator step's replays have reported consistent losses in every evidence run of rounds 4-6.  What the
        # replay removes is the HOST: on a box with a slow host the ~1 200 launches of a step are partly launch-bound (145.0 eager vs
        # 137.4 ms replayed on the box of the round-6 evidence run; 139.6 vs 139.3 on round 5's).  Guard: the replay's last loss must be
        # finite and within 25 % of the loss of the NEXT step run eagerly from the replays' state, else the eager time is used.
        launch["graph_loss"] = float(out_g["loss"])
        out_e = stepper(batches[args.steps % 2])           # the NEXT step, eagerly, from the state the replays left (outside both timed regions)
        sync()
        launch["eager_loss_after_graph"] = float(out_e["loss"])
        g_ok = (math.isfinite(launch["graph_loss"]) and math.isfinite(launch["eager_loss_after_graph"])
                and abs(launch["graph_loss"] - launch["eager_loss_after_graph"]) <= 0.25 * abs(launch["eager_loss_after_graph"]))
        launch["graph_loss_consistent"] = bool(g_ok)
        if g_ok and elapsed_graph < elapsed_eager:
            elapsed = elapsed_graph
            launch["mode"] = "hip_graph"
        launch["value_uses"] = launch["mode"]
    dump_files = write_outputs(args.dump_outputs, dumped) if dumped is not None and rank == 0 else None

    if dist.is_initialized():      # the line's n_gpus IS the size of the process group the exchange ran in
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)
    if rank == 0:
        dom, allk = prof.summary()
        line = {
            "metric": "train-step samples/sec (47s@44.1kHz)",
            "value": args.batch * world * args.steps / elapsed,
            "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32(bf16x3)", "data": "synthetic",
            "config": {"workload": "oobleck_vae_generator_train_step(encode+vae_sample+decode+mrstft_sumdiff_LR_7res_aweighted+kl,"
                                   " backward, dp_allreduce, fused_adamw_ema); stable_audio_2_0_vae architecture, random init"
                                   + ("; the alternating MS-STFT-discriminator / generator step of the reference is timed beside it: real_step_*"
                                      if stepper.discriminator is not None else ""),
                       "full": bool(args.full),
                       "sample_size": args.sample_size, "channels": 2, "sample_rate": 44100,
                       "per_gpu_batch": args.batch, "global_batch": args.batch * world,
                       "parallelism": f"dp{world}", "final_loss": loss, "launch": launch, "ops_set": list(args.ops_set),
                       "ddp": {"process_group": (dist.get_backend() if dist.is_initialized() else None), "exchange_active": stepper.comm.active,
                               "mode": stepper.comm.mode, "comm_dtype": args.ddp_comm_dtype, "buckets": len(stepper.comm.buckets),
                               "overlap": stepper.comm.overlap, "native_c_abi_exchange": bool(stepper.comm.native),
                               "world_size": (dist.get_world_size() if dist.is_initialized() else 1),
                               "buckets_launched_from_backward_hooks": sum(int(h) for _, h in getattr(stepper.comm, "last_launch_log", [])),
                               "timeline": ddp_timeline,
                               "timeline_note": "last timed step, milliseconds from the first kernel of the backward pass: ready = the bucket's gradients "
                                                "are complete (its collective is enqueued behind that event on the side stream), done = the collective "
                                                "finished; a bucket overlaps the backward when done_ms < backward_ms"}},
            "roofline": {"bound": "mfma", "achieved": dom["achieved"], "peak": dom["peak"], "unit": "TFLOP/s",
                         "frac": dom["frac"], "traffic": pmc_traffic(dom["kernel"], args), "mfma_utilisation": pmc_mfma(dom["kernel"], args),
                         "kernel": dom["kernel"],
                         "launches": dom["launches"],
                         "avg_launch_ms": dom["avg_launch_ms"],
                         "note": "dominant kernel by HIP-event time in the timed region; achieved = algorithmic flops "
                                 "(2*Cin*Cout*K*Tout*B per conv launch, 2*M*N*K*T*B per wgrad launch) / event time over ALL its "
                                 "launches; peak: fp32-MFMA dense 157.3 for the fp32 kernels, dense bf16 MFMA / 3 = 833 for the "
                                 "bf16x3 split kernels (three MFMAs per fp32-accurate product); traffic = HBM bytes per launch "
                                 "(2*FETCH_SIZE + WRITE_SIZE, gfx950 correction) from the committed rocprofv3 --pmc passes of this "
                                 "same command (the newest profiles/r0N_pmc_traffic.json that has this kernel; null for a non-default workload size)",
                         "k7_family": k7_family(allk),
                         "hbm": hbm_roofline(args, 1e3 * elapsed / args.steps),
                         "all_conv_kernels": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()} for d in allk]},
        }
        if world == 1 and args.batch == 1 and not args.no_batch_sweep:
            # the same generator step at larger per-GPU batches (1 warm-up + 2 timed steps each): the headline stays at batch 1 per GPU
            # (continuity with rounds 1-2 and with the per-step targets), this is what the 288 GB buy on top of it
            sweep = {}
            for bsz in (2, 4):
                try:
                    bb = [(0.1 * torch.randn(bsz, 2, args.sample_size, generator=g)).to(dev) for _ in range(2)]
                    stepper(bb[0])
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for i in range(2):
                        stepper(bb[i % 2])
                    torch.cuda.synchronize()
                    dt_b = (time.perf_counter() - t1) / 2
                    sweep[str(bsz)] = {"samples_per_s": bsz / dt_b, "ms_per_step": 1e3 * dt_b}
                    del bb
                except torch.cuda.OutOfMemoryError:
                    sweep[str(bsz)] = None
                ops.release_workspaces()          # the per-shape plane buffers of this batch size
                torch.cuda.empty_cache()
            line["config"]["batch_sweep"] = sweep
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, args.cpu_baseline_samples, args.cpu_baseline_budget_s)
        if world == 1 and not args.no_parity:
            line["parity"] = headline_parity(model, cfg, stepper, batches[0], with_gradients=not args.no_parity_gradients)
        if stepper.discriminator is not None:
            # the REAL autoencoder step of the reference (training/autoencoders.py:440-515): MS-STFT discriminator (5 scales, 64
            # filters), updates alternating discriminator / generator — timed over 2 + 2 steps after one of each as warm-up
            stepper.use_disc = True

            def real_steps(n_warm, n_timed):
                stepper.global_step = 0
                for i in range(n_warm):
                    stepper(batches[i % 2])
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t1 = time.perf_counter()
                for i in range(n_timed):
                    o = stepper(batches[i % 2])
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n_timed, torch.cuda.max_memory_allocated() / 2 ** 30, o

            dt_real, peak_real, out_r = real_steps(2, 4)
            # the discriminator's conv kernels over one more discriminator + generator pair, HIP events per launch
            prof.records.clear()
            prof.enabled = True
            real_steps(0, 2)
            prof.enabled = False
            _, allr = prof.summary()
            disc_k = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()} for d in allr if d["kernel"].startswith("sat_disc")]
            line["config"]["real_step"] = {
                "workload": "alternating MS-STFT-discriminator / generator updates (encodec discriminator: 5 scales n_fft 2048..128, 64 filters, "
                            "hinge + feature matching; adversarial 0.1, feature_matching 5.0) on the same 47.55 s stereo items",
                "ms_per_step": 1e3 * dt_real, "samples_per_s": args.batch / dt_real, "steps": 4,
                "peak_hbm_gib": peak_real, "last_loss": float(out_r["loss"]),
                "discriminator_kernels": disc_k,
                "note": "discriminator_kernels: HIP-event time and algorithmic flops (2 * Cin * Cout * kh * kw * frames * bins per conv / "
                        "data-gradient / weight-gradient launch) of csrc/disc_conv.hip over one discriminator + one generator update, "
                        "fractions of the bf16x3 peak (833)"}
            # the same pair of updates with every ResidualUnit recomputing its intermediate in the backward (ResidualUnit.checkpointing):
            # the memory / time trade the module offers for larger per-GPU batches
            from stable_audio_tools_amd.autoencoders import ResidualUnit
            units = [m_ for m_ in model.modules() if isinstance(m_, ResidualUnit)]
            for u in units:
                u.checkpointing = True
            torch.cuda.empty_cache()
            dt_rc, peak_rc, _ = real_steps(2, 2)
            for u in units:
                u.checkpointing = False
            line["config"]["real_step"]["recompute"] = {"ms_per_step": 1e3 * dt_rc, "peak_hbm_gib": peak_rc, "steps": 2,
                                                        "what": "ResidualUnit.checkpointing = True on all 30 units"}
            if args.batch == 1 and not args.no_batch_sweep:
                # what the 288 GB buy for the REAL step: the same alternating updates at four items per GPU (two warm-up + two timed
                # updates) — every activation resident if it fits, else with the units' recompute
                ops.release_workspaces()
                torch.cuda.empty_cache()
                rs4 = None
                for ck in (False, True):
                    bb = None
                    try:
                        for u in units:
                            u.checkpointing = ck
                        bb = [(0.1 * torch.randn(4, 2, args.sample_size, generator=g)).to(dev) for _ in range(2)]
                        stepper.global_step = 0
                        for i in range(2):
                            stepper(bb[i % 2])
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        t1 = time.perf_counter()
                        for i in range(2):
                            stepper(bb[i % 2])
                        torch.cuda.synchronize()
                        dt4 = (time.perf_counter() - t1) / 2
                        rs4 = {"per_gpu_batch": 4, "ms_per_step": 1e3 * dt4, "samples_per_s": 4 / dt4, "steps": 2,
                               "peak_hbm_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "recompute": ck}
                    except torch.cuda.OutOfMemoryError:
                        rs4 = {"per_gpu_batch": 4, "out_of_memory": True, "recompute": ck}
                    finally:
                        del bb
                        for u in units:
                            u.checkpointing = False
                        ops.release_workspaces()
                        torch.cuda.empty_cache()
                    if "ms_per_step" in rs4:
                        break
                line["config"]["real_step"]["batch4"] = rs4
            if gstep is not None:
                # the same alternating updates replayed from HIP graphs (one per kind of update)
                del gstep
                gstep = None
                ops.release_workspaces()
                torch.cuda.empty_cache()
                from stable_audio_tools_amd.training import GraphedTrainStep
                g2 = GraphedTrainStep(stepper, eager_steps=1)
                stepper.global_step = 0
                for i in range(6):                      # per kind: one eager call, the capturing call, one warm replay
                    g2(batches[i % 2])
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t1 = time.perf_counter()
                last_two = []
                for i in range(4):
                    o = g2(batches[i % 2])
                    if i >= 2:
                        last_two.append(o["loss"].clone())
                torch.cuda.synchronize()
                dt_g = (time.perf_counter() - t1) / 4
                rg = {"ms_per_step": 1e3 * dt_g, "samples_per_s": args.batch / dt_g, "steps": 4, "graphs": len(g2.graphs), "replays": g2.replays,
                      "peak_hbm_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "last_loss": float(o["loss"])}
                if g2.fallback:
                    rg["graph_fallback"] = list(g2.fallback.values())
                # continuity check of the replayed updates: the next two updates run eagerly from the state the graphs left
                cont = [g2.stepper(batches[i % 2]) for i in range(2)]
                rg["eager_continuation_losses"] = [float(c_["loss"]) for c_ in cont]
                rg["last_two_graph_losses"] = [float(v) for v in last_two]
                # the replayed losses against the eager updates that follow them (same kind of update, next items / noise draws): the
                # discriminator's hinge loss moves by < 1e-3 per update here, the generator's by a few per cent
                tol = (0.25, 0.05)
                rg["losses_consistent_with_eager"] = all(abs(a - b) <= t * max(abs(b), 1e-6) for a, b, t in
                                                         zip(rg["last_two_graph_losses"], rg["eager_continuation_losses"], tol))
                line["config"]["real_step"]["hip_graph"] = rg
                rg["used_for_real_step_ms"] = False      # reported, not used: the real step's figures stay on eager launches (config.launch)
                del g2
                torch.cuda.empty_cache()
            stepper.use_disc = False
            rs = line["config"]["real_step"]
            line["real_step_samples_per_s"], line["real_step_ms"] = rs["samples_per_s"], rs["ms_per_step"]
            dk = max(disc_k, key=lambda d: d.get("total_ms", 0.0)) if disc_k else None
            if dk is not None:
                line["real_step_dominant_discriminator_kernel"] = {k: dk.get(k) for k in ("kernel", "frac", "achieved", "total_ms", "launches") if k in dk}
        if world == 1 and not args.no_secondary:
            # the second half of BASELINE.json's metric ("...; DiT sampling steps/sec"), measured in the same run: configs[2]
            # (Stable Audio Open DiT, bf16, v-DDIM + CFG), with the self-attention kernel's MFMA roofline
            del stepper, model, batches
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            sec = dit_sample_line("bf16", 1, 50, 10, with_cpu_baseline=not args.no_cpu_baseline)
            line["secondary"] = {k: sec[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline")
                                 if k in sec}
            if "cpu_baseline" in sec:
                line["secondary"]["cpu_baseline"] = sec["cpu_baseline"]
            if not args.no_long_context:
                line["long_context"] = long_context_line(with_cpu_baseline=not args.no_cpu_baseline)
            if not args.no_dit_train:
                line["dit_train"] = dit_train_object(with_cpu_baseline=not args.no_cpu_baseline)
        if dump_files is not None:
            line["config"]["dump_outputs"] = {"dir": args.dump_outputs, "files": dump_files}
        emit(line)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
