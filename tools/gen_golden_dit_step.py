#!/usr/bin/env python
"""Fixture of the DiT train step's timestep machinery (tests/test_dit_step_options.py) from the reference's own functions
(stable_audio_tools/inference/sampling.py:24-95), CPU fp32: tests/golden/dit_step_timesteps.npz with, for n = 64,
  z: the standard-normal draw torch.randn(n) after torch.manual_seed(SEED) — the generator is re-seeded before every reference call, so
     each sampler below consumed exactly this draw;
  trunc_logit_normal: truncated_logistic_normal_rescaled(n);
  log_snr, log_snr_0.5_1.0: sample_timesteps_logsnr(n) with the defaults and with (mean_logsnr, std_logsnr) = (0.5, 1.0);
  shift_t: linspace(0, 0.999, 32); shift_<len>, shift_sine_<len>: DistributionShift(use_sine=False | True).time_shift(shift_t, len) for
     len = 100, 1024, 8000 (below min_length, inside, above max_length).
Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_dit_step.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refimport               # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dit_step_timesteps.npz")
SEED, N = 7310, 64
SHIFT_LENGTHS = (100, 1024, 8000)


def seeded(fn, *args, **kw):
    torch.manual_seed(SEED)
    return fn(*args, **kw)


def generate():
    refimport.import_reference()
    from stable_audio_tools.inference import sampling as ref
    out = {"z": seeded(torch.randn, N).numpy()}
    out["trunc_logit_normal"] = seeded(ref.truncated_logistic_normal_rescaled, N).numpy()
    out["log_snr"] = seeded(ref.sample_timesteps_logsnr, N).numpy()
    out["log_snr_0.5_1.0"] = seeded(ref.sample_timesteps_logsnr, N, mean_logsnr=0.5, std_logsnr=1.0).numpy()
    t = torch.linspace(0, 0.999, 32)
    out["shift_t"] = t.numpy()
    for use_sine in (False, True):
        shift = ref.DistributionShift(use_sine=use_sine)
        for length in SHIFT_LENGTHS:
            out[f"shift_{'sine_' if use_sine else ''}{length}"] = shift.time_shift(t, length).numpy()
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print(f"{os.path.basename(OUT)}: {os.path.getsize(OUT)} bytes, keys {sorted(out)}")


if __name__ == "__main__":
    main()
