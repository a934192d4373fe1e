#!/usr/bin/env python
"""Fixtures of the sliding-window DiT cases (tests/sliding_window_cases.py) from the reference's DiffusionTransformer, CPU fp32:
tests/golden/dit_window_<case>.npz with
  plain, guided (cfg 6.0, phi 0.75), keys (sorted state-dict keys);
  plain_bf16w: the fp32 reference on bf16-rounded weights and inputs (what the bf16 model is compared with);
  sampler: 3 v-DDIM steps with CFG (the loop tests/test_dit_parity.py::_sampler_case restates) around the reference model;
  dense_plain: `plain` of the same model built WITHOUT the window — the generator asserts that `plain` lies farther than 10 x 1e-3 from
               it, so that a model which silently ignores its window cannot pass the tests.

The window itself is NOT the reference's code path.  The reference hands ContinuousTransformer(sliding_window=[left, right]) down to
Attention.apply_attn as flash_attn_sliding_window (transformer.py:845, :683, :704, :523) and applies it only inside flash_attn_func
(:436); where the flash-attn package is absent — as on the machine that builds these fixtures — apply_attn prints a warning and runs dense
attention (:414-415, :440), and with the package it would first round an fp32 model's q / k / v to fp16 (:433-434).  This generator
therefore rebinds the reference's Attention.apply_attn to a dense banded softmax of its own, in the model's dtype, with flash-attn's
window_size semantics: query i sees key j iff (left < 0 or j >= i - left) and (right < 0 or j <= i + right), -1 = unbounded, kv heads
repeated over their query heads as apply_attn does (:408-411), scale 1 / sqrt(head dim), no other mask.  Everything else — projections,
qk_norm, rotary, the blocks, the conditioning, CFG — is the reference's.  Calls without a window (cross-attention, the dense model) go
through the same function with no band, and the generator asserts that it then matches the reference's own apply_attn.

No gradients: the window is inference-only here.  Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_sliding_window.py"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refimport                     # noqa: E402
import seeded                        # noqa: E402
import sliding_window_cases as cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3      # the DiT parity bar of the tests


def banded_apply_attn(self, q, k, v, causal=None, flex_attention_block_mask=None, flex_attention_score_mod=None,
                      flash_attn_sliding_window=None):
    """Attention.apply_attn with the window applied as a dense band mask (module docstring)."""
    assert not causal and flex_attention_block_mask is None and flex_attention_score_mod is None
    if self.num_heads != self.kv_heads:
        rep = self.num_heads // self.kv_heads
        k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    if flash_attn_sliding_window is not None:
        left, right = flash_attn_sliding_window
        nq, nk = q.shape[-2], k.shape[-2]
        assert nq == nk, "a window on cross-attention is not part of the fixtures"
        i, j = torch.arange(nq)[:, None], torch.arange(nk)[None, :]
        vis = torch.ones(nq, nk, dtype=torch.bool)
        if left >= 0:
            vis &= j >= i - left
        if right >= 0:
            vis &= j <= i + right
        s = s.masked_fill(~vis, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _model(i, window):
    from stable_audio_tools.models.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i, window=window)).float()
    model.train(False)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    model.load_state_dict(sd, strict=False)
    return model


def generate(i):
    refimport.import_reference()
    from stable_audio_tools.models import transformer as ref_transformer
    original = ref_transformer.Attention.apply_attn
    inp = cases.inputs(i)
    kw = dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], prepend_cond=inp.get("prepend_cond"),
              prepend_cond_mask=inp.get("prepend_cond_mask"))
    with torch.no_grad():
        dense_model = _model(i, window=False)
        dense_ref = dense_model(inp["x"], inp["t"], cfg_scale=1.0, **kw)      # the reference's own attention, no window anywhere
        ref_transformer.Attention.apply_attn = banded_apply_attn
        try:
            out = {"dense_plain": dense_model(inp["x"], inp["t"], cfg_scale=1.0, **kw).numpy()}
            assert _rel(torch.from_numpy(out["dense_plain"]), dense_ref) < 1e-5, "the rebound apply_attn without a band is not the reference's"
            model = _model(i, window=True)
            assert list(model.transformer.sliding_window) == cases.case_config(i)["sliding_window"]
            out["keys"] = np.array(sorted(model.state_dict().keys()))
            out["plain"] = model(inp["x"], inp["t"], cfg_scale=1.0, **kw).numpy()
            gap = _rel(torch.from_numpy(out["plain"]), torch.from_numpy(out["dense_plain"]))
            assert gap > 10 * TOL, f"{cases.case_id(i)}: the window moves the output by {gap:.2e} only: a model that ignores it would pass"
            out["guided"] = model(inp["x"], inp["t"], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw).numpy()
            # v-DDIM with CFG
            steps = cases.SAMPLER_STEPS
            x = inp["x"]
            ts = torch.linspace(1.0, 0, steps + 1)[:-1]
            alphas, sigmas = torch.cos(ts * math.pi / 2), torch.sin(ts * math.pi / 2)
            for s in range(steps):
                v = model(x, torch.ones(x.shape[0]) * ts[s], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw)
                pred = x * alphas[s] - v * sigmas[s]
                eps = x * sigmas[s] + v * alphas[s]
                if s < steps - 1:
                    x = pred * alphas[s + 1] + eps * sigmas[s + 1]
            out["sampler"] = pred.numpy()

            # the fp32 reference on bf16-rounded weights and inputs
            def q(a):
                return a.to(torch.bfloat16).float() if a is not None and a.is_floating_point() else a
            full = {k: v.clone() for k, v in model.state_dict().items()}
            model.load_state_dict({k: q(v) for k, v in full.items()})
            out["plain_bf16w"] = model(q(inp["x"]), q(inp["t"]), cfg_scale=1.0, **{k: q(v) for k, v in kw.items()}).numpy()
            model.load_state_dict(full)
        finally:
            ref_transformer.Attention.apply_attn = original
    out["window_gap"] = np.float32(gap)
    return out


def main():
    for i in range(len(cases.CASES)):
        out = generate(i)
        path = os.path.join(OUT, f"dit_window_{cases.case_id(i)}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, |plain| {np.abs(out['plain']).max():.3f} "
              f"|guided| {np.abs(out['guided']).max():.3f} |sampler| {np.abs(out['sampler']).max():.3f} window gap {out['window_gap']:.3f}")


if __name__ == "__main__":
    main()
