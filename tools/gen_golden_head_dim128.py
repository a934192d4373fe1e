#!/usr/bin/env python
"""Fixtures of the head dim 128 DiT cases (tests/head_dim128_cases.py) from the reference's DiffusionTransformer, CPU fp32:
tests/golden/dit_hd128_<case>.npz with
  plain, guided (cfg 6.0, phi 0.75), hidden_first, hidden_last, keys (sorted state-dict keys);
  plain_bf16w: the fp32 reference on bf16-rounded weights and inputs (what the bf16 model is compared with);
  sampler: 3 v-DDIM steps with CFG (the loop tests/test_dit_parity.py::_sampler_case restates) around the reference model.
No gradients: head dim 128 is inference-only here.  Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_head_dim128.py"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import head_dim128_cases as cases   # noqa: E402
import refimport                    # noqa: E402
import seeded                       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def generate(i):
    refimport.import_reference()
    from stable_audio_tools.models.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i)).float()
    model.train(False)
    attn = model.transformer.layers[0].self_attn
    assert attn.dim_heads == 128 and model.transformer.rotary_pos_emb.inv_freq.numel() == 32
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    model.load_state_dict(sd, strict=False)
    inp = cases.inputs(i)
    kw = dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], prepend_cond=inp.get("prepend_cond"),
              prepend_cond_mask=inp.get("prepend_cond_mask"))
    out = {"keys": np.array(sorted(model.state_dict().keys()))}
    with torch.no_grad():
        out["plain"] = model(inp["x"], inp["t"], cfg_scale=1.0, **kw).numpy()
        out["guided"] = model(inp["x"], inp["t"], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw).numpy()
        hidden = model(inp["x"], inp["t"], return_info=True, **kw)[1]["hidden_states"]
        out["hidden_first"], out["hidden_last"] = hidden[0].numpy(), hidden[-1].numpy()
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
    return out


def main():
    for i in range(len(cases.CASES)):
        out = generate(i)
        path = os.path.join(OUT, f"dit_hd128_{cases.case_id(i)}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, |plain| {np.abs(out['plain']).max():.3f} "
              f"|guided| {np.abs(out['guided']).max():.3f} |sampler| {np.abs(out['sampler']).max():.3f}")


if __name__ == "__main__":
    main()
