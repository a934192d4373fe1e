#!/usr/bin/env python
"""Fixtures of the inpainting DiT cases (tests/inpaint_cases.py) from the reference's DiffusionTransformer and random_inpaint_mask
(models/inpainting.py), CPU fp32: tests/golden/dit_inpaint_<case>.npz with
  keys (sorted state-dict keys);
  mask/<draw>, next/<draw>: random_inpaint_mask's (B, 1, T) mask for every (python seed, mask_kwargs) pair of cases.MASK_DRAWS at the
  real lengths cases.LENGTHS, and the random.random() drawn right after the call (what pins the state of the stream);
  plain, guided (cfg 6.0, phi 0.75): forward outputs with input_concat_cond = the inpaint conditioning of draw cases.COND_DRAW,
  concatenated in the case's input_concat_ids order;  plain_bf16w: the fp32 reference on bf16-rounded weights and inputs;
  sampler: 3 v-DDIM steps with CFG and that constant input_concat_cond;
  loss and grad/<name>: gradients of the case's objective MSE for the input ("<input>") and every parameter — tensors of at most
  seeded.FULL_KEEP_NUMEL elements whole, larger ones at seeded.probe_index positions;
  train_loss, train_mask, upd/<name>: cases.TRAIN_STEPS steps of torch.optim.AdamW(**cases.OPT) on the reference model with
  random.seed(cases.TRAIN_SEED) before the first, random_inpaint_mask on the padding mask of cases.LENGTHS, timesteps and noise of
  cases.train_data, cfg_dropout_prob 0: the losses, the drawn masks and the parameter updates (stored like the gradients).
Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_inpaint.py"""
import math
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import inpaint_cases as cases   # noqa: E402
import refimport                # noqa: E402
import seeded                   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def stored(name, t):
    """What the fixture keeps of gradient / update `name`."""
    a = t.detach().reshape(-1).numpy()
    return a if a.size <= seeded.FULL_KEEP_NUMEL else a[seeded.probe_index(name, a.size)]


def noise_targets(objective, x0, noise, t):
    if objective == "v":
        alpha, sigma = torch.cos(t * math.pi / 2)[:, None, None], torch.sin(t * math.pi / 2)[:, None, None]
        return x0 * alpha + noise * sigma, noise * alpha - x0 * sigma
    alpha, sigma = (1 - t)[:, None, None], t[:, None, None]
    return x0 * alpha + noise * sigma, noise - x0


def generate(i):
    refimport.import_reference()
    from stable_audio_tools.models.dit import DiffusionTransformer
    from stable_audio_tools.models.inpainting import random_inpaint_mask
    model = DiffusionTransformer(**cases.case_config(i)).float()
    model.train(False)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    model.load_state_dict(sd, strict=False)
    inp = cases.inputs(i)
    pad = cases.padding_mask()
    out = {"keys": np.array(sorted(model.state_dict().keys()))}
    masks = {}
    for name, (seed, kwargs) in cases.MASK_DRAWS.items():
        random.seed(seed)
        _, masks[name] = random_inpaint_mask(inp["x"], padding_masks=pad, **kwargs)
        out["next/" + name] = np.float64(random.random())
        out["mask/" + name] = masks[name].numpy()
    cond = cases.concat_cond(i, inp["x"], masks[cases.COND_DRAW])
    kw = dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], input_concat_cond=cond)
    with torch.no_grad():
        out["plain"] = model(inp["x"], inp["t"], cfg_scale=1.0, **kw).numpy()
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
    # gradients of the objective's MSE
    objective = cases.objective(i)
    noise = torch.from_numpy(seeded.seeded_array(tuple(inp["x"].shape), cases.NOISE_SEED))
    noised, target = noise_targets(objective, inp["x"], noise, inp["t"])
    xin = noised.clone().requires_grad_(True)
    model.train(True)
    loss = torch.nn.functional.mse_loss(model(xin, inp["t"], **kw), target)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in model.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(loss, [xin] + params, allow_unused=True)
    out["loss"] = np.float32(loss.item())
    for n, g in zip(["<input>"] + names, grads):
        if g is not None:
            out["grad/" + n] = stored(n, g)
    # train steps
    before = {n: p.detach().clone() for n, p in zip(names, params)}
    opt = torch.optim.AdamW(params, **cases.OPT)
    losses, drawn = [], []
    random.seed(cases.TRAIN_SEED)
    for s in range(cases.TRAIN_STEPS):
        x0, noise, t = cases.train_data(i, s)
        noised, target = noise_targets(objective, x0, noise, t)
        masked, mask = random_inpaint_mask(x0, padding_masks=pad)
        parts = [mask, masked]
        cond = torch.cat(parts if cases.mask_first(i) else parts[::-1], dim=1)
        o = model(noised, t, cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], input_concat_cond=cond,
                  cfg_dropout_prob=0.0)
        loss = torch.nn.functional.mse_loss(o, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        drawn.append(mask.numpy())
    out["train_loss"] = np.array(losses, dtype=np.float32)
    out["train_mask"] = np.stack(drawn)
    for n, p in zip(names, params):
        out["upd/" + n] = stored(n, p.detach() - before[n])
    return out


def main():
    for i in range(len(cases.CASES)):
        out = generate(i)
        path = os.path.join(OUT, f"dit_inpaint_{cases.case_id(i)}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, |plain| {np.abs(out['plain']).max():.3f} "
              f"|guided| {np.abs(out['guided']).max():.3f} loss {out['loss']:.5f} train {out['train_loss']} "
              f"grads {sum(k.startswith('grad/') for k in out)} masked frames "
              + " ".join(f"{k[5:]}:{int((out[k] == 0).sum())}" for k in out if k.startswith("mask/")))


if __name__ == "__main__":
    main()
