#!/usr/bin/env python
"""Fixtures of the transformer-autoencoder cases (tests/taae_cases.py) from the reference's TAAEEncoder / TAAEDecoder (cases hd128,
hd64_snake, no_scale) and its create_autoencoder_from_config (case vae), CPU fp32: tests/golden/taae_<case>.npz with
  keys     sorted state-dict keys ("encoder." / "decoder." prefixed, as inside an AudioAutoencoder);
  encoder  the encoder's output on the seeded audio (vae: encode()'s pre_bottleneck_latents);
  decoder  the decoder's output on the seeded latent (vae: decode() of the latent mean);
  block0   the first encoder TAAEBlock alone on a seeded (B, C, T) input, every BLOCK0_STEP-th channel;
  dense_*  the same three from the same weights with a window that hides nothing;
  noscale_* the same three with every LayerScale parameter set to zero — the transformer blocks are then the identity (absent from
           no_scale, which has no LayerScale).
The generator asserts that each dense_* and noscale_* output lies farther than 10 x 1e-3 from its counterpart, so that a model which
ignores its window or skips its blocks cannot pass the tests.  Outputs only: the weights come from seeded.seeded_state_dict over the
reference model's shapes and are never stored.

The window is applied by rebinding the reference's Attention.apply_attn to the banded softmax of tools/gen_golden_sliding_window.py
(its docstring says why: without the flash-attn package the reference drops the window); without a band that function is asserted to
match the reference's own apply_attn.

Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_taae.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refimport                     # noqa: E402
import taae_cases as cases           # noqa: E402
from gen_golden_sliding_window import banded_apply_attn     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3      # the parity bar of the tests


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


class _Pair(torch.nn.Module):
    """encoder + decoder under the names an AudioAutoencoder gives them"""

    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder


def _model(i, window, zero_scale=False):
    from stable_audio_tools.models import autoencoders as ref
    if cases.case_id(i) == "vae":
        model = ref.create_autoencoder_from_config(cases.model_config(i, window))
    else:
        model = _Pair(ref.create_encoder_from_config({"type": "taae", "config": cases.case_config(i, "encoder", window)}),
                      ref.create_decoder_from_config({"type": "taae", "config": cases.case_config(i, "decoder", window)}))
    model = model.float().train(False)
    sd = cases.state_dict(model, cases.case_seed(i))
    if zero_scale:
        sd = {k: (torch.zeros_like(v) if k.endswith(".scale") else v) for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model


def _outputs(i, model):
    inp = cases.inputs(i)
    if cases.case_id(i) == "vae":
        _, info = model.encode(inp["audio"], return_info=True)
        enc = info["pre_bottleneck_latents"]
        dec = model.decode(enc.chunk(2, dim=1)[0])
    else:
        enc, dec = model.encoder(inp["audio"]), model.decoder(inp["latent"])
    block0 = model.encoder.layers[1](inp["block_input"])[:, ::cases.BLOCK0_STEP]
    return {"encoder": enc.numpy(), "decoder": dec.numpy(), "block0": block0.contiguous().numpy()}


def generate(i):
    refimport.import_reference()
    from stable_audio_tools.models import transformer as ref_transformer
    original = ref_transformer.Attention.apply_attn
    with torch.no_grad():
        dense = _model(i, window=False)
        dense_ref = _outputs(i, dense)      # the reference's own attention, nothing hidden
        ref_transformer.Attention.apply_attn = banded_apply_attn
        try:
            out = {"dense_" + k: v for k, v in _outputs(i, dense).items()}
            for k in cases.OUTPUTS:
                assert _rel(torch.from_numpy(out["dense_" + k]), torch.from_numpy(dense_ref[k])) < 1e-5, "the rebound apply_attn without a band is not the reference's"
            model = _model(i, window=True)
            out["keys"] = np.array(sorted(model.state_dict().keys()))
            out.update(_outputs(i, model))
            gaps = {k: _rel(torch.from_numpy(out[k]), torch.from_numpy(out["dense_" + k])) for k in cases.OUTPUTS}
            assert min(gaps.values()) > 10 * TOL, f"{cases.case_id(i)}: the window moves an output by {gaps} only"
            out["window_gap"] = np.float32(min(gaps.values()))
            if cases.has_scale(i):
                out.update({"noscale_" + k: v for k, v in _outputs(i, _model(i, window=True, zero_scale=True)).items()})
                gaps = {k: _rel(torch.from_numpy(out[k]), torch.from_numpy(out["noscale_" + k])) for k in cases.OUTPUTS}
                assert min(gaps.values()) > 10 * TOL, f"{cases.case_id(i)}: the blocks move an output by {gaps} only"
                out["block_gap"] = np.float32(min(gaps.values()))
        finally:
            ref_transformer.Attention.apply_attn = original
    return out


def main():
    for i in range(len(cases.CASES)):
        out = generate(i)
        path = os.path.join(OUT, f"taae_{cases.case_id(i)}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, " + " ".join(f"|{k}| {np.abs(out[k]).max():.3f}" for k in cases.OUTPUTS)
              + f" window gap {out['window_gap']:.3f} block gap {float(out.get('block_gap', np.nan)):.3f}")


if __name__ == "__main__":
    main()
