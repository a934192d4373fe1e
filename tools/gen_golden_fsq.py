#!/usr/bin/env python
"""Fixtures of the dithered-FSQ cases (tests/fsq_cases.py) from the reference on the CPU, fp32, eval mode.

Kernel cases, tests/golden/fsq_<case>.npz, from the reference's DitheredFSQ(levels, num_codebooks) on the seeded input:
  codes     (B, C, T) fp32: forward()'s codes, moved back to the conv stack's layout;
  indices   (B, T, Q) int64: forward()'s indices as they come;
  odd_codes (case l6543x2 only) indices_to_codes(fsq_cases.odd_tokens()) as (B, C, T): negative tokens and tokens >= codebook_size.
The codec case, tests/golden/fsq_codec.npz, from create_autoencoder_from_config(fsq_cases.codec_config()) with the seeded state dict:
  keys                    sorted state-dict keys (the bottleneck adds none);
  pre_bottleneck_latents  (1, 8, 130), quantizer_indices (1, 130, 2), latents (1, 8, 130): encode(audio, return_info=True);
  decoded                 decoder(indices_to_codes(quantizer_indices).transpose(1, 2)): the reference's decode_tokens with the layout
                          mended (as it stands it hands (B, T, C) to a decoder that takes (B, C, T));
(DitheredFSQBottleneck.encode on the latents alone is asserted to give `latents` again.)
The window of the TAAE is applied as tools/gen_golden_taae.py applies it.

Asserted on the reference's own data before anything is written, so that no fixture makes a test vacuous:
  - codes == table[d][level] with the host table arange(L) * half_l - 1, and indices_to_codes(indices) == codes, bit for bit;
  - at most fsq_cases.TIE_SHARE_CAP of a case's elements (planted columns aside) lie within TIE_BAND of a rounding tie, and away from
    a tie the reference's level is round(li64);
  - the planted columns give the expected levels (x = 0: round-half-to-even of fp32's 1 / half_l, the even neighbour of the exact tie at
    L = 6, 4, 2; +-20, +-9: the last / first level);
  - codec: with the largest latent error the tests admit (E = 1e-3 * max |latent|) at most CODEC_BAND_CAP of the digits lie inside
    the band (L - 1) / 2 * E + TIE_BAND around a tie.
Writes tests/golden/fsq_MANIFEST.json (generator, files, versions, measured near-tie shares) beside them; tests/golden/MANIFEST.json
belongs to oracle/gen_golden.py, which rewrites it whole, and is left alone.

Needs the reference checkout (oracle/refimport.py): build container only.
    python tools/gen_golden_fsq.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fsq_cases as cases            # noqa: E402
import refimport                     # noqa: E402
from gen_golden_sliding_window import banded_apply_attn     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TOL = 1e-3      # the parity bar of the TAAE tests


def li64(x, levels):
    """(tanh(x) + 1) * (L_d - 1) / 2 in fp64 for x (B, C, T), channel c = q * D + d"""
    d = len(levels)
    lm1 = torch.tensor([levels[c % d] - 1 for c in range(x.shape[1])], dtype=torch.float64)[None, :, None]
    return (torch.tanh(x.double()) + 1.0) * lm1 / 2.0


def tie_distance(li):
    return (li - li.floor() - 0.5).abs()


def _levels_of(indices, levels):
    """(B, T, Q) indices -> (B, C, T) integer levels, by the reference's rule"""
    b, t, q = indices.shape
    lv = torch.tensor(levels, dtype=torch.int64)
    digits = (indices[..., None] // torch.tensor(cases.basis(levels), dtype=torch.int64)) % lv       # (B, T, Q, D)
    return digits.reshape(b, t, q * len(levels)).transpose(1, 2)


def _check_quantiser(name, x, codes, indices, levels, planted):
    d = len(levels)
    half_l = 1.0 * 2 / (torch.tensor(levels, dtype=torch.int64) - 1)
    lev = _levels_of(indices, levels)
    table = torch.stack([(torch.arange(max(levels), dtype=torch.float32) * half_l[c % d] - 1.0) for c in range(x.shape[1])])   # (C, Lmax)
    from_table = torch.gather(table[None].expand(x.shape[0], -1, -1), 2, lev)
    assert torch.equal(from_table, codes), f"{name}: the reference's codes are not table[d][level]"
    li = li64(x, levels)
    near = tie_distance(li) < cases.TIE_BAND
    near[:, :, :planted] = False
    share = float(near.sum()) / x.numel()
    assert share <= cases.TIE_SHARE_CAP, f"{name}: {share:.2e} of the elements lie near a tie"
    free = ~near
    free[:, :, :planted] = False
    assert torch.equal(lev[free], li.round().to(torch.int64)[free]), f"{name}: away from a tie the reference's level is not round(li64)"
    if planted:
        top = torch.tensor([levels[c % d] - 1 for c in range(x.shape[1])], dtype=torch.int64)
        # x = 0: li = 1 / half_l in fp32, the exact half-integer (L - 1) / 2 for the small even level counts (6, 4, 2: the even neighbour wins);
        # at L = 64 fp32's 1 / fl(2 / 63) is not 31.5 and the level is simply the nearest
        at_zero = torch.stack([(1.0 / half_l[c % d]).round().to(torch.int64) for c in range(x.shape[1])])
        for L, want in ((6, 2), (4, 2), (2, 0)):
            assert all(int(at_zero[c]) == want for c in range(x.shape[1]) if levels[c % d] == L), f"{name}: x = 0 at L = {L}"
        for t, want in enumerate((at_zero, top, 0 * top, top, 0 * top)):
            assert torch.equal(lev[:, :, t], want[None].expand(x.shape[0], -1)), f"{name}: planted column {t}"
    return share


def generate_kernel_case(i):
    refimport.import_reference()
    from stable_audio_tools.models.fsq import DitheredFSQ
    shape, levels, q = cases.case(i)
    x = cases.inputs(i)
    fsq = DitheredFSQ(levels, num_codebooks=q).train(False)
    with torch.no_grad():
        codes, indices = fsq(x.transpose(1, 2))
        back = fsq.indices_to_codes(indices)
        assert torch.equal(back, codes), "indices_to_codes(indices) != codes"
        codes = codes.transpose(1, 2).contiguous()
        assert indices.dtype == torch.int64 and tuple(indices.shape) == (shape[0], shape[2], q)
        share = _check_quantiser(cases.CASES[i], x, codes, indices, levels, cases.planted_columns(i))
        out = {"codes": codes.numpy(), "indices": indices.numpy(), "tie_share": np.float64(share)}
        if cases.CASES[i] == cases.ODD_CASE:
            out["odd_codes"] = fsq.indices_to_codes(cases.odd_tokens()).transpose(1, 2).contiguous().numpy()
    return out


def generate_codec():
    refimport.import_reference()
    from stable_audio_tools.models import autoencoders as ref
    from stable_audio_tools.models import transformer as ref_transformer
    original = ref_transformer.Attention.apply_attn
    ref_transformer.Attention.apply_attn = banded_apply_attn
    try:
        with torch.no_grad():
            model = ref.create_autoencoder_from_config(cases.codec_config()).float().train(False)
            missing, unexpected = model.load_state_dict(cases.codec_state_dict(model), strict=False)
            assert not unexpected and all(k.endswith("inv_freq") for k in missing)
            assert not [k for k in model.state_dict() if k.startswith("bottleneck.")]
            latents, info = model.encode(cases.codec_audio(), return_info=True)
            pre, tokens = info["pre_bottleneck_latents"], info["quantizer_indices"]
            decoded = model.decoder(model.bottleneck.quantizer.indices_to_codes(tokens).transpose(1, 2))
            alone = model.bottleneck.encode(pre)
    finally:
        ref_transformer.Attention.apply_attn = original
    levels, q = cases.BOTTLENECK["config"]["levels"], cases.BOTTLENECK["config"]["num_codebooks"]
    assert torch.equal(alone, latents) and tuple(tokens.shape) == (1, pre.shape[2], q)
    share = _check_quantiser("codec", pre, latents, tokens, levels, 0)
    e = TOL * float(pre.abs().max())
    d = len(levels)
    band = torch.tensor([(levels[c % d] - 1) / 2.0 * e + cases.TIE_BAND for c in range(pre.shape[1])], dtype=torch.float64)[None, :, None]
    band_share = float((tie_distance(li64(pre, levels)) <= band).sum()) / pre.numel()
    assert band_share <= cases.CODEC_BAND_CAP, f"codec: {band_share:.3f} of the digits inside the band at the largest admitted encoder error"
    return {"keys": np.array(sorted(model.state_dict().keys())), "pre_bottleneck_latents": pre.numpy(), "quantizer_indices": tokens.numpy(),
            "latents": latents.numpy(), "decoded": decoded.numpy(), "tie_share": np.float64(share),
            "band_share_at_tol": np.float64(band_share)}


def main():
    shares = {}
    for i, name in enumerate(cases.CASES):
        out = generate_kernel_case(i)
        path = os.path.join(OUT, f"fsq_{name}.npz")
        np.savez_compressed(path, **out)
        shares[name] = float(out["tie_share"])
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, near-tie share {shares[name]:.2e}, largest index {int(out['indices'].max())}")
    out = generate_codec()
    path = os.path.join(OUT, "fsq_codec.npz")
    np.savez_compressed(path, **out)
    shares["codec"] = float(out["tie_share"])
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, |latent| {np.abs(out['pre_bottleneck_latents']).max():.3f} "
          f"|decoded| {np.abs(out['decoded']).max():.3f} near-tie share {shares['codec']:.2e} band share at the bar {float(out['band_share_at_tol']):.4f}")
    m = {"generator": "tools/gen_golden_fsq.py", "reference": "Stability-AI/stable-audio-tools v0.0.19",
         "files": [f"fsq_{n}.npz" for n in cases.CASES] + ["fsq_codec.npz"], "torch": torch.__version__, "numpy": np.__version__,
         "near_tie_share": shares}
    with open(os.path.join(OUT, "fsq_MANIFEST.json"), "w") as f:
        json.dump(m, f, indent=1)


if __name__ == "__main__":
    main()
