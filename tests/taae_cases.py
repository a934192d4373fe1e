"""The transformer-autoencoder (TAAE) fixture cases, shared by tools/gen_golden_taae.py (which writes tests/golden/taae_<case>.npz from
the reference's TAAEEncoder / TAAEDecoder / AudioAutoencoder) and the tests.  Seeds 1700 + 10 * i.
  hd128       channels 128, c_mults [1, 2], strides [2, 4], depths [1, 2], latent 8, window [5, 6], no snake, layer scale, stereo, 1040
              samples: 520 tokens of width 128 (one head of 128), then 130 of width 256 (two heads); rotary on 64 of 128 dims;
  hd64_snake  channels 64, c_mults [1, 1], strides [2, 4], depths [2, 1], window [-1, 8] (unbounded to the left), SnakeBeta prologues and
              ResidualUnits, mono, batch 2, 776 samples: 388 tokens, then 97, of width 64 (head dim min(128, 64) = 64);
  no_scale    hd128 without LayerScale and with strides [1, 4] — the first block's conv is the Identity — 520 samples;
  vae         the model-config JSON through create_autoencoder_from_config: TAAE encoder (2 x latent channels) and decoder around a "vae"
              bottleneck; stored are pre_bottleneck_latents and decode() of the latent mean.
Every first block sees a token count that is no multiple of 64 and spans at least three 128-query workgroups and part of another, and every window hides keys.
The first encoder TAAEBlock is also run alone, on block_input(); of its (B, C, T) output every BLOCK0_STEP-th channel is stored."""
import copy

import torch

import seeded

_HD128 = dict(channels=128, latent_dim=8, c_mults=[1, 2], strides=[2, 4], transformer_depths=[1, 2], sliding_window=[5, 6],
              use_snake=False, layer_scale=True)
_HD64 = dict(channels=64, latent_dim=8, c_mults=[1, 1], strides=[2, 4], transformer_depths=[2, 1], sliding_window=[-1, 8],
             use_snake=True, use_dilated_conv=True, layer_scale=True)
_NOSCALE = dict(_HD128, strides=[1, 4], layer_scale=False)
_VAE = dict(channels=128, c_mults=[1, 2], strides=[2, 4], transformer_depths=[1, 1], sliding_window=[5, 6], use_snake=False,
            layer_scale=True)

CONFIGS = {
    "hd128": {"encoder": dict(_HD128, in_channels=2), "decoder": dict(_HD128, out_channels=2)},
    "hd64_snake": {"encoder": dict(_HD64, in_channels=1), "decoder": dict(_HD64, out_channels=1)},
    "no_scale": {"encoder": dict(_NOSCALE, in_channels=2), "decoder": dict(_NOSCALE, out_channels=2)},
    "vae": {"encoder": dict(_VAE, in_channels=2, latent_dim=16), "decoder": dict(_VAE, out_channels=2, latent_dim=8)},
}
LENGTHS = {"hd128": 1040, "hd64_snake": 776, "no_scale": 520, "vae": 1040}
BATCH = {"hd128": 1, "hd64_snake": 2, "no_scale": 1, "vae": 1}
CASES = list(CONFIGS)
BLOCK0_STEP = 4
OUTPUTS = ("encoder", "decoder", "block0")


def case_id(i):
    return CASES[i]


def case_seed(i):
    return 1700 + 10 * i


def case_config(i, kind, window=True):
    """the TAAEEncoder / TAAEDecoder kwargs (kind "encoder" | "decoder"); window=False: a window that hides nothing"""
    cfg = copy.deepcopy(CONFIGS[CASES[i]][kind])
    if not window:
        cfg["sliding_window"] = [-1, -1]
    return cfg


def has_scale(i):
    return bool(CONFIGS[CASES[i]]["encoder"]["layer_scale"])


def downsampling(i):
    r = 1
    for s in CONFIGS[CASES[i]]["encoder"]["strides"]:
        r *= s
    return r


def model_config(i, window=True):
    """the full model-config JSON of the "vae" case, as create_autoencoder_from_config takes it"""
    dec = case_config(i, "decoder", window)
    return {"model_type": "autoencoder", "sample_size": LENGTHS[CASES[i]], "sample_rate": 44100, "audio_channels": 2,
            "model": {"encoder": {"type": "taae", "config": case_config(i, "encoder", window)},
                      "decoder": {"type": "taae", "config": dec},
                      "bottleneck": {"type": "vae"}, "latent_dim": dec["latent_dim"], "downsampling_ratio": downsampling(i),
                      "io_channels": 2}}


def inputs(i):
    """audio (B, in_channels, L), a latent (B, decoder latent_dim, L / ratio) and the lone first block's input (B, channels, L)"""
    name, seed = CASES[i], case_seed(i)
    enc, dec = CONFIGS[name]["encoder"], CONFIGS[name]["decoder"]
    b, n = BATCH[name], LENGTHS[name]
    return {"audio": torch.from_numpy(seeded.seeded_array((b, enc["in_channels"], n), seed + 1, scale=0.5)),
            "latent": torch.from_numpy(seeded.seeded_array((b, dec["latent_dim"], n // downsampling(i)), seed + 2)),
            "block_input": torch.from_numpy(seeded.seeded_array((b, enc["channels"] * enc["c_mults"][0], n), seed + 3))}


def state_dict(model, seed):
    """the seeded state dict over `model`'s shapes (every key but the rotary inv_freq buffers, which keep their constructed values)"""
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    return {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, seed).items()}
