"""The inpainting (`diffusion_cond_inpaint`) fixture cases, shared by tools/gen_golden_inpaint.py (which writes
tests/golden/dit_inpaint_<case>.npz from the reference's DiffusionTransformer and random_inpaint_mask) and the tests.
Both cases: io_channels 4 + input_concat_dim 5 (mask channel + masked latent), so dim_in = 9 — not a multiple of 8, the padded-K
path of project_in and of the 1x1 pre-conv; batch 6, length 37, 11 context tokens, head dim 64; seeds 1500 + 10 * i.
  prepend_v  global conditioning prepended, v objective, input_concat_ids = (inpaint_mask, inpaint_masked_input)
  adaln_rf   adaLN, rectified flow, qk_norm "ln", input_concat_ids = (inpaint_masked_input, inpaint_mask)
LENGTHS are the real (unpadded) latent frames of the six items: a full item, a short one, one frame, none, ...; the recorded masks
are random_inpaint_mask's for the (python seed, mask_kwargs) pairs of MASK_DRAWS — with the default weights seeds 58 and 90 put all
three mask types into the batch."""
import numpy as np
import torch

import seeded

_BASE = dict(io_channels=4, input_concat_dim=5, embed_dim=128, depth=2, num_heads=2, cond_token_dim=64, global_cond_dim=64)
CONFIGS = {
    "prepend_v": dict(_BASE, global_cond_type="prepend"),
    "adaln_rf": dict(_BASE, global_cond_type="adaLN", diffusion_objective="rectified_flow", attn_kwargs={"qk_norm": "ln"}),
}
CONCAT_IDS = {
    "prepend_v": ("inpaint_mask", "inpaint_masked_input"),
    "adaln_rf": ("inpaint_masked_input", "inpaint_mask"),
}
CASES = list(CONFIGS)
BATCH, LENGTH, CTX_LEN = 6, 37, 11
LENGTHS = [37, 19, 1, 0, 37, 25]
MASK_DRAWS = {
    "seed58": (58, {}),
    "seed90": (90, {}),
    "segments3": (7, dict(max_mask_segments=3, mask_type_probabilities=[1.0, 0.0, 0.0])),
    "causal3": (7, dict(max_mask_segments=3, mask_type_probabilities=[0.0, 0.0, 1.0])),
}
COND_DRAW = "seed58"            # the inpaint conditioning of the forward / gradient / sampler fixtures
SAMPLER_STEPS = 3
CFG_SCALE, SCALE_PHI = 6.0, 0.75
NOISE_SEED = 999
TRAIN_STEPS = 2
TRAIN_SEED = 58                 # random.seed before the first train step; the draws of the second step continue the stream
OPT = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-3)


def case_id(i):
    return CASES[i]


def case_seed(i):
    return 1500 + 10 * i


def case_config(i):
    cfg = dict(CONFIGS[CASES[i]])
    if "attn_kwargs" in cfg:
        cfg["attn_kwargs"] = dict(cfg["attn_kwargs"])
    return cfg


def objective(i):
    return CONFIGS[CASES[i]].get("diffusion_objective", "v")


def mask_first(i):
    return CONCAT_IDS[CASES[i]][0] == "inpaint_mask"


def padding_mask():
    """(BATCH, LENGTH) bool: a true prefix of LENGTHS[b] frames per item."""
    return torch.arange(LENGTH)[None, :] < torch.tensor(LENGTHS)[:, None]


def inputs(i, seed=600):
    cfg = CONFIGS[CASES[i]]
    rs = np.random.RandomState(seed)
    return {
        "x": torch.from_numpy(seeded.seeded_array((BATCH, cfg["io_channels"], LENGTH), seed + 1)),
        "t": torch.from_numpy(rs.uniform(0.05, 0.95, size=(BATCH,)).astype(np.float32)),
        "cross_attn_cond": torch.from_numpy(seeded.seeded_array((BATCH, CTX_LEN, cfg["cond_token_dim"]), seed + 2)),
        "global_embed": torch.from_numpy(seeded.seeded_array((BATCH, cfg["global_cond_dim"]), seed + 3)),
    }


def concat_cond(i, x, mask):
    """input_concat_cond (BATCH, 5, LENGTH) of latents x and a (BATCH, 1, LENGTH) float mask, in the case's input_concat_ids order."""
    parts = [mask, x * mask]
    return torch.cat(parts if mask_first(i) else parts[::-1], dim=1)


def train_data(i, step):
    """(latents, noise, timesteps) of train step `step`."""
    shape = (BATCH, CONFIGS[CASES[i]]["io_channels"], LENGTH)
    t = torch.tensor([0.3, 0.8, 0.55, 0.12, 0.91, 0.47]) + 0.05 * step
    return (torch.from_numpy(seeded.seeded_array(shape, 1000 + step)), torch.from_numpy(seeded.seeded_array(shape, 2000 + step)), t)
