"""The head dim 128 fixture cases, shared by tools/gen_golden_head_dim128.py (which writes tests/golden/dit_hd128_<case>.npz from the
reference's DiffusionTransformer) and the tests.  Every case has dim_heads = embed_dim // num_heads = 128 and a rotary of 32
frequencies (RotaryEmbedding(max(128 // 2, 32)): the first 64 of the 128 dims are rotated); seeds 1300 + 10 * i.
tiny_adaln_ln is the Stable-Audio-Open-Small style: adaLN, qk_norm "ln", grouped-query cross-attention (2 query heads on the 1
key / value head of the unprojected 128-wide context); the other two cross-attend on 2 key / value heads.
inputs() builds what oracle/gen_golden.py::dit_inputs builds (batch 2, length 37, 11 context tokens, seed 600) for these configs."""
import numpy as np
import torch

import seeded

CONFIGS = {
    "tiny_adaln_ln": dict(io_channels=4, embed_dim=256, depth=4, num_heads=2, cond_token_dim=128, global_cond_dim=64,
                          project_cond_tokens=False, global_cond_type="adaLN", attn_kwargs={"qk_norm": "ln"}),
    "tiny_prepend": dict(io_channels=4, embed_dim=256, depth=4, num_heads=2, cond_token_dim=64, global_cond_dim=64,
                         project_cond_tokens=True, global_cond_type="prepend"),
    "small_rf_l2": dict(io_channels=6, embed_dim=256, depth=2, num_heads=2, cond_token_dim=48, global_cond_dim=32,
                        prepend_cond_dim=24, project_cond_tokens=True, global_cond_type="prepend",
                        diffusion_objective="rectified_flow", attn_kwargs={"qk_norm": "l2"}),
}
CASES = list(CONFIGS)
SAMPLER_STEPS = 3
CFG_SCALE, SCALE_PHI = 6.0, 0.75


def case_id(i):
    return CASES[i]


def case_seed(i):
    return 1300 + 10 * i


def case_config(i):
    cfg = dict(CONFIGS[CASES[i]])
    if "attn_kwargs" in cfg:
        cfg["attn_kwargs"] = dict(cfg["attn_kwargs"])
    return cfg


def inputs(i, batch=2, length=37, ctx_len=11, seed=600):
    cfg = CONFIGS[CASES[i]]
    rs = np.random.RandomState(seed)
    out = {
        "x": torch.from_numpy(seeded.seeded_array((batch, cfg["io_channels"], length), seed + 1)),
        "t": torch.from_numpy(rs.uniform(0.05, 0.95, size=(batch,)).astype(np.float32)),
        "cross_attn_cond": torch.from_numpy(seeded.seeded_array((batch, ctx_len, cfg["cond_token_dim"]), seed + 2)),
        "global_embed": torch.from_numpy(seeded.seeded_array((batch, cfg["global_cond_dim"]), seed + 3)),
    }
    if cfg.get("prepend_cond_dim", 0) > 0:
        out["prepend_cond"] = torch.from_numpy(seeded.seeded_array((batch, 3, cfg["prepend_cond_dim"]), seed + 4))
        out["prepend_cond_mask"] = torch.ones(batch, 3, dtype=torch.bool)      # the reference concatenates prepend masks unconditionally
    return out
