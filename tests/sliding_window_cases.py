"""The sliding-window fixture cases, shared by tools/gen_golden_sliding_window.py (which writes tests/golden/dit_window_<case>.npz from
the reference's DiffusionTransformer) and the tests.  Each is a tiny DiT with ContinuousTransformer(sliding_window=[left, right]) on
every layer's self-attention; seeds 1500 + 10 * i.
  hd64_prepend_cross   head dim 64, the global embedding prepended as a token, grouped-query cross-attention, 70 latent frames (71
                       positions: two key tiles), window [5, 6];
  hd128_adaln_ln       head dim 128, adaLN, qk_norm "ln", 130 frames (three key tiles, two workgroups), window [31, 32];
  hd64_right           head dim 64, prepend conditioning tokens, 37 frames, window [-1, 8]: unbounded to the left.
Prepended tokens are ordinary sequence positions of the window, as in the reference.
inputs() builds what oracle/gen_golden.py::dit_inputs builds (batch 2, 11 context tokens, seed 700) at each case's length."""
import numpy as np
import torch

import seeded

CONFIGS = {
    "hd64_prepend_cross": dict(io_channels=4, embed_dim=256, depth=3, num_heads=4, cond_token_dim=64, global_cond_dim=64,
                               project_cond_tokens=False, global_cond_type="prepend", sliding_window=[5, 6]),
    "hd128_adaln_ln": dict(io_channels=4, embed_dim=256, depth=3, num_heads=2, cond_token_dim=128, global_cond_dim=64,
                           project_cond_tokens=False, global_cond_type="adaLN", attn_kwargs={"qk_norm": "ln"}, sliding_window=[31, 32]),
    "hd64_right": dict(io_channels=6, embed_dim=128, depth=2, num_heads=2, cond_token_dim=48, global_cond_dim=32,
                       prepend_cond_dim=24, project_cond_tokens=True, global_cond_type="prepend", sliding_window=[-1, 8]),
}
LENGTHS = {"hd64_prepend_cross": 70, "hd128_adaln_ln": 130, "hd64_right": 37}
CASES = list(CONFIGS)
SAMPLER_STEPS = 3
CFG_SCALE, SCALE_PHI = 6.0, 0.75


def case_id(i):
    return CASES[i]


def case_seed(i):
    return 1500 + 10 * i


def case_config(i, window=True):
    """the DiffusionTransformer kwargs; window=False: the same model without the window"""
    cfg = dict(CONFIGS[CASES[i]])
    if "attn_kwargs" in cfg:
        cfg["attn_kwargs"] = dict(cfg["attn_kwargs"])
    cfg["sliding_window"] = list(cfg["sliding_window"])
    if not window:
        del cfg["sliding_window"]
    return cfg


def inputs(i, batch=2, ctx_len=11, seed=700):
    cfg = CONFIGS[CASES[i]]
    length = LENGTHS[CASES[i]]
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
