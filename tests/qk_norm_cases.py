"""The qk_norm fixture cases, shared by tools/gen_golden_qk_norm.py (which writes tests/golden/dit_qknorm_<case>.npz from the
reference's DiffusionTransformer) and the tests: a seeded.DIT_CONFIGS entry with attn_kwargs={"qk_norm": mode}; seeds 900 + 10 * i.
tiny_adaln / tiny_prepend have GQA cross-attention (4 query heads on 1 key / value head)."""
import seeded

CASES = [("tiny_adaln", "ln"), ("tiny_prepend", "l2"), ("small_rf", "ln")]
SAMPLER_STEPS = 3
CFG_SCALE, SCALE_PHI = 6.0, 0.75
NOISE_SEED = 999


def case_id(i):
    name, mode = CASES[i]
    return f"{name}_{mode}"


def case_seed(i):
    return 900 + 10 * i


def case_config(i):
    name, mode = CASES[i]
    return dict(seeded.DIT_CONFIGS[name], attn_kwargs={"qk_norm": mode})
