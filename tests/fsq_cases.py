"""The dithered-FSQ fixture cases, shared by tools/gen_golden_fsq.py (which writes tests/golden/fsq_<case>.npz from the reference's
DitheredFSQ / DitheredFSQBottleneck / AudioAutoencoder) and the tests.  Kernel cases, seeds 1900 + 10 * i, (B, C, T), levels, codebooks:
  one       (1, 1, 1),    [2], 1          a single element, x = 0.3
  l6543x2   (2, 8, 1043), [6, 5, 4, 3], 2 mixed levels, two codebooks, several blocks, T no multiple of 64; also the odd tokens (ODD_TOKENS)
  l17x6     (1, 6, 257),  [17] * 6, 1     the codec configuration's levels
  l23x3     (3, 6, 63),   [2, 3], 3       the smallest levels, three codebooks, T below a wave
  d16       (1, 16, 130), [3] * 16, 1     D at its limit
  sum512    (1, 8, 65),   [64] * 8, 1     sum of the levels at its limit, indices up to 2^48: int64 arithmetic
  offset    (2, 8, 12),   [6, 5, 4, 3], 2 run by the tests at a base address offset by one element
Inputs are 1.5 * N(0, 1); every case with T >= 5 has PLANTED columns for all channels: x = 0 at t = 0 (an exact rounding tie for every
even level count), 20 and -20 (tanh saturates to +-1 exactly) at t = 1, 2, and 9 and -9 (tanh = +-0.99999994) at t = 3, 4.
The codec case is taae_cases' "vae" TAAE shape with encoder and decoder latent_dim 8 around {"type": "dithered_fsq", "config": {"dim": 4,
"levels": [6, 5, 4, 3], "num_codebooks": 2}}, seed 1990, 1040 stereo samples -> 130 latent frames -> (1, 130, 2) tokens."""
import copy

import torch

import seeded
import taae_cases

KERNEL_CASES = {
    "one": ((1, 1, 1), [2], 1),
    "l6543x2": ((2, 8, 1043), [6, 5, 4, 3], 2),
    "l17x6": ((1, 6, 257), [17] * 6, 1),
    "l23x3": ((3, 6, 63), [2, 3], 3),
    "d16": ((1, 16, 130), [3] * 16, 1),
    "sum512": ((1, 8, 65), [64] * 8, 1),
    "offset": ((2, 8, 12), [6, 5, 4, 3], 2),
}
CASES = list(KERNEL_CASES)
PLANTED = (0.0, 20.0, -20.0, 9.0, -9.0)
ODD_CASE = "l6543x2"
ODD_TOKENS = (-1, -361, 360, 2 ** 40, -2 ** 62)
TIE_BAND = 1e-4         # |li64 - floor(li64) - 0.5| below this: the element is near a rounding tie
TIE_SHARE_CAP = 1e-3    # of a case's elements
CODEC_SEED = 1990
CODEC_BAND_CAP = 0.05   # of the codec case's digits inside the band the encoder's error opens around a tie


def case_seed(i):
    return 1900 + 10 * i


def case(i):
    """(shape, levels, num_codebooks)"""
    shape, levels, q = KERNEL_CASES[CASES[i]]
    return shape, list(levels), q


def planted_columns(i):
    return len(PLANTED) if case(i)[0][2] >= len(PLANTED) else 0


def inputs(i):
    """x fp32 (B, C, T)"""
    shape = case(i)[0]
    x = 1.5 * torch.from_numpy(seeded.seeded_array(shape, case_seed(i)))
    if planted_columns(i):
        for t, v in enumerate(PLANTED):
            x[:, :, t] = v
    elif x.numel() == 1:
        x.fill_(0.3)
    return x.contiguous()


def odd_tokens():
    """(1, len(ODD_TOKENS), 2) int64: every odd token in codebook 0, the same list reversed in codebook 1"""
    t = torch.tensor(ODD_TOKENS, dtype=torch.int64)
    return torch.stack([t, t.flip(0)], dim=-1)[None].contiguous()


def basis(levels):
    out, b = [], 1
    for v in levels:
        out.append(b)
        b *= v
    return out


def torch_fsq(x, levels, q):
    """The eval-mode quantiser of the reference (models/fsq.py quantize / _codes_to_indices) restated on (B, C, T) with torch ops on x's
    device: (codes (B, C, T), indices (B, T, Q)).  The tests' reference where no fixture can be stored (the 2^24 + 3 case)."""
    b, c, t = x.shape
    d = len(levels)
    half_l = (1.0 * 2 / (torch.tensor(levels, dtype=torch.int64) - 1)).to(x.device)
    z = torch.tanh(x.transpose(1, 2).reshape(b, t, q, d))
    r = ((z + 1.0) / half_l).round()
    codes = r * half_l - 1.0
    idx = (r.to(torch.int64) * torch.tensor(basis(levels), dtype=torch.int64, device=x.device)).sum(dim=-1)
    return codes.reshape(b, t, c).transpose(1, 2).contiguous(), idx


# ---- the rule the quantiser is held to (tests/test_fsq_kernels.py's docstring derives it) -----------------------------------------------
def _per_channel(levels, c, device, dtype):
    d = len(levels)
    return torch.tensor([levels[ch % d] for ch in range(c)], dtype=dtype, device=device)[None, :, None]


def check_rule(name, x, codes, indices, levels, q, want_codes=None, want_indices=None, planted=0):
    """The rule of the module docstring on x / codes (B, C, T) and indices (B, T, Q); want_*: the reference's output, compared bit for
    bit on the planted columns and away from ties.  Returns the near-tie share."""
    b, c, t = x.shape
    d = len(levels)
    dev = x.device
    assert codes.shape == x.shape and codes.dtype == torch.float32 and indices.shape == (b, t, q) and indices.dtype == torch.int64
    lm1 = _per_channel(levels, c, dev, torch.float64) - 1.0
    li64 = (torch.tanh(x.double()) + 1.0) * lm1 / 2.0
    near = (li64 - li64.floor() - 0.5).abs() < TIE_BAND
    near[:, :, :planted] = False
    share = float(near.sum()) / x.numel()
    print(f"fsq {name}: near-tie share {share:.2e} ({int(near.sum())} of {x.numel()})")
    # the levels, read back from the returned codes; the code must be exactly the host table's entry
    level = ((codes.double() + 1.0) * lm1 / 2.0).round().to(torch.int64)
    assert bool(((level >= 0) & (level <= lm1.to(torch.int64))).all())
    half_l = (1.0 * 2 / (torch.tensor(levels, dtype=torch.int64) - 1)).to(dev)
    table = torch.stack([torch.arange(max(levels), dtype=torch.float32, device=dev) * half_l[ch % d] - 1.0 for ch in range(c)])
    assert torch.equal(torch.gather(table[None].expand(b, -1, -1), 2, level), codes), "a code is not table[d][level]"
    weights = torch.tensor(basis(levels), dtype=torch.int64, device=dev)
    idx = (level.view(b, q, d, t) * weights[None, None, :, None]).sum(dim=2).transpose(1, 2)
    assert torch.equal(idx, indices), "an index is not sum(level * basis) of the returned codes' levels"
    # away from a tie: round(li64); near one: either neighbour
    free = ~near
    free[:, :, :planted] = False
    assert torch.equal(level[free], li64.round().to(torch.int64)[free]), "a level away from a tie is not round(li64)"
    assert bool(((level == li64.floor().to(torch.int64)) | (level == li64.ceil().to(torch.int64)))[near].all())
    if want_codes is not None:
        want_codes, want_indices = want_codes.to(dev), want_indices.to(dev)
        assert torch.equal(codes[:, :, :planted], want_codes[:, :, :planted]) and torch.equal(indices[:, :planted], want_indices[:, :planted]), \
            "planted columns differ from the reference"
        assert torch.equal(codes[free], want_codes[free]), "a code away from a tie differs from the reference"
        free_idx = free.view(b, q, d, t).all(dim=2).transpose(1, 2)      # every digit of the token away from a tie
        assert torch.equal(indices[free_idx], want_indices[free_idx]), "an index away from a tie differs from the reference"
    assert share <= TIE_SHARE_CAP, f"{share:.2e} of the elements lie near a tie: the case no longer pins the quantiser"
    return share


# ---- the codec case --------------------------------------------------------------------------------------------------------------
_VAE = taae_cases.CASES.index("vae")
BOTTLENECK = {"type": "dithered_fsq", "config": {"dim": 4, "levels": [6, 5, 4, 3], "num_codebooks": 2}}


def codec_config(window=True):
    """the model-config JSON of the codec case, as create_autoencoder_from_config takes it"""
    cfg = copy.deepcopy(taae_cases.model_config(_VAE, window))
    cfg["model"]["encoder"]["config"]["latent_dim"] = 8
    cfg["model"]["decoder"]["config"]["latent_dim"] = 8
    cfg["model"]["latent_dim"] = 8
    cfg["model"]["bottleneck"] = copy.deepcopy(BOTTLENECK)
    return cfg


def codec_audio():
    n = taae_cases.LENGTHS["vae"]
    return torch.from_numpy(seeded.seeded_array((1, 2, n), CODEC_SEED + 1, scale=0.5))


def codec_state_dict(model):
    return taae_cases.state_dict(model, CODEC_SEED)
