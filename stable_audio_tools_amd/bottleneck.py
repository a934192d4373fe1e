"""Bottlenecks on the HIP path (reference: stable_audio_tools/models/bottleneck.py): the VAE bottleneck (:6-23, :105-134) and, for
inference, the dithered-FSQ bottleneck of the transformer autoencoder codec (:22-31, :426-484; models/fsq.py)."""
import torch
from torch import nn

from . import functional as Fn
from . import ops as _ops


class Bottleneck(nn.Module):
    def __init__(self, is_discrete: bool = False):
        super().__init__()
        self.is_discrete = is_discrete

    def encode(self, x, return_info=False, **kwargs):
        raise NotImplementedError

    def decode(self, x):
        raise NotImplementedError


class VAEBottleneck(Bottleneck):
    """encode: (B, 2C, T) -> z = randn*softplus(scale)+1e-4 .. + mean, info['kl'].

    Like the reference it samples on EVERY call, inference included (bottleneck.py:109, :124).  The
    N(0,1) draw comes from ``torch.randn_like`` (same generator the reference uses), or from the
    ``noise=`` kwarg so parity tests can inject it; the arithmetic runs in csrc/elementwise.hip."""

    def __init__(self):
        super().__init__(is_discrete=False)

    def encode(self, x, return_info=False, noise=None, **kwargs):
        info = {}
        c = x.shape[1] // 2
        if noise is None:
            noise = torch.randn_like(x[:, :c])
        z, kl = Fn.VaeSampleFn.apply(x, noise)
        info["kl"] = kl
        if return_info:
            return z, info
        return z

    def decode(self, x):
        return x


class DiscreteBottleneck(Bottleneck):
    """bottleneck.py:22-31"""

    def __init__(self, num_quantizers, codebook_size, tokens_id):
        super().__init__(is_discrete=True)
        self.num_quantizers = num_quantizers
        self.codebook_size = codebook_size
        self.tokens_id = tokens_id

    def decode_tokens(self, codes, **kwargs):
        raise NotImplementedError


class DitheredFSQ(nn.Module):
    """The quantiser of models/fsq.py:26-134 in eval mode, the only mode built: codes = round((tanh(z) + 1) / half_l) * half_l - 1 per
    digit, index = sum of digit * basis per codebook, deterministic (`dither_inference` is stored and, as in the reference, never read;
    the dither and `noise_dropout` act only while training).  The arithmetic is csrc/fsq.hip (ops.fsq_encode / ops.fsq_decode_tokens);
    forward / indices_to_codes keep the reference's token-major shapes and are thin transposing wrappers over those ops —
    DitheredFSQBottleneck calls the ops directly and never transposes.  The three buffers are non-persistent as in the reference: the
    state dict has no keys."""

    def __init__(self, levels, dither_inference=False, num_codebooks=1, noise_dropout=0.5, scale=1.0):
        super().__init__()
        if scale != 1.0:
            raise NotImplementedError("DitheredFSQ(scale != 1.0) is not built (DitheredFSQBottleneck never passes it)")
        self.levels = levels
        _levels = torch.tensor(levels, dtype=torch.int64)
        self.register_buffer("_levels", _levels, persistent=False)
        self.register_buffer("_basis", torch.cumprod(torch.tensor([1] + list(levels[:-1])), dim=0, dtype=torch.int64), persistent=False)
        self.codebook_dim = len(levels)
        self.codebook_size = _levels.prod().item()
        self.num_codebooks = num_codebooks
        self.dim = self.codebook_dim * num_codebooks
        self.dither_inference = dither_inference
        self.scale = scale
        self.register_buffer("half_l", self.scale * 2 / (self._levels - 1), persistent=False)
        self.allowed_dtypes = (torch.float32,)
        self.noise_dropout = noise_dropout

    def _check(self, z, what, training=False):
        if self.training or training:
            raise NotImplementedError(f"{what}: the training branch (dither, noise dropout, straight-through gradient) is not built — "
                                      "call .eval()")
        if torch.is_grad_enabled() and z.requires_grad:
            raise NotImplementedError(f"{what}: inference-only — the straight-through gradient is not built; call it under torch.no_grad()")
        if z.dtype != torch.float32:
            raise NotImplementedError(f"{what}: float32 latents only, got {z.dtype} (the reference's float64 detour is not built)")

    def forward(self, z, skip_tanh=False):
        """z fp32 (B, N, C) -> (codes (B, N, C), indices (B, N, Q))"""
        if skip_tanh:
            raise NotImplementedError("DitheredFSQ.forward(skip_tanh=True) is not built (DitheredFSQBottleneck never passes it)")
        self._check(z, "DitheredFSQ.forward")
        assert z.shape[-1] == self.dim, f"expected dimension of {self.dim} but found dimension of {z.shape[-1]}"
        codes, indices = _ops.get_ops().fsq_encode(z.transpose(1, 2).contiguous(), self.levels, self.num_codebooks)
        return codes.transpose(1, 2).contiguous(), indices

    def indices_to_codes(self, indices):
        """indices (B, N, Q), any integer dtype -> codes fp32 (B, N, C)"""
        assert indices.shape[-1] == self.num_codebooks, \
            f"expected last dimension of {self.num_codebooks} but found last dimension of {indices.shape[-1]}"
        return _ops.get_ops().fsq_decode_tokens(indices.contiguous(), self.levels).transpose(1, 2).contiguous()


class DitheredFSQBottleneck(DiscreteBottleneck):
    """bottleneck.py:426-484, inference only.  encode: latents fp32 (B, C, T) -> quantised latents (B, C, T), with
    info["quantizer_indices"] of shape (B, T, Q) — token-major, as the reference's DitheredFSQBottleneck returns them (its FSQBottleneck
    returns (B, Q, T)).  One launch on the conv stack's layout (ops.fsq_encode), no transpose.  Under autocast the bottleneck still runs
    in fp32: the TAAE's last conv yields fp32 and the op takes nothing else.

    decode_tokens returns (B, C, T).  This deviates from the reference on purpose: there decode_tokens returns indices_to_codes(tokens) as
    (B, T, C) and AudioAutoencoder.decode_tokens hands that to a decoder that expects (B, C, T), so the reference's own path fails unless
    T == C.  The transposed shape is the only usable one, and it is what encode returns."""

    def __init__(self, dim, levels, num_codebooks=1, dither_inference=True, noise_dropout=0.05):
        if isinstance(levels, int):
            codebook_size = levels ** dim
            quantizer_levels = [levels] * dim
        elif isinstance(levels, list):
            if len(levels) != dim:
                raise ValueError(f"Length of levels list ({len(levels)}) must match dim ({dim}).")
            codebook_size = 1
            for level in levels:
                codebook_size *= level
            quantizer_levels = levels
        else:
            raise TypeError("Levels must be either an int or a list of ints.")
        super().__init__(num_quantizers=num_codebooks, codebook_size=codebook_size, tokens_id="quantizer_indices")
        self.quantizer = DitheredFSQ(levels=quantizer_levels, dither_inference=dither_inference, num_codebooks=num_codebooks,
                                     noise_dropout=noise_dropout)

    def norm_std_loss(self, x):
        return (x.std() - 1.0) ** 2

    def encode(self, x, return_info=False):
        q = self.quantizer
        q._check(x, "DitheredFSQBottleneck.encode", self.training)
        codes, indices = _ops.get_ops().fsq_encode(x.contiguous(), q.levels, q.num_codebooks)
        info = {"quantizer_indices": indices}
        if return_info:
            return codes, info
        return codes

    def decode(self, x):
        return x

    def decode_tokens(self, tokens, **kwargs):
        """tokens (B, T, Q) -> latents (B, C, T) (the class docstring says why not the reference's (B, T, C))"""
        q = self.quantizer
        assert tokens.shape[-1] == q.num_codebooks, f"expected last dimension of {q.num_codebooks} but found last dimension of {tokens.shape[-1]}"
        return self.decode(_ops.get_ops().fsq_decode_tokens(tokens.contiguous(), q.levels), **kwargs)
