"""The bounds of the kernel-against-float64 tests (test_dit_pointwise_kernels, test_vae_sample_kernels, test_spectrogram_adjoint, the
FIR cases of test_stft_parity).  No bound here comes from running a kernel:

  fp32 outputs   scaled absolute error  max |got - ref64| / S,  S = the largest, over the output, of the sum of the magnitudes of the
                 terms that form an entry (the caller computes it in float64).  Bound: FACTOR x the same measure of the SAME formula
                 evaluated with ordinary torch float32 ops on the CPU, on the same inputs.  The factor covers the kernel's different
                 operation order and the device's expf / logf / log1pf / sincos, each a few ulp from torch's.
  bf16 outputs   the kernels compute in fp32 and round once: element-wise  |got - ref64| <= 2^-8 |ref64| + (the fp32 allowance) x S.
                 A second rounding or a truncating conversion (2^-7) does not fit.

Every check prints its two figures (torch-fp32, kernel) before it asserts: `pytest -s` shows them."""
import torch

FACTOR = 4.0
BF16_HALF_ULP = 2.0 ** -8


def f64(t):
    return t.detach().cpu().double()


def leaf(t, dtype):
    """an autograd leaf holding t's values in `dtype` (never t itself)"""
    return t.detach().to(dtype).clone().requires_grad_(True)


def smax(t):
    """S from a float64 tensor of per-entry term-magnitude sums."""
    s = float(t.max())
    assert s > 0.0 and s == s
    return s


def check(name, got, ref64, f32, s):
    """got: the kernel's output (fp32 or bf16, any device); ref64: float64 reference; f32: the formula in torch float32; s: the scale S."""
    assert got.shape == ref64.shape == f32.shape, (name, got.shape, ref64.shape, f32.shape)
    assert f32.dtype == torch.float32 and ref64.dtype == torch.float64
    assert bool(torch.isfinite(f64(got)).all()), name
    e32 = float((f64(f32) - ref64).abs().max()) / s
    diff = (f64(got) - ref64).abs()
    ek = float(diff.max()) / s
    leg = "gpu" if got.is_cuda else "sim"
    print(f"FIGURE {name} {leg} {str(got.dtype)[6:]}: torch-fp32 {e32:.3e}  kernel {ek:.3e}  (S = {s:.3e})")
    if got.dtype == torch.float32:
        assert ek <= FACTOR * e32, f"{name}: kernel {ek:.3e} of S against {FACTOR:g} x torch-fp32 {e32:.3e} (S = {s:.3e})"
    else:
        assert got.dtype == torch.bfloat16
        excess = float((diff - BF16_HALF_ULP * ref64.abs()).max()) / s
        assert excess <= FACTOR * e32, (f"{name}: bf16 error exceeds 2^-8 |ref| by {excess:.3e} of S; allowance {FACTOR:g} x torch-fp32 "
                                        f"{e32:.3e} (S = {s:.3e})")
    return e32, ek
