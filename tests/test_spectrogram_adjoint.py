"""The discriminator's spectrogram pair (csrc/stft.hip: sat_spec_fwd and its adjoint sat_spec_bwd) against float64 torch: frames by
`unfold`, periodic Hann, torch.fft.rfft / ||w||, real and imaginary parts concatenated on the channel axis (the layout of
SatOps.spec_fwd); the adjoint against float64 autograd of (z * dz).sum() for a random dz.  test_spectrogram_closed_form.py pins the
forward against closed forms; the adjoint was reached through the discriminator only.

sat_spec_bwd writes even and odd workgroups to two planes, so workgroups 0 and 2 share one: every shape here has at least three
workgroups along the frame axis, hop = n/4, n/2 and n, mono and stereo, and a tail of samples that no frame touches (exactly zero
in dx).  Bounds: tests/fp64_bounds.py."""
import pytest
import torch

from fp64_bounds import check, leaf, smax

NI = 2
SHAPES = [(32, 8, 1205, 2), (32, 16, 2439, 1), (64, 64, 4489, 2), (128, 32, 1411, 2), (512, 256, 5637, 2), (1024, 256, 3331, 1),
          (2048, 512, 6733, 2)]
GPU_ONLY = [(256, 64, 256 + 64 * 70 + 9, 2)]
FRAMES = {(32, 8): 147, (32, 16): 151, (64, 64): 70, (128, 32): 41, (512, 256): 21, (1024, 256): 10, (2048, 512): 10, (256, 64): 71}


def _spectrogram(x, n_fft, hop):
    """(NI, C, T) -> (NI, 2C, frames, n_fft/2 + 1) in x's dtype"""
    w = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    spec = torch.fft.rfft(x.unfold(-1, n_fft, hop) * w, dim=-1) / w.square().sum().sqrt()
    return torch.cat([spec.real, spec.imag], dim=1)


def _spec_case(ops, dev, n_fft, hop, t, c, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(NI, c, t, generator=gen)
    frames = (t - n_fft) // hop + 1
    assert frames == FRAMES[(n_fft, hop)] and ops.lib.sat_spec_frames(n_fft, hop, t) == frames
    touched = (frames - 1) * hop + n_fft
    assert touched < t                                            # a tail no frame touches
    dz = torch.randn(NI, 2 * c, frames, n_fft // 2 + 1, generator=gen)
    tag = f"spec[{n_fft}/{hop} T={t} C={c}]"

    z = ops.spec_fwd(x.to(dev), n_fft, hop)
    dx = ops.spec_bwd(dz.to(dev), c, t, n_fft, hop)
    assert dx.shape == x.shape

    def formula(dt):
        xr = leaf(x, dt)
        out = _spectrogram(xr, n_fft, hop)
        (out * dz.to(dt)).sum().backward()
        return out.detach(), xr.grad
    z64, dx64 = formula(torch.float64)
    z32, dx32 = formula(torch.float32)
    check(tag + " fwd", z, z64, z32, smax(z64.abs()))
    check(tag + " bwd", dx, dx64, dx32, smax(dx64.abs()))
    assert torch.equal(dx[..., touched:].cpu(), torch.zeros(NI, c, t - touched))


@pytest.mark.parametrize("shape", SHAPES)
def test_spectrogram_adjoint_sim(emu, shape):
    _spec_case(emu, "cpu", *shape, seed=71)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + GPU_ONLY)
def test_spectrogram_adjoint_gpu(hip, shape):
    _spec_case(hip, "cuda", *shape, seed=72)


def _refusal_case(ops, dev):
    """n_fft 2048 at hop 256: a workgroup's span (3 * 256 + 2048) exceeds twice its stride (4 * 256), three workgroups would write one
    sample — the launcher refuses, the wrapper raises and hands back no tensor."""
    n_fft, hop, t = 2048, 256, 4096
    frames = (t - n_fft) // hop + 1
    x = torch.randn(1, 1, t).to(dev)
    assert ops.spec_fwd(x, n_fft, hop).shape == (1, 2, frames, n_fft // 2 + 1)       # the forward has no such limit
    out = None
    with pytest.raises(RuntimeError, match="hop too small"):
        out = ops.spec_bwd(torch.randn(1, 2, frames, n_fft // 2 + 1).to(dev), 1, t, n_fft, hop)
    assert out is None


def test_spec_bwd_refuses_hop_too_small_sim(emu):
    _refusal_case(emu, "cpu")


@pytest.mark.gpu
def test_spec_bwd_refuses_hop_too_small_gpu(hip):
    _refusal_case(hip, "cuda")
