"""The VAE bottleneck kernels (csrc/elementwise.hip: sat_vae_sample_fwd / _bwd) on their own against float64 torch of the reference's
vae_sample (models/bottleneck.py: stdev = softplus(scale) + 1e-4, z = noise * stdev + mean, kl = (mean^2 + var - log var - 1).sum(1).mean()).
The whole-model tests mix the KL gradient into a decoder gradient at weight 0.1 or 1e-4; here it is checked alone as well.
Shapes: a small odd one, and one past the 1024 x 256 threads of the capped grid (the stride loop; > 1024 KL partials would not fit either).
Scale-channel values on both sides of softplus's threshold (20) and at the tiny-stdev end are planted.  Bounds: tests/fp64_bounds.py."""
import pytest
import torch
import torch.nn.functional as F

from fp64_bounds import check, leaf, smax

SHAPES = [(2, 3, 37), (1, 4, 65603)]
PLANTED_SCALES = (25.0, 20.01, 20.0, 19.99, 0.0, -30.0)
LEGS = [("both", True, 0.7), ("kl_only", False, 1.0), ("dz_only", True, None)]     # (name, with dz, dkl)


def _sample(pre, noise):
    c = pre.shape[1] // 2
    mean, scale = pre[:, :c], pre[:, c:]
    stdev = F.softplus(scale) + 1e-4
    var = stdev * stdev
    z = noise * stdev + mean
    kl_terms = mean * mean + var - torch.log(var) - 1
    return z, kl_terms.sum(1).mean(), kl_terms, stdev


def _vae_case(ops, dev, b, c, t, seed):
    gen = torch.Generator().manual_seed(seed)
    pre = torch.randn(b, 2 * c, t, generator=gen)
    pre[:, c:] *= 2.0
    flat = pre[0, c]                                              # first scale channel: start, and (long shape) the stride-loop end
    for i, v in enumerate(PLANTED_SCALES):
        flat[2 + 3 * i] = v
        pre[b - 1, 2 * c - 1, t - 1 - 4 * i] = v
    noise = torch.randn(b, c, t, generator=gen)
    dz = torch.randn(b, c, t, generator=gen)
    tag = f"vae[{b}x{c}x{t}]"

    z, kl = ops.vae_sample_fwd(pre.to(dev), noise.to(dev))
    assert z.shape == (b, c, t) and kl.shape == ()
    z64, kl64, terms64, std64 = _sample(pre.double(), noise.double())
    z32, kl32, _, _ = _sample(pre, noise)
    check(tag + " z", z, z64, z32, smax((noise.double() * std64).abs() + pre[:, :c].double().abs()))
    check(tag + " kl", kl, kl64, kl32, float(terms64.abs().sum()) / (b * t))

    for name, with_dz, w in LEGS:
        dkl = None if w is None else torch.tensor(w, dtype=torch.float32)
        dpre = ops.vae_sample_bwd(pre.to(dev), noise.to(dev), dz.to(dev) if with_dz else None, dkl.to(dev) if dkl is not None else None)
        assert dpre.shape == pre.shape

        def formula(dt):
            p = leaf(pre, dt)
            zz, kk, _, _ = _sample(p, noise.to(dt))
            loss = (zz * dz.to(dt)).sum() * (1.0 if with_dz else 0.0) + (w if w is not None else 0.0) * kk
            loss.backward()
            return p.grad
        g64, g32 = formula(torch.float64), formula(torch.float32)
        gkl = (w if w is not None else 0.0) / (b * t)
        d = dz.double() if with_dz else torch.zeros(b, c, t, dtype=torch.float64)
        sig = torch.sigmoid(pre[:, c:].double())
        s_mean = smax(d.abs() + abs(gkl) * 2 * pre[:, :c].double().abs())
        s_scale = smax(((d * noise.double()).abs() + abs(gkl) * (2 * std64 + 2 / std64)) * sig)
        check(f"{tag} {name} d_mean", dpre[:, :c], g64[:, :c], g32[:, :c], s_mean)
        check(f"{tag} {name} d_scale", dpre[:, c:], g64[:, c:], g32[:, c:], s_scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_vae_sample_sim(emu, shape):
    _vae_case(emu, "cpu", *shape, seed=61)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_vae_sample_gpu(hip, shape):
    _vae_case(hip, "cuda", *shape, seed=62)


def test_large_shape_reaches_the_stride_loop(emu):
    b, c, t = SHAPES[1]
    assert b * c * t > 1024 * 256 and emu.lib.sat_vae_nblocks(b * c * t) == 1024
