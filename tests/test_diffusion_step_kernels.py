"""Kernel-level tests of csrc/diffusion_step.hip — sat_diffusion_noise (training/diffusion.py:377-379, :406-420) and the padding-masked
MSE, forward and backward (training/losses/losses.py:76-89) — against float64 torch written out here.  CPU: the simulator; `-m gpu`: the
gfx950 library.

Shapes (B, C, T): (3, 5, 37) odd everything, rows not 16-byte aligned; (2, 64, 1031) several workgroups per row and a real second
reduction stage; (1, 1, 1) a single element; (2, 4, 4096) the aligned vector path.

Bounds.  Noising: |got - ref| <= 2e-6 (|x| / scale + |noise|) elementwise — about five fp32 roundings (2-ulp trig, two products, one sum),
roughly 3e-7 relative, with a sixfold margin.  Loss: 1e-5 relative (fp32 sums of at most 132k squares in 1024 partials); a bf16 `out` is
compared with float64 on the same bf16-rounded values (the widening is exact).  Gradient: golden_util.rel_err < 1e-5 for fp32 and
< 5e-3 for bf16 (one bf16 rounding, the style of bound of tests/test_qk_norm_kernels.py); exactly 0 at masked positions."""
import ctypes
import math

import pytest
import torch

from golden_util import rel_err

SHAPES = [(3, 5, 37), (2, 64, 1031), (1, 1, 1), (2, 4, 4096)]
T_VALUES = torch.tensor([0.0, 1.0, 0.37, 0.83])


def _data(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * 1.3 + 0.2, torch.randn(shape, generator=g)


def _mask(b, t):
    """Row r: all true / a true prefix of ceil(T / 2) (what padding looks like) / true only at the last position, in turn."""
    m = torch.zeros(b, t, dtype=torch.bool)
    for r in range(b):
        if r % 3 == 0:
            m[r] = True
        elif r % 3 == 1:
            m[r, :(t + 1) // 2] = True
        else:
            m[r, -1] = True
    return m


# ------------------------------------------------------------------------------------------------ noising
def _noise_reference(x, noise, t, objective, scale):
    x, noise, t = x.double() / scale, noise.double(), t.double()[:, None, None]
    if objective == "v":
        alpha, sigma = torch.cos(t * math.pi / 2), torch.sin(t * math.pi / 2)
        return x * alpha + noise * sigma, noise * alpha - x * sigma
    return x * (1 - t) + noise * t, noise - x


def _noise_cases(ops, dev):
    for si, shape in enumerate(SHAPES):
        x, noise = _data(shape, 10 + si)
        bound = 2e-6
        for objective in ("v", "rectified_flow", "rf_denoiser"):
            for scale in (1.0, 0.5):
                for roll in (0, 2):
                    t = torch.roll(T_VALUES, -roll)[:shape[0]].clone()
                    got = ops.diffusion_noise(x.to(dev), noise.to(dev), t.to(dev), objective, latent_scale=scale)
                    again = ops.diffusion_noise(x.to(dev), noise.to(dev), t.to(dev), objective, latent_scale=scale)
                    ref = _noise_reference(x, noise, t, objective, scale)
                    lim = bound * (x.double().abs() / scale + noise.double().abs())
                    for name, g, a, r in zip(("noised", "targets"), got, again, ref):
                        assert g.dtype == torch.float32 and tuple(g.shape) == shape
                        assert torch.equal(g, a), (shape, objective, name, "two runs differ")
                        excess = ((g.cpu().double() - r).abs() - lim).max()
                        print(f"noise {shape} {objective} scale {scale} t {t.tolist()} {name}: max(|err| - bound) {float(excess):.3e}")
                        assert float(excess) <= 0.0, (shape, objective, scale, name, float(excess))
    # tensors whose bases are aligned differently: the kernel must fall back to scalar accesses, not fault or misread
    shape = (2, 3, 41)
    n = shape[0] * shape[1] * shape[2]
    x, noise = _data(shape, 99)
    xb = torch.zeros(n + 4)
    xb[1:n + 1] = x.reshape(-1)
    xd = xb.to(dev)[1:n + 1].view(shape)
    t = torch.tensor([0.25, 0.6])
    got = ops.diffusion_noise(xd, noise.to(dev), t.to(dev), "v")
    ref = _noise_reference(x, noise, t, "v", 1.0)
    lim = 2e-6 * (x.double().abs() + noise.double().abs())
    for g, r in zip(got, ref):
        assert float(((g.cpu().double() - r).abs() - lim).max()) <= 0.0


def test_diffusion_noise_simulator(emu):
    _noise_cases(emu, "cpu")


@pytest.mark.gpu
def test_diffusion_noise_gpu(hip):
    _noise_cases(hip, "cuda")


# ------------------------------------------------------------------------------------------------ masked MSE
def _mse_reference(out, targets, mask, gloss):
    """out: the values the kernel reads, as float64.  (loss, count, dout)."""
    b, c, t = out.shape
    sel = torch.ones(b, c, t, dtype=torch.bool) if mask is None else mask[:, None, :].expand(b, c, t)
    diff = out - targets.double()
    count = int(sel.sum())
    loss = (diff[sel] ** 2).sum() / count if count else torch.tensor(float("nan"), dtype=torch.float64)
    dout = torch.where(sel, 2 * diff * gloss / max(count, 1), torch.zeros_like(diff))
    return loss, count, dout


def _mse_cases(ops, dev):
    for si, shape in enumerate(SHAPES):
        b, c, t = shape
        out32, targets = _data(shape, 30 + si)
        for mask in (None, _mask(b, t)):
            md = mask.to(dev) if mask is not None else None
            for dtype, gbar in ((torch.float32, 1e-5), (torch.bfloat16, 5e-3)):
                out = out32.to(dtype)
                od, td = out.to(dev), targets.to(dev)
                res = ops.masked_mse(od, td, md)
                res2 = ops.masked_mse(od, td, md)
                assert torch.equal(res, res2), (shape, dtype, "two forward runs differ")
                for gloss in (1.0, 0.37):
                    ref_loss, ref_count, ref_dout = _mse_reference(out.double(), targets, mask, gloss)
                    gl = torch.tensor(gloss, dtype=torch.float32).to(dev)
                    dout = ops.masked_mse_bwd(od, td, md, res, gl)
                    assert torch.equal(dout, ops.masked_mse_bwd(od, td, md, res, gl)), (shape, dtype, "two backward runs differ")
                    assert dout.dtype == dtype and tuple(dout.shape) == shape
                    loss_err = abs(float(res[0]) - float(ref_loss)) / abs(float(ref_loss))
                    grad_err = rel_err(dout.float().cpu(), ref_dout)
                    print(f"mse {shape} {dtype} mask {mask is not None} gloss {gloss}: loss rel err {loss_err:.3e} count {float(res[1])} "
                          f"dout rel_err {grad_err:.3e}")
                    assert float(res[1]) == ref_count == c * (int(mask.sum()) if mask is not None else b * t)
                    assert loss_err < 1e-5, (shape, dtype, loss_err)
                    assert grad_err < gbar, (shape, dtype, gloss, grad_err)
                    if mask is not None:
                        masked = ~mask[:, None, :].expand(b, c, t)
                        assert float(dout.float().cpu()[masked].abs().sum()) == 0.0 if masked.any() else True
                if mask is not None and (~mask).any():
                    # non-finite values at masked positions are skipped, not multiplied by zero
                    bad = out.clone()
                    hole = (~mask)[:, None, :].expand(b, c, t)
                    bad[hole] = float("inf")
                    bad[..., 0][hole[..., 0]] = float("nan")
                    res_bad = ops.masked_mse(bad.to(dev), td, md)
                    assert torch.equal(res_bad, res) and math.isfinite(float(res_bad[0])), (shape, dtype, res_bad, res)
                    dbad = ops.masked_mse_bwd(bad.to(dev), td, md, res_bad, torch.ones((), dtype=torch.float32).to(dev))
                    assert float(dbad.float().cpu()[hole].abs().sum()) == 0.0 and bool(torch.isfinite(dbad.float()).all())
        # nothing selected: the mean of an empty selection is NaN, the gradient all zero
        none = torch.zeros(b, t, dtype=torch.bool).to(dev)
        res = ops.masked_mse(out32.to(dev), targets.to(dev), none)
        assert math.isnan(float(res[0])) and float(res[1]) == 0.0
        dout = ops.masked_mse_bwd(out32.to(dev), targets.to(dev), none, res, torch.ones((), dtype=torch.float32).to(dev))
        assert float(dout.abs().sum()) == 0.0


def test_masked_mse_simulator(emu):
    _mse_cases(emu, "cpu")


@pytest.mark.gpu
def test_masked_mse_gpu(hip):
    _mse_cases(hip, "cuda")


def _autograd_node(ops, dev):
    """functional.MaskedMSEFn: a 0-d fp32 loss whose backward is the kernel's gradient, scaled by what arrives from above."""
    from stable_audio_tools_amd import functional as fn
    shape = (3, 5, 37)
    out32, targets = _data(shape, 50)
    mask = _mask(3, 37)
    # (B, C, T) as a transposed view of token-major memory: what the DiT hands to the loss
    leaf = out32.transpose(1, 2).contiguous().to(dev).requires_grad_(True)
    loss = fn.masked_mse(leaf.transpose(1, 2), targets.to(dev), mask.to(dev), ops)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * 0.37).backward()
    ref_loss, _, ref_dout = _mse_reference(out32.double(), targets, mask, 0.37)
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-5 * abs(float(ref_loss))
    assert rel_err(leaf.grad.transpose(1, 2).cpu(), ref_dout) < 1e-5


def test_masked_mse_autograd_simulator(emu):
    _autograd_node(emu, "cpu")


@pytest.mark.gpu
def test_masked_mse_autograd_gpu(hip):
    _autograd_node(hip, "cuda")


# ------------------------------------------------------------------------------------------------ argument validation
def _validation(ops):
    """Bad arguments come back as a status and a message before any launch (null pointers would fault otherwise)."""
    lib, null = ops.lib, ctypes.c_void_p(None)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sat_diffusion_noise(null, null, null, null, null, 0, 4, 16, 0, 1.0, null) != 0
    assert b"sat_diffusion_noise" in lib.sat_last_error() and b"empty" in lib.sat_last_error()
    assert lib.sat_diffusion_noise(null, null, null, null, null, -1, 4, 16, 0, 1.0, null) != 0
    assert lib.sat_diffusion_noise(p, p, p, p, p, 1, 1, 1, 2, 1.0, null) != 0
    assert b"objective" in lib.sat_last_error()
    assert lib.sat_diffusion_noise(null, p, p, p, p, 1, 1, 1, 0, 1.0, null) != 0
    assert b"null" in lib.sat_last_error()
    assert lib.sat_masked_mse_fwd(null, p, null, p, p, 1, 1, 1, 0, null) != 0
    assert b"sat_masked_mse_fwd" in lib.sat_last_error() and b"null" in lib.sat_last_error()
    assert lib.sat_masked_mse_fwd(p, p, null, p, p, 0, 1, 1, 0, null) != 0
    assert b"empty" in lib.sat_last_error()
    assert lib.sat_masked_mse_fwd(p, p, null, p, p, 1, 1, 1, 3, null) != 0
    assert b"dtype" in lib.sat_last_error()
    assert lib.sat_masked_mse_bwd(null, p, null, p, p, p, 1, 1, 1, 0, null) != 0
    assert b"sat_masked_mse_bwd" in lib.sat_last_error() and b"null" in lib.sat_last_error()
    assert lib.sat_masked_mse_bwd(p, p, null, p, p, p, 0, 1, 1, 0, null) != 0
    assert lib.sat_masked_mse_nblocks(0, 1, 1) == -1
    assert lib.sat_masked_mse_nblocks(1, 1, 1) == 1 and lib.sat_masked_mse_nblocks(2, 64, 1031) == 256
    with pytest.raises(ValueError, match="objective"):
        ops.diffusion_noise(torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), torch.zeros(1), "eps")


def test_argument_validation_simulator(emu):
    _validation(emu)


@pytest.mark.gpu
def test_argument_validation_gpu(hip):
    _validation(hip)
