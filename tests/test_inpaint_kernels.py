"""Kernel-level tests of sat_diffusion_noise_inpaint (csrc/diffusion_step.hip): sat_diffusion_noise plus the inpainting conditioning of
training/diffusion.py:429-438 in the same launch.  CPU: the simulator; `-m gpu`: the gfx950 library.

Everything here is an exact comparison.  noised / targets: torch.equal to ops.diffusion_noise on the same inputs (the same device
functions).  Mask channel: torch.equal to the interval table expanded by a loop written out here.  Masked latent: torch.equal to
torch.where(mask, x * inv_scale, 0) with inv_scale the fp32 value the binding passes (one fp32 product, one select), and +0.0 — not
-0.0 — where the mask is 0.

Shapes (B, C, T): (6, 4, 37) the fixture batch; (2, 3, 37) rows of x (111 floats) and of concat (148 floats) both off 16-byte
alignment; (1, 5, 1030) a vector body with head and tail whose concat rows are aligned differently from the rows of x (T % 4 = 2);
(3, 2, 1) T = 1; GPU only (4, 64, 1024) the train shape, where every store is a 16-byte one.  Each runs with both objectives,
latent_scale 1.0 and 0.37, both channel orders, S = 1 and S = 10, and tables whose items cycle through: no interval (unused rows
only, one of them (5, 5)), the full item, overlapping intervals, an interval ending at T, and a used row after unused ones — the
cycle is rotated from one combination to the next so that a batch of one sees every pattern.

Fused against torch formulation (DiTTrainStep._inpaint_front with ops.dit_step_fused on / off): the concat tensor is bit-equal at
latent_scale 1.0 and 0.5 — the torch arm divides by the scale as the reference does, the kernel multiplies by its fp32 reciprocal,
and the two agree exactly when the scale is a power of two; noised / targets differ by the roundings of torch's own cos / sin:
tests/test_diffusion_step_kernels.py holds the kernel to 2e-6 (|x| / scale + |noise|) of float64, the torch arm is the same five
fp32 roundings, so the two are held to twice that of each other."""
import ctypes

import pytest
import torch

import inpaint_cases as cases

SHAPES = [(6, 4, 37), (2, 3, 37), (1, 5, 1030), (3, 2, 1)]
TRAIN_SHAPE = (4, 64, 1024)
T_VALUES = torch.tensor([0.0, 1.0, 0.37, 0.83, 0.5, 0.21])


def _data(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * 1.3 + 0.2, torch.randn(shape, generator=g)


def _table(b, s, t, roll):
    """(B, S, 2) int32: item r follows pattern (r + roll) % 5 (module docstring); with S = 1 only the first interval of a pattern fits."""
    table = torch.zeros(b, s, 2, dtype=torch.int32)
    for r in range(b):
        kind = (r + roll) % 5
        rows = []
        if kind == 0:
            rows = [(5, 5), (0, 0)]
        elif kind == 1:
            rows = [(0, t)]
        elif kind == 2:
            rows = [(1, t // 2 + 1), (t // 3, t // 2 + 3), (t // 2, t // 2 + 1)]
        elif kind == 3:
            rows = [(max(0, t - 3), t)]
        else:
            rows = [(0, 0)] * (s - 1) + [(0, 1)]
        for k, (lo, hi) in enumerate(rows[:s]):
            table[r, k, 0], table[r, k, 1] = lo, hi
    return table


def _expand(table, t):
    """(B, 1, T) bool, False inside any interval — a plain loop, independent of the library's own expansion."""
    keep = torch.ones(table.shape[0], 1, t, dtype=torch.bool)
    for r in range(table.shape[0]):
        for lo, hi in table[r].tolist():
            for j in range(max(lo, 0), min(hi, t)):
                keep[r, 0, j] = False
    return keep


def _split(concat, c, mask_first):
    return (concat[:, :1], concat[:, 1:]) if mask_first else (concat[:, c:], concat[:, :c])


def _check(ops, dev, shape, x, noise, combo, objective, scale, mask_first, s):
    b, c, t = shape
    tv = torch.roll(T_VALUES, -combo)[:b].clone()
    table = _table(b, s, t, combo)
    keep = _expand(table, t)
    xd, nd, td = x.to(dev), noise.to(dev), tv.to(dev)
    noised, targets, concat = ops.diffusion_noise_inpaint(xd, nd, td, table.to(dev), objective, latent_scale=scale, mask_first=mask_first)
    ref_noised, ref_targets = ops.diffusion_noise(xd, nd, td, objective, latent_scale=scale)
    what = (shape, objective, scale, mask_first, s, combo)
    assert concat.dtype == torch.float32 and tuple(concat.shape) == (b, 1 + c, t), what
    assert torch.equal(noised, ref_noised) and torch.equal(targets, ref_targets), what
    mask, masked = _split(concat.cpu(), c, mask_first)
    assert torch.equal(mask, keep.to(torch.float32)), what
    inv = torch.tensor(1.0 / float(scale), dtype=torch.float32)
    assert torch.equal(masked, torch.where(keep, x * inv, torch.zeros(()))), what
    hole = ~keep.expand(b, c, t)
    assert not bool(torch.signbit(masked[hole]).any()), what
    return int(hole.sum())


def _cases(ops, dev, shapes):
    for si, shape in enumerate(shapes):
        x, noise = _data(shape, 70 + si)
        combo, holes = 0, 0
        for objective in ("v", "rectified_flow"):
            for scale in (1.0, 0.37):
                for mask_first in (True, False):
                    for s in (1, 10):
                        holes += _check(ops, dev, shape, x, noise, combo, objective, scale, mask_first, s)
                        combo += 1
        assert holes > 0
        print(f"inpaint kernel {shape}: {combo} combinations exact, {holes} masked elements in all")


def test_noise_inpaint_simulator(emu):
    _cases(emu, "cpu", SHAPES)


@pytest.mark.gpu
def test_noise_inpaint_gpu(hip):
    _cases(hip, "cuda", SHAPES + [TRAIN_SHAPE])


# ------------------------------------------------------------------------------------------------ non-finite values
def _non_finite(ops, dev):
    """inf / nan inside an inpainted interval: 0 in the masked latent (a select, not a product), still inf / nan in `noised`."""
    for shape in ((2, 3, 37), (1, 5, 1030)):
        b, c, t = shape
        x, noise = _data(shape, 90)
        table = torch.zeros(b, 2, 2, dtype=torch.int32)
        table[:, 1, 0], table[:, 1, 1] = 4, 9
        x[:, :, 5] = float("inf")
        x[:, 0, 7] = float("nan")
        x[:, 1, 8] = float("-inf")
        tv = torch.full((b,), 0.37)
        for mask_first in (True, False):
            noised, _, concat = ops.diffusion_noise_inpaint(x.to(dev), noise.to(dev), tv.to(dev), table.to(dev), "v", mask_first=mask_first)
            mask, masked = _split(concat.cpu(), c, mask_first)
            assert bool(torch.isfinite(masked).all()) and float(masked[:, :, 4:9].abs().sum()) == 0.0
            assert not bool(torch.signbit(masked[:, :, 4:9]).any())
            assert bool(torch.isinf(noised.cpu()[:, :, 5]).all()) and bool(torch.isnan(noised.cpu()[:, 0, 7]).all())
            assert torch.equal(masked[:, :, 9:], x[:, :, 9:]) and torch.equal(masked[:, :, :4], x[:, :, :4])
            assert float(mask[:, :, 4:9].sum()) == 0.0 and float(mask.sum()) == b * (t - 5)


def test_noise_inpaint_non_finite_simulator(emu):
    _non_finite(emu, "cpu")


@pytest.mark.gpu
def test_noise_inpaint_non_finite_gpu(hip):
    _non_finite(hip, "cuda")


# ------------------------------------------------------------------------------------------------ argument validation
def _validation(ops, dev):
    """Bad arguments come back as a status and a message before any launch (null pointers would fault otherwise)."""
    lib, null = ops.lib, ctypes.c_void_p(None)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    name = b"sat_diffusion_noise_inpaint"
    f = lib.sat_diffusion_noise_inpaint
    for bad in ((0, 4, 16), (1, 0, 16), (1, 4, 0), (-1, 4, 16)):
        assert f(*([null] * 7), *bad, 1, 0, 1.0, 1, null) != 0
        assert name in lib.sat_last_error() and b"empty" in lib.sat_last_error()
    assert f(*([p] * 7), 65536, 1, 1, 1, 0, 1.0, 1, null) != 0
    assert name in lib.sat_last_error() and b"B > 65535" in lib.sat_last_error()
    for s in (0, -3):
        assert f(*([p] * 7), 1, 1, 1, s, 0, 1.0, 1, null) != 0
        assert name in lib.sat_last_error() and b"S <= 0" in lib.sat_last_error()
    assert f(*([p] * 7), 1, 1, 1, 257, 0, 1.0, 1, null) != 0
    assert b"S > 256" in lib.sat_last_error()
    assert f(*([p] * 7), 1, 1, 1, 1, 2, 1.0, 1, null) != 0
    assert name in lib.sat_last_error() and b"objective" in lib.sat_last_error()
    for hole in range(7):
        args = [p] * 7
        args[hole] = null
        assert f(*args, 1, 1, 1, 1, 0, 1.0, 1, null) != 0
        assert name in lib.sat_last_error() and b"null" in lib.sat_last_error()
    x, t = torch.zeros(2, 1, 4).to(dev), torch.zeros(2).to(dev)
    seg = torch.zeros(2, 1, 2, dtype=torch.int32).to(dev)
    with pytest.raises(ValueError, match="objective"):
        ops.diffusion_noise_inpaint(x, x, t, seg, "eps")
    for bad in (seg.long(), seg[:1], seg[:, :, :1].contiguous(), seg.reshape(2, 2), torch.zeros(2, 0, 2, dtype=torch.int32).to(dev)):
        with pytest.raises((ValueError, RuntimeError), match="segments|S <= 0"):
            ops.diffusion_noise_inpaint(x, x, t, bad, "v")
    with pytest.raises(ValueError, match="x, noise"):
        ops.diffusion_noise_inpaint(x, x[:1], t, seg, "v")


def test_noise_inpaint_validation_simulator(emu):
    _validation(emu, "cpu")


@pytest.mark.gpu
def test_noise_inpaint_validation_gpu(hip):
    _validation(hip, "cuda")


# ------------------------------------------------------------------------------------------------ fused against the torch formulation
def _fused_against_torch(device):
    from stable_audio_tools_amd import ops as ops_mod
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.training import DiTTrainStep
    o = ops_mod.get_ops()
    assert o.dit_step_fused is True
    shape = (cases.BATCH, 4, cases.LENGTH)
    x, noise = _data(shape, 95)
    tv = T_VALUES.clone()
    table = _table(cases.BATCH, 10, cases.LENGTH, 1)
    try:
        for i in range(len(cases.CASES)):
            model = DiffusionTransformer(**cases.case_config(i)).to(device)
            for scale in (1.0, 0.5):
                stepper = DiTTrainStep(model, inpainting_config={}, input_concat_ids=cases.CONCAT_IDS[cases.case_id(i)], latent_scale=scale,
                                       use_ema=False)
                seen = {}
                for fused in (True, False):
                    o.dit_step_fused = fused
                    seen[fused] = [a.cpu() for a in stepper._inpaint_front(x.to(device), noise.to(device), tv.to(device), table.to(device))]
                assert seen[False][2].dtype == torch.float32
                assert torch.equal(seen[True][2], seen[False][2]), (cases.case_id(i), scale)
                lim = 4e-6 * (x.double().abs() / scale + noise.double().abs())
                for a, b in zip(seen[True][:2], seen[False][:2]):
                    assert float(((a.double() - b.double()).abs() - lim).max()) <= 0.0, (cases.case_id(i), scale)
    finally:
        o.dit_step_fused = True


def test_inpaint_front_fused_matches_torch_simulator(emu_modules):
    _fused_against_torch("cpu")


@pytest.mark.gpu
def test_inpaint_front_fused_matches_torch_gpu(hip):
    _fused_against_torch("cuda")
