"""The variants of the planes weight gradient (csrc/conv_wgrad7_planes.h, sat_conv_wgrad7_planes_v): 2 = 16x16x32 MFMAs (the shipped form),
0 = 32x32x16 (the A/B arm).  Integer data is exact for every variant (any fragment, tap or store-map error shows); random data with
SnakeBeta stays within twice the pipelined fp32 kernel's own relative L2 error against the float64 formula (the bound of
test_wgrad7_planes.py).  Shapes: the smallest at which each mechanism can go wrong (_CASES).  The variants whose LDS-DMA pieces sat between
the MFMAs (1, 3) did not ship: nothing is left to be bit-identical to, and the entry refuses them."""
import ctypes
import functools

import pytest
import torch

from test_wgrad7_planes import _p, _planes, _ref64, _rel, _snake64

VARIANTS = (0, 2)
# (C, T, B, dil)
_CASES = [(64, 64, 2, 1),        # one stage, half-empty co tile, rows past M
          (128, 200, 2, 3),      # two ci tiles, ragged last stage
          (64, 448, 2, 9),       # halo in the second act piece
          (256, 4160, 2, 1),     # 130 stages over 8 tiles: 44 splits of three stages (the double buffer is re-used), the last split has one
          (256, 4160, 2, 9)]     # stage, a batch boundary falls inside a split
_BIG_T = 4160


@functools.lru_cache(maxsize=None)
def _inputs(c, t, bsz, dil, integer):
    """CPU inputs and the float64 reference of one case, computed once and shared (never modified)."""
    g = torch.Generator().manual_seed(c + t + dil)
    if integer:
        dy = torch.randint(-3, 4, (bsz, c, t), generator=g).float()
        x = torch.randint(-3, 4, (bsz, c, t), generator=g).float()
        snake, act64 = None, x.double()
    else:
        dy = torch.randn(bsz, c, t, generator=g)
        x = torch.randn(bsz, c, t, generator=g)
        snake = (0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g))
        act64 = _snake64(x, *snake)
    return dy, x, snake, _ref64(dy, act64, dil, 3 * dil)


def _slabs(ops, dyp, actp, bsz, c, t, dil, variant):
    saved = ops.wgrad7_planes_variant
    try:
        ops.wgrad7_planes_variant = variant
        return ops.conv_wgrad7_planes(dyp, actp, bsz, c, c, t, dil, 3 * dil, raw=True)
    finally:
        ops.wgrad7_planes_variant = saved


def _case(ops, dev, c, t, bsz, dil, variants):
    if t == _BIG_T:
        assert ops.lib.sat_conv_wgrad7_planes_nsplit(bsz, c, c, t) == 44
    for integer in (True, False):
        dy, x, snake, ref = _inputs(c, t, bsz, dil, integer)
        dy, x = dy.to(dev), x.to(dev)
        sn = None if snake is None else (snake[0].to(dev), snake[1].to(dev))
        dyp, actp = _planes(ops, dy, None), _planes(ops, x, sn)
        assert ops.conv_wgrad7_planes_ok(bsz, c, c, t, dil, 3 * dil, dyp[2], actp[2])
        e_old = None if integer else _rel(ops.conv_wgrad7_bf16x3(dy, x, dil, 3 * dil, snake=sn), ref)
        for v in variants:
            new = _slabs(ops, dyp, actp, bsz, c, t, dil, v).reduce(ops)
            if integer:
                assert torch.equal(new.double().cpu(), ref), f"variant {v}: integer data must be exact (C={c}, T={t}, dil={dil})"
            else:
                e_new = _rel(new, ref)
                print(f"wgrad7 variant {v} C={c} T={t} dil={dil} B={bsz}: rel L2 vs float64  pipelined {e_old:.3e}  planes {e_new:.3e}")
                assert e_new <= 2 * e_old, f"variant {v}: {e_new:.3e} > 2 x pipelined kernel {e_old:.3e} (C={c}, T={t}, dil={dil})"


@pytest.mark.parametrize("c,t,bsz,dil", _CASES)
def test_wgrad7_planes_variants_sim(emu, c, t, bsz, dil):
    # the 130-stage case takes the simulator about 30 s per launch: the shipped variant alone there, every variant on the GPU
    _case(emu, "cpu", c, t, bsz, dil, (2,) if t == _BIG_T else VARIANTS)


@pytest.mark.gpu
@pytest.mark.parametrize("c,t,bsz,dil", _CASES)
def test_wgrad7_planes_variants_gpu(hip, c, t, bsz, dil):
    _case(hip, "cuda", c, t, bsz, dil, VARIANTS)


def test_wgrad7_planes_variant_out_of_range(emu):
    """A variant outside 0 .. 3, or one of the two that did not ship, is refused before anything is launched: the output stays untouched."""
    c, t, dil = 64, 64, 1
    dy, x, _, _ = _inputs(c, t, 2, dil, True)
    dyp, actp = _planes(emu, dy, None), _planes(emu, x, None)
    nsplit = emu.lib.sat_conv_wgrad7_planes_nsplit(2, c, c, t)
    out = torch.full((nsplit, c * c * 7), -1.0)
    for v in (-1, 4, 1, 3):
        assert emu.lib.sat_conv_wgrad7_planes_v(_p(dyp[0]), _p(dyp[1]), dyp[2], _p(actp[0]), _p(actp[1]), actp[2], _p(out), c, 1, c * c,
                                                2, c, c, t, dil, 3 * dil, v, None) != 0
        assert bool((out == -1.0).all())
    assert emu.lib.sat_conv_wgrad7_planes_v(_p(dyp[0]), _p(dyp[1]), dyp[2], _p(actp[0]), _p(actp[1]), actp[2], _p(out), c, 1, c * c,
                                            2, c, c, t, dil, 3 * dil, 2, None) == 0
    assert not bool((out == -1.0).all())
