"""csrc/ru_k1_bwd.hip's pipelined tile loop (epilogue of tile i - 1 and conversion of tile i in one phase, the matrix work of tile i in
the next, the LDS-DMA two tiles ahead) at the smallest shapes where such a loop can go wrong, in each of the kernel's three output modes,
against float64 autograd of conv1d(snake(h), W2) + b2 — the comparison and tolerances of test_conv_kernels._ru_k1_bwd_case.

Tiles per workgroup follow from sat_ru_k1_bwd_nsplit (one workgroup per CU), on the MI355X's 256 CUs:
  (1, 128, 32)     one tile: prologue and epilogue are the same tile
  (1, 128, 16384)  512 tiles, two per workgroup: nothing is ever issued two tiles ahead
  (1, 128, 32768)  1024 tiles, four per workgroup: every form of the counted wait (first tile, steady state, last two tiles)
  (2, 128, 12320)  770 tiles in ranges of four that cross the batch boundary; the last range is short
The simulator is told it has 8 CUs (sat_emu_set_cu_count), which gives the same tiles per workgroup at 1 / 16 / 32 / 2 x 13 tiles."""
import math

import pytest
import torch
import torch.nn.functional as F

# (B, C, T, seed, tiles per workgroup on 256 CUs)
SHAPES = [(1, 128, 32, 51, 1), (1, 128, 16384, 52, 2), (1, 128, 32768, 53, 4), (2, 128, 12320, 54, 4)]
SIM_CUS = 8
SIM_SHAPES = [(1, 128, 32, 51, 1), (1, 128, 512, 52, 2), (1, 128, 1024, 53, 4), (2, 128, 416, 54, 4)]


def _snake(x, la, lb):
    a = la.exp()[None, :, None]
    b = lb.exp()[None, :, None]
    return x + (1.0 / (b + 1e-9)) * torch.sin(x * a) ** 2


def _planes(em, B, C, T):
    rows = em["rows"]
    hi, lo = em["hi"].view(B, C // 8, rows, 8), em["lo"].view(B, C // 8, rows, 8)
    for pl in (hi, lo):         # rows around the sequence stay as the caller zeroed them
        assert not pl[:, :, :32].any() and not pl[:, :, 32 + T:].any()
    return hi[:, :, 32:32 + T].clone(), lo[:, :, 32:32 + T].clone()


def _case(ops, dev, B, C, T, seed, per):
    gen = torch.Generator().manual_seed(seed)
    dy = torch.randn(B, C, T, generator=gen).to(dev)
    h = torch.randn(B, C, T, generator=gen).to(dev)
    w2 = (torch.randn(C, C, 1, generator=gen) * (.5 / math.sqrt(C / 8))).to(dev)
    a2, b2 = (torch.randn(C, generator=gen) * .3).to(dev), (torch.randn(C, generator=gen) * .3).to(dev)
    assert ops.ru_k1_bwd_ok(B, C, T)
    ns = ops.lib.sat_ru_k1_bwd_nsplit(B, C, T)
    assert -(-(B * T // 32) // ns) == per, (ns, per)

    hd, wd, ad, bd = (t.detach().double().cpu().requires_grad_(True) for t in (h, w2, a2, b2))
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv1d(_snake(hd, ad, bd), wd, bias).backward(dy.double().cpu())
    refs = (hd.grad, ad.grad, bd.grad, wd.grad, bias.grad, hd.grad.sum(dim=(0, 2)))
    names = ("dh", "dalpha", "dbeta", "dW2", "dbias2", "dbias1")

    def check(outs, with_dh):
        for got, ref, name in zip(outs, refs, names):
            if name == "dh" and not with_dh:
                continue
            err = (got.double().cpu() - ref).abs().max().item()
            print(f"{(B, C, T)} {name}: err {err:.3e} max|ref| {ref.abs().max().item():.3e}")
            assert err <= 2e-5 * max(ref.abs().max().item(), 1e-3) + 1e-6 * math.sqrt(B * T), (name, (B, C, T), err, ref.abs().max().item())

    def run(**kw):
        outs = ops.ru_k1_bwd(dy, h, w2, (a2, b2), **kw)
        em = ops._take_emitted(outs[0], None)
        planes = None
        if kw.get("emit"):
            assert em is not None
            planes = _planes(em, B, C, T)
        return [o.clone() for o in outs], planes

    # emit=True: dh, its planes, every sum
    full, pl_full = run(emit=True)
    check(full, True)
    dh = full[0]
    rec = (pl_full[0].view(torch.bfloat16).float() + pl_full[1].view(torch.bfloat16).float()).permute(0, 1, 3, 2).reshape(B, C, T)
    assert (rec - dh).abs().max().item() <= 2.0 ** -15 * dh.abs().max().item()
    # planes only: the same planes, the same sums
    try:
        skip, pl_skip = run(emit=True, skip_dh=True)
    finally:
        ops.dh_written()
    check(skip, False)
    assert torch.equal(pl_skip[0], pl_full[0]) and torch.equal(pl_skip[1], pl_full[1])
    for a, b, name in zip(skip[1:], full[1:], names[1:]):
        assert torch.equal(a, b), name
    # fp32 dh only
    plain, _ = run(emit=False)
    check(plain, True)
    for a, b, name in zip(plain, full, names):
        assert torch.equal(a, b), name
    # two calls on the same inputs agree in every output
    again, pl_again = run(emit=True)
    for a, b, name in zip(again, full, names):
        assert torch.equal(a, b), name
    assert torch.equal(pl_again[0], pl_full[0]) and torch.equal(pl_again[1], pl_full[1])


@pytest.mark.parametrize("shape", SIM_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_ru_k1_bwd_phases_sim(emu, shape):
    emu.lib.sat_emu_set_cu_count(SIM_CUS)
    try:
        _case(emu, "cpu", *shape)
    finally:
        emu.lib.sat_emu_set_cu_count(0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_ru_k1_bwd_phases_gpu(hip, shape):
    _case(hip, "cuda", *shape)
