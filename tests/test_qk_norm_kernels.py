"""Kernel-level tests of the q / k head normalisation (Attention(qk_norm="ln" | "l2"), transformer.py:374-376, :397-403, :485-489):
the standalone forward / backward kernels of csrc/dit_ops.hip against torch written out here (F.layer_norm / F.normalize with fp32
statistics, then dit_oracle.apply_rotary; dx / dgamma / dbeta through autograd), and the fused projection epilogue of csrc/gemm.hip
against fp32 matmul -> norm -> rotary -> bf16 on the same bf16-rounded operands.  CPU: the simulator; `-m gpu`: the gfx950 library.

Bounds: the fp32 kernels are elementwise fp32 ops plus 64-term sums — a few ulp x sqrt(64) ~ 1e-6 — so 1e-5 leaves ten times that;
bf16 storage is compared with the fp32 result of the same bf16-rounded inputs at 1e-2 (about one bf16 ulp of the maximum); the fused
epilogue keeps the 6e-3 of tests/test_gemm_kernels.py's heads-epilogue test (bf16 output rounding).  The 256 x 256 tile has no norm
instantiation (ops.gemm_heads_bf16 picks among 0, 7, 8; the library refuses tile 4)."""
import pytest
import torch
import torch.nn.functional as F

import dit_oracle
from golden_util import rel_err

INV = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))


def _torch_norm(x, mode, g, b):
    """x (..., 64) fp32."""
    if mode == "ln":
        return F.layer_norm(x, (64,), weight=g, bias=b, eps=1e-6)
    return F.normalize(x, dim=-1)


def _reference(x, nh, hq, mode, tabs, freqs):
    """x (B, N, C) fp32 leaf; the first nh heads normalised (+ rotary), the rest passed through."""
    b, n, c = x.shape
    heads = x[..., :nh * 64].unflatten(-1, (nh, 64))
    gq, bq, gk, bk = tabs if tabs is not None else (None,) * 4
    parts = []
    if hq:
        parts.append(_torch_norm(heads[:, :, :hq], mode, gq, bq))
    if hq < nh:
        parts.append(_torch_norm(heads[:, :, hq:], mode, gk, bk))
    y = torch.cat(parts, dim=2)
    if freqs is not None:
        y = dit_oracle.apply_rotary(y.permute(0, 2, 1, 3), freqs).permute(0, 2, 1, 3)
    return torch.cat([y.flatten(2), x[..., nh * 64:]], dim=-1)


def _kernel_case(ops, dev, b, n, nh, hq, extra_heads, mode, rotary, seed=0):
    torch.manual_seed(seed)
    c = (nh + extra_heads) * 64
    x = torch.randn(b, n, c) * 1.7 + 0.3
    tabs = [torch.randn(64) for _ in range(4)] if mode == "ln" else None      # N(0, 1) gammas: near-zero and negative values included
    freqs = dit_oracle.rotary_freqs(INV, n + 3)[-n:] if rotary else None
    cs = ops.rope_tables(INV.to(dev), n + 3) if rotary else None
    w = torch.randn(b, n, c)
    # torch, fp32, autograd
    xr = x.clone().requires_grad_(True)
    tr = [t.clone().requires_grad_(True) for t in tabs] if tabs is not None else None
    yr = _reference(xr, nh, hq, mode, tr, freqs)
    (yr * w).sum().backward()
    tabs_d = [t.to(dev) for t in tabs] if tabs is not None else None
    errs = {}
    for dtype, bar in ((torch.float32, 1e-5), (torch.bfloat16, 1e-2)):
        xd = x.to(dev).to(dtype)
        out = torch.zeros_like(xd)
        y, stat = ops.qk_norm(xd, nh, hq, mode, tabs_d, cs, out=out, save_stats=True)
        y = y.float().cpu()
        if extra_heads:                                                  # columns past the normed heads are not written
            assert float(y[..., nh * 64:].abs().max()) == 0.0
        ref_y = yr.detach()[..., :nh * 64]
        if dtype == torch.bfloat16:      # bf16 storage against the fp32 result of the same (bf16-rounded) input
            ref_y = _reference(x.bfloat16().float(), nh, hq, mode, tabs, freqs)[..., :nh * 64]
        errs[(dtype, "y")] = rel_err(y[..., :nh * 64], ref_y)
        assert errs[(dtype, "y")] < bar, errs
        if dtype == torch.float32:
            dy = w.to(dev).clone()
            grads = ops.qk_norm_bwd_(dy, xd, stat, nh, hq, mode, tabs_d, cs)
            errs["dx"] = rel_err(dy.cpu()[..., :nh * 64], xr.grad[..., :nh * 64])
            assert errs["dx"] < 1e-5, errs
            assert torch.equal(dy.cpu()[..., nh * 64:], w[..., nh * 64:])
            if mode == "ln":
                for i, (got, want) in enumerate(zip(grads, tr)):
                    if (i < 2 and hq == 0) or (i >= 2 and hq == nh):
                        assert got is None
                        continue
                    errs[f"dtab{i}"] = rel_err(got.cpu(), want.grad)
                    assert errs[f"dtab{i}"] < 1e-5, errs
            else:
                assert grads is None
        else:
            dy = w.to(dev).to(dtype)
            grads16 = ops.qk_norm_bwd_(dy, xd, stat, nh, hq, mode, tabs_d, cs)
            x16 = x.bfloat16().float().requires_grad_(True)
            t16 = [t.clone().requires_grad_(True) for t in tabs] if tabs is not None else None
            (_reference(x16, nh, hq, mode, t16, freqs) * w.bfloat16().float()).sum().backward()
            if mode == "ln":     # fp32 sums of fp32 products of the bf16-rounded inputs: the parameter gradients keep the fp32 bar
                for i, (got, want) in enumerate(zip(grads16, t16)):
                    if got is not None:
                        errs[f"dtab16_{i}"] = rel_err(got.cpu(), want.grad)
                        assert errs[f"dtab16_{i}"] < 1e-5, errs
            errs["dx16"] = rel_err(dy.float().cpu()[..., :nh * 64], x16.grad[..., :nh * 64])
            assert errs["dx16"] < 1e-2, errs
    return errs


def _kernel_cases(ops, dev, shapes):
    for mode in ("ln", "l2"):
        for (b, n, h) in shapes["self"]:
            _kernel_case(ops, dev, b, n, 2 * h, h, h, mode, True)           # q and k of a fused (B, N, 3*H*64) projection, rotary
            _kernel_case(ops, dev, b, n, h, h, 0, mode, False)              # to_q of a cross-attention
        for (b, m, hkv) in shapes["cross_k"]:
            _kernel_case(ops, dev, b, m, hkv, 0, hkv, mode, False)          # the k half of (B, M, 2*Hkv*64)
            _kernel_case(ops, dev, b, m, hkv, 0, hkv, mode, True)


def test_qk_norm_kernels_simulator(emu):
    _kernel_cases(emu, "cpu", {"self": [(2, 37, 4)], "cross_k": [(2, 37, 1)]})


@pytest.mark.gpu
def test_qk_norm_kernels_gpu(hip):
    _kernel_cases(hip, "cuda", {"self": [(2, 1025, 24)], "cross_k": [(2, 130, 12)]})


def _heads_case(ops, dev, nb, ntok, heads, k, tiles=(0, 7, 8, None)):
    """As tests/test_gemm_kernels.py::_heads_case, with the norm between projection and rotary (None: the tile the cost model picks)."""
    torch.manual_seed(1)
    x = torch.randn(nb * ntok, k).bfloat16().to(dev)
    w = (torch.randn(3 * heads * 64, k) / k ** 0.5).bfloat16().to(dev)
    cs = ops.rope_tables(INV.to(dev), ntok + 3)
    freqs = dit_oracle.rotary_freqs(INV, ntok + 3)[-ntok:]
    qkv = (x.float().cpu() @ w.float().cpu().t()).view(nb, ntok, 3, heads, 64)
    q, kk, v = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    tabs = [torch.randn(64) for _ in range(4)]
    tabs_d = [t.to(dev) for t in tabs]
    for mode in ("ln", "l2"):
        qn, kn = _torch_norm(q, mode, tabs[0], tabs[1]), _torch_norm(kk, mode, tabs[2], tabs[3])
        qr, kr = dit_oracle.apply_rotary(qn, freqs), dit_oracle.apply_rotary(kn, freqs)
        for tile in tiles:
            ops.gemm_tile = tile
            try:
                plain = ops.gemm_heads_bf16(x, w, cs, heads, nb, ntok, 0, 3)
                pl = ops.gemm_heads_bf16(x, w, cs, heads, nb, ntok, 0, 3, qk_norm=mode, norm_tables=tabs_d)
                qp, kp = [pl[n].view(torch.bfloat16).float().cpu() for n in ("q", "k")]
                eq, ek = rel_err(qp[:, :, :ntok], qr.bfloat16().float()), rel_err(kp[:, :, :ntok], kr.bfloat16().float())
                assert eq < 6e-3 and ek < 6e-3, (mode, tile, eq, ek)
                assert float(qp[:, :, ntok:].abs().max()) == 0.0 and float(kp[:, :, ntok:].abs().max()) == 0.0
                assert torch.equal(pl["v_tr"], plain["v_tr"])                       # v never sees the norm
                # cross-attention projections: q only / k + v of a context, no rotary
                pq = ops.gemm_heads_bf16(x, w[:heads * 64], None, heads, nb, ntok, 0, 1, qk_norm=mode, norm_tables=tabs_d)
                assert rel_err(pq["q"].view(torch.bfloat16).float().cpu()[:, :, :ntok], qn.bfloat16().float()) < 6e-3
                pkv = ops.gemm_heads_bf16(x, w[heads * 64:], None, heads, nb, ntok, 1, 2, qk_norm=mode, norm_tables=tabs_d)
                assert rel_err(pkv["k"].view(torch.bfloat16).float().cpu()[:, :, :ntok], kn.bfloat16().float()) < 6e-3
                assert torch.equal(pkv["v_tr"], plain["v_tr"])
            finally:
                ops.gemm_tile = None


def test_qk_norm_heads_epilogue_simulator(emu):
    _heads_case(emu, "cpu", 2, 71, 3, 72)
    _heads_case(emu, "cpu", 2, 70, 2, 136, tiles=(7, 8))


@pytest.mark.gpu
def test_qk_norm_heads_epilogue_gpu(hip):
    _heads_case(hip, "cuda", 2, 71, 3, 72)
    _heads_case(hip, "cuda", 2, 1025, 24, 1536)
