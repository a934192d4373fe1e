"""The plain C entry points sat_attn_prepare and sat_qk_norm_fwd against their head-dim forms at 64.  The Python side calls only
sat_attn_prepare_hd / sat_qk_norm_fwd_hd (ops.attn_planes, ops.qk_norm), so nothing else reaches the plain names of the C ABI: each
is called here next to its `_hd(..., 64, ...)` form on the same input, and every output must be bit-equal.  CPU: the simulator build;
`-m gpu`: the gfx950 library."""
import itertools

import pytest
import torch

from stable_audio_tools_amd.ops import _ptr

D = 64
INV = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))      # RotaryEmbedding(max(64 // 2, 32)): 16 frequencies


def _prepare_pair(ops, dev):
    b, h, n = 2, 3, 70                      # a ragged last tile (70 = 64 + 6) and, with Np = 192, a tile of padding alone
    npad = 192
    torch.manual_seed(11)
    src = (torch.randn(b, n, h, D) * 3.0).to(dev).permute(0, 2, 1, 3)      # (B, H, N, 64) view of (B, N, H, 64) storage
    assert not src.is_contiguous()
    for dtype, (row_major, transposed) in itertools.product((torch.float32, torch.bfloat16), ((True, True), (True, False), (False, True))):
        t = src.to(dtype)
        dt = 0 if dtype == torch.float32 else 1
        outs = []
        for hd_form in (False, True):
            def alloc(shape, want):         # a sentinel no kernel writes: an element left alone shows up in both comparisons below
                return torch.full(shape, 0x7fc1, dtype=torch.int16, device=dev) if want else None
            pl = [alloc((b, h, npad, D), row_major), alloc((b, h, npad, D), row_major and dt == 0),
                  alloc((b, h, D, npad), transposed), alloc((b, h, D, npad), transposed and dt == 0)]
            head = (_ptr(t), t.stride(0), t.stride(1), t.stride(2), *(_ptr(p) for p in pl), b, h, n, npad)
            if hd_form:
                rc = ops.lib.sat_attn_prepare_hd(*head, D, dt, ops._stream(t))
            else:
                rc = ops.lib.sat_attn_prepare(*head, dt, ops._stream(t))
            assert rc == 0, ops.lib.sat_last_error()
            outs.append(pl)
        for plain, hd in zip(*outs):
            assert (plain is None) == (hd is None)
            if plain is not None:
                assert torch.equal(plain, hd), (dtype, row_major, transposed)
                assert not bool((plain == 0x7fc1).any())      # every element written, the padding rows included


def _qk_norm_pair(ops, dev):
    n, nh, hq = 5, 4, 2
    torch.manual_seed(12)
    x32 = (torch.randn(1, n, nh * D) * 1.7 + 0.3).to(dev)
    tabs = [torch.randn(D).to(dev) for _ in range(4)]
    cs_tab = ops.rope_tables(INV.to(dev), n)
    for dtype, (mode, code), cs in itertools.product((torch.float32, torch.bfloat16), (("ln", 1), ("l2", 2)), (cs_tab, None)):
        x = x32.to(dtype)
        dt = 0 if dtype == torch.float32 else 1
        g = [_ptr(t) for t in tabs] if mode == "ln" else [None] * 4
        outs = []
        for hd_form in (False, True):
            y = torch.full_like(x, 7.0)
            stat = torch.full((2 if code == 1 else 1, n * nh), 7.0, device=dev)
            head = (_ptr(x), x.stride(1), _ptr(y), y.stride(1), *g, _ptr(cs), 0, _ptr(stat), n, n, nh, hq, code, 1e-6)
            if hd_form:
                rc = ops.lib.sat_qk_norm_fwd_hd(*head, D, dt, ops._stream(x))
            else:
                rc = ops.lib.sat_qk_norm_fwd(*head, dt, ops._stream(x))
            assert rc == 0, ops.lib.sat_last_error()
            outs.append((y, stat))
        (y0, s0), (y1, s1) = outs
        assert torch.equal(y0, y1) and torch.equal(s0, s1), (dtype, mode, cs is not None)
        assert not bool((y0 == 7.0).any()) and not bool((s0 == 7.0).any())      # every row and every statistic written


def test_plain_entry_points_match_hd64_sim(emu):
    _prepare_pair(emu, "cpu")
    _qk_norm_pair(emu, "cpu")


@pytest.mark.gpu
def test_plain_entry_points_match_hd64_gpu(hip):
    _prepare_pair(hip, "cuda")
    _qk_norm_pair(hip, "cuda")
