"""Kernel-level tests of the head dim 128 inference path (the D = 128 instantiations of sat_attn_fwd_kernel / sat_attn_prepare_kernel in csrc/attention.hip, sat_qk_norm_fwd_hd in csrc/dit_ops.hip): the forward
attention in fp32 (two bf16 planes) and bf16, the plane preparation, the 128-wide q / k normalisation with its rotary, and the argument
validation of the two new entry points.  CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library.

Bounds.  Attention output: the project's own (tests/test_dit_kernels.py): max abs error <= 2e-4 (fp32) / 3e-2 (bf16) x max(|ref|max,
1e-2) against F.scaled_dot_product_attention in fp32 on the same (bf16-rounded, for bf16) inputs, scale 128 ** -0.5.  LSE against
torch.logsumexp of the fp64 scaled scores: fp32 <= 2e-4 x max(|lse|, 1); bf16 <= 3e-2 absolute — the worst case of one extra bf16
rounding (2^-9 relative) of the pre-scaled Q over 128 unit-variance products; the deferred-max case, whose spiked keys are not
unit-variance, takes the same derivation with its rows' own magnitudes (_attn_case).  qk_norm: the bars tests/test_qk_norm_kernels.py holds
the 64-wide kernel to (rel-L2 1e-5 in fp32, 1e-2 for bf16 storage), against F.layer_norm / F.normalize and the rotation formula in
fp64.  Planes: hi + lo reproduces an fp32 source to 2^-16 relative (two bf16 roundings: 2^-9 x 2^-9 = 2^-18, with room)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from golden_util import rel_err
from test_dit_kernels import SPIKES

D = 128
SCALE = D ** -0.5
# (B, H, Hkv, Nq, Nk): the tile edges, the peeled first tile, a ragged last tile with <= 32 and > 32 keys, fewer than 64 keys in all, GQA
ATT_CASES = [(1, 2, 2, 64, 64), (2, 2, 2, 65, 65), (1, 4, 2, 130, 37), (1, 2, 1, 37, 200), (1, 2, 2, 193, 193), (1, 4, 4, 1, 70),
             (1, 2, 1, 70, 257), (1, 2, 2, 20, 20)]
GPU_CASES = [(2, 8, 8, 1025, 1025), (2, 8, 8, 1025, 130)]


def _attn_case(ops, dev, dtype, case, seed, spikes=(), permuted=False):
    b, h, hkv, nq, nk = case
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, h, nq, D, generator=gen)
    k = torch.randn(b, hkv, nk, D, generator=gen)
    for (qi, ki, gain) in spikes:        # key ki lines up with query qi: its score jumps by gain * |q|^2 * scale at that key tile
        k[:, :, ki] = gain * q[:, ::h // hkv, qi]
    v = torch.randn(b, hkv, nk, D, generator=gen)
    q, k, v = (t.to(dev).to(dtype) for t in (q, k, v))
    if permuted:      # (B, N, H, 128) storage seen as (B, H, N, 128): what the model hands over
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))
        assert not q.is_contiguous() or nq == 1 or h == 1
    assert not ops.cross_ok(h, hkv, nk, D, 1)      # the short-key kernels are head dim 64 only
    o, lse = ops.attention(q, k, v, SCALE, need_lse=True)
    assert o.shape == (b, nq, h * D) and o.dtype == dtype and lse.shape == (b, h, nq)
    assert torch.equal(ops.attention(q, k, v, SCALE), o)
    rep = h // hkv
    qr, kr, vr = (t.float().cpu() for t in (q, k, v))
    kr, vr = kr.repeat_interleave(rep, 1), vr.repeat_interleave(rep, 1)
    ref = F.scaled_dot_product_attention(qr, kr, vr, scale=SCALE).permute(0, 2, 1, 3).reshape(b, nq, h * D)
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    err = (o.float().cpu() - ref).abs().max().item()
    bound = tol * max(ref.abs().max().item(), 1e-2)
    lse_ref = torch.logsumexp(qr.double() @ kr.double().transpose(-1, -2) * SCALE, dim=-1)
    lerr = (lse.cpu().double() - lse_ref).abs()
    lbound = 2e-4 * lse_ref.abs().clamp_min(1.0) if dtype == torch.float32 else torch.full_like(lse_ref, 3e-2)
    if spikes and dtype == torch.bfloat16:
        # The spiked keys are 6 - 8 x copies of a query: their products are not unit-variance (scores, and LSEs, near 76), which is the
        # premise of the 3e-2.  Same derivation with the row's own magnitudes: one bf16 rounding (2^-9) of every pre-scaled q_d moves
        # a score by at most 2^-9 * scale * sum_d |q_d k_d|, and the LSE by at most the largest such move over the row's keys.
        # Measured on the simulator: 6.9e-2 at query 5 (LSE 76.3; this bound there: 1.5e-1), the kernel within 1.7e-3 of torch's
        # logsumexp over the bf16-rounded pre-scaled Q.
        worst = (qr.abs().double() @ kr.abs().double().transpose(-1, -2)).amax(dim=-1) * SCALE * 2.0 ** -9
        lbound = torch.maximum(lbound, worst)
    print(f"hd128 attention {case} {dtype}: o err {err:.3e} (bound {bound:.3e}); lse err {lerr.max().item():.3e}")
    assert err <= bound, (case, err, bound)
    assert bool((lerr <= lbound).all()), (case, lerr.max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ATT_CASES)
def test_attention_hd128_sim(emu, case, dtype):
    _attn_case(emu, "cpu", dtype, case, seed=31)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_hd128_deferred_max_sim(emu, dtype):
    _attn_case(emu, "cpu", dtype, (1, 2, 2, 130, 193), seed=33, spikes=SPIKES)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_hd128_permuted_views_sim(emu, dtype):
    _attn_case(emu, "cpu", dtype, (2, 2, 1, 70, 130), seed=34, permuted=True)


# The bf16 kernel has two workgroup shapes: 4 waves (128 queries), and 8 waves (256 queries) once ceil(Nq / 256) * H * B reaches the CU
# count.  The simulator is told it has 2 CUs, which puts every case below on the 8-wave shape; ops.attn_q64 = False forces the 4-wave one,
# and both are held to the same reference: one, two and three 256-query workgroups per head, idle waves, a GQA group, the spikes.
WIDE_CASES = [(1, 2, 2, 64, 64), (1, 2, 1, 257, 200), (1, 2, 2, 193, 37), (1, 2, 2, 600, 70)]


def _wide_case(ops, dev, case, seed, spikes=()):
    saved = ops.attn_q64
    try:
        for forced4 in (False, True):
            ops.attn_q64 = False if forced4 else None
            _attn_case(ops, dev, torch.bfloat16, case, seed, spikes)
    finally:
        ops.attn_q64 = saved


def test_attention_hd128_wide_workgroup_sim(emu):
    emu.lib.sat_emu_set_cu_count(2)
    try:
        for case in WIDE_CASES:
            _wide_case(emu, "cpu", case, seed=35)
        _wide_case(emu, "cpu", (1, 2, 2, 130, 193), seed=33, spikes=SPIKES)
    finally:
        emu.lib.sat_emu_set_cu_count(0)


@pytest.mark.gpu
def test_attention_hd128_wide_workgroup_gpu(hip):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b, h, nq = 4, 32, 300
    assert -(-nq // 256) * h * b >= cus, "this shape no longer reaches the 8-wave kernel: raise the head count"
    _wide_case(hip, "cuda", (b, h, 16, nq, 130), seed=36)
    _wide_case(hip, "cuda", (b, h, h, 257, 193), seed=37, spikes=SPIKES)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_hd128_gpu(hip, dtype):
    for case in ATT_CASES + GPU_CASES:
        _attn_case(hip, "cuda", dtype, case, seed=31)
    _attn_case(hip, "cuda", dtype, (1, 2, 2, 130, 193), seed=33, spikes=SPIKES)
    _attn_case(hip, "cuda", dtype, (2, 2, 1, 70, 130), seed=34, permuted=True)


def _refusals(ops, dev):
    q = torch.randn(1, 2, 40, D).to(dev)
    with pytest.raises(NotImplementedError, match="inference"):
        ops.attention(q, q, q, SCALE, return_planes=True)
    planes = {n: ops.attn_planes(q, row_major=True, transposed=True) for n in ("q", "k", "v")}
    o = torch.empty(1, 40, 2 * D).to(dev)
    with pytest.raises(NotImplementedError, match="inference"):
        ops.attention_bwd(planes, o, o, torch.empty(1, 2, 40).to(dev), SCALE, 2, 40)
    with pytest.raises(NotImplementedError):
        ops.attn_planes(torch.randn(1, 2, 40, 32).to(dev))
    # the C entry points themselves: the backward names inference-only, the forced 64-query kernel does not exist at 128
    pl = planes["q"]
    arr = (ctypes.c_void_p * 16)(*([pl["rm"][0].data_ptr()] * 16))
    lse = torch.zeros(1, 2, 40).to(dev)
    rc = ops.lib.sat_attention_bwd(arr, lse.data_ptr(), lse.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), 1, 2, 2, 40, 40, 64, 64, D,
                                   SCALE, 0, None)
    assert rc != 0 and b"inference-only" in ops.lib.sat_last_error()
    ptr = pl["rm"][0].data_ptr()
    rc = ops.lib.sat_attention_fwd(ptr, None, ptr, None, ptr, None, o.data_ptr(), None, 1, 2, 2, 40, 40, 64, 64, D, SCALE, 3, None)
    assert rc != 0 and b"head_dim == 64 only" in ops.lib.sat_last_error()
    rc = ops.lib.sat_attention_fwd(ptr, None, ptr, None, ptr, None, o.data_ptr(), None, 1, 2, 2, 40, 40, 64, 64, 96, SCALE, 1, None)
    assert rc != 0


def test_hd128_refusals_sim(emu):
    _refusals(emu, "cpu")


@pytest.mark.gpu
def test_hd128_refusals_gpu(hip):
    _refusals(hip, "cuda")


def test_hd_entry_points_validate_sim(emu):
    """Argument validation of sat_attn_prepare_hd / sat_qk_norm_fwd_hd: every call below must fail BEFORE any launch (the pointers are
    real, small buffers all the same)."""
    lib = emu.lib
    src = torch.zeros(1, 1, 64, D)
    out = torch.zeros(1, 1, 64, D, dtype=torch.int16)

    def prepare(n, npad, hd, dt=0):
        return lib.sat_attn_prepare_hd(src.data_ptr(), src.stride(0), src.stride(1), src.stride(2), out.data_ptr(), None, None, None,
                                       1, 1, n, npad, hd, dt, None)
    for hd in (0, 32, 96, 256):
        assert prepare(64, 64, hd) != 0 and b"head_dim" in lib.sat_last_error()
    for hd in (64, D):
        assert prepare(40, 40, hd) != 0 and b"multiple of 64" in lib.sat_last_error()      # Np not a multiple of 64
        assert prepare(64, 0, hd) != 0                                                      # Np < N
        assert prepare(0, 64, hd) != 0
        assert prepare(64, 64, hd, dt=2) != 0
    x = torch.zeros(1, 4, 2 * D)
    tab = torch.ones(D)

    def norm(hd, xs=2 * D, nh=2, mode=2, dt=0):
        return lib.sat_qk_norm_fwd_hd(x.data_ptr(), xs, x.data_ptr(), xs, tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), None, 0,
                                      None, 4, 4, nh, nh, mode, 1e-6, hd, dt, None)
    for hd in (0, 32, 96, 256):
        assert norm(hd) != 0 and b"head_dim" in lib.sat_last_error()
    assert norm(D, xs=D, nh=2) != 0 and b"nh * 128" in lib.sat_last_error()      # rows shorter than nh heads of 128
    assert norm(D, mode=3) != 0 and norm(D, dt=2) != 0 and norm(D, nh=0) != 0
    assert norm(64, mode=3) != 0


# ---------------------------------------------------------------------------------------------------------------------
# planes
# ---------------------------------------------------------------------------------------------------------------------
def _planes_case(ops, dev):
    torch.manual_seed(5)
    b, h, n = 2, 3, 70
    src = (torch.randn(b, n, h, D) * 3.0).to(dev)
    wide = (torch.randn(b, n - 1, h, D + 4) * 3.0).to(dev)
    # strided, contiguous, and rows that are neither 16-byte aligned nor a multiple of 8 elements apart (the scalar load path)
    for t in (src.permute(0, 2, 1, 3), src.permute(0, 2, 1, 3).contiguous(), wide[..., 2:2 + D].permute(0, 2, 1, 3)):
        nn_ = t.shape[2]
        pl = ops.attn_planes(t, row_major=True, transposed=True)
        assert pl["np"] == 128 and pl["rm"][0].shape == (b, h, 128, D) and pl["tr"][0].shape == (b, h, D, 128)
        hi, lo = (p.view(torch.bfloat16).float().cpu() for p in pl["rm"])
        rec = (hi + lo)[:, :, :nn_]
        want = t.cpu()
        assert float(((rec - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
        assert torch.equal(hi[:, :, :nn_], want.bfloat16().float())
        assert float(hi[:, :, nn_:].abs().max()) == 0.0 and float(lo[:, :, nn_:].abs().max()) == 0.0      # padding rows are zero
        for i in range(2):
            assert torch.equal(pl["tr"][i], pl["rm"][i].transpose(2, 3))
        t16 = t.bfloat16()
        p16 = ops.attn_planes(t16, row_major=True, transposed=True)
        assert p16["rm"][1] is None and p16["tr"][1] is None
        assert torch.equal(p16["rm"][0][:, :, :nn_].view(torch.bfloat16), t16) and float(p16["rm"][0][:, :, nn_:].abs().max()) == 0.0
        assert torch.equal(p16["tr"][0], p16["rm"][0].transpose(2, 3))
        only_tr = ops.attn_planes(t16, row_major=False, transposed=True)
        assert only_tr["rm"][0] is None and torch.equal(only_tr["tr"][0], p16["tr"][0])


def test_attn_planes_hd128_sim(emu):
    _planes_case(emu, "cpu")


@pytest.mark.gpu
def test_attn_planes_hd128_gpu(hip):
    _planes_case(hip, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# qk_norm at 128
# ---------------------------------------------------------------------------------------------------------------------
INV = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))      # RotaryEmbedding(max(128 // 2, 32)): 32 frequencies


def _norm_reference(x, nh, hq, mode, tabs, pos):
    """fp64: F.layer_norm / F.normalize over rows of 128, then the reference's rotation of the first 64 dims:
    t * cos + rotate_half(t) * sin with freqs = cat(pos x inv_freq, pos x inv_freq) and rotate_half = (-x2, x1)."""
    x = x.double()
    b, n, _ = x.shape
    heads = x[..., :nh * D].unflatten(-1, (nh, D))
    parts = []
    for lo, hi_, g, bb in ((0, hq, 0, 1), (hq, nh, 2, 3)):
        if hi_ > lo:
            if mode == "ln":
                parts.append(F.layer_norm(heads[:, :, lo:hi_], (D,), weight=tabs[g].double(), bias=tabs[bb].double(), eps=1e-6))
            else:
                parts.append(F.normalize(heads[:, :, lo:hi_], dim=-1))
    y = torch.cat(parts, dim=2)
    if pos is not None:
        freqs = torch.einsum("i,j->ij", pos.double(), INV.double())
        freqs = torch.cat((freqs, freqs), dim=-1)[None, :, None, :]      # (1, n, 1, 64)
        t, rest = y[..., :64], y[..., 64:]
        x1, x2 = t[..., :32], t[..., 32:]
        t = t * freqs.cos() + torch.cat((-x2, x1), dim=-1) * freqs.sin()
        y = torch.cat((t, rest), dim=-1)
    return y.flatten(2)


def _norm_case(ops, dev, b, n, nh, hq, extra_heads, mode, rotary, tab_off=0, seed=0):
    torch.manual_seed(seed)
    c = (nh + extra_heads) * D
    x = torch.randn(b, n, c) * 1.7 + 0.3
    tabs = [torch.randn(D) for _ in range(4)] if mode == "ln" else None
    pos = torch.arange(tab_off, tab_off + n).float() if rotary else None
    cs = ops.rope_tables(INV.to(dev), n + tab_off) if rotary else None
    tabs_d = [t.to(dev) for t in tabs] if tabs is not None else None
    for dtype, bar in ((torch.float32, 1e-5), (torch.bfloat16, 1e-2)):
        xd = x.to(dev).to(dtype)
        out = torch.zeros_like(xd)
        y = ops.qk_norm(xd, nh, hq, mode, tabs_d, cs, out=out, head_dim=D)
        assert y is out
        y = y.float().cpu()
        if extra_heads:                                                  # columns past the normed heads are not written
            assert float(y[..., nh * D:].abs().max()) == 0.0
        ref = _norm_reference(xd.float().cpu(), nh, hq, mode, tabs, pos)
        err = rel_err(y[..., :nh * D].double(), ref)
        assert err < bar, (mode, rotary, dtype, nh, hq, err)
        if mode == "ln" or rotary:      # the head dim is read off the tables / the rotary table when it is not given
            assert torch.equal(ops.qk_norm(xd, nh, hq, mode, tabs_d, cs, out=torch.zeros_like(xd)), out)
        y2, stat = ops.qk_norm(xd, nh, hq, mode, tabs_d, cs, out=torch.zeros_like(xd), save_stats=True, head_dim=D)
        assert torch.equal(y2, out) and stat.shape == ((2 if mode == "ln" else 1), b * n * nh) and bool(torch.isfinite(stat).all())


def _norm_cases(ops, dev):
    for mode in ("ln", "l2"):
        for rotary in (True, False):
            _norm_case(ops, dev, 2, 37, 4, 2, 2, mode, rotary)               # q and k heads of a fused projection (v heads follow)
        _norm_case(ops, dev, 2, 37, 4, 2, 0, mode, True, tab_off=5)          # freqs[-seq_len:]: the table is longer than the sequence
        _norm_case(ops, dev, 1, 11, 1, 0, 1, mode, False)                    # the k half of a cross-attention's (B, M, 2*Hkv*128)
        _norm_case(ops, dev, 1, 11, 2, 2, 0, mode, False)                    # to_q of a cross-attention
    with pytest.raises(ValueError):
        ops.qk_norm(torch.zeros(1, 4, 2 * D).to(dev), 2, 2, "ln", [torch.ones(96).to(dev)] * 4)
    with pytest.raises(ValueError):      # a 64-wide rotary table under a 128-wide norm
        ops.qk_norm(torch.zeros(1, 4, 2 * D).to(dev), 2, 2, "l2", None, torch.zeros(4, 16, 2).to(dev), head_dim=D)


def test_qk_norm_hd128_simulator(emu):
    _norm_cases(emu, "cpu")


@pytest.mark.gpu
def test_qk_norm_hd128_gpu(hip):
    _norm_cases(hip, "cuda")
