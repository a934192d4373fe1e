"""Float64 reference, storage-precision yardstick and per-row check of the head dim 64 attention kernels (tests/test_attention_fp64.py).
The rule is fp64_bounds.py's, applied per ROW: nothing here comes from running a kernel.

  reference   S, P, LSE, O, D = sum_d dO O, dP, dS, dQ, dK, dV in float64 from the inputs the kernel saw (the bf16-rounded ones in the
              bf16 mode), kv heads repeated over their query heads as the reference model does (transformer.py:408-411).
  yardstick   the same formulas in torch float32 on the CPU at the kernel's storage precision:
              bf16: float32 matmuls, and a `.bfloat16().float()` rounding where the kernels round — Q pre-scaled by scale * log2(e)
                    (attention.hip:505, attention_cross.h:126; forward and dQ, not dK / dV: see yardstick), P before the P V and dV
                    products (sat_att_pack), the normaliser taken as the sum of those ROUNDED probabilities (attention.hip:310-312, :371-384; attention_cross.h:170-174), dS / scale before
                    the dQ and dK products, O before it enters D (sat_attention_rowdot reads the stored output), every output;
              fp32: every matrix operand, P and dS included, is hi + lo with hi = bf16(x), lo = bf16(x - hi), and a product is
                    hi.hi + hi.lo + lo.hi in float32 (sat_att_mma<2>).
  row scale   S_row, float64: the largest, over the row's 64 entries, of the sum of the magnitudes of the terms that form the entry
              (reference's srow); floored at 2^-24 of the tensor's largest S_row, so that underflow cannot fail a correct kernel.
  assert      for every row:  max_d |kernel - ref64| / S_row  <=  FACTOR x the largest such ratio of the yardstick over the tensor's rows;
              bf16 outputs first take 2^-8 |ref64| off the error (one final rounding), as fp64_bounds.check does."""
import torch

from fp64_bounds import BF16_HALF_ULP, FACTOR, f64

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
NAMES = ("o", "lse", "dq", "dk", "dv")


def make_inputs(case, dtype, seed, spikes=(), permuted=False):
    """CPU tensors q (B,H,Nq,64), k, v (B,Hkv,Nk,64), do (B,Nq,H*64) in `dtype`; permuted: q / k / v are (B, N, H, 64) storage seen as
    (B, H, N, 64), what the model hands over."""
    b, h, hkv, nq, nk = case
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, h, nq, 64, generator=gen)
    k = torch.randn(b, hkv, nk, 64, generator=gen)
    for (qi, ki, gain) in spikes:        # key ki lines up with query qi (test_dit_kernels.SPIKES)
        k[:, :, ki] = gain * q[:, ::h // hkv, qi]
    v = torch.randn(b, hkv, nk, 64, generator=gen)
    do = torch.randn(b, nq, h * 64, generator=gen)
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    if permuted:
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))
    return q, k, v, do


def _heads(do, h):
    b, nq, _ = do.shape
    return do.view(b, nq, h, 64).permute(0, 2, 1, 3)


def _group_sum(t, hkv):
    """(B, H, Nk, 64) per query head -> (B, Hkv, Nk, 64): the gradient of a repeated kv head is the sum over its query heads"""
    b, h, nk, d = t.shape
    return t.view(b, hkv, h // hkv, nk, d).sum(2)


def reference(q, k, v, do, scale):
    """float64 outputs and row scales: (ref, srow), dicts over NAMES.  o and its scale in the kernel's (B, Nq, H*64) row order, i.e.
    one row per (b, q, h): shaped (B, Nq, H, 64) / (B, Nq, H)."""
    q, k, v, do = (f64(t) for t in (q, k, v, do))
    b, h, nq, _ = q.shape
    hkv = k.shape[1]
    rep = h // hkv
    kr, vr = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    g = _heads(do, h)
    s = scale * (q @ kr.transpose(-1, -2))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    del s
    o = p @ vr
    dsum = (g * o).sum(-1, keepdim=True)
    ds = p * (g @ vr.transpose(-1, -2) - dsum)
    ref = {"o": o.permute(0, 2, 1, 3).contiguous(), "lse": lse, "dq": scale * (ds @ kr),
           "dk": _group_sum(scale * (ds.transpose(-1, -2) @ q), hkv), "dv": _group_sum(p.transpose(-1, -2) @ g, hkv)}
    del ds
    # the magnitudes of the terms: |dS_ij| <= P_ij (sum_e |dO_ie v_je| + sum_e |dO_ie o_ie|)
    w = p * (g.abs() @ vr.abs().transpose(-1, -2) + (g * o).abs().sum(-1, keepdim=True))
    srow = {"o": (p @ vr.abs()).amax(-1).permute(0, 2, 1).contiguous(),
            "lse": (scale * (q.abs() @ kr.abs().transpose(-1, -2))).amax(-1).clamp_min(1.0),
            "dq": scale * (w @ kr.abs()).amax(-1),
            "dk": scale * _group_sum(w.transpose(-1, -2) @ q.abs(), hkv).amax(-1),
            "dv": _group_sum(p.transpose(-1, -2) @ g.abs(), hkv).amax(-1)}
    for n in NAMES:
        top = float(srow[n].max())
        assert top > 0.0 and top == top, n
        srow[n] = srow[n].clamp_min(top * 2.0 ** -24)
    return ref, srow


def _r(x):
    return x.bfloat16().float()


def _split(x):
    hi = _r(x)
    return hi, _r(x - hi)


def _mm(a, b, two_plane):
    """a @ b in float32 on bf16 operands (the caller rounded them), or on hi + lo pairs: hi.hi + hi.lo + lo.hi"""
    if not two_plane:
        return a @ b
    (ah, al), (bh, bl) = _split(a), _split(b)
    return ah @ bh + ah @ bl + al @ bh


def yardstick(q, k, v, do, scale):
    """The formulas of `reference` in float32 at the kernels' storage precision; outputs in float32, shaped as reference's."""
    bf = q.dtype == torch.bfloat16
    two = not bf
    q, k, v, do = (t.detach().cpu().float() for t in (q, k, v, do))
    b, h, nq, _ = q.shape
    hkv = k.shape[1]
    rep = h // hkv
    kr, vr = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    g = _heads(do, h)
    out = (lambda t: _r(t)) if bf else (lambda t: t)
    qs = q * (scale * LOG2E)
    if bf:
        qs = _r(qs)
    x = _mm(qs, kr.transpose(-1, -2), two)          # the scores in the exp2 domain
    m = x.amax(-1, keepdim=True)
    p = torch.exp2(x - m)
    if bf:
        p = _r(p)
    l = p.sum(-1, keepdim=True)
    o = out(_mm(p, vr, two) / l)
    lse2 = m + torch.log2(l)
    del p
    dsum = (g * o).sum(-1, keepdim=True)
    # The backward recomputes P from the forward's LSE.  Only the bf16 dQ kernels do so from the forward's operands (the rounded pre-scaled
    # Q: attention.hip:999-1001, attention_cross.h:259); the bf16 dK / dV kernels (attention.hip:1487, attention_cross.h:447) and the
    # two-plane backward (attention.hip:962, :1286) multiply the product of the UNSCALED Q by scale * log2(e) in fp32.
    x_raw = _mm(q, kr.transpose(-1, -2), two) * (scale * LOG2E)
    dpd = _mm(g, vr.transpose(-1, -2), two) - dsum
    ds_q = torch.exp2((x if bf else x_raw) - lse2) * dpd      # dS / scale
    del x
    p = torch.exp2(x_raw - lse2)
    del x_raw
    ds_k = p * dpd
    if bf:
        p, ds_q, ds_k = _r(p), _r(ds_q), _r(ds_k)
    return {"o": o.permute(0, 2, 1, 3).contiguous(), "lse": (lse2 * LN2).squeeze(-1), "dq": out(scale * _mm(ds_q, kr, two)),
            "dk": out(scale * _group_sum(_mm(ds_k.transpose(-1, -2), q, two), hkv)),
            "dv": out(_group_sum(_mm(p.transpose(-1, -2), g, two), hkv))}


def row_ratio(got, ref64, srow):
    """per row: max_d of the error (less the final bf16 rounding's 2^-8 |ref| for a bf16 tensor) over S_row"""
    err = (f64(got) - ref64).abs()
    if got.dtype == torch.bfloat16:
        err = (err - BF16_HALF_ULP * ref64.abs()).clamp_min(0.0)
    return (err.amax(-1) if err.dim() > srow.dim() else err) / srow


def check_rows(name, got, ref64, yard, srow):
    """got: the kernel's tensor; ref64 / yard / srow from reference() / yardstick().  A bf16 tensor's yardstick holds bf16 values too:
    its error takes the same 2^-8 |ref| off as the kernel's.  Prints both figures, then asserts every row."""
    got = got.detach().cpu()
    got = got.reshape(ref64.shape)
    assert bool(torch.isfinite(got.double()).all()), f"{name}: not finite"
    ry = float(row_ratio(yard.bfloat16() if got.dtype == torch.bfloat16 else yard, ref64, srow).max())
    rk = row_ratio(got, ref64, srow)
    worst = float(rk.max())
    print(f"FIGURE {name} {str(got.dtype)[6:]}: yardstick {ry:.3e}  kernel {worst:.3e}  (rows {rk.numel()}, S_row {float(srow.min()):.3e} .. "
          f"{float(srow.max()):.3e})")
    bad = rk > FACTOR * ry
    if bool(bad.any()):
        i = int(rk.argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), rk.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {rk.numel()} rows beyond {FACTOR:g} x yardstick {ry:.3e}; worst row {idx}: "
                             f"{worst:.3e} of S_row {float(srow[idx]):.3e}")
    return ry, worst


def xatt_per_wg(cus, units_bhk, nwb):
    """sat_xatt_per_wg (csrc/attention_cross.h) restated: wave blocks per workgroup of the short-key forward and dQ kernels"""
    nchunks = max(1, -(-4 * cus // units_bhk))
    return max(4, -(-(-(-nwb // nchunks)) // 4) * 4)


def xatt_dkv_plan(cus, case):
    """sat_xatt_dkv_plan restated: (64-query tiles of a kv group, tiles per range, ranges) of the short-key dK / dV kernel"""
    b, h, hkv, nq, _ = case
    ntiles = (h // hkv) * -(-nq // 64)
    want = min(ntiles, max(1, -(-2 * cus // (b * hkv))))
    per = -(-ntiles // want)
    return ntiles, per, -(-ntiles // per)

