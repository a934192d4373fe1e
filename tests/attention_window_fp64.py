"""Float64 reference and storage-precision yardstick of the sliding-window attention forward (tests/test_sliding_window_kernels.py):
the forward half of tests/attention_fp64.py restated with the band mask and a free head dim (64 or 128).  Nothing here comes from
running a kernel; the assertion is attention_fp64.check_rows (fp64_bounds.FACTOR x the yardstick's worst row, per row).

  window      flash-attn's window_size = (left, right): query i sees key j iff (left < 0 or j >= i - left) and (right < 0 or
              j <= i + right); -1 = unbounded; None = dense.  Self-attention: Nq == Nk == N.
  reference   S, LSE, O in float64 with the scores outside the band at -inf, kv heads repeated over their query heads.
  yardstick   the same in torch float32 at the kernel's storage precision — bf16: Q pre-scaled by scale * log2(e) and rounded, P rounded
              before the P V product, the normaliser the sum of the ROUNDED probabilities; fp32: every matrix operand as hi + lo, a
              product as hi.hi + hi.lo + lo.hi (attention_fp64._mm).
  row scale   o: max_d sum_j P_ij |v_jd|;  lse: the largest in-band scale * sum_d |q_id k_jd|, at least 1; floored at 2^-24 of the
              tensor's largest."""
import torch

from attention_fp64 import LN2, LOG2E, _mm, _r
from fp64_bounds import f64

NAMES = ("o", "lse")


def band(n, window):
    """(N, N) bool: True where query i (row) sees key j (column)"""
    i = torch.arange(n)[:, None]
    j = torch.arange(n)[None, :]
    vis = torch.ones(n, n, dtype=torch.bool)
    if window is not None:
        left, right = window
        if left >= 0:
            vis &= j >= i - left
        if right >= 0:
            vis &= j <= i + right
    return vis


def make_inputs(case, d, dtype, seed, spikes=(), permuted=False):
    """CPU tensors q (B,H,N,D), k, v (B,Hkv,N,D) in `dtype`; spikes: key j = gain * query i; permuted: (B, N, H, D) storage seen as
    (B, H, N, D), what the model hands over."""
    b, h, hkv, n = case
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, h, n, d, generator=gen)
    k = torch.randn(b, hkv, n, d, generator=gen)
    for (qi, ki, gain) in spikes:
        k[:, :, ki] = gain * q[:, ::h // hkv, qi]
    v = torch.randn(b, hkv, n, d, generator=gen)
    q, k, v = (t.to(dtype) for t in (q, k, v))
    if permuted:
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))
    return q, k, v


_CAT = {"o": 2, "lse": 1}      # the head axis of o (B, N, H, D), of its row scale (B, N, H) and of lse (B, H, N)


def _per_kv_head(fn, q, k, v, *args):
    """fn on one kv head (and its query heads) at a time, results joined along the head axis: bounds the (N, N) temporaries"""
    rep = q.shape[1] // k.shape[1]
    parts = [fn(q[:, g * rep:(g + 1) * rep], k[:, g:g + 1], v[:, g:g + 1], *args) for g in range(k.shape[1])]
    if isinstance(parts[0], tuple):
        return tuple({n: torch.cat([pt[i][n] for pt in parts], _CAT[n]) for n in NAMES} for i in range(len(parts[0])))
    return {n: torch.cat([pt[n] for pt in parts], _CAT[n]) for n in NAMES}


def reference(q, k, v, scale, window):
    """float64 (ref, srow), dicts over NAMES; o and its scale one row per (b, q, h): (B, N, H, D) / (B, N, H)"""
    ref, srow = _per_kv_head(_reference, q, k, v, scale, window)
    for name in NAMES:
        top = float(srow[name].max())
        assert top > 0.0 and top == top, name
        srow[name] = srow[name].clamp_min(top * 2.0 ** -24)
    return ref, srow


def yardstick(q, k, v, scale, window):
    """`reference` in float32 at the kernels' storage precision; shaped as reference's"""
    return _per_kv_head(_yardstick, q, k, v, scale, window)


def _reference(q, k, v, scale, window):
    q, k, v = (f64(t) for t in (q, k, v))
    n = q.shape[2]
    rep = q.shape[1] // k.shape[1]
    kr, vr = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    vis = band(n, window)
    s = (scale * (q @ kr.transpose(-1, -2))).masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    ref = {"o": (p @ vr).permute(0, 2, 1, 3).contiguous(), "lse": lse}
    mag = (scale * (q.abs() @ kr.abs().transpose(-1, -2))).masked_fill(~vis, 0.0)
    srow = {"o": (p @ vr.abs()).amax(-1).permute(0, 2, 1).contiguous(), "lse": mag.amax(-1).clamp_min(1.0)}
    return ref, srow


def _yardstick(q, k, v, scale, window):
    bf = q.dtype == torch.bfloat16
    two = not bf
    q, k, v = (t.detach().cpu().float() for t in (q, k, v))
    n = q.shape[2]
    rep = q.shape[1] // k.shape[1]
    kr, vr = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    vis = band(n, window)
    qs = q * (scale * LOG2E)
    if bf:
        qs = _r(qs)
    x = _mm(qs, kr.transpose(-1, -2), two).masked_fill(~vis, float("-inf"))      # the scores in the exp2 domain
    m = x.amax(-1, keepdim=True)
    p = torch.exp2(x - m)
    if bf:
        p = _r(p)
    l = p.sum(-1, keepdim=True)
    o = _mm(p, vr, two) / l
    if bf:
        o = _r(o)
    return {"o": o.permute(0, 2, 1, 3).contiguous(), "lse": ((m + torch.log2(l)) * LN2).squeeze(-1)}
