"""Float64 reference, yardstick and per-ELEMENT scale of the conv WEIGHT-gradient kernels (csrc/conv_wgrad_bf16x3.hip, conv_wgrad7_bf16x3_pipe.h,
conv_wgrad7_planes.h, conv_wgrad.hip, edge_conv.hip's wgrad, ru_k1_bwd.hip) and of sat_reduce_splits / sat_rowsum, for
tests/test_wgrad_fp64.py.  The rule is gemm_fp64.py's; the assertion IS gemm_fp64.check.  Nothing here comes from running a kernel.

  reference   the TRUE operation in float64 from the fp32 tensors the kernel (or, for the planes kernel, the pre-pass) was handed: the hi / lo
              truncation is part of what is tested.  With a = A(lo) (B, M, Tlo) and h = Bf(hi) (B, N, Thi), SnakeBeta on whichever side the call names,
              dW[m][n][k] = sum_{b,t} a[b,m,t] h[b,n,t s + k d - pad] (samples outside [0, Thi) are zero; SnakeBeta(0) = 0).  Row sums: sum_{b,t} lo[b,m,t].
  scale S     per element, float64: conv_fp64's S_act on the activated operand, |.| on the other; dW: S = sum_{b,t} S_lo S_hi; row sums:
              sum |lo|; gemm_fp64.check floors S at 2^-24 of the tensor's largest.
  yardstick   the same formulas in torch float32 on the CPU, the LARGEST figure of two evaluations.  bf16x3 kernels: both operands split as
              conv_fp64.split and the product formed as hi.hi + hi.lo + lo.hi; the two fp32 kernels (sat_conv_wgrad, sat_edge_conv_wgrad): plain fp32.
              (a) a blocked einsum per tap; (b) a running chain over (b, t) in that order, one addcmul_ per product and step.  Where
              B * T > 16384 the chain advances by 64-step BLOCKS instead, each block summed by torch (an einsum over its 64 steps) and added to the
              running value: 2^14 Python steps per product is what a test can afford, and a block is the kernels' own stage.  The row sums' chain
              does the same.
  ru_k1_bwd   dh, d log-alpha2, d log-beta2: conv_fp64.conv / dgrad on a K = 1 Geom with W2^T; emitted dh: conv_fp64.check_planes; dW2: the wgrad of
              (dy, snake2(h)); dbias2 = sum dy; dbias1 = sum dh with S = sum S_dh.
  reduce      ref = scale sum_z slab_z (+ out_before), S = |scale| sum |slab| (+ |out_before|); yardstick: a running fp32 sum over the slabs and
              torch's .sum(0).
  assert      max over the elements of |kernel - ref64| / S  <=  FACTOR x the yardstick's."""
import torch
import torch.nn.functional as F

from fp64_bounds import f64
from gemm_fp64 import Terms, check  # noqa: F401  (check: re-exported for the tests)
from conv_fp64 import Geom, _snake32, _snake64, act, check_planes, conv, dgrad, inp, planes_value, split  # noqa: F401

CHAIN_STEPS = 16384          # above this many (b, t) steps the chain advances by 64-step blocks
BLOCK = 64


def _windows(h, taps, stride, dil, pad, tlo):
    """(B, N, Thi) -> K views (B, N, Tlo): h[b, n, t stride + k dil - pad], zero outside the tensor"""
    need = (tlo - 1) * stride + (taps - 1) * dil + 1
    hp = F.pad(h, (pad, max(need - pad - h.shape[2], 0)))
    span = (tlo - 1) * stride + 1
    return [hp[:, :, k * dil:k * dil + span:stride] for k in range(taps)]


def _products(a, w, x3):
    """the (lo-side, hi-side) float32 pairs whose products a kernel adds: three of split operands, or one"""
    if not x3:
        return [(a, w)]
    (ah, al), (wh, wl) = split(a), split(w)
    return [(ah, wh), (ah, wl), (al, wh)]


def _taps(a, wins):
    return torch.stack([torch.einsum("bmt,bnt->mn", a, w) for w in wins], dim=2)


def _blocked(pairs):
    out = None
    for a, w in pairs:
        term = _taps(a, w)
        out = term if out is None else out + term
    return out


def _chain(pairs):
    a0, w0 = pairs[0]
    b, m, t = a0.shape
    n, k = w0[0].shape[1], len(w0)
    acc = torch.zeros(m, n, k)
    if b * t <= CHAIN_STEPS:
        cols = [(a.permute(0, 2, 1).reshape(b * t, m, 1, 1), torch.stack(w, dim=3).permute(0, 2, 1, 3).reshape(b * t, 1, n, k)) for a, w in pairs]
        for i in range(b * t):
            for ac, wc in cols:
                acc.addcmul_(ac[i], wc[i])
        return acc
    for bi in range(b):
        for t0 in range(0, t, BLOCK):
            for a, w in pairs:
                acc += _taps(a[bi:bi + 1, :, t0:t0 + BLOCK], [v[bi:bi + 1, :, t0:t0 + BLOCK] for v in w])
    return acc


def wgrad(lo, hi, k, stride=1, dil=1, pad=0, snake=None, snake_on=0, x3=True):
    """lo (B, M, Tlo), hi (B, N, Thi): the fp32 CPU tensors; snake = (log-alpha, log-beta) of the side snake_on names (1: lo, 2: hi) -> Terms
    of dW (M, N, K)"""
    lo64, hi64 = f64(lo), f64(hi)
    tlo = lo.shape[2]
    a64, sa, w64, sw = lo64, lo64.abs(), hi64, hi64.abs()
    a32, w32 = lo64.float(), hi64.float()
    if snake is not None:
        assert snake_on in (1, 2)
        la, lb = snake
        if snake_on == 1:
            v = _snake64(lo64, la, lb)
            a64, sa, a32 = v[0], v[4], _snake32(a32, la, lb)[0]
        else:
            v = _snake64(hi64, la, lb)
            w64, sw, w32 = v[0], v[4], _snake32(w32, la, lb)[0]
    win = lambda h: _windows(h, k, stride, dil, pad, tlo)
    ref, s = _taps(a64, win(w64)), _taps(sa, win(sw))
    pairs = [(a, win(w)) for a, w in _products(a32, w32, x3)]
    return Terms(ref, s, [_blocked(pairs), _chain(pairs)])


def _running_rows(p):
    """(B, C, T) float32 -> (C,): one add per (b, t) in order; above CHAIN_STEPS steps one add per 64-step block (summed by torch)"""
    b, c, t = p.shape
    acc = torch.zeros(c)
    if b * t <= CHAIN_STEPS:
        for row in p.permute(0, 2, 1).reshape(-1, c):
            acc += row
        return acc
    for bi in range(b):
        for t0 in range(0, t, BLOCK):
            acc += p[bi, :, t0:t0 + BLOCK].sum(1)
    return acc


def rowsum(lo):
    """sum_{b,t} lo[b, m, t]: S = sum |lo|"""
    lo64 = f64(lo)
    lo32 = lo64.float()
    return Terms(lo64.sum(dim=(0, 2)), lo64.abs().sum(dim=(0, 2)), [lo32.sum(dim=(0, 2)), _running_rows(lo32)])


def sum_bt(t):
    """sum_{b,t} of a computed tensor (dbias1 = sum dh): S = sum S"""
    return Terms(t.ref.sum(dim=(0, 2)), t.s.sum(dim=(0, 2)), [v for y in t.yards for v in (y.sum(dim=(0, 2)), _running_rows(y))])


def ru_k1_bwd(dy, h, w2, la2, lb2):
    """The backward of y = x + conv1x1(snake2(h)) w.r.t. everything but x -> {"dh", "dla", "dlb", "dw2", "dbias2", "dbias1"}: Terms"""
    c, t = dy.shape[1], dy.shape[2]
    wt = f64(w2)[:, :, 0].t().contiguous()[:, :, None].float()          # W2^T as the (C_in, C_out, 1) weight of the conv dy -> dh
    acc = conv(act(inp(dy), None), wt, Geom("conv", 1, tout=t))
    dh, dla, dlb = dgrad(acc, h, la2, lb2)
    return {"dh": dh, "dla": dla, "dlb": dlb, "dw2": wgrad(dy, h, 1, snake=(la2, lb2), snake_on=2), "dbias2": rowsum(dy), "dbias1": sum_bt(dh)}


def reduce_splits(slabs, scale=1.0, before=None):
    """slabs (nsplit, count) float32, scale as the kernel gets it (a float32 value) -> Terms of out"""
    s64 = f64(slabs)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    ref, s = sc * s64.sum(0), abs(sc) * s64.abs().sum(0)
    run = torch.zeros(slabs.shape[1])
    for z in range(slabs.shape[0]):
        run += slabs[z].cpu()
    yards = [run * sc, slabs.cpu().sum(0) * sc]
    if before is not None:
        b64 = f64(before)
        ref, s, yards = ref + b64, s + b64.abs(), [y + b64.float() for y in yards]
    return Terms(ref, s, yards)
