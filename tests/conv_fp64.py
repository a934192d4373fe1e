"""Float64 reference, bf16x3 yardstick and per-ELEMENT scale of the bf16x3 conv kernels (csrc/conv1d_bf16x3.hip, conv1d_bf16x3_k7.h,
conv1d_planes.h + conv1d_bf16x3_k7q.h, conv_epilogue.h) for tests/test_conv_fp64.py.  The rule is gemm_fp64.py's; the assertion IS
gemm_fp64.check.  Nothing here comes from running a kernel.

  reference   the TRUE operation in float64 from the fp32 tensors the kernel was handed (x, log-alpha, log-beta, w, bias, res, x2): not
              the operation on split operands — the hi / lo truncation is part of what the kernel is held to.  SnakeBeta is
              x + sin(e^la x)^2 / (e^lb + 1e-9); the data-gradient and the two parameter sums come from float64 autograd.
  scale S     per element, float64, to first order: S_act = |x| + ib (sin^2(ax) + |a x sin(2ax)|) (no activation: |x|); conv: the same
              conv of S_act with |w|, + |bias|; data-gradient epilogue: |dsnake(x2)| S_acc + |acc| S_dsnake + |res| with
              S_dsnake = 1 + ib a (|sin(2ax)| + |2ax cos(2ax)|), the terms of the factor 1 + ib a sin(2ax) itself: where they cancel
              (ib a > 1) the factor's own float32 rounding is what is left of the element; residual: + |res|; tanh: x (1 - tanh^2), and a second check with + |tanh|, the result's own rounding (tanh());
              parameter sums: S_c = sum_{b,t} S_acc |d snake / d log-param|; an activation of a computed tensor h:
              |dsnake(h)| S_h + S_act(h).  gemm_fp64.check floors S at 2^-24 of the tensor's largest.
  yardstick   the same formulas in torch float32 on the CPU with the product formed as the kernels form it: act and w split as
              hi = x.bfloat16(), lo = (x - hi).bfloat16(); y = conv(hi_a, hi_w) + conv(hi_a, lo_w) + conv(lo_a, hi_w), taken two ways —
              torch's F.conv1d / F.conv_transpose1d, and a (channel, tap)-ordered fp32 chain over the unfolded operand (gemm_fp64.projection's
              chain on the im2col of the conv).  Every epilogue runs on both; parameter sums by torch's .sum and by a running sum over
              (b, t); the LARGEST figure is the yardstick.
  assert      max over the elements of |kernel - ref64| / S  <=  FACTOR x the yardstick's."""
import torch
import torch.nn.functional as F

from fp64_bounds import FACTOR, f64
from gemm_fp64 import Terms, check  # noqa: F401  (check: re-exported for the tests)

PLANE_LEAD = 32              # zero rows before t = 0 in an activation plane
SPLIT_REL = 2.0 ** -17       # |x - hi - lo| <= 2^-17 |x|: two bf16 roundings


def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


class Geom:
    """One conv as torch states it.  kind "conv": y[co][t] = sum w[co][ci][k] a[ci][t stride + k dil - pad], w (Cout, Cin, K);
    kind "tr": y[co][q stride + k - pad] += w[ci][co][k] a[ci][q], w (Cin, Cout, K).  tout: the output length (zeros beyond the input)."""

    def __init__(self, kind, k, stride=1, dil=1, pad=0, tout=None):
        self.kind, self.k, self.stride, self.dil, self.pad, self.tout = kind, k, stride, dil, pad, tout

    def _padded(self, a):
        need = (self.tout - 1) * self.stride + self.dil * (self.k - 1) + 1
        a = F.pad(a, (self.pad, max(need - self.pad - a.shape[2], 0)))
        return a[..., :need]

    def _crop(self, full):
        full = full[..., self.pad:self.pad + self.tout]
        return F.pad(full, (0, self.tout - full.shape[2]))

    def torch(self, a, w):
        if self.kind == "conv":
            return F.conv1d(self._padded(a), w, stride=self.stride, dilation=self.dil)
        return self._crop(F.conv_transpose1d(a, w, stride=self.stride))

    def chain(self, ah, al, wh, wl):
        """acc += hi.hi, += hi.lo, += lo.hi per (channel, tap), in that order (products of bf16 values are exact in float32: one rounding per step)"""
        if self.kind == "conv":
            ah, al = self._padded(ah), self._padded(al)
            acc = torch.zeros(ah.shape[0], wh.shape[0], self.tout)
            span = (self.tout - 1) * self.stride + 1
            for ci in range(ah.shape[1]):
                for k in range(self.k):
                    sh, sl = (t[:, ci, None, k * self.dil:k * self.dil + span:self.stride] for t in (ah, al))
                    ch, cl = wh[None, :, ci, k, None], wl[None, :, ci, k, None]
                    acc.addcmul_(sh, ch).addcmul_(sh, cl).addcmul_(sl, ch)
            return acc
        tin = ah.shape[2]
        full = torch.zeros(ah.shape[0], wh.shape[1], (tin - 1) * self.stride + self.k)
        for ci in range(ah.shape[1]):
            for k in range(self.k):
                view = full[:, :, k:k + (tin - 1) * self.stride + 1:self.stride]
                sh, sl = ah[:, ci, None, :], al[:, ci, None, :]
                ch, cl = wh[None, ci, :, k, None], wl[None, ci, :, k, None]
                view.addcmul_(sh, ch).addcmul_(sh, cl).addcmul_(sl, ch)
        return self._crop(full)


def _bc(p):
    return p[None, :, None]


def _d(t):
    return t if t.dtype == torch.float64 else f64(t)       # (a float64 autograd leaf stays in its graph)


def _snake64(x, la, lb):
    """float64: value, d / dx, d / d log-alpha, d / d log-beta, S_act, S of d / dx"""
    a, eb = _bc(_d(la).exp()), _bc(_d(lb).exp())
    ib = 1.0 / (eb + 1e-9)
    sn2, s2 = torch.sin(a * x) ** 2, torch.sin(2.0 * a * x)
    s_dx = 1.0 + ib * a * (s2.abs() + (2.0 * a * x * torch.cos(2.0 * a * x)).abs())
    return x + ib * sn2, 1.0 + ib * a * s2, ib * a * x * s2, -sn2 * eb * ib * ib, x.abs() + ib * (sn2 + (a * x * s2).abs()), s_dx


def _snake32(x, la, lb):
    a, eb = _bc(la.detach().cpu().float().exp()), _bc(lb.detach().cpu().float().exp())
    ib = 1.0 / (eb + 1e-9)
    sn2, s2 = torch.sin(x * a) ** 2, torch.sin(2.0 * (x * a))
    return x + ib * sn2, 1.0 + ib * a * s2, ib * a * x * s2, -sn2 * eb * ib * ib


def inp(x):
    """a tensor the kernel is handed: exact (s None until an activation or a conv gives it one)"""
    x64 = f64(x)
    return Terms(x64, None, [x64.float()])


def act(t, snake):
    """SnakeBeta (or nothing) of an input (S_act) or of a computed tensor (|dsnake| S + S_act; nothing: S)"""
    if snake is None:
        return Terms(t.ref, t.ref.abs() if t.s is None else t.s, t.yards)
    la, lb = snake
    ref, dx, _, _, s_act, _ = _snake64(t.ref, la, lb)
    s = s_act if t.s is None else dx.abs() * t.s + s_act
    return Terms(ref, s, [_snake32(y, la, lb)[0] for y in t.yards])


def conv(a, w, geom, bias=None):
    """a: Terms of the (activated) operand, one or two float32 evaluations; w: the fp32 weight in geom's layout.  -> Terms with two
    evaluations: torch's conv and the chain (of a's first / second evaluation)."""
    w64 = f64(w)
    wh, wl = split(w64.float())
    a0, a1 = a.yards[0], a.yards[-1]
    h0, l0 = split(a0)
    h1, l1 = split(a1)
    yards = [geom.torch(h0, wh) + geom.torch(h0, wl) + geom.torch(l0, wh), geom.chain(h1, l1, wh, wl)]
    ref, s = geom.torch(a.ref, w64), geom.torch(a.s, w64.abs())
    if bias is not None:
        b = _bc(f64(bias))
        ref, s, yards = ref + b, s + b.abs(), [y + b.float() for y in yards]
    return Terms(ref, s, yards)


def add_res(t, res):
    r = f64(res)
    return Terms(t.ref + r, t.s + r.abs(), [y + r.float() for y in t.yards])


def tanh(t, own=False):
    """S (1 - tanh^2); own: + |tanh|, the result's own float32 rounding — where tanh saturates nothing else is left of the element, and the
    first form's figure is then that rounding over a vanishing S, for the yardstick and for the kernel alike (the tests assert both forms)"""
    th = torch.tanh(t.ref)
    return Terms(th, t.s * (1.0 - th * th) + (th.abs() if own else 0.0), [torch.tanh(y) for y in t.yards])


def _running_sum(p):
    """(B, C, T) float32 -> (C,): one add per (b, t), in order"""
    cols = p.permute(0, 2, 1).reshape(-1, p.shape[1])
    acc = torch.zeros(p.shape[1])
    for row in cols:
        acc += row
    return acc


def dgrad(t, x2, la2, lb2, res=None):
    """The data-gradient epilogue on the accumulator t (bias included): dx = t dsnake(x2) + res (S: |dsnake| S_t + |t| S_dsnake + |res|), d log-alpha2 = sum_{b,t} t d snake / d log-alpha,
    d log-beta2 likewise.  The three references are float64 AUTOGRAD of SnakeBeta with upstream gradient t.ref.  -> (dx, dla, dlb) Terms."""
    leaves = [f64(v).clone().requires_grad_(True) for v in (x2, la2, lb2)]
    gx, ga, gb = torch.autograd.grad(_snake64(*leaves)[0], leaves, t.ref)
    _, dx, dla, dlb, _, s_dx = _snake64(f64(x2), la2, lb2)
    r64 = f64(res) if res is not None else torch.zeros_like(gx)
    x32 = f64(x2).float()
    _, dx32, dla32, dlb32 = _snake32(x32, la2, lb2)
    ydx = [y * dx32 + r64.float() for y in t.yards]
    out = [Terms(gx + r64, dx.abs() * t.s + t.ref.abs() * s_dx + r64.abs(), ydx)]
    for g, d64, d32 in ((ga, dla, dla32), (gb, dlb, dlb32)):
        yards = []
        for y in t.yards:
            yards += [(y * d32).sum(dim=(0, 2)), _running_sum(y * d32)]
        out.append(Terms(g, (t.s * d64.abs()).sum(dim=(0, 2)), yards))
    return out


def conv_dgrad_ref(dy, w_fwd, pad, dil, tin):
    """float64 autograd of the forward conv1d(x (B, Cin, tin), w_fwd (Cout, Cin, K), pad, dil) with upstream gradient dy: d / dx"""
    xin = torch.zeros(dy.shape[0], w_fwd.shape[1], tin, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(xin, f64(w_fwd), padding=pad, dilation=dil)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    return torch.autograd.grad(y, xin, f64(dy))[0]


def planes_value(em, b, cout, t):
    """hi + lo of emitted planes [B][ceil(C / 8)][rows][8], rows 32 .. 32 + t: (B, cout, t) float64"""
    c8, rows = (cout + 7) // 8, em["rows"]
    parts = [em[n].view(torch.bfloat16).cpu().double().view(b, c8, rows, 8) for n in ("hi", "lo")]
    return (parts[0] + parts[1]).permute(0, 1, 3, 2).reshape(b, c8 * 8, rows)[:, :cout, PLANE_LEAD:PLANE_LEAD + t]


def check_planes(name, got, t):
    """got: hi + lo of emitted planes (float64); t: Terms of act(y).  The split may lose 2^-17 |ref| per element; what is left of the error
    is held to FACTOR x the float32 evaluation's figure, as in check."""
    ref = t.ref
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    top = float(t.s.max())
    assert top > 0.0 and top == top, name
    s = t.s.clamp_min(top * 2.0 ** -24)
    ry = max(float(((f64(y) - ref).abs() / s).max()) for y in t.yards)
    rk = ((got - ref).abs() - SPLIT_REL * ref.abs()).clamp_min(0.0) / s
    worst = float(rk.max())
    print(f"FIGURE {name} planes: yardstick {ry:.3e}  kernel {worst:.3e}  (elements {rk.numel()}, S {float(s.min()):.3e} .. {top:.3e})")
    bad = rk > FACTOR * ry
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.unravel_index(rk.argmax(), rk.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {rk.numel()} plane elements beyond 2^-17 |ref| + {FACTOR:g} x yardstick {ry:.3e}; worst {idx}: "
                             f"{worst:.3e} of S {float(s[idx]):.3e} (planes {float(got[idx]):.9g}, ref {float(ref[idx]):.9g})")
    return ry, worst
