"""Float64 reference, storage-precision yardstick and per-ELEMENT check of the projection GEMMs of csrc/gemm.hip
(tests/test_gemm_fp64.py).  The rule is fp64_bounds.py's with a scale per element: nothing here comes from running a kernel.

  reference   the operation in float64 from the operands the kernel saw: the bf16-rounded values (for the fp32-model path the
              [hi|hi|lo] x [hi|lo|hi] planes that split_bf16x3 produced, whose products are hi.hi + hi.lo + lo.hi), the fp32 bias,
              the residual and gate in the output dtype, the fp32 rotary table the library built.
  scale S     per element, float64: the sum of the magnitudes of the terms that form the element, carried to first order through the
              epilogue (each function below states its line); floored at 2^-24 of the tensor's largest S, so that underflow (a
              saturated sigmoid) cannot fail a correct kernel.
  yardstick   the same formulas in torch float32 on the CPU.  The matmul is taken two ways, torch's blocked `a @ b.t()` and a k-ordered
              chain `acc += a[:, k] * b[:, k]` (the order a K loop of MFMAs adds in); every epilogue runs on both and the LARGER figure
              is the yardstick.  sigmoid = 1 / (1 + exp(-x)) in fp32; the rotary table is the library's, in fp32.
  assert      max over the elements of |kernel - ref64| / S  <=  FACTOR x the yardstick's; a bf16 tensor first takes 2^-8 |ref64| off
              the kernel's error, element by element (one final rounding: a truncating store, a second rounding or an operand rounded
              on the way do not fit).  The allowance of a bf16 tensor is the float32 evaluation's figure, unrounded, as in
              fp64_bounds.check: the kernel computes in fp32 and rounds once, so its error past 2^-8 |ref64| is its fp32 error.  (Rounding
              the yardstick to bf16 and taking 2^-8 |ref64| off it as well leaves only the elements where a rounding tie fell the other
              way — a figure that is 0 for whole tensors, e.g. the 150800 elements of RES at (290, 520, 328), and would then refuse every
              kernel that adds in another order than the yardstick, split-K for one.)"""
import torch

from fp64_bounds import BF16_HALF_ULP, FACTOR, f64

F32, BF16 = torch.float32, torch.bfloat16


class Terms:
    """ref: float64 values; s: float64 per-element scale; yards: the float32 evaluations (one per matmul order)"""

    def __init__(self, ref, s, yards):
        self.ref, self.s, self.yards = ref, s, list(yards)

    def cols(self, lo, hi):
        return Terms(self.ref[:, lo:hi], self.s[:, lo:hi], [y[:, lo:hi] for y in self.yards])


def projection(a, b, planes=1):
    """A . B^T without bias.  S = |A| . |B|^T.  planes = 3: a, b are split_bf16x3 planes (M, 3K) / (N, 3K); the blocked yardstick then
    forms hi.hi + hi.lo + lo.hi as three float32 matmuls, the chain runs over the 3K columns in the kernel's order."""
    a64, b64 = f64(a), f64(b)
    a32, b32 = a64.float(), b64.float()
    assert torch.equal(a32.double(), a64) and torch.equal(b32.double(), b64)      # bf16 values: exact in float32
    k = a32.shape[1] // planes
    blocked = a32[:, :k] @ b32[:, :k].t()
    for i in range(1, planes):
        blocked = blocked + a32[:, i * k:(i + 1) * k] @ b32[:, i * k:(i + 1) * k].t()
    chain = torch.zeros(a32.shape[0], b32.shape[0])
    bt = b32.t().contiguous()
    for j in range(a32.shape[1]):        # (products of bf16 values are exact in float32: fused or not, the chain rounds once per step)
        chain.addcmul_(a32[:, j, None], bt[j][None, :])
    return Terms(a64 @ b64.t(), a64.abs() @ b64.abs().t(), [blocked, chain])


def add_bias(t, bias):
    """+ bias: S_x = |A| . |B|^T + |bias|"""
    b64 = f64(bias)
    return Terms(t.ref + b64, t.s + b64.abs(), [y + b64.float() for y in t.yards])


def sigmoid32(x):
    return 1.0 / (1.0 + torch.exp(-x))


def epi_res(t, res):
    """x + res: S = S_x + |res|"""
    r = f64(res)
    return Terms(t.ref + r, t.s + r.abs(), [y + r.float() for y in t.yards])


def epi_gate_res(t, res, gate, rows_per_gate):
    """x sigmoid(1 - g[m // rows_per_gate]) + res: S = sigmoid(1 - g) S_x + |res|"""
    r = f64(res)
    g = f64(gate)[torch.arange(t.ref.shape[0]) // rows_per_gate]
    sg = torch.sigmoid(1.0 - g)
    return Terms(t.ref * sg + r, sg * t.s + r.abs(), [y * sigmoid32(1.0 - g.float()) + r.float() for y in t.yards])


def epi_swiglu(t):
    """out = x silu(g) over columns [x | g]: S = |silu(g)| S_x + |x silu'(g)| S_g"""
    f = t.ref.shape[1] // 2
    x, g, sx, sgate = t.ref[:, :f], t.ref[:, f:], t.s[:, :f], t.s[:, f:]
    sig = torch.sigmoid(g)
    silu, dsilu = g * sig, sig * (1.0 + g * (1.0 - sig))
    return Terms(x * silu, silu.abs() * sx + (x * dsilu).abs() * sgate, [y[:, :f] * y[:, f:] * sigmoid32(y[:, f:]) for y in t.yards])


# ---- head-split epilogues: per-head norm, partial rotary, plane layout -------------------------------------------------------------
def _norm(x, mode, gamma, beta, eps, s=None):
    """x (..., 64) in its own dtype -> (y, S_y or None).  "ln": y = (x - mean) rstd gamma + beta, biased variance; "l2": x / max(|x|, 1e-12).
    S to first order: dy_d = gamma_d (rstd (dx_d - dmean) + (x_d - mean) drstd), |dmean| <= mean(S), |drstd| <= rstd^3 / 64 sum_j
    |x_j - mean| (S_j + mean(S)); beta enters in magnitude.  l2: dy_d = dx_d / n - x_d / n^3 sum_j x_j dx_j."""
    if mode == "ln":
        mean = x.sum(-1, keepdim=True) * (1.0 / 64.0)
        xc = x - mean
        rstd = 1.0 / torch.sqrt((xc * xc).sum(-1, keepdim=True) * (1.0 / 64.0) + eps)
        y = xc * rstd * gamma + beta
        if s is None:
            return y, None
        sc = s + s.mean(-1, keepdim=True)
        srstd = rstd ** 3 / 64.0 * (xc.abs() * sc).sum(-1, keepdim=True)
        return y, gamma.abs() * (rstd * sc + xc.abs() * srstd) + beta.abs()
    assert mode == "l2"
    nrm = torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)
    y = x / nrm
    if s is None:
        return y, None
    return y, s / nrm + x.abs() / nrm ** 3 * (x.abs() * s).sum(-1, keepdim=True)


def _rotary(x, c, sn, s=None):
    """x (nb, ntok, H, 64), c / sn (ntok, 1, 16): pairs (d, d + 16) of the first 32 dims (transformer.py's rotate_half on a 32-dim
    rotary).  S = |cos| S_d + |sin| S_partner."""
    lo, hi, rest = x[..., :16], x[..., 16:32], x[..., 32:]
    y = torch.cat([lo * c - hi * sn, hi * c + lo * sn, rest], dim=-1)
    if s is None:
        return y, None
    slo, shi = s[..., :16], s[..., 16:32]
    return y, torch.cat([slo * c.abs() + shi * sn.abs(), shi * c.abs() + slo * sn.abs(), s[..., 32:]], dim=-1)


def heads(t, cs, heads_, nb, ntok, sec0, nsec, mode=None, tabs=None, eps=1e-6):
    """t: projection Terms of x (nb ntok, K) . w (nsec H 64, K)^T.  -> {"q" / "k": Terms shaped (nb, H, ntok, 64), "v_tr": (nb, H, 64, ntok)},
    the valid part of the planes gemm_heads_bf16 returns.  cs: the (ntab, 16, 2) fp32 table (rows ntab - ntok .. are used) or None;
    tabs: (q gamma, q beta, k gamma, k beta) fp32 for "ln"."""
    out = {}
    if cs is not None:
        tab = cs.detach().cpu()[cs.shape[0] - ntok:]
        c32, s32 = tab[:, None, :, 0], tab[:, None, :, 1]
    for i in range(nsec):
        which = sec0 + i
        sec = t.cols(i * heads_ * 64, (i + 1) * heads_ * 64)
        shape = (nb, ntok, heads_, 64)
        ref, s, yards = sec.ref.reshape(shape), sec.s.reshape(shape), [y.reshape(shape) for y in sec.yards]
        if which == 2:
            out["v_tr"] = Terms(ref.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1), [y.permute(0, 2, 3, 1) for y in yards])
            continue
        if mode is not None:
            g, b = (tabs[2 * which], tabs[2 * which + 1]) if mode == "ln" else (None, None)
            g64, b64 = (f64(g), f64(b)) if mode == "ln" else (None, None)
            ref, s = _norm(ref, mode, g64, b64, eps, s)
            yards = [_norm(y, mode, g.cpu() if g is not None else None, b.cpu() if b is not None else None, eps)[0] for y in yards]
        if cs is not None:
            ref, s = _rotary(ref, c32.double(), s32.double(), s)
            yards = [_rotary(y, c32, s32)[0] for y in yards]
        out["qk"[which]] = Terms(ref.permute(0, 2, 1, 3), s.permute(0, 2, 1, 3), [y.permute(0, 2, 1, 3) for y in yards])
    return out


# ---- the check ------------------------------------------------------------------------------------------------------------------------
def _ratio(x, ref64, s):
    err = (f64(x) - ref64).abs()
    if x.dtype == BF16:
        err = (err - BF16_HALF_ULP * ref64.abs()).clamp_min(0.0)
    return err / s


def check(name, got, t):
    """got: the kernel's tensor (fp32 or bf16, any device), t: Terms of the same shape.  Prints both figures, then asserts every element."""
    got = got.detach().cpu()
    ref, s = t.ref, t.s
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    assert got.dtype in (F32, BF16)
    assert bool(torch.isfinite(got.double()).all()), f"{name}: not finite"
    top = float(s.max())
    assert top > 0.0 and top == top, name
    s = s.clamp_min(top * 2.0 ** -24)
    ry = max(float(((f64(y) - ref).abs() / s).max()) for y in t.yards)
    rk = _ratio(got, ref, s)
    worst = float(rk.max())
    print(f"FIGURE {name} {str(got.dtype)[6:]}: yardstick {ry:.3e}  kernel {worst:.3e}  (elements {rk.numel()}, S {float(s.min()):.3e} .. {top:.3e})")
    bad = rk > FACTOR * ry
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.unravel_index(rk.argmax(), rk.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {rk.numel()} elements beyond {FACTOR:g} x yardstick {ry:.3e}; worst {idx}: {worst:.3e} "
                             f"of S {float(s[idx]):.3e} (kernel {float(got[idx]):.9g}, ref {float(ref[idx]):.9g})")
    return ry, worst
