"""The bf16x3 conv kernels held to float64 PER ELEMENT, under every plan of the C ABI and every epilogue: the generic kernel (K = 1, 2, 3, 4,
the strided gather, the transposed depth-to-space), the direct K = 5..8 kernel, the planes path (pre-pass + k7q kernel, K = 5, 6, 7, both
launches, both DMA schedules) and the fused ResidualUnit forward; bias, residual, tanh, the data-gradient epilogue with its two parameter
sums, and plane emission.  Reference, scale and yardstick are tests/conv_fp64.py's, the assertion is gemm_fp64.check (no bound here comes
from running a kernel); `pytest -s` shows every FIGURE line.

What the whole-tensor `max|got - ref| <= 2e-4 max|ref|` bar of tests/test_conv_kernels.py cannot see and this module does: one product of the
three lost on one channel of many or on one tap (the old figure shrinks as 1 / Cin), an element small next to its tensor's largest, an error
that the device's own fp32 conv shares.  K = 4, 6 and 8 and the planes kernel at K = 6 run nowhere else.  And the structure the model relies on:
`out=` views inside a sentinel-filled buffer (both epilogue widths), operands inside NaN-filled buffers, out aliasing res, batch items that do
not see each other.

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import math

import pytest
import torch

import conv_fp64 as C

_terms = {}


def _leg(ops):
    return "sim" if ops.simulator else "gpu"


def _collect(fails, name, got, terms):
    """every tensor's figures are printed before the first failure is raised"""
    try:
        C.check(name, got, terms)
    except AssertionError as e:
        fails.append(str(e))


class _Knobs:
    """attributes of the ops object set for a block, put back whatever happens"""

    def __init__(self, ops, **kw):
        self.ops, self.kw = ops, kw

    def __enter__(self):
        self.keep = {k: getattr(self.ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.ops, k, v)

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            setattr(self.ops, k, v)


class Spec:
    """One conv launch: input (B, Cin, T) -> output (B, Cout, tout).  kind "conv" (weight (Cout, Cin, K)) or "tr" ((Cin, Cout, K)); mode: how
    ops.pack_bf16x3 gets the weight (0 conv, 1 data-gradient of the stride-1 conv with the transposed, tap-flipped weight, 2 transposed conv)."""

    def __init__(self, kind, b, cin, cout, t, k, stride, dil, pad, tout, mode, q=False):
        self.kind, self.b, self.cin, self.cout, self.t, self.k = kind, b, cin, cout, t, k
        self.stride, self.dil, self.pad, self.tout, self.mode, self.q = stride, dil, pad, tout, mode, q
        self.geom = C.Geom(kind, k, stride, dil, pad, tout)

    def key(self):
        return (self.kind, self.b, self.cin, self.cout, self.t, self.k, self.stride, self.dil, self.pad, self.tout, self.mode, self.q)

    def __repr__(self):
        name = {0: "conv", 1: "dgrad", 2: "convtr"}[self.mode] + ("-q" if self.q else "")
        return f"{name}-B{self.b}-{self.cin}to{self.cout}-T{self.t}-K{self.k}-s{self.stride}-d{self.dil}"


def s1(b, cin, cout, t, k, dil=1, q=False):
    """stride 1; even K: the asymmetric padding the model's contract allows (pad = (K - 1) dil // 2 and the resulting tout)"""
    pad = (k - 1) * dil // 2
    return Spec("conv", b, cin, cout, t, k, 1, dil, pad, t + 2 * pad - (k - 1) * dil, 0, q)


def s1_dgrad(b, cin, cout, t, k, dil=1, q=False):
    """the data-gradient of s1(b, cout, cin, t, ...): reads dy (B, cin, t + 2 pad_f - (K - 1) dil), writes (B, cout, t)"""
    pad_f = (k - 1) * dil // 2
    return Spec("conv", b, cin, cout, t + 2 * pad_f - (k - 1) * dil, k, 1, dil, (k - 1) * dil - pad_f, t, 1, q)


def down(b, cin, cout, t, s):
    pad = math.ceil(s / 2)
    return Spec("conv", b, cin, cout, t, 2 * s, s, 1, pad, (t + 2 * pad - 2 * s) // s + 1, 0)


def up(b, cin, cout, t, s):
    pad = math.ceil(s / 2)
    return Spec("tr", b, cin, cout, t, 2 * s, s, 1, pad, (t - 1) * s - 2 * pad + 2 * s, 2)


def _data(sp):
    """CPU tensors of one spec, seeded per case, made once and never written: the distributions of test_conv_kernels.py"""
    key = ("data",) + sp.key()
    if key not in _terms:
        gen = torch.Generator().manual_seed(hash((sp.kind == "tr",) + sp.key()[1:-1]) % 2 ** 31)      # (ints only: the same in every process; q or not: the same tensors)
        rn = lambda *shape, s=1.0: torch.randn(*shape, generator=gen) * s
        wshape = (sp.cin, sp.cout, sp.k) if sp.kind == "tr" else (sp.cout, sp.cin, sp.k)
        _terms[key] = {"x": rn(sp.b, sp.cin, sp.t), "la": rn(sp.cin, s=.3), "lb": rn(sp.cin, s=.3), "w": rn(*wshape, s=.2), "bias": rn(sp.cout),
                       "res": rn(sp.b, sp.cout, sp.tout), "x2": rn(sp.b, sp.cout, sp.tout), "la2": rn(sp.cout, s=.3), "lb2": rn(sp.cout, s=.3),
                       "ela": rn(sp.cout, s=.3), "elb": rn(sp.cout, s=.3)}
    return _terms[key]


def _acc_terms(sp, snake, bias):
    """Terms of conv(act(x)) [+ bias], shared by every epilogue of the spec"""
    key = ("acc", snake, bias) + sp.key()[:-1]
    if key not in _terms:
        d = _data(sp)
        t = C.conv(C.act(C.inp(d["x"]), (d["la"], d["lb"]) if snake else None), d["w"], sp.geom, d["bias"] if bias else None)
        if sp.mode == 1 and not bias and not snake:        # the data-gradient's reference is autograd of the forward conv
            w_fwd = d["w"].flip(2).transpose(0, 1).contiguous()
            t = C.Terms(C.conv_dgrad_ref(d["x"], w_fwd, (sp.k - 1) * sp.dil - sp.pad, sp.dil, sp.tout), t.s, t.yards)
        _terms[key] = t
    return _terms[key]


def _weights(ops, dev, sp):
    w = _data(sp)["w"]
    if sp.mode == 1:
        w = w.flip(2).transpose(0, 1).contiguous()           # the forward conv's (Cout_f, Cin_f, K)
    return ops.pack_bf16x3(w.to(dev), sp.mode, sp.stride, q=sp.q)


def _launch(ops, dev, sp, snake=False, bias=False, res=False, tanh_out=False, dsn=False, out=None, emit=None, t=None):
    """one call through the ABI; t: device tensors in place of the spec's own (x, res, x2)"""
    d = _data(sp)
    t = t or {}
    g = lambda n: t[n] if n in t else d[n].to(dev)
    kw = {"tout": sp.tout, "bias": g("bias") if bias else None, "snake": (g("la"), g("lb")) if snake else None, "res": g("res") if res else None,
          "tanh_out": tanh_out, "dsnake": (g("x2"), g("la2"), g("lb2")) if dsn else None}
    wp = _weights(ops, dev, sp)
    if sp.kind == "tr":
        assert out is None and emit is None
        return ops.convtr1d_bf16x3(g("x"), wp, sp.cout, sp.k, sp.stride, sp.pad, **kw)
    return ops.conv1d_bf16x3(g("x"), wp, sp.cout, sp.k, sp.stride, sp.dil, sp.pad, out=out, emit=emit, **kw)


def _forward(ops, dev, sp, fails, snake=True, tag=""):
    got = _launch(ops, dev, sp, snake=snake, bias=True)
    _collect(fails, f"{sp} fwd{'' if snake else ' plain'}{tag} {_leg(ops)}", got, _acc_terms(sp, snake, True))
    return got


def _ids(cases):
    return [repr(c) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the generic kernel: 128-channel x 128-step tiles, four waves of 64 x 64
# ---------------------------------------------------------------------------------------------------------------------
# K = 1, plan (4, 4), 32-channel chunks.  Cin: a partial group of 8 / a partial chunk / 1 .. 5 chunks; Cout: one 32-row half / a second half / a
# second wave row / a partial second channel tile; T: under one tile / one tile / one step past it / a partial third tile (Tout % 4 == 0 and != 0:
# both epilogue widths)
K1_CASES = [s1(1, 24, 8, 100, 1), s1(1, 64, 40, 128, 1), s1(1, 70, 70, 130, 1), s1(2, 160, 130, 388, 1), s1(1, 24, 130, 131, 1), s1(1, 70, 8, 388, 1)]
# K = 2: plan (8, 4); K = 3, 4: plan (8, 2), 16-channel chunks (K = 4: four taps per sub-block)
K234_CASES = [s1(1, cin, cout, t, k) for k, rows in ((2, ((9, 5, 140), (12, 40, 300), (40, 130, 261))), (3, ((9, 130, 261), (12, 5, 300), (40, 40, 140))),
                                                     (4, ((9, 40, 300), (12, 130, 140), (40, 5, 261), (9, 5, 131)))) for cin, cout, t in rows]
# strided, K = 2 S: the gather instantiation (8, 4).  Cin S below / at / above one 32-virtual-channel chunk; three and more time tiles (interior tiles
# take the vector staging loads): S = 2 at T = 800, S = 4 at T = 1100, S = 8 at T = 2120 (the smallest lengths with an interior tile)
DOWN_CASES = [down(1, 5, 16, 256, 2), down(1, 16, 20, 333, 2), down(2, 40, 6, 800, 2), down(1, 5, 9, 1100, 4), down(1, 8, 130, 300, 4), down(2, 12, 20, 333, 4),
              down(1, 3, 8, 300, 8), down(1, 4, 20, 520, 8), down(1, 6, 130, 2120, 8), down(1, 6, 9, 264, 2),
              down(1, 40, 6, 300, 4)]        # 160 virtual channels: five chunks
# transposed: the depth-to-space epilogue (out_shift = pad).  Cout S on both sides of the 128 tile, odd Cout; T of 3, 33 and one with interior tiles
UP_CASES = [up(1, 16, 7, 3, 2), up(2, 12, 70, 33, 2), up(1, 6, 5, 300, 2), up(1, 12, 5, 33, 4), up(1, 40, 40, 3, 4), up(1, 8, 31, 300, 4), up(1, 6, 33, 132, 4),
            up(1, 6, 5, 3, 8), up(2, 24, 20, 33, 8), up(1, 10, 7, 300, 8), up(1, 12, 16, 70, 8), up(1, 130, 12, 68, 8)]       # (130 input channels: five chunks)
GENERIC_CASES = K1_CASES + K234_CASES + DOWN_CASES + UP_CASES


def _generic(ops, dev, sp):
    fails = []
    _forward(ops, dev, sp, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("sp", GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_generic_sim(emu, sp):
    _generic(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_generic_gpu(hip, sp):
    _generic(hip, "cuda", sp)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the direct K = 5..8 kernel: 128 x 256 tiles, eight waves, 8-channel chunks (plain weights).  Cin: fewer than 8 channels and 1 .. 5 chunks
#    (prologue, steady state, tail; Cin % 8 != 0: the EXACT = false clamp); K = 8: the only K whose tap group 7 holds a real tap
# ---------------------------------------------------------------------------------------------------------------------
DIRECT_CASES = [s1(1, 3, 8, 131, 7, 1), s1(1, 8, 70, 256, 7, 3), s1(2, 20, 130, 257, 7, 9), s1(1, 40, 6, 520, 7, 3),
                s1(1, 20, 40, 257, 5, 2), s1(1, 8, 5, 131, 5, 1), s1(1, 40, 130, 256, 6, 1), s1(1, 3, 40, 520, 6, 3),
                s1(1, 20, 70, 257, 8, 1), s1(1, 40, 8, 131, 8, 3), s1(1, 3, 130, 300, 8, 3), s1(1, 8, 8, 520, 8, 1)]


def _direct(ops, dev, sp):
    fails = []
    _forward(ops, dev, sp, fails, snake=True)        # both SNAKE instantiations
    _forward(ops, dev, sp, fails, snake=False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("sp", DIRECT_CASES, ids=_ids(DIRECT_CASES))
def test_direct_sim(emu, sp):
    _direct(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", DIRECT_CASES, ids=_ids(DIRECT_CASES))
def test_direct_gpu(hip, sp):
    _direct(hip, "cuda", sp)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the planes path: pre-pass + k7q kernel, 16-channel chunks (q-packed weights), K = 5, 6, 7; the persistent and the one-tile launch, the DMA
#    inside and beside the MFMA sections: four runs, each within the bound, all bit-equal
# ---------------------------------------------------------------------------------------------------------------------
PLANES_CASES = [s1(1, 20, 5, 90, 5, 1, q=True), s1(1, 24, 130, 300, 6, 3, q=True), s1(2, 40, 136, 517, 7, 9, q=True), s1(1, 24, 136, 90, 7, 1, q=True),
                s1(1, 40, 5, 300, 5, 9, q=True), s1(1, 20, 130, 517, 6, 1, q=True), s1(1, 20, 136, 300, 7, 3, q=True), s1(1, 40, 130, 90, 6, 9, q=True),
                s1(1, 24, 5, 517, 5, 3, q=True)]
PLANES_RUNS = [(p, v) for p in ("force", False) for v in (True, False)]


def _planes(ops, dev, sp):
    fails, first = [], None
    for persist, in_mfma in PLANES_RUNS:
        with _Knobs(ops, k7q=True, k7q_min_cin=1, k7q_min_cout=1, k7q_persist=persist, k7q_dma_in_mfma=in_mfma):
            got = _forward(ops, dev, sp, fails, tag=f" persist={persist} dma_in_mfma={in_mfma}")
        first = got if first is None else first
        assert torch.equal(got, first), (sp, persist, in_mfma)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("sp", PLANES_CASES, ids=_ids(PLANES_CASES))
def test_planes_sim(emu, sp):
    _planes(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", PLANES_CASES, ids=_ids(PLANES_CASES))
def test_planes_gpu(hip, sp):
    _planes(hip, "cuda", sp)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the fused ResidualUnit forward: y = x + conv1(snake2(conv7(snake1(x)) + b1)) + b2 in one launch; y and the kept h, with and without emission
# ---------------------------------------------------------------------------------------------------------------------
RU_CASES = [(1, 16, 256, 1, 7), (2, 24, 520, 3, 7), (1, 72, 260, 9, 7), (1, 128, 256, 3, 7), (1, 24, 260, 9, 5), (1, 128, 520, 1, 7)]     # (B, C, T, dil, K)


def _ru(ops, dev, case):
    b, c, t, dil, k = case
    gen = torch.Generator().manual_seed(c * 1000 + t + dil + k)
    rn = lambda *shape, s=1.0: torch.randn(*shape, generator=gen) * s
    x = rn(b, c, t)
    sn1, sn2, esn = (rn(c, s=.3), rn(c, s=.3)), (rn(c, s=.3), rn(c, s=.3)), (rn(c, s=.3), rn(c, s=.3))
    w1, b1 = rn(c, c, k, s=.2 / math.sqrt(c / 8)), rn(c)
    w2, b2 = rn(c, c, 1, s=.5 / math.sqrt(c / 8)), rn(c)
    th = C.conv(C.act(C.inp(x), sn1), w1, s1(b, c, c, t, k, dil).geom, b1)
    ty = C.add_res(C.conv(C.act(th, sn2), w2, C.Geom("conv", 1, tout=t), b2), x)
    dv = lambda v: tuple(i.to(dev) for i in v) if isinstance(v, tuple) else v.to(dev)
    fails = []
    with _Knobs(ops, k7q=True, k7q_min_cin=1, k7q_min_cout=1):
        assert ops.ru_fused_ok(c, k, dil, t)
        args = (dv(x), dv(sn1), ops.pack_k7q(dv(w1)), dv(b1), dv(sn2), ops.pack_k7q(dv(w2)), dv(b2), k, dil)
        h, y = ops.residual_unit_fwd(*args)
        esn_d = dv(esn)
        h_e, y_e = ops.residual_unit_fwd(*args, emit=esn_d)
        em = ops._take_emitted(y_e, esn_d)
        h_n, y_n = ops.residual_unit_fwd(*args, keep_h=False)
    _collect(fails, f"ru {case} h {_leg(ops)}", h, th)
    _collect(fails, f"ru {case} y {_leg(ops)}", y, ty)
    assert h_n is None and torch.equal(y_n, y) and torch.equal(y_e, y) and torch.equal(h_e, h), "emission / keep_h changed the unit's output"
    assert em is not None
    try:
        C.check_planes(f"ru {case} emitted snake(y) {_leg(ops)}", C.planes_value(em, b, c, t), C.act(ty, esn))
    except AssertionError as e:
        fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", RU_CASES, ids=_ids(RU_CASES))
def test_residual_unit_sim(emu, case):
    _ru(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RU_CASES, ids=_ids(RU_CASES))
def test_residual_unit_gpu(hip, case):
    _ru(hip, "cuda", case)


# ---------------------------------------------------------------------------------------------------------------------
# 5. epilogues, one multi-tile case per kernel: no bias, residual, tanh(bias + residual), and the data-gradient form (B = 2, three and more
#    time tiles: every per-(b, tile) partial row is summed) with dx, d log-alpha2, d log-beta2.  The stride-1 data-gradients run on mode-1
#    weights with tout=, as the model's backward does; the strided / transposed plans take the same epilogue on their own weights.
# ---------------------------------------------------------------------------------------------------------------------
EPI_CASES = [s1(2, 70, 70, 388, 1), s1(2, 12, 40, 301, 3), s1(2, 40, 9, 300, 4), down(2, 6, 20, 1100, 4), up(2, 12, 7, 300, 2),
             s1(2, 20, 40, 520, 7, 3), s1(2, 8, 130, 521, 8, 1), s1(2, 24, 130, 520, 7, 3, q=True), s1(2, 20, 5, 517, 6, 1, q=True)]
DGRAD_CASES = [s1_dgrad(2, 70, 70, 388, 1), s1_dgrad(2, 40, 12, 301, 3), s1_dgrad(2, 9, 40, 300, 4), down(2, 6, 20, 1100, 4), up(2, 12, 7, 300, 2),
               s1_dgrad(2, 40, 20, 520, 7, 3), s1_dgrad(2, 130, 8, 521, 8, 1), s1_dgrad(2, 130, 24, 520, 7, 3, q=True), s1_dgrad(2, 5, 20, 517, 6, 1, q=True),
               s1_dgrad(2, 20, 130, 600, 5, 9),
               # 128 and more output channels with a time tile inside the tensor: the 16-byte epilogue's unchecked x2 / res loads
               s1_dgrad(2, 24, 130, 388, 1), s1_dgrad(2, 24, 136, 520, 7, 1, q=True)]


def _epilogues(ops, dev, sp):
    d, fails = _data(sp), []
    plain, full = _acc_terms(sp, True, False), _acc_terms(sp, True, True)
    with _Knobs(ops, k7q_persist="force"):
        _collect(fails, f"{sp} no-bias {_leg(ops)}", _launch(ops, dev, sp, snake=True), plain)
        _collect(fails, f"{sp} res {_leg(ops)}", _launch(ops, dev, sp, snake=True, res=True), C.add_res(plain, d["res"]))
        got = _launch(ops, dev, sp, snake=True, bias=True, res=True, tanh_out=True)
        _collect(fails, f"{sp} tanh(bias + res) {_leg(ops)}", got, C.tanh(C.add_res(full, d["res"])))
        _collect(fails, f"{sp} tanh(bias + res), own rounding in S {_leg(ops)}", got, C.tanh(C.add_res(full, d["res"]), own=True))
    assert not fails, "\n".join(fails)


def _dgrad(ops, dev, sp):
    d, fails = _data(sp), []
    for res in (False, True):
        terms = C.dgrad(_acc_terms(sp, False, False), d["x2"], d["la2"], d["lb2"], d["res"] if res else None)
        with _Knobs(ops, k7q_persist="force"):
            got = _launch(ops, dev, sp, dsn=True, res=res)
        for name, g, t in zip(("dx", "dlog-alpha2", "dlog-beta2"), got, terms):
            _collect(fails, f"{sp} {name}{' + res' if res else ''} {_leg(ops)}", g, t)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("sp", EPI_CASES, ids=_ids(EPI_CASES))
def test_epilogues_sim(emu, sp):
    _epilogues(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", EPI_CASES, ids=_ids(EPI_CASES))
def test_epilogues_gpu(hip, sp):
    _epilogues(hip, "cuda", sp)


@pytest.mark.parametrize("sp", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_data_gradient_sim(emu, sp):
    _dgrad(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_data_gradient_gpu(hip, sp):
    _dgrad(hip, "cuda", sp)


# plane emission of the generic kernel's 16-byte epilogue (K = 1 and strided plans; Tout % 4 == 0): hi + lo of the planes against float64
# act(reference y), per element: 2^-17 |ref| for the split + FACTOR x the float32 evaluation's figure
EMIT_CASES = [s1(2, 24, 20, 132, 1), s1(1, 70, 40, 388, 1), s1(1, 24, 128, 260, 1), down(2, 6, 20, 1040, 4), down(1, 12, 130, 528, 2)]


def _emission(ops, dev, sp):
    d, fails = _data(sp), []
    ty = _acc_terms(sp, True, True)
    esn = (d["ela"].to(dev), d["elb"].to(dev))
    for emit in (esn, True):
        snake = None if emit is True else emit
        y = _launch(ops, dev, sp, snake=True, bias=True, emit=emit)
        em = ops._take_emitted(y, snake)
        assert em is not None
        _collect(fails, f"{sp} y emit={'act' if snake else 'plain'} {_leg(ops)}", y, ty)
        try:
            C.check_planes(f"{sp} emitted {'snake(y)' if snake else 'y'} {_leg(ops)}", C.planes_value(em, sp.b, sp.cout, sp.tout), C.act(ty, snake))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("sp", EMIT_CASES, ids=_ids(EMIT_CASES))
def test_emission_sim(emu, sp):
    _emission(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", EMIT_CASES, ids=_ids(EMIT_CASES))
def test_emission_gpu(hip, sp):
    _emission(hip, "cuda", sp)


# ---------------------------------------------------------------------------------------------------------------------
# structure: the generic (K = 1, K = 3, strided), the direct and the planes kernel.  Partial last time tile and partial channel tile; Tout % 4 == 0
# and != 0
# ---------------------------------------------------------------------------------------------------------------------
STRUCT_CASES = [s1(2, 24, 130, 132, 1), s1(2, 24, 130, 131, 1), s1(2, 12, 40, 261, 3), down(2, 6, 130, 1100, 4), s1(2, 20, 130, 260, 7, 3), s1(2, 20, 130, 261, 8, 1),
                s1(2, 24, 130, 260, 7, 3, q=True), s1(2, 24, 130, 259, 6, 1, q=True)]
SENTINEL = -7.75
GUARD = 64                   # floats around a view (a multiple of 4: the view's alignment is its offset's)


def _view(buf_fill, like, off):
    """a dense copy of `like` inside a larger buffer filled with buf_fill, starting `off` floats past GUARD"""
    buf = torch.full((like.numel() + 2 * GUARD + 8,), buf_fill, dtype=torch.float32, device=like.device)
    view = buf[GUARD + off:GUARD + off + like.numel()].view(like.shape)
    view.copy_(like)
    return buf, view


def _outside(buf, view, off):
    return torch.cat([buf[:GUARD + off], buf[GUARD + off + view.numel():]])


def _output_guard(ops, dev, sp):
    fails = []
    d = _data(sp)
    terms = C.add_res(_acc_terms(sp, True, True), d["res"])
    shape = torch.empty(sp.b, sp.cout, sp.tout, device=dev)
    outs = {}
    for off in (4, 5):
        buf, view = _view(SENTINEL, shape, off)
        view.fill_(SENTINEL)
        assert view.data_ptr() % 16 == (0 if off == 4 else 4)
        with _Knobs(ops, k7q_persist="force"):
            got = _launch(ops, dev, sp, snake=True, bias=True, res=True, out=view)
        assert got.data_ptr() == view.data_ptr()
        assert bool((_outside(buf, view, off) == SENTINEL).all()), f"{sp} out= at offset {off}: a float outside the view was written"
        outs[off] = view
    with _Knobs(ops, k7q_persist="force"):                 # only now, the sentinels found intact, the call that allocates its own output
        base = _launch(ops, dev, sp, snake=True, bias=True, res=True)
    assert torch.equal(outs[4], base), f"{sp}: the aligned out= view differs from the call without out="
    _collect(fails, f"{sp} out= offset 4 {_leg(ops)}", outs[4], terms)
    _collect(fails, f"{sp} out= offset 5 (4-byte epilogue) {_leg(ops)}", outs[5], terms)
    assert not fails, "\n".join(fails)


def _input_guard(ops, dev, sp, dsp):
    fails = []
    for off in (4, 5):
        d = _data(sp)
        t = {n: _view(float("nan"), d[n].to(dev), off)[1] for n in ("x", "res")}
        with _Knobs(ops, k7q_persist="force"):
            got = _launch(ops, dev, sp, snake=True, bias=True, res=True, t=t)
        _collect(fails, f"{sp} operands in NaN at offset {off} {_leg(ops)}", got, C.add_res(_acc_terms(sp, True, True), d["res"]))
        d = _data(dsp)
        t = {n: _view(float("nan"), d[n].to(dev), off)[1] for n in ("x", "res", "x2")}
        with _Knobs(ops, k7q_persist="force"):
            got = _launch(ops, dev, dsp, dsn=True, res=True, t=t)
        terms = C.dgrad(_acc_terms(dsp, False, False), d["x2"], d["la2"], d["lb2"], d["res"])
        for name, g, tt in zip(("dx", "dlog-alpha2", "dlog-beta2"), got, terms):
            _collect(fails, f"{dsp} {name} operands in NaN at offset {off} {_leg(ops)}", g, tt)
    assert not fails, "\n".join(fails)


def _in_place(ops, dev, sp):
    d = _data(sp)
    with _Knobs(ops, k7q_persist="force"):
        base = _launch(ops, dev, sp, snake=True, bias=True, res=True)
        acc = d["res"].to(dev).clone()
        got = _launch(ops, dev, sp, snake=True, bias=True, res=True, out=acc, t={"res": acc})
        assert got.data_ptr() == acc.data_ptr() and torch.equal(acc, base), f"{sp}: out aliasing res"
        dbase = _launch(ops, dev, sp, dsn=True, res=True)
        acc = d["res"].to(dev).clone()
        dgot = _launch(ops, dev, sp, dsn=True, res=True, out=acc, t={"res": acc})
        assert all(torch.equal(a, b) for a, b in zip(dgot, dbase)), f"{sp}: data-gradient with out aliasing res"


def _batch_independence(ops, dev, sp):
    assert sp.b == 2
    d = _data(sp)
    one = Spec(sp.kind, 1, sp.cin, sp.cout, sp.t, sp.k, sp.stride, sp.dil, sp.pad, sp.tout, sp.mode, sp.q)
    _terms[("data",) + one.key()] = {n: (v[:1].contiguous() if v.dim() == 3 and n != "w" else v) for n, v in d.items()}
    t = {}
    for n in ("x", "res", "x2"):
        t[n] = d[n].to(dev).clone()
        t[n][1] = float("nan")
    with _Knobs(ops, k7q_persist="force"):
        for kw in ({"snake": True, "bias": True, "res": True}, {"dsn": True, "res": True}):
            two, ref = _launch(ops, dev, sp, t=t, **kw), _launch(ops, dev, one, **kw)
            two, ref = (two[0], ref[0]) if "dsn" in kw else (two, ref)        # (the parameter sums run over the batch)
            assert bool(torch.isfinite(ref).all()) and torch.equal(two[:1], ref), f"{sp} {sorted(kw)}: item 0 saw item 1"


_DG = {sp.key(): Spec(sp.kind, sp.b, sp.cout, sp.cin, sp.tout, sp.k, 1, sp.dil, (sp.k - 1) * sp.dil - sp.pad, sp.t, 1, sp.q) if sp.stride == 1 else sp
       for sp in STRUCT_CASES}      # the stride-1 convs' own data-gradients; the strided plan takes the epilogue on its own weights


@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_output_guard_sim(emu, sp):
    _output_guard(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_output_guard_gpu(hip, sp):
    _output_guard(hip, "cuda", sp)


@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_input_guard_sim(emu, sp):
    _input_guard(emu, "cpu", sp, _DG[sp.key()])


@pytest.mark.gpu
@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_input_guard_gpu(hip, sp):
    _input_guard(hip, "cuda", sp, _DG[sp.key()])


@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_in_place_sim(emu, sp):
    _in_place(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_in_place_gpu(hip, sp):
    _in_place(hip, "cuda", sp)


@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_batch_independence_sim(emu, sp):
    _batch_independence(emu, "cpu", sp)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_batch_independence_gpu(hip, sp):
    _batch_independence(hip, "cuda", sp)
