"""The conv WEIGHT-gradient kernels held to float64 PER ELEMENT, under every split plan of the C ABI: the 4-wave and the pipelined k = 7 kernel
(csrc/conv_wgrad_bf16x3.hip, conv_wgrad7_bf16x3_pipe.h), the planes kernel (conv_wgrad7_planes.h, both MFMA shapes), the short-kernel wgrad
(K = 1, K = 2 S, both conv orientations), the fp32 kernel (conv_wgrad.hip, every instantiation), the edge wgrad (edge_conv.hip, both forms), the
fused 1x1 backward (ru_k1_bwd.hip, six outputs + emitted planes), sat_reduce_splits and sat_rowsum.  Reference, scale and yardstick are
tests/wgrad_fp64.py's, the assertion is gemm_fp64.check (no bound here comes from running a kernel); `pytest -s` shows every FIGURE line.

What the whole-tensor `max|got - ref| <= 2e-4 max|ref|` bar of tests/test_conv_kernels.py and the `2 x the pipelined kernel's L2` bar of
tests/test_wgrad7_planes.py cannot see and this module does: one lo x hi product lost on one channel or tap, one 64-step stage skipped in one
split of many, an element small next to its tensor's largest, an error two kernels share.  Every test asserts the plan it means to reach (slabs,
stages per split, a ragged last split, a split that crosses a batch boundary) through the library's own *_nsplit / *_fuses_rowsum / *_ok entry points
BEFORE it looks at a value.  And the structure: every element of every slab and every [m][split] row sum written, nothing written beyond them,
both slab layouts, operands inside NaN-filled buffers, exact results on small integers.

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import ctypes
import math

import pytest
import torch

import wgrad_fp64 as W

_cache = {}
GPU_CUS = 256                # the MI355X; the plans of the edge wgrad and of ru_k1_bwd depend on it


def _leg(ops):
    return "sim" if ops.simulator else "gpu"


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _collect(fails, name, got, terms):
    """every tensor's figures are printed before the first failure is raised"""
    try:
        W.check(name, got, terms)
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


class _Cus:
    """the simulator's CU count for a block (the GPU leg runs on the device's own)"""

    def __init__(self, ops, cus):
        self.ops, self.cus = ops, cus

    def __enter__(self):
        if self.cus:
            assert self.ops.simulator
            self.ops.lib.sat_emu_set_cu_count(self.cus)

    def __exit__(self, *exc):
        if self.cus:
            self.ops.lib.sat_emu_set_cu_count(0)


UNIT = {"w4": 64, "pipe": 64, "planes": 64, "small": 64, "fp32": 32, "edge": 1024}     # time steps of one stage / chunk / tile


class Case:
    """One weight-gradient launch: lo (B, M, T), hi (B, N, thi) -> dW (M, N, K).  kern: the kernel the shape must reach; snake_on 0 / 1 (lo) / 2 (hi);
    rowsum: also the row sums of lo; plan: (slabs, stages per split, ragged last split, a split crossing a batch boundary) as the planner's source
    gives them; cus: the simulator's CU count (edge wgrad: a case with cus runs on the simulator only); variants: the planes kernel's."""

    def __init__(self, kern, b, m, n, t, k=7, stride=1, dil=1, pad=None, snake_on=2, rowsum=False, thi=None, plan=None, cus=0, variants=(2,), integer=False):
        self.kern, self.b, self.m, self.n, self.t, self.k, self.stride, self.dil = kern, b, m, n, t, k, stride, dil
        self.pad = (k - 1) * dil // 2 if pad is None else pad
        self.snake_on, self.rowsum, self.plan, self.cus, self.variants, self.integer = snake_on, rowsum, plan, cus, variants, integer
        self.thi = t if thi is None else thi
        self.x3 = kern not in ("fp32", "edge")

    def key(self):
        return (self.kern, self.b, self.m, self.n, self.t, self.k, self.stride, self.dil, self.pad, self.snake_on, self.thi, self.integer)

    def but(self, **kw):
        c = Case(self.kern, self.b, self.m, self.n, self.t, self.k, self.stride, self.dil, self.pad, self.snake_on, self.rowsum, self.thi, self.plan,
                 self.cus, self.variants, self.integer)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def __repr__(self):
        tag = f"{self.kern}-B{self.b}-{self.m}x{self.n}-T{self.t}-K{self.k}-s{self.stride}-d{self.dil}-p{self.pad}-sn{self.snake_on}"
        return tag + ("-rs" if self.rowsum else "") + (f"-thi{self.thi}" if self.thi != self.t else "") + (f"-cu{self.cus}" if self.cus else "") + \
            ("-int" if self.integer else "") + ("" if self.variants == (2,) else "-v" + "".join(map(str, self.variants)))


def _ids(cases):
    return [repr(c) for c in cases]


def _data(c):
    """CPU tensors of one case, seeded per shape, made once and never written"""
    key = ("data", c.b, c.m, c.n, c.t, c.thi, c.integer)
    if key not in _cache:
        gen = torch.Generator().manual_seed(hash(key[1:]) % 2 ** 31)      # (ints only: the same in every process)
        if c.integer:
            mk = lambda *shape: torch.randint(-3, 4, shape, generator=gen).float()
        else:
            mk = lambda *shape: torch.randn(*shape, generator=gen)
        rn = lambda *shape: torch.randn(*shape, generator=gen) * .3
        _cache[key] = {"lo": mk(c.b, c.m, c.t), "hi": mk(c.b, c.n, c.thi), "la1": rn(c.m), "lb1": rn(c.m), "la2": rn(c.n), "lb2": rn(c.n)}
    return _cache[key]


def _snake(c, d, dev="cpu"):
    if c.snake_on == 0:
        return None
    return (d["la1"].to(dev), d["lb1"].to(dev)) if c.snake_on == 1 else (d["la2"].to(dev), d["lb2"].to(dev))


def _terms(c):
    key = ("dw", c.x3) + c.key()[1:]
    if key not in _cache:
        d = _data(c)
        _cache[key] = W.wgrad(d["lo"], d["hi"], c.k, c.stride, c.dil, c.pad, _snake(c, d), c.snake_on, x3=c.x3)
    return _cache[key]


def _rs_terms(c):
    key = ("rs", c.b, c.m, c.n, c.t, c.thi, c.integer)
    if key not in _cache:
        _cache[key] = W.rowsum(_data(c)["lo"])
    return _cache[key]


def _split_plan(nsplit, b, nt):
    """(slabs, stages per split, ragged last split, a split crossing a batch boundary) of nsplit slabs over b items of nt stages"""
    stages = b * nt
    assert 1 <= nsplit <= stages
    per = -(-stages // nsplit)
    assert -(-stages // per) == nsplit
    cross = any((s * per) // nt != (min((s + 1) * per, stages) - 1) // nt for s in range(nsplit))
    return nsplit, per, stages % per != 0, cross


def _rows(ops, t):
    return ops.lib.sat_conv1d_k7_plane_rows(t, t, 0)


def _assert_plan(ops, c):
    """the kernel and the split plan this case means to reach, read through the library; -> the number of slabs"""
    lib, nt = ops.lib, -(-c.t // UNIT[c.kern])
    if c.kern in ("w4", "pipe"):
        assert lib.sat_conv_wgrad7_bf16x3_fuses_rowsum(c.b, c.m, c.n, c.t) == (1 if c.kern == "w4" else 0), f"{c}: the other k = 7 kernel takes this shape"
        assert (c.kern == "pipe") == (c.n >= 64 and c.t % 4 == 0)
        ns = lib.sat_conv_wgrad7_bf16x3_nsplit(c.b, c.m, c.n, c.t)
    elif c.kern == "planes":
        assert lib.sat_conv_wgrad7_planes_ok(c.b, c.m, c.n, c.t, c.dil, c.pad, _rows(ops, c.t), _rows(ops, c.t)) == 1, c
        ns = lib.sat_conv_wgrad7_planes_nsplit(c.b, c.m, c.n, c.t)
    elif c.kern == "small":
        assert ops.use_bf16x3 and c.dil == 1
        ns = lib.sat_conv_wgrad_bf16x3_nsplit(c.b, c.m, c.n, c.t, c.k, c.stride)
        assert ns > 0, f"{c}: the short-kernel planner declines"
    elif c.kern == "fp32":
        ns = lib.sat_conv_wgrad_nsplit(c.b, c.m, c.n, c.t, c.k, c.stride, c.dil)
    else:
        assert c.kern == "edge" and ops.edge_ok(c.n, c.m, c.k, 1, 1, c.pad)
        ns = lib.sat_edge_conv_wgrad_nsplit(c.b, c.m, c.n, c.t)
        assert ns % c.b == 0
        plan = _split_plan(ns // c.b, 1, nt)            # per batch item: a slab never crosses one
        assert (ns,) + plan[1:] == c.plan, f"{c}: plan {(ns,) + plan[1:]}, meant {c.plan}"
        return ns
    plan = _split_plan(ns, c.b, nt)
    assert plan == c.plan, f"{c}: plan {plan}, meant {c.plan}"
    if plan[1] > 1:
        assert ns < c.b * nt
    return ns


def _prepass(ops, x, snake):
    """x (B, C, T) -> (hi, lo, rows): the bf16 planes of act(x) by sat_conv1d_k7_planes (tests/test_wgrad7_planes.py::_planes)"""
    b, ch, t = x.shape
    rows = _rows(ops, t)
    n = b * ((ch + 7) // 8) * rows * 8
    hi = torch.zeros(n, dtype=torch.int16, device=x.device)
    lo = torch.zeros(n, dtype=torch.int16, device=x.device)
    sa, sib = ops.snake_consts(*snake) if snake is not None else (None, None)
    assert ops.lib.sat_conv1d_k7_planes(_p(x), _p(sa), _p(sib), _p(hi), _p(lo), b, ch, t, rows, ops._stream(x)) == 0
    return hi, lo, rows


def _launch(ops, dev, c, variant=2, t=None):
    """one call through the ops wrapper -> (dW, row sums | None); t: device tensors in place of the case's own (lo, hi)"""
    d = _data(c)
    lo, hi = (t or {}).get("lo", None), (t or {}).get("hi", None)
    lo = d["lo"].to(dev) if lo is None else lo
    hi = d["hi"].to(dev) if hi is None else hi
    snake = _snake(c, d, dev)
    if c.kern in ("w4", "pipe"):
        out = ops.conv_wgrad7_bf16x3(lo, hi, c.dil, c.pad, snake=snake, dy_rowsum=c.rowsum)
    elif c.kern == "planes":
        assert c.snake_on in (0, 2) and not c.rowsum
        with _Knobs(ops, wgrad7_planes_variant=variant):
            out = ops.conv_wgrad7_planes(_prepass(ops, lo, None), _prepass(ops, hi, snake), c.b, c.m, c.n, c.t, c.dil, c.pad)
    elif c.kern == "small":
        out = ops.conv_wgrad(lo, hi, c.k, c.stride, 1, c.pad, snake=snake, snake_on=c.snake_on, lo_rowsum=c.rowsum)
    elif c.kern == "fp32":
        with _Knobs(ops, use_bf16x3=False):
            out = ops.conv_wgrad(lo, hi, c.k, c.stride, c.dil, c.pad, snake=snake, snake_on=c.snake_on, lo_rowsum=c.rowsum)
    else:
        out = ops.edge_conv_wgrad(lo, hi, c.k, c.pad, snake=snake, dy_rowsum=c.rowsum)
    return out if c.rowsum else (out, None)


def _run(ops, dev, c):
    fails = []
    with _Cus(ops, c.cus):
        _assert_plan(ops, c)
        for v in c.variants:
            dw, rs = _launch(ops, dev, c, v)
            tag = f" variant {v}" if c.kern == "planes" else ""
            if c.integer:
                assert torch.equal(dw.double().cpu(), _terms(c).ref), f"{c}{tag}: integer data, dW must be exact"
                assert rs is None or torch.equal(rs.double().cpu(), _rs_terms(c).ref), f"{c}: integer data, the row sums must be exact"
                continue
            _collect(fails, f"{c} dW{tag} {_leg(ops)}", dw, _terms(c))
            if rs is not None:
                _collect(fails, f"{c} rowsum {_leg(ops)}", rs, _rs_terms(c))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# a. the 4-wave k = 7 kernel (sat_wgrad7_bf16x3_kernel<1|3|9>): 128 co x 32 ci tiles, taken when N < 64 or T % 4 != 0, want = 512 / tiles.
#    M: one wave row / two / a partial second tile; N: below a chunk of 8 / one tile / a partial second tile, and N >= 64 at T % 4 != 0; T: under
#    one stage / one stage / one past it / ragged; the three dilations at pad = 3 dil and at a pad that is not; SnakeBeta and the fused row sums
#    on and off.  (3, 130, 40, 2700): 4 tiles, 129 stages, 65 splits of two, the last of one, split 21 = the end of item 0 + the start of item 1.
# ---------------------------------------------------------------------------------------------------------------------
W4_CASES = [Case("w4", 1, 8, 3, 20, dil=1, rowsum=True, plan=(1, 1, False, False)),
            Case("w4", 2, 40, 32, 64, dil=3, snake_on=0, plan=(2, 1, False, False)),
            Case("w4", 1, 130, 40, 65, dil=9, snake_on=0, rowsum=True, plan=(2, 1, False, False)),
            Case("w4", 2, 130, 70, 203, dil=1, rowsum=True, plan=(8, 1, False, False)),
            Case("w4", 1, 40, 3, 203, dil=9, plan=(4, 1, False, False)),
            Case("w4", 2, 8, 32, 65, dil=3, rowsum=True, plan=(4, 1, False, False)),
            Case("w4", 2, 40, 40, 203, dil=3, pad=4, rowsum=True, plan=(8, 1, False, False)),          # pad other than 3 dil
            Case("w4", 1, 8, 32, 65, dil=1, pad=0, snake_on=0, plan=(2, 1, False, False)),
            Case("w4", 1, 130, 3, 64, dil=9, pad=30, rowsum=True, plan=(1, 1, False, False)),
            Case("w4", 3, 130, 40, 2700, dil=3, rowsum=True, plan=(65, 2, True, True))]
# b. the pipelined k = 7 kernel (128 x 64 tiles, N >= 64 and T % 4 == 0): 1, 2, 3 and 4 stages per split = prologue only / the prefetch of stage
#    c + 2 with nothing to fetch / steady state / tail.  N partial in its last 64-tile and not a multiple of 8 (70, 130); dy_rowsum=True takes
#    the unfused path (fuses_rowsum == 0, asserted) and is still held.
#    (2, 130, 70, 4164): 4 tiles, want 128, 132 stages: 66 splits of two.  (2, 130, 130, 5504): 6 tiles, want 85, 172 stages: 58 splits of three, the
#    last of one, split 28 = stages 84 .. 86 crosses from item 0 into item 1.  (3, 260, 200, 2752): 12 tiles, want 42, 129 stages: 33 splits of four,
#    the last of one, split 10 = stages 40 .. 43 crosses from item 0 into item 1.
PIPE_CASES = [Case("pipe", 1, 64, 64, 64, dil=1, plan=(1, 1, False, False)),
              Case("pipe", 2, 130, 70, 200, dil=3, rowsum=True, plan=(8, 1, False, False)),
              Case("pipe", 2, 130, 70, 200, dil=9, snake_on=0, plan=(8, 1, False, False)),
              Case("pipe", 1, 8, 136, 68, dil=1, snake_on=0, rowsum=True, plan=(2, 1, False, False)),
              Case("pipe", 2, 130, 70, 4164, dil=1, plan=(66, 2, False, False)),
              Case("pipe", 2, 130, 130, 5504, dil=9, plan=(58, 3, True, True)),
              Case("pipe", 3, 260, 200, 2752, dil=3, rowsum=True, plan=(33, 4, True, True))]
# c. the planes kernel (sat_conv_wgrad7_planes_v), variants 2 and 0, operands through sat_conv1d_k7_planes: M != N, neither a multiple of 8 or of
#    the tile, T no multiple of 64; 1, 2 (the double-buffered loop) and 3 stages per split; the three dilations
PLANES = [Case("planes", 1, 64, 64, 64, dil=1, variants=(2, 0), plan=(1, 1, False, False)),
          Case("planes", 2, 130, 70, 200, dil=3, variants=(2, 0), plan=(8, 1, False, False)),
          Case("planes", 1, 72, 136, 90, dil=9, variants=(2, 0), plan=(2, 1, False, False)),
          Case("planes", 1, 70, 130, 90, dil=1, snake_on=0, variants=(2, 0), plan=(2, 1, False, False)),
          Case("planes", 1, 130, 200, 4130, dil=9, variants=(2, 0), plan=(33, 2, True, False)),
          Case("planes", 3, 130, 250, 2740, dil=3, plan=(43, 3, False, True)),
          Case("planes", 1, 130, 40, 90, dil=1), Case("planes", 1, 64, 64, 64, dil=2, pad=6), Case("planes", 1, 64, 64, 64, dil=9, pad=40)]     # refused


def _down(b, m, n, tin, s, **kw):
    """the wgrad of the strided down conv (B, n, tin) -> (B, m, tout), K = 2 S: lo = dy, hi = x, SnakeBeta on hi"""
    pad = math.ceil(s / 2)
    return Case("small", b, m, n, (tin + 2 * pad - 2 * s) // s + 1, k=2 * s, stride=s, pad=pad, thi=tin, **kw)


def _up(b, m, n, tin, s, **kw):
    """the wgrad of the transposed conv (B, m, tin) -> (B, n, tout) as functional.py calls it: lo = x (SnakeBeta on lo), hi = dy"""
    pad = math.ceil(s / 2)
    return Case("small", b, m, n, tin, k=2 * s, stride=s, pad=pad, thi=(tin - 1) * s - 2 * pad + 2 * s, **kw)


# d. the short-kernel wgrad (sat_wgrad_small_bf16x3_kernel<1|2>): K = 1 and K = 2 S (S = 2, 4, 8), both orientations and no activation, the fused
#    row sums on and off (snake_on == 1: not fused), N S below / at / above one 128 virtual-row tile, M partial, Tlo % 4 == 0 and != 0 (the
#    vector-staged and the scalar path), a last window partly past the end of hi (thi=), several stages per split with a ragged last one
SMALL_CASES = [Case("small", 2, 40, 24, 128, k=1, rowsum=True, plan=(4, 1, False, False)),           # fast1: pad 0, Tlo % 4 == 0
               Case("small", 1, 130, 130, 203, k=1, plan=(4, 1, False, False)),
               Case("small", 2, 8, 70, 65, k=1, snake_on=0, rowsum=True, plan=(4, 1, False, False)),
               Case("small", 1, 40, 40, 100, k=1, snake_on=1, rowsum=True, plan=(2, 1, False, False)),
               _down(1, 40, 20, 400, 2, rowsum=True, plan=(4, 1, False, False)), _down(2, 130, 64, 266, 2, plan=(6, 1, False, False)),
               _down(1, 8, 20, 400, 4, snake_on=0, rowsum=True, plan=(2, 1, False, False)), _down(1, 40, 32, 1050, 4, rowsum=True, plan=(5, 1, False, False)),
               _down(2, 130, 40, 530, 4, plan=(6, 1, False, False)), _down(1, 40, 8, 1040, 8, rowsum=True, plan=(3, 1, False, False)),
               _down(2, 20, 16, 530, 8, snake_on=0, plan=(4, 1, False, False)), _down(1, 130, 20, 2090, 8, rowsum=True, plan=(5, 1, False, False)),
               _up(1, 20, 40, 200, 2, snake_on=1, plan=(4, 1, False, False)), _up(2, 130, 8, 67, 4, snake_on=1, rowsum=True, plan=(4, 1, False, False)),
               _up(1, 40, 20, 130, 8, snake_on=1, plan=(3, 1, False, False)), _up(1, 70, 33, 65, 4, snake_on=0, plan=(2, 1, False, False)),
               _down(1, 8, 20, 403, 4, rowsum=True, plan=(2, 1, False, False)).but(thi=401),          # the last window ends one sample past hi
               _down(2, 130, 40, 33100, 4, rowsum=True, plan=(87, 3, True, True))]
# e. the fp32 kernel (sat_conv_wgrad_kernel<NSUB, KT>, ops.use_bf16x3 = False): every instantiation — (4, 1) K = 1; (2, 3) K = 3; (2, 4) K = 4 at
#    stride 2; (1, 7) K = 7 at dilation 2; (1, 8) K = 5 and K = 16 at stride 8 (two tap groups) — each with partial M and N tiles, T % 32 != 0, both
#    snake_on values and one shape with several 32-step chunks per split.  K = 3, K = 5 and K = 7 at dilation 2 are also what the bf16x3
#    planners decline (asserted below)
FP32_CASES = [Case("fp32", 2, 130, 140, 75, k=1, rowsum=True, plan=(6, 1, False, False)), Case("fp32", 1, 40, 20, 33, k=1, snake_on=1, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 140, 6200, k=1, snake_on=1, plan=(194, 2, False, False)),
              Case("fp32", 2, 130, 70, 75, k=3, plan=(6, 1, False, False)), Case("fp32", 1, 40, 20, 33, k=3, snake_on=1, rowsum=True, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 70, 6200, k=3, plan=(194, 2, False, False)),
              Case("fp32", 2, 130, 70, 75, k=4, stride=2, pad=1, thi=150, plan=(6, 1, False, False)),
              Case("fp32", 1, 20, 40, 33, k=4, stride=2, pad=1, thi=66, snake_on=1, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 70, 6200, k=4, stride=2, pad=1, thi=12400, plan=(194, 2, False, False)),
              Case("fp32", 2, 130, 40, 75, k=7, dil=2, plan=(6, 1, False, False)), Case("fp32", 1, 20, 33, 33, k=7, dil=2, snake_on=1, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 40, 6200, k=7, dil=2, snake_on=0, plan=(194, 2, False, False)),
              Case("fp32", 2, 130, 40, 75, k=5, plan=(6, 1, False, False)), Case("fp32", 1, 20, 33, 33, k=5, snake_on=1, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 40, 6200, k=5, plan=(194, 2, False, False)),
              Case("fp32", 2, 130, 40, 75, k=16, stride=8, pad=4, thi=600, plan=(6, 1, False, False)),
              Case("fp32", 1, 20, 33, 33, k=16, stride=8, pad=4, thi=264, snake_on=1, plan=(2, 1, False, False)),
              Case("fp32", 2, 130, 40, 3300, k=16, stride=8, pad=4, thi=26400, plan=(104, 2, False, False))]
# f. the edge wgrad (sat_edge_wgrad_kernel<1|2>), both forms: narrow input (N = 1, 2; M = 8, 40, 130; with and without row sums) and narrow output
#    (M = 1, 2; SnakeBeta on the wide x; taps flipped); K = 3, 5, 7; T = 333, 1024, 1027, 2050.  Its plan depends on the CU count: on 256 CUs every
#    1024-step tile is a split of its own; the simulator is told 1 or 2 CUs to reach 2 and 3 tiles per split and a ragged last split.
EDGE_CASES = [Case("edge", 2, 8, 1, 333, k=3, snake_on=0, rowsum=True, plan=(2, 1, False, False)), Case("edge", 1, 40, 2, 1024, k=5, snake_on=0, plan=(1, 1, False, False)),
              Case("edge", 2, 130, 2, 1027, k=7, snake_on=0, rowsum=True, plan=(4, 1, False, False)), Case("edge", 1, 130, 1, 2050, k=7, snake_on=0, plan=(3, 1, False, False)),
              Case("edge", 1, 40, 1, 2050, k=5, snake_on=0, rowsum=True, plan=(3, 1, False, False)),
              Case("edge", 2, 1, 8, 333, k=7, plan=(2, 1, False, False)), Case("edge", 1, 2, 40, 1024, k=3, plan=(1, 1, False, False)),
              Case("edge", 2, 2, 130, 1027, k=5, plan=(4, 1, False, False)), Case("edge", 1, 1, 130, 2050, k=7, snake_on=0, plan=(3, 1, False, False)),
              Case("edge", 1, 2, 40, 2050, k=7, plan=(3, 1, False, False))]
EDGE_SIM_CASES = [Case("edge", 1, 8, 2, 4100, k=7, snake_on=0, rowsum=True, cus=1, plan=(3, 2, True, False)),        # 5 tiles, want 4: 2 + 2 + 1
                  Case("edge", 2, 40, 1, 4100, k=5, snake_on=0, rowsum=True, cus=2, plan=(4, 3, True, False)),       # 5 tiles, want 2: (3 + 2) per item
                  Case("edge", 1, 2, 8, 4100, k=7, cus=1, plan=(3, 2, True, False)),
                  Case("edge", 2, 1, 8, 5000, k=3, cus=1, plan=(4, 3, True, False))]
ALL = {"w4": W4_CASES, "pipe": PIPE_CASES, "small": SMALL_CASES, "fp32": FP32_CASES, "edge": EDGE_CASES}


@pytest.mark.parametrize("c", W4_CASES + PIPE_CASES, ids=_ids(W4_CASES + PIPE_CASES))
def test_k7_sim(emu, c):
    _run(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", W4_CASES + PIPE_CASES, ids=_ids(W4_CASES + PIPE_CASES))
def test_k7_gpu(hip, c):
    _run(hip, "cuda", c)


def _planes_case(ops, dev, c):
    if c.plan is not None:
        return _run(ops, dev, c)
    # a shape the kernel cannot serve is refused by _ok and by the launch, not computed wrongly
    rows = _rows(ops, c.t)
    assert ops.lib.sat_conv_wgrad7_planes_ok(c.b, c.m, c.n, c.t, c.dil, c.pad, rows, rows) == 0, c
    d = _data(c)
    dyp, actp = _prepass(ops, d["lo"].to(dev), None), _prepass(ops, d["hi"].to(dev), None)
    out = torch.full((c.m * c.n * 7 * 4,), SENTINEL, device=dev)
    for v in (2, 0):
        assert ops.lib.sat_conv_wgrad7_planes_v(_p(dyp[0]), _p(dyp[1]), rows, _p(actp[0]), _p(actp[1]), rows, _p(out), c.n, 1, c.m * c.n, c.b, c.m, c.n, c.t,
                                                c.dil, c.pad, v, ops._stream(out)) != 0
    assert bool((out == SENTINEL).all()), f"{c}: a refused launch wrote"


@pytest.mark.parametrize("c", PLANES, ids=_ids(PLANES))
def test_planes_sim(emu, c):
    _planes_case(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", PLANES, ids=_ids(PLANES))
def test_planes_gpu(hip, c):
    _planes_case(hip, "cuda", c)


def _planes_emitted(ops, dev):
    """dy's planes as a producer emits them: a K = 1 conv with emit=True writes its output y and y's planes; the planes kernel reads those, the
    reference the fp32 y it was handed beside them"""
    b, cin, m, n, t, dil = 2, 24, 130, 70, 200, 3
    gen = torch.Generator().manual_seed(77)
    x0, w0 = torch.randn(b, cin, t, generator=gen).to(dev), (torch.randn(m, cin, 1, generator=gen) * .2).to(dev)
    c = Case("planes", b, m, n, t, dil=dil, plan=(8, 1, False, False))
    d = _data(c)
    with _Knobs(ops, k7q=True, k7q_min_cin=1, k7q_min_cout=1):
        assert ops.emit_ok(m, 1, 1, t, dil)
        y = ops.conv1d_bf16x3(x0, ops.pack_bf16x3(w0, 0, 1), m, 1, emit=True)
        em = ops._take_emitted(y, None)
    assert em is not None
    _assert_plan(ops, c)
    assert ops.lib.sat_conv_wgrad7_planes_ok(b, m, n, t, dil, c.pad, em.rows, _rows(ops, t)) == 1
    snake = _snake(c, d, dev)
    fails = []
    for v in (2, 0):
        with _Knobs(ops, wgrad7_planes_variant=v):
            dw = ops.conv_wgrad7_planes((em.hi, em.lo, em.rows), _prepass(ops, d["hi"].to(dev), snake), b, m, n, t, dil, c.pad)
        _collect(fails, f"{c} dy emitted by a K = 1 conv, dW variant {v} {_leg(ops)}", dw, W.wgrad(y.cpu(), d["hi"], 7, 1, dil, c.pad, _snake(c, d), 2))
    assert not fails, "\n".join(fails)


def test_planes_emitted_dy_sim(emu):
    _planes_emitted(emu, "cpu")


@pytest.mark.gpu
def test_planes_emitted_dy_gpu(hip):
    _planes_emitted(hip, "cuda")


@pytest.mark.parametrize("c", SMALL_CASES, ids=_ids(SMALL_CASES))
def test_small_sim(emu, c):
    _run(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SMALL_CASES, ids=_ids(SMALL_CASES))
def test_small_gpu(hip, c):
    _run(hip, "cuda", c)


def _fp32(ops, dev, c):
    if c.k in (3, 5) or c.dil != 1:          # reached without the knob too: the bf16x3 planners decline
        assert ops.lib.sat_conv_wgrad_bf16x3_nsplit(c.b, c.m, c.n, c.t, c.k, c.stride) == -1 or c.dil != 1
        assert not ops.wgrad7_bf16x3_ok(c.n, c.k, c.stride, c.dil)
        if c.plan[1] == 1:
            d = _data(c)
            direct = ops.conv_wgrad(d["lo"].to(dev), d["hi"].to(dev), c.k, c.stride, c.dil, c.pad, snake=_snake(c, d, dev), snake_on=c.snake_on)
            assert torch.equal(direct, _launch(ops, dev, c.but(rowsum=False))[0]), f"{c}: ops.conv_wgrad takes another kernel with the bf16x3 knob on"
    _run(ops, dev, c)


@pytest.mark.parametrize("c", FP32_CASES, ids=_ids(FP32_CASES))
def test_fp32_sim(emu, c):
    _fp32(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", FP32_CASES, ids=_ids(FP32_CASES))
def test_fp32_gpu(hip, c):
    _fp32(hip, "cuda", c)


@pytest.mark.parametrize("c", EDGE_CASES + EDGE_SIM_CASES, ids=_ids(EDGE_CASES + EDGE_SIM_CASES))
def test_edge_sim(emu, c):
    _run(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", EDGE_CASES, ids=_ids(EDGE_CASES))
def test_edge_gpu(hip, c):
    assert torch.cuda.get_device_properties(0).multi_processor_count == GPU_CUS
    _run(hip, "cuda", c)


# ---------------------------------------------------------------------------------------------------------------------
# g. ru_k1_bwd (C = 128, T % 32 == 0): dh, d log-alpha2, d log-beta2, dW2, dbias2, dbias1 and dh's emitted planes; skip_dh=True gives bit-equal planes
#    and sums, raw=True slabs that reduce to the same dW2.  One workgroup per CU walks `per` 32-step tiles: the simulator at 8 CUs reaches 1, 2 and 3
#    tiles per workgroup, a ragged last range and ranges that cross batch boundaries; the GPU (256 CUs): (2, 128, 96) and (3, 128, 2752) = 258
#    tiles, 129 workgroups of two.
# ---------------------------------------------------------------------------------------------------------------------
RU_SIM = [(2, 128, 96, 8, (6, 1, False, False)), (1, 128, 512, 8, (8, 2, False, False)), (3, 128, 224, 8, (7, 3, False, True)), (2, 128, 320, 8, (7, 3, True, True))]
RU_GPU = [(2, 128, 96, 0, (6, 1, False, False)), (3, 128, 2752, 0, (129, 2, False, False))]


def _ru_data(b, c, t, integer=False):
    key = ("ru", b, c, t, integer)
    if key not in _cache:
        gen = torch.Generator().manual_seed(b * 100003 + t)
        if integer:
            mk = lambda *shape: torch.randint(-3, 4, shape, generator=gen).float()
            d = {"dy": mk(b, c, t), "h": mk(b, c, t), "w2": mk(c, c, 1), "la2": torch.zeros(c), "lb2": torch.full((c,), 60.0)}
        else:
            rn = lambda *shape, s=1.0: torch.randn(*shape, generator=gen) * s
            d = {"dy": rn(b, c, t), "h": rn(b, c, t), "w2": rn(c, c, 1, s=.5 / math.sqrt(c / 8)), "la2": rn(c, s=.3), "lb2": rn(c, s=.3)}
            d["terms"] = W.ru_k1_bwd(d["dy"], d["h"], d["w2"], d["la2"], d["lb2"])
        _cache[key] = d
    return _cache[key]


def _ru_call(ops, dev, d, **kw):
    outs = ops.ru_k1_bwd(d["dy"].to(dev), d["h"].to(dev), d["w2"].to(dev), (d["la2"].to(dev), d["lb2"].to(dev)), **kw)
    em = ops._take_emitted(outs[0], None)
    if kw.get("skip_dh"):
        ops.dh_written()
    return outs, em


def _ru(ops, dev, case):
    b, c, t, cus, plan = case
    names = ("dh", "dla", "dlb", "dw2", "dbias2", "dbias1")
    fails = []
    with _Cus(ops, cus):
        assert ops.ru_k1_bwd_ok(b, c, t)
        got = _split_plan(ops.lib.sat_ru_k1_bwd_nsplit(b, c, t), b, t // 32)
        assert got == plan, f"ru_k1_bwd {(b, c, t)}: plan {got}, meant {plan}"
        d = _ru_data(b, c, t)
        full, em = _ru_call(ops, dev, d, emit=True)
        assert em is not None
        planes = W.planes_value(em, b, c, t)
        for name, g in zip(names, full):
            _collect(fails, f"ru_k1_bwd {(b, c, t)} {name} {_leg(ops)}", g, d["terms"][name])
        try:
            W.check_planes(f"ru_k1_bwd {(b, c, t)} emitted dh {_leg(ops)}", planes, d["terms"]["dh"])
        except AssertionError as e:
            fails.append(str(e))
        skip, em_s = _ru_call(ops, dev, d, emit=True, skip_dh=True)
        assert em_s is not None and torch.equal(W.planes_value(em_s, b, c, t), planes), "skip_dh changes the emitted planes"
        for name, a, g in list(zip(names, skip, full))[1:]:
            assert torch.equal(a, g), f"skip_dh changes {name}"
        raw, _ = _ru_call(ops, dev, d, raw=True)
        assert raw[3].nsplit == plan[0] and torch.equal(raw[3].reduce(ops).view(c, c, 1), full[3]), "raw=True slabs do not reduce to dW2"
        for i in (0, 1, 2, 4, 5):
            assert torch.equal(raw[i], full[i]), f"emit=False changes {names[i]}"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", RU_SIM, ids=_ids(RU_SIM))
def test_ru_k1_bwd_sim(emu, case):
    _ru(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RU_GPU, ids=_ids(RU_GPU))
def test_ru_k1_bwd_gpu(hip, case):
    assert torch.cuda.get_device_properties(0).multi_processor_count == GPU_CUS
    _ru(hip, "cuda", case)


# ---------------------------------------------------------------------------------------------------------------------
# h. sat_reduce_splits: nsplit 1, 2, 3, 4, 5, 9 (the unrolled four and its tail); count % 4 == 0 with aligned pointers (the vector kernel), count odd
#    and an `out` 4 bytes off 16 (the scalar kernel); scale != 1; accumulate on and off.  sat_rowsum: T % 4 == 0 and != 0, T over 16384 (splits and
#    the second pass), partial=True
# ---------------------------------------------------------------------------------------------------------------------
def _reduce(ops, dev, nsplit):
    fails = []
    gen = torch.Generator().manual_seed(900 + nsplit)
    for count, off, what in ((1028, 0, "vector"), (1027, 0, "odd count"), (1028, 1, "out 4 bytes off 16")):
        slabs = torch.randn(nsplit, count, generator=gen)
        before = torch.randn(count, generator=gen)
        sd = slabs.to(dev)
        assert sd.data_ptr() % 16 == 0
        for scale, acc in ((1.0, 0), (0.37, 0), (1.0, 1), (-2.5, 1)):
            buf = torch.full((count + 2 * GUARD,), SENTINEL, device=dev)
            out = buf[GUARD + off:GUARD + off + count]
            assert out.data_ptr() % 16 == 4 * off
            if acc:
                out.copy_(before)
            assert ops.lib.sat_reduce_splits(_p(sd), _p(out), count, nsplit, scale, acc, ops._stream(sd)) == 0
            assert bool((torch.cat([buf[:GUARD + off], buf[GUARD + off + count:]]) == SENTINEL).all()), f"reduce_splits {what}: a float outside out was written"
            _collect(fails, f"reduce_splits nsplit {nsplit} {what} scale {scale} accumulate {acc} {_leg(ops)}", out, W.reduce_splits(slabs, scale, before if acc else None))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 5, 9])
def test_reduce_splits_sim(emu, nsplit):
    _reduce(emu, "cpu", nsplit)


@pytest.mark.gpu
@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 5, 9])
def test_reduce_splits_gpu(hip, nsplit):
    _reduce(hip, "cuda", nsplit)


ROWSUM_CASES = [(2, 5, 300), (2, 5, 301), (1, 3, 16388), (2, 3, 40001), (1, 2, 16384)]


def _rowsum(ops, dev, shape):
    b, c, t = shape
    key = ("rowsum",) + shape
    if key not in _cache:
        x = torch.randn(b, c, t, generator=torch.Generator().manual_seed(t))
        _cache[key] = (x, W.rowsum(x))
    x, terms = _cache[key]
    ns = ops.lib.sat_rowsum_nsplit(t)
    assert ns == -(-t // 16384)
    fails = []
    _collect(fails, f"rowsum {shape} {_leg(ops)}", ops.rowsum(x.to(dev)), terms)
    part = ops.rowsum(x.to(dev), partial=True)
    assert tuple(part.shape) == (c, ns)
    _collect(fails, f"rowsum {shape} partial=True, columns summed in float64 {_leg(ops)}", part.double().sum(1).float(), terms)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", ROWSUM_CASES, ids=_ids(ROWSUM_CASES))
def test_rowsum_sim(emu, shape):
    _rowsum(emu, "cpu", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ROWSUM_CASES, ids=_ids(ROWSUM_CASES))
def test_rowsum_gpu(hip, shape):
    _rowsum(hip, "cuda", shape)


# ---------------------------------------------------------------------------------------------------------------------
# i. structure, one multi-tile, multi-split case per kernel, through ops.lib: the slabs (and the [M][nsplit] row sums) are views inside a sentinel-
#    filled buffer with 64 guard floats on both sides, themselves pre-filled with the sentinel — afterwards no sentinel is left inside (every
#    element of every slab and every [m][split] was written) and every guard float is intact; both slab layouts, each reduced and checked, bit-equal
#    to each other; the fp32 operands sit 16-byte aligned inside NaN-filled buffers (row lengths no multiple of 4 where the kernel takes them).
#    All of it before the first call that lets ops allocate.
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.75
GUARD = 64
STRUCT_CASES = [Case("w4", 2, 130, 40, 203, dil=3, rowsum=True, plan=(8, 1, False, False)), Case("pipe", 2, 130, 70, 200, dil=9, plan=(8, 1, False, False)),
                Case("planes", 2, 130, 70, 200, dil=3, variants=(2, 0), plan=(8, 1, False, False)),
                _down(2, 130, 40, 530, 4, rowsum=True, plan=(6, 1, False, False)), Case("small", 1, 130, 130, 203, k=1, rowsum=True, plan=(4, 1, False, False)),
                Case("fp32", 2, 130, 70, 75, k=3, plan=(6, 1, False, False)), Case("fp32", 2, 130, 40, 75, k=16, stride=8, pad=4, thi=600, plan=(6, 1, False, False)),
                Case("edge", 2, 130, 2, 1027, k=7, snake_on=0, rowsum=True, plan=(4, 1, False, False)), Case("edge", 2, 2, 130, 1027, k=5, plan=(4, 1, False, False))]


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _in_nan(x, dev):
    """a dense copy of x, 16-byte aligned, inside a NaN-filled buffer"""
    buf = torch.full((x.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[GUARD:GUARD + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 0
    return view


def _raw_call(ops, c, lo, hi, snake, partial, so, rs, variant):
    lib, st = ops.lib, ops._stream(lo)
    al, be = (snake if snake is not None else (None, None))
    on = c.snake_on if snake is not None else 0
    if c.kern in ("w4", "pipe"):
        return lib.sat_conv_wgrad7_bf16x3(_p(lo), _p(hi), _p(al), _p(be), _p(partial), *so, c.b, c.m, c.n, c.t, c.dil, c.pad, _p(rs), st)
    if c.kern == "planes":
        dyp, actp = _prepass(ops, lo, None), _prepass(ops, hi, snake)
        return lib.sat_conv_wgrad7_planes_v(_p(dyp[0]), _p(dyp[1]), dyp[2], _p(actp[0]), _p(actp[1]), actp[2], _p(partial), *so, c.b, c.m, c.n, c.t, c.dil, c.pad, variant, st)
    if c.kern == "small":
        return lib.sat_conv_wgrad_bf16x3(_p(lo), _p(hi), _p(al), _p(be), on, _p(partial), *so, c.b, c.m, c.n, c.t, c.thi, c.k, c.stride, c.pad, _p(rs), st)
    if c.kern == "fp32":
        return lib.sat_conv_wgrad(_p(lo), _p(hi), _p(al), _p(be), on, _p(partial), *so, c.b, c.m, c.n, c.t, c.thi, c.k, c.stride, c.dil, c.pad, st)
    assert so == (c.n * c.k, c.k, 1)
    return lib.sat_edge_conv_wgrad(_p(lo), _p(hi), _p(al), _p(be), _p(partial), _p(rs), c.b, c.m, c.n, c.t, c.k, c.pad, st)


def _structure(ops, dev, c):
    fails = []
    ns = _assert_plan(ops, c)
    assert ns > 1 and max(c.m, c.n) > 128
    d = _data(c)
    lo, hi = _in_nan(d["lo"], dev), _in_nan(d["hi"], dev)
    snake = _snake(c, d, dev)
    count = c.m * c.n * c.k
    fused = c.rowsum and c.kern != "fp32" and c.kern != "pipe"
    layouts = [("torch order", (c.n * c.k, c.k, 1))] + ([] if c.kern == "edge" else [("tap-major", (c.n, 1, c.m * c.n))])
    dws = []
    for variant in c.variants:
        for lname, so in layouts:
            buf, partial = _guarded(ns * count, dev)
            rbuf, rs = _guarded(c.m * ns, dev) if fused else (None, None)
            assert _raw_call(ops, c, lo, hi, snake, partial, so, rs, variant) == 0, ops.lib.sat_last_error().decode()
            tag = f"{c} {lname}" + (f" variant {variant}" if c.kern == "planes" else "")
            assert not bool((partial == SENTINEL).any()), f"{tag}: {int((partial == SENTINEL).sum())} slab elements were not written"
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + ns * count:] == SENTINEL).all()), f"{tag}: a float outside the slabs was written"
            if fused:
                assert not bool((rs == SENTINEL).any()), f"{tag}: {int((rs == SENTINEL).sum())} of the [m][split] row sums were not written"
                assert bool((rbuf[:GUARD] == SENTINEL).all()) and bool((rbuf[GUARD + c.m * ns:] == SENTINEL).all()), f"{tag}: a float outside the row sums was written"
            obuf, out = _guarded(count, dev)
            assert ops.lib.sat_reduce_splits(_p(partial), _p(out), count, ns, 1.0, 0, ops._stream(partial)) == 0
            assert bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + count:] == SENTINEL).all())
            dw = out.view(c.m, c.n, c.k) if so[2] == 1 else out.view(c.k, c.m, c.n).permute(1, 2, 0)
            _collect(fails, f"{tag} operands in NaN, dW {_leg(ops)}", dw.contiguous(), _terms(c))
            if fused:
                _collect(fails, f"{tag} operands in NaN, rowsum (columns summed in float64) {_leg(ops)}", rs.view(c.m, ns).double().sum(1).float(), _rs_terms(c))
            dws.append((variant, dw))
    for v, dw in dws[1:]:
        if v == dws[0][0]:
            assert torch.equal(dw, dws[0][1]), f"{c}: the two slab layouts give different dW"
    # only now the calls that let ops allocate: the same values
    for variant in c.variants:
        dw, rs = _launch(ops, dev, c, variant)
        assert torch.equal(dw, [x for v, x in dws if v == variant][0]), f"{c}: ops' own slabs give another dW"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_structure_sim(emu, c):
    _structure(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_structure_gpu(hip, c):
    _structure(hip, "cuda", c)


def _ru_structure(ops, dev, case):
    b, c, t, cus, plan = case
    with _Cus(ops, cus):
        ns = ops.lib.sat_ru_k1_bwd_nsplit(b, c, t)
        assert _split_plan(ns, b, t // 32) == plan and ns > 1
        d = _ru_data(b, c, t)
        dy, h = _in_nan(d["dy"], dev), _in_nan(d["h"], dev)
        w2, la2, lb2 = d["w2"].to(dev), d["la2"].to(dev), d["lb2"].to(dev)
        wt_hi, wt_lo = ops.ru_k1_pack(w2)
        bufs = [_guarded(n, dev) for n in (b * c * t, ns * c * c, 4 * c * ns)]
        (_, dh), (_, slabs), (_, part) = bufs
        assert ops.lib.sat_ru_k1_bwd(_p(dy), _p(h), _p(wt_hi), _p(wt_lo), _p(la2), _p(lb2), _p(dh), None, None, 0, _p(slabs), _p(part), b, c, t, ops._stream(dy)) == 0
        for name, (buf, view) in zip(("dh", "dW2 slabs", "partial sums"), bufs):
            assert not bool((view == SENTINEL).any()), f"ru_k1_bwd {(b, c, t)}: {int((view == SENTINEL).sum())} elements of {name} were not written"
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + view.numel():] == SENTINEL).all()), f"ru_k1_bwd {(b, c, t)}: a float outside {name} was written"
        full, _ = _ru_call(ops, dev, d)
        assert torch.equal(dh.view(b, c, t), full[0])
        assert torch.equal(ops._reduce_rows(slabs.view(ns, c * c).contiguous(), ns, c * c).view(c, c, 1), full[3])
        sums = ops._sum_last(part.view(4 * c, ns).contiguous())
        for i, j in ((1, 0), (2, 1), (5, 2), (4, 3)):
            assert torch.equal(sums[j * c:(j + 1) * c], full[i])


def test_ru_k1_bwd_structure_sim(emu):
    _ru_structure(emu, "cpu", RU_SIM[3])


@pytest.mark.gpu
def test_ru_k1_bwd_structure_gpu(hip):
    _ru_structure(hip, "cuda", RU_GPU[1])


# ---------------------------------------------------------------------------------------------------------------------
# j. exact integers: operands drawn from {-3 .. 3}, no activation, one multi-split shape per kernel: dW (and the row sums) EQUAL the float64 value —
#    an index or order error shows with no tolerance at all.  ru_k1_bwd has no form without SnakeBeta: log-beta2 = 60 makes snake2 the identity
#    in float32 (h + 8.8e-27 sin^2 rounds to h, the derivative to 1), and dh, dW2 and both bias gradients are then sums of small integers.
# ---------------------------------------------------------------------------------------------------------------------
INT_CASES = [c.but(snake_on=0, integer=True) for c in (W4_CASES[9], PIPE_CASES[1], PLANES[1], SMALL_CASES[1], SMALL_CASES[8], SMALL_CASES[13], FP32_CASES[0],
                                                       FP32_CASES[3], FP32_CASES[6], FP32_CASES[9], FP32_CASES[12], FP32_CASES[15], EDGE_CASES[2], EDGE_CASES[7],
                                                       EDGE_SIM_CASES[1])]


@pytest.mark.parametrize("c", INT_CASES, ids=_ids(INT_CASES))
def test_integers_sim(emu, c):
    _run(emu, "cpu", c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in INT_CASES if not c.cus], ids=_ids([c for c in INT_CASES if not c.cus]))
def test_integers_gpu(hip, c):
    _run(hip, "cuda", c)


def _ru_integers(ops, dev, case):
    b, c, t, cus, plan = case
    with _Cus(ops, cus):
        assert _split_plan(ops.lib.sat_ru_k1_bwd_nsplit(b, c, t), b, t // 32) == plan
        d = _ru_data(b, c, t, integer=True)
        (dh, _, _, dw2, dbias2, dbias1), _ = _ru_call(ops, dev, d)
    dy64, h64, w64 = d["dy"].double(), d["h"].double(), d["w2"].double()
    ref_dh = torch.einsum("oi,bot->bit", w64[:, :, 0], dy64)
    assert torch.equal(dh.double().cpu(), ref_dh), "integer data: dh must be exact"
    assert torch.equal(dw2.double().cpu(), torch.einsum("bot,bit->oi", dy64, h64)[:, :, None]), "integer data: dW2 must be exact"
    assert torch.equal(dbias2.double().cpu(), dy64.sum(dim=(0, 2))) and torch.equal(dbias1.double().cpu(), ref_dh.sum(dim=(0, 2))), "integer data: the bias gradients must be exact"


def test_ru_k1_bwd_integers_sim(emu):
    _ru_integers(emu, "cpu", RU_SIM[3])


@pytest.mark.gpu
def test_ru_k1_bwd_integers_gpu(hip):
    _ru_integers(hip, "cuda", RU_GPU[1])
