"""The projection GEMMs of csrc/gemm.hip held to float64 PER ELEMENT, under every shipped tile (0, 4, 7, 8) and every epilogue: STORE,
RES, GATE_RES, SWIGLU (and its pre-activation copy), the fp32-model path on split_bf16x3 planes, split-K with the slab reduction and with
sat_splitk_epilogue, the head-split / rotary / plane-layout epilogue and its qk_norm ("ln", "l2") variant.  Reference, scale, yardstick
and the assertion are tests/gemm_fp64.py's (fp64_bounds.py's rule with a scale per element: no bound here comes from running a kernel);
`pytest -s` shows every FIGURE line.

What the whole-matrix `max|a - b| / max|b|` bars of tests/test_gemm_kernels.py and tests/test_qk_norm_kernels.py (1e-5 fp32, 6e-3 bf16)
cannot see and this module does: an element that is small next to its matrix's largest; the bf16-only code (sat_store4<false>,
sat_load4<false>, the transposed-V pack, the QKV and QKV_NORM epilogues), where 6e-3 passes a truncating store or a rotary table rounded to
bf16; and the structure the model relies on — operands and residuals with free row strides and NaN in the padding, no row written past M,
no column written past the logical width, and persistent planes (ops._head_planes(reuse=...)) whose rows / columns past ntok keep what
they held, checked against a NON-ZERO sentinel.

fp8 is not tightened: the MX MFMA's internal accumulation is not documented, so a bound for it would have to come from running the kernel.
Its bars in tests/test_gemm_kernels.py stay; here fp8 takes part in the structural cases only (strided operands, guard rows, plane
padding), with the values bit-equal between the padded and the packed call.

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import pytest
import torch

import gemm_fp64 as G
from test_gemm_kernels import RING_SHAPES, SHAPES

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
TILES = (0, 4, 7, 8)
WRAP = (136, 264, 584)          # 10 K-steps with a K tail of 8: the 3- and 4-stage rings wrap twice
GATE3 = (129, 136, 72)          # three batch items of 43 rows: both boundaries fall inside a 4-row pass of the epilogue
EPI_SHAPES = list(dict.fromkeys(SHAPES + RING_SHAPES + [WRAP, GATE3]))
INV = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
SPIKES = (30.0, -30.0, 100.0, -100.0)       # saturated sigmoids, both sides

_prepared = {}


def _collect(fails, name, got, terms):
    """every tensor's figures are printed before the first failure is raised"""
    try:
        G.check(name, got, terms)
    except AssertionError as e:
        fails.append(str(e))


def _leg(ops):
    return "sim" if ops.simulator else "gpu"


class _Forced:
    """ops.gemm_tile (or gemm_fp8_tile) forced for a block, reset whatever happens"""

    def __init__(self, ops, tile, attr="gemm_tile"):
        self.ops, self.tile, self.attr = ops, tile, attr

    def __enter__(self):
        setattr(self.ops, self.attr, self.tile)

    def __exit__(self, *exc):
        setattr(self.ops, self.attr, None)


def _items(m):
    return 3 if m % 3 == 0 else 2 if m % 2 == 0 else 1


def _operands(shape):
    """CPU operands and the float64 / float32 projection of one (M, N, K): computed once, shared by every test, never written"""
    if shape not in _prepared:
        m, n, k = shape
        gen = torch.Generator().manual_seed(7000 + m + 31 * n + 977 * k)
        o = {"a": torch.randn(m, k, generator=gen).bfloat16(), "b": torch.randn(n, k, generator=gen).bfloat16(),
             "bias": torch.randn(n, generator=gen), "res": torch.randn(m, n, generator=gen)}
        gate = torch.randn(_items(m), n, generator=gen)
        n16 = n // 16 * 16                   # SwiGLU needs N = 2F, F % 8 == 0: it runs on the first n16 rows of b
        sbias = torch.randn(n16, generator=gen)
        for i, v in enumerate(SPIKES):
            gate[i % gate.shape[0], 1 + 2 * i] = v
            gate[-1, n - 1 - i] = v
            sbias[n16 // 2 + 1 + 2 * i] = v  # ... of the GATE half: silu saturates
            sbias[n16 - 1 - i] = v
        o["gate"], o["sbias"], o["n16"] = gate, sbias, n16
        o["proj"] = G.projection(o["a"], o["b"])
        _prepared[shape] = o
    return _prepared[shape]


def _epi_terms(o, dtype):
    key = ("terms", dtype)
    if key not in o:
        res, gate = o["res"].to(dtype), o["gate"].to(dtype)
        full = G.add_bias(o["proj"], o["bias"])
        pre = G.add_bias(o["proj"].cols(0, o["n16"]), o["sbias"])
        o[key] = {"store": o["proj"], "bias": full, "res": G.epi_res(full, res),
                  "gate_res": G.epi_gate_res(full, res, gate, o["a"].shape[0] // gate.shape[0]), "pre": pre, "swiglu": G.epi_swiglu(pre)}
    return o[key]


def _epi_calls(ops, dev, o, dtype):
    """the five launches of one (shape, dtype) under the current tile: {label: tensor}"""
    a, b, bias, sbias = (o[n].to(dev) for n in ("a", "b", "bias", "sbias"))
    res, gate = o["res"].to(dtype).to(dev), o["gate"].to(dtype).to(dev)
    rpg = a.shape[0] // gate.shape[0]
    out = {"store": ops.gemm_bf16(a, b, out_dtype=dtype), "bias": ops.gemm_bf16(a, b, bias=bias, out_dtype=dtype),
           "res": ops.gemm_bf16(a, b, bias=bias, res=res, epilogue=ops.EPI_RES, out_dtype=dtype),
           "gate_res": ops.gemm_bf16(a, b, bias=bias, res=res, gate=gate, rows_per_gate=rpg, epilogue=ops.EPI_GATE_RES, out_dtype=dtype)}
    out["swiglu"], out["pre"] = ops.gemm_bf16(a, b[:o["n16"]], bias=sbias, epilogue=ops.EPI_SWIGLU, out_dtype=dtype, want_pre=True)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. every epilogue, fp32 and bf16 output, every tile
# ---------------------------------------------------------------------------------------------------------------------
def _epilogues(ops, dev, shape, dtype):
    o = _operands(shape)
    terms = _epi_terms(o, dtype)
    fails = []
    for tile in TILES:
        with _Forced(ops, tile):
            got = _epi_calls(ops, dev, o, dtype)
        for label, t in got.items():
            assert t.dtype == dtype
            _collect(fails, f"gemm {shape} tile {tile} {label} {_leg(ops)}", t, terms[label])
    assert not fails, "\n".join(fails)


_EPI_IDS = ["x".join(map(str, s)) for s in EPI_SHAPES]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=_EPI_IDS)
def test_epilogues_sim(emu, shape, dtype):
    _epilogues(emu, "cpu", shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=_EPI_IDS)
def test_epilogues_gpu(hip, shape, dtype):
    _epilogues(hip, "cuda", shape, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fp32-model path: split_bf16x3 planes, fp32 output, with and without split-K
# ---------------------------------------------------------------------------------------------------------------------
X3_CASES = [((130, 136, 72), False), ((70, 264, 200), False), ((72, 136, 104), True)]      # True: columns span 2^-20 .. 2^20


def _x3(ops, dev, shape, spread):
    m, n, k = shape
    gen = torch.Generator().manual_seed(7100 + m + k)
    a, b = torch.randn(m, k, generator=gen), torch.randn(n, k, generator=gen)
    if spread:      # a's columns grow as b's shrink: every product is O(1), every lo plane matters
        e = torch.exp2(torch.linspace(-20, 20, k).round())
        a, b = a * e, b / e
    a3, b3 = ops.split_bf16x3(a.to(dev), 0), ops.split_bf16x3(b.to(dev), 1)
    for x, p, order in ((a, a3.cpu(), (0, 0, 1)), (b, b3.cpu(), (0, 1, 0))):      # [hi|hi|lo] and [hi|lo|hi], lo = bf16(x - hi)
        hi = x.bfloat16()
        planes = (hi, (x - hi.float()).bfloat16())
        assert torch.equal(p, torch.cat([planes[i] for i in order], dim=1))
    terms = G.projection(a3, b3, planes=3)
    fails = []
    for tile in TILES:
        with _Forced(ops, tile):
            for s in (1, 2, 3):
                got = ops.gemm_bf16(a3, b3, out_dtype=F32, splits=s)
                _collect(fails, f"gemm bf16x3 {shape}{' spread' if spread else ''} tile {tile} splits {s} {_leg(ops)}", got, terms)
    assert not fails, "\n".join(fails)


_X3_IDS = ["x".join(map(str, s)) + ("-spread" if sp else "") for s, sp in X3_CASES]


@pytest.mark.parametrize("case", X3_CASES, ids=_X3_IDS)
def test_fp32_model_path_sim(emu, case):
    _x3(emu, "cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", X3_CASES, ids=_X3_IDS)
def test_fp32_model_path_gpu(hip, case):
    _x3(hip, "cuda", *case)


# ---------------------------------------------------------------------------------------------------------------------
# 3. split-K: the slab reduction (gemm_bf16(splits=)) and sat_splitk_epilogue (bias, residual, one bf16 rounding)
#    K = 328: 5 K-steps; 4 slices are 128, 128, 72 and an empty one.  K = 8 and K = 72: slices that start past K.
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [(290, 520, 328), (33, 64, 8), (130, 136, 72)]


def _splitk(ops, dev, shape):
    o = _operands(shape)
    a, b, bias = (o[n].to(dev) for n in ("a", "b", "bias"))
    fails = []
    for tile in TILES:
        with _Forced(ops, tile):
            for s in (2, 4, 8):
                _collect(fails, f"gemm {shape} tile {tile} splits {s} {_leg(ops)}", ops.gemm_bf16(a, b, out_dtype=F32, splits=s), o["proj"])
            for s in (2, 3, 4):
                for dtype in DTYPES:
                    res = o["res"].to(dtype)
                    got = ops.gemm_bf16_splitk(a, b, s, bias=bias, res=res.to(dev), out_dtype=dtype)
                    assert got.dtype == dtype
                    _collect(fails, f"gemm {shape} tile {tile} splitk-epilogue {s} {_leg(ops)}", got, _epi_terms(o, dtype)["res"])
    assert not fails, "\n".join(fails)


_SPLIT_IDS = ["x".join(map(str, s)) for s in SPLIT_SHAPES]


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=_SPLIT_IDS)
def test_split_k_sim(emu, shape):
    _splitk(emu, "cpu", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=_SPLIT_IDS)
def test_split_k_gpu(hip, shape):
    _splitk(hip, "cuda", shape)


# ---------------------------------------------------------------------------------------------------------------------
# 4. head-split epilogues, plain and qk_norm: q, k and V^T element by element to the bf16 rule
# ---------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(2, 71, 3, 72), (3, 70, 2, 64), (2, 69, 2, 64), (2, 70, 2, 136)]      # (nb, ntok, heads, K): every ntok residue mod 4 but 0
SECTIONS = [(0, 3), (0, 1), (1, 2)]


def _head_operands(case):
    key = ("heads",) + case
    if key not in _prepared:
        nb, ntok, heads, k = case
        gen = torch.Generator().manual_seed(7200 + ntok + k)
        o = {"x": torch.randn(nb * ntok, k, generator=gen).bfloat16(), "w": (torch.randn(3 * heads * 64, k, generator=gen) / k ** 0.5).bfloat16(),
             # LayerNorm tables far from (1, 0): q gamma, q beta, k gamma, k beta
             "tabs": [2.0 * torch.randn(64, generator=gen), 3.0 * torch.randn(64, generator=gen),
                      0.5 + 2.0 * torch.randn(64, generator=gen), -1.0 + 3.0 * torch.randn(64, generator=gen)]}
        o["proj"] = G.projection(o["x"], o["w"])
        _prepared[key] = o
    return _prepared[key]


def _valid(pl, name, ntok):
    """(valid part, padding) of a plane as bf16"""
    t = pl[name].view(BF16)
    return (t[..., :ntok], t[..., ntok:]) if name == "v_tr" else (t[:, :, :ntok], t[:, :, ntok:])


def _heads(ops, dev, case, mode, tiles):
    nb, ntok, heads, k = case
    o = _head_operands(case)
    x, w = o["x"].to(dev), o["w"].to(dev)
    tabs_d = [t.to(dev) for t in o["tabs"]]
    hd = heads * 64
    fails = []
    for rope in (True, False):
        cs = ops.rope_tables(INV.to(dev), ntok + 3) if rope else None      # longer table: the rows ntok + 3 - ntok .. are the sequence's
        for sec0, nsec in SECTIONS:
            terms = G.heads(o["proj"].cols(sec0 * hd, (sec0 + nsec) * hd), cs, heads, nb, ntok, sec0, nsec, mode, o["tabs"])
            for tile in tiles:
                with _Forced(ops, tile):
                    pl = ops.gemm_heads_bf16(x, w[sec0 * hd:(sec0 + nsec) * hd], cs, heads, nb, ntok, sec0, nsec, qk_norm=mode, norm_tables=tabs_d)
                assert set(terms) == {n for n in ("q", "k", "v_tr") if n in pl}
                for name, t in terms.items():
                    got, pad = _valid(pl, name, ntok)
                    assert float(pad.float().abs().max()) == 0.0
                    _collect(fails, f"heads {case} {mode or 'plain'} rope {int(rope)} sections {sec0}+{nsec} tile {tile} {name} {_leg(ops)}", got, t)
    assert not fails, "\n".join(fails)


_HEAD_IDS = ["x".join(map(str, c)) for c in HEAD_CASES]


@pytest.mark.parametrize("case", HEAD_CASES, ids=_HEAD_IDS)
def test_heads_epilogue_sim(emu, case):
    _heads(emu, "cpu", case, None, TILES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=_HEAD_IDS)
def test_heads_epilogue_gpu(hip, case):
    _heads(hip, "cuda", case, None, TILES)


@pytest.mark.parametrize("mode", ["ln", "l2"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=_HEAD_IDS)
def test_heads_norm_epilogue_sim(emu, case, mode):
    _heads(emu, "cpu", case, mode, (0, 7, 8, None))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ln", "l2"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=_HEAD_IDS)
def test_heads_norm_epilogue_gpu(hip, case, mode):
    _heads(hip, "cuda", case, mode, (0, 7, 8, None))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the library's own tile choice: the tile is asserted first, so the case cannot silently change what it covers
# ---------------------------------------------------------------------------------------------------------------------
def _own_choice(ops, dev):
    assert ops.gemm_tile is None
    shape = (290, 520, 328)
    o = _operands(shape)
    assert ops._pick_tile(290, 520, 1, 328) == 8          # 15 workgroups of 128 x 128 on eight waves: the cheapest under _TILE_MODEL
    fails = []
    for dtype in DTYPES:
        _collect(fails, f"gemm {shape} own tile bias {_leg(ops)}", ops.gemm_bf16(o["a"].to(dev), o["b"].to(dev), bias=o["bias"].to(dev), out_dtype=dtype),
                 _epi_terms(o, dtype)["bias"])
    case = (2, 70, 2, 136)
    nb, ntok, heads, k = case
    h = _head_operands(case)
    assert ops._pick_tile(nb * ntok, 3 * heads * 64, 1, k) == 8
    cs = ops.rope_tables(INV.to(dev), ntok + 3)
    pl = ops.gemm_heads_bf16(h["x"].to(dev), h["w"].to(dev), cs, heads, nb, ntok, 0, 3)
    for name, t in G.heads(h["proj"], cs, heads, nb, ntok, 0, 3).items():
        _collect(fails, f"heads {case} own tile {name} {_leg(ops)}", _valid(pl, name, ntok)[0], t)
    assert not fails, "\n".join(fails)


def test_own_tile_choice_sim(emu):
    _own_choice(emu, "cpu")


@pytest.mark.gpu
def test_own_tile_choice_gpu(hip):
    _own_choice(hip, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 6. structure
# ---------------------------------------------------------------------------------------------------------------------
NAN8 = 0x7F       # e4m3 NaN
FP8_SHAPE = (130, 144, 144)


def _padded(t, left, right, fill):
    """t's values as a column slice of a wider buffer whose padding holds `fill`: row stride = columns + left + right"""
    buf = torch.full((t.shape[0], t.shape[1] + left + right), fill, dtype=t.dtype, device=t.device)
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return view


def _same(name, got, want):
    got, want = (t if isinstance(t, tuple) else (t,) for t in (got, want))
    for g, w in zip(got, want):
        assert bool(torch.isfinite(g.float()).all()), f"{name}: not finite"
        assert torch.equal(g, w), f"{name}: differs from the packed call"


def _fp8_operands(ops, dev, shape=FP8_SHAPE):
    m, n, k = shape
    gen = torch.Generator().manual_seed(7300)
    x, w = torch.randn(m, k, generator=gen).to(dev), (torch.randn(n, k, generator=gen) / 12).to(dev)
    qx, sx = ops.quant_fp8(x)
    qw, sw = ops.quant_fp8(w)
    return qx, qw, sx * sw, torch.randn(n, generator=gen).to(dev), torch.randn(m, n, generator=gen).to(dev)


def _strided(ops, dev, shape):
    """lda = K + 24, ldb = K + 8, ldr = N + 8 (and a strided gate), NaN in all padding: finite, bit-equal to the contiguous call"""
    o = _operands(shape)
    nan = float("nan")
    a, b = o["a"].to(dev), o["b"].to(dev)
    ap, bp = _padded(a, 8, 16, nan), _padded(b, 0, 8, nan)
    assert ap.stride(0) == a.shape[1] + 24 and bp.stride(0) == b.shape[1] + 8
    for dtype in DTYPES:
        packed = dict(o, res=o["res"].to(dtype).to(dev), gate=o["gate"].to(dtype).to(dev))
        padded = dict(packed, a=ap, b=bp, res=_padded(packed["res"], 0, 8, nan), gate=_padded(packed["gate"], 0, 8, nan))
        for tile in TILES:
            with _Forced(ops, tile):
                want, got = _epi_calls(ops, dev, packed, dtype), _epi_calls(ops, dev, padded, dtype)
            for label in want:
                _same(f"strided {shape} tile {tile} {label} {str(dtype)[6:]}", got[label], want[label])
    if shape != STRIDED_SHAPES[0]:      # fp8 (130, 144, 144): once
        return
    qx, qw, alpha, bias, res = _fp8_operands(ops, dev)
    qxp, qwp, resp = _padded(qx, 16, 16, NAN8), _padded(qw, 0, 16, NAN8), _padded(res, 0, 8, nan)
    for tile in TILES:
        with _Forced(ops, tile, "gemm_fp8_tile"):
            for epi in (ops.EPI_RES, ops.EPI_SWIGLU):
                kw = dict(bias=bias, epilogue=epi, out_dtype=F32)
                want = ops.gemm_fp8(qx, qw, alpha, res=res if epi == ops.EPI_RES else None, **kw)
                got = ops.gemm_fp8(qxp, qwp, alpha, res=resp if epi == ops.EPI_RES else None, **kw)
                _same(f"strided fp8 tile {tile} epilogue {epi}", got, want)


STRIDED_SHAPES = [(130, 136, 72), (70, 264, 200)]


@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=["130x136x72", "70x264x200"])
def test_strided_operands_sim(emu, shape):
    _strided(emu, "cpu", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=["130x136x72", "70x264x200"])
def test_strided_operands_gpu(hip, shape):
    _strided(hip, "cuda", shape)


SENTINEL = 7.0


def _guarded(m, ncols, dtype, dev):
    buf = torch.full((m + 16, ncols), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[8:8 + m]


def _guard_ok(name, buf, m, want):
    """want: the same call without `out`, made only after the sentinel has been found intact"""
    assert bool((buf[:8] == SENTINEL).all()) and bool((buf[8 + m:] == SENTINEL).all()), f"{name}: a row outside [0, M) was written"
    assert torch.equal(buf[8:8 + m], want()), f"{name}: differs from the call without `out`"


def _guard_rows(ops, dev, shape):
    """`out=` is rows 8 .. 8 + M of a sentinel-filled buffer: the sentinel survives above and below (M = 130: a partial MFMA block in a
    wave's rows; M = 33: whole idle waves), every tile, fp32 and bf16, the split-K epilogue and fp8 included"""
    o = _operands(shape)
    m, n, _ = shape
    a, b, bias, sbias = (o[x].to(dev) for x in ("a", "b", "bias", "sbias"))
    for dtype in DTYPES:
        res = o["res"].to(dtype).to(dev)
        for tile in TILES:
            with _Forced(ops, tile):
                name = f"guard rows {shape} tile {tile} {str(dtype)[6:]}"
                buf, out = _guarded(m, n, dtype, dev)
                ops.gemm_bf16(a, b, bias=bias, res=res, epilogue=ops.EPI_RES, out_dtype=dtype, out=out)
                _guard_ok(name + " res", buf, m, lambda: ops.gemm_bf16(a, b, bias=bias, res=res, epilogue=ops.EPI_RES, out_dtype=dtype))
                buf, out = _guarded(m, o["n16"] // 2, dtype, dev)
                ops.gemm_bf16(a, b[:o["n16"]], bias=sbias, epilogue=ops.EPI_SWIGLU, out_dtype=dtype, out=out)
                _guard_ok(name + " swiglu", buf, m, lambda: ops.gemm_bf16(a, b[:o["n16"]], bias=sbias, epilogue=ops.EPI_SWIGLU, out_dtype=dtype))
                buf, out = _guarded(m, n, dtype, dev)
                ops.gemm_bf16_splitk(a, b, 2, bias=bias, res=res, out_dtype=dtype, out=out)
                _guard_ok(name + " splitk", buf, m, lambda: ops.gemm_bf16_splitk(a, b, 2, bias=bias, res=res, out_dtype=dtype))
    mf = m                           # fp8: (130 | 33, 144, 144)
    qx, qw, alpha, bias8, res8 = _fp8_operands(ops, dev, (mf,) + FP8_SHAPE[1:])
    for dtype in DTYPES:
        for tile in TILES:
            with _Forced(ops, tile, "gemm_fp8_tile"):
                buf, out = _guarded(mf, FP8_SHAPE[1], dtype, dev)
                kw = dict(bias=bias8, res=res8.to(dtype), epilogue=ops.EPI_RES, out_dtype=dtype)
                ops.gemm_fp8(qx, qw, alpha, out=out, **kw)
                _guard_ok(f"guard rows fp8 M {mf} tile {tile} {str(dtype)[6:]}", buf, mf, lambda: ops.gemm_fp8(qx, qw, alpha, **kw))


GUARD_SHAPES = [(130, 136, 72), (33, 64, 8)]


@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=["M130", "M33"])
def test_guard_rows_sim(emu, shape):
    _guard_rows(emu, "cpu", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=["M130", "M33"])
def test_guard_rows_gpu(hip, shape):
    _guard_rows(hip, "cuda", shape)


def _column_padding(ops, dev, shape=(130, 136, 72)):
    """Through the C entry, once per epilogue (and tile, and output type): ldc, ldr, ldg, ldp wider than the logical width (multiples of 4,
    as the 8- and 16-byte accesses need), a sentinel in the output padding and NaN in the input padding — the sentinel survives and the
    values are bit-equal to the packed call."""
    from stable_audio_tools_amd.ops import _ptr
    o = _operands(shape)
    m, n, k = shape
    nan = float("nan")
    a, b, bias, sbias = (o[x].to(dev) for x in ("a", "b", "bias", "sbias"))
    n16 = o["n16"]
    for dtype in DTYPES:
        packed = dict(o, res=o["res"].to(dtype).to(dev), gate=o["gate"].to(dtype).to(dev))
        res, gate = _padded(packed["res"], 0, 12, nan), _padded(packed["gate"], 0, 4, nan)
        rpg = m // gate.shape[0]
        for tile in TILES:
            with _Forced(ops, tile):
                want = _epi_calls(ops, dev, packed, dtype)
            for label, epi in (("bias", ops.EPI_STORE), ("res", ops.EPI_RES), ("gate_res", ops.EPI_GATE_RES), ("swiglu", ops.EPI_SWIGLU)):
                glu = epi == ops.EPI_SWIGLU
                nn = n16 if glu else n
                nout = nn // 2 if glu else nn
                c = torch.full((m, nout + 8), SENTINEL, dtype=dtype, device=dev)
                pre = torch.full((m, nn + 16), SENTINEL, dtype=dtype, device=dev) if glu else None
                use_res, use_gate = epi in (ops.EPI_RES, ops.EPI_GATE_RES), epi == ops.EPI_GATE_RES
                ops._chk(ops.lib.sat_gemm_bf16(_ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(c), c.stride(0), _ptr(sbias if glu else bias),
                                               _ptr(res) if use_res else None, res.stride(0) if use_res else 0,
                                               _ptr(gate) if use_gate else None, gate.stride(0) if use_gate else 0, rpg if use_gate else 0,
                                               _ptr(pre), pre.stride(0) if glu else 0, _ptr(ops._zeros_page(a.device)), m, nn, k, epi,
                                               int(dtype == F32), 1, tile, ops._stream(a)))
                name = f"column padding {shape} tile {tile} {label} {str(dtype)[6:]}"
                assert bool((c[:, nout:] == SENTINEL).all()), f"{name}: a column past the logical width was written"
                _same(name, c[:, :nout], want[label])
                if glu:
                    assert bool((pre[:, nn:] == SENTINEL).all()), f"{name}: a column of `pre` past the logical width was written"
                    _same(name + " pre", pre[:, :nn], want["pre"])


def test_column_padding_sim(emu):
    _column_padding(emu, "cpu")


@pytest.mark.gpu
def test_column_padding_gpu(hip):
    _column_padding(hip, "cuda")


PLANE_CASES = [(2, 71, 3, 80), (3, 70, 2, 80), (3, 69, 2, 80)]      # nb = 2 and 3: windows straddle batch items in every V^T store phase
PLANE_SENTINEL = 0x4242                                                # 48.5 as bf16


def _planes_once(ops, name, call, tag, ntok):
    """`call(reuse=tag)` twice with the planes filled with a non-zero sentinel in between: the same storage comes back, every row / column
    past ntok keeps the sentinel, the valid part is bit-equal to the first call's"""
    pl = call(reuse=tag)
    names = [n for n in ("q", "k", "v_tr") if n in pl]
    first = {n: _valid(pl, n, ntok)[0].clone() for n in names}
    ptrs = {n: pl[n].data_ptr() for n in names}
    for n in names:
        pl[n].fill_(PLANE_SENTINEL)
    del pl
    again = call(reuse=tag)
    for n in names:
        assert again[n].data_ptr() == ptrs[n], f"{name} {n}: the persistent plane moved"
        valid, pad = _valid(again, n, ntok)
        assert pad.numel() > 0 and bool((pad.view(torch.int16) == PLANE_SENTINEL).all()), f"{name} {n}: the padding past ntok was written"
        assert torch.equal(valid, first[n]), f"{name} {n}: the valid part changed"


def _persistent_planes(ops, dev, case):
    nb, ntok, heads, k = case
    gen = torch.Generator().manual_seed(7400 + ntok)
    x32, w32 = torch.randn(nb * ntok, k, generator=gen).to(dev), (torch.randn(3 * heads * 64, k, generator=gen) / k ** 0.5).to(dev)
    x, w = x32.bfloat16(), w32.bfloat16()
    tabs = [torch.randn(64, generator=gen).to(dev) for _ in range(4)]
    cs = ops.rope_tables(INV.to(dev), ntok + 3)
    for tile in TILES:
        with _Forced(ops, tile):
            _planes_once(ops, f"planes {case} tile {tile} plain", lambda reuse: ops.gemm_heads_bf16(x, w, cs, heads, nb, ntok, 0, 3, reuse=reuse),
                         ("gemm_fp64", "plain", tile), ntok)
            if tile != 4:
                for mode in ("ln", "l2"):
                    _planes_once(ops, f"planes {case} tile {tile} {mode}", lambda reuse: ops.gemm_heads_bf16(
                        x, w, cs, heads, nb, ntok, 0, 3, reuse=reuse, qk_norm=mode, norm_tables=tabs), ("gemm_fp64", mode, tile), ntok)
    qx, sx = ops.quant_fp8(x32)
    qw, sw = ops.quant_fp8(w32)
    for tile in TILES:
        with _Forced(ops, tile, "gemm_fp8_tile"):
            _planes_once(ops, f"planes {case} tile {tile} fp8", lambda reuse: ops.gemm_heads_fp8(qx, qw, sx * sw, cs, heads, nb, ntok, 0, 3, reuse=reuse),
                         ("gemm_fp64", "fp8", tile), ntok)


_PLANE_IDS = ["x".join(map(str, c)) for c in PLANE_CASES]


@pytest.mark.parametrize("case", PLANE_CASES, ids=_PLANE_IDS)
def test_persistent_planes_sim(emu, case):
    _persistent_planes(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLANE_CASES, ids=_PLANE_IDS)
def test_persistent_planes_gpu(hip, case):
    _persistent_planes(hip, "cuda", case)
