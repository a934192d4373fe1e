"""The DiT's pointwise kernels (csrc/dit_ops.hip: sat_swiglu, sat_gate_residual / _bwd, sat_rope_tables, sat_rope_apply), one at a time,
against plain float64 torch of the reference's own formulas (transformer.py: GLU.forward :274-275, the gated residual :684-701,
RotaryEmbedding.forward :125-138, apply_rotary_pos_emb :155-174) on the inputs the kernel gets.  Shapes: the scalar tails, a column one
past a 256-wide block, several row chunks of the dgate reduction, a strided q|k view, heads wider than the rotary, a table longer than
the sequence — and one size per flat kernel past the 8192 x 256 threads its capped grid covers in one trip (the stride loop).
Bounds: tests/fp64_bounds.py.  CPU leg under the host simulator, GPU leg through the gfx950 library."""
import pytest
import torch
import torch.nn.functional as F

from fp64_bounds import check, f64, leaf, smax

DTYPES = [torch.float32, torch.bfloat16]
GRID_CAP = 8192 * 256                       # elements one trip of the capped grid covers

# ---------------------------------------------------------------------------------------------------------------------
# SwiGLU: x * silu(gate) on (rows, 2F) = [x | gate]
# ---------------------------------------------------------------------------------------------------------------------
SWIGLU_SHAPES = [(3, 5), (7, 200), (2, 1536), (1366, 1536)]
PLANTED_GATES = (30.0, -30.0, -100.0, 0.0)  # sigmoid saturated both ways, expf(100) overflows fp32, the midpoint


def _plant(flat, values):
    """values at known positions near the start and, on tensors long enough, at the very end (the stride-loop trip of the large shape)"""
    for i, v in enumerate(values):
        flat[1 + 3 * i] = v
        if flat.numel() > 64:
            flat[flat.numel() - 1 - 5 * i] = v


def _swiglu_case(ops, dev, dtype, rows, f, seed):
    gen = torch.Generator().manual_seed(seed)
    a, b = torch.randn(rows, f, generator=gen), 2.0 * torch.randn(rows, f, generator=gen)
    _plant(b.view(-1), PLANTED_GATES)
    xin = torch.cat([a, b], dim=1).to(dtype)
    dout = torch.randn(rows, f, generator=gen).to(dtype)
    out = ops.swiglu(xin.to(dev))
    dxin = ops.swiglu_bwd(xin.to(dev), dout.to(dev))
    assert out.dtype == dtype and dxin.dtype == dtype and out.shape == (rows, f) and dxin.shape == (rows, 2 * f)

    def formula(t):
        xi = leaf(xin, t)
        y = xi[:, :f] * F.silu(xi[:, f:])
        y.backward(dout.to(t))
        return y.detach(), xi.grad[:, :f], xi.grad[:, f:]
    y64, da64, db64 = formula(torch.float64)
    y32, da32, db32 = formula(torch.float32)
    x, g, d = f64(xin[:, :f]), f64(xin[:, f:]), f64(dout)
    sg = torch.sigmoid(g)
    tag = f"swiglu[{rows}x{f}]"
    check(tag + " fwd", out, y64, y32, smax(y64.abs()))                                   # one product
    check(tag + " d_x", dxin[:, :f], da64, da32, smax(da64.abs()))                        # one product
    check(tag + " d_gate", dxin[:, f:], db64, db32, smax((d * x * sg).abs() + (d * x * sg * g * (1 - sg)).abs()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SWIGLU_SHAPES)
def test_swiglu_sim(emu, shape, dtype):
    _swiglu_case(emu, "cpu", dtype, *shape, seed=31)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SWIGLU_SHAPES)
def test_swiglu_gpu(hip, shape, dtype):
    _swiglu_case(hip, "cuda", dtype, *shape, seed=32)


def test_swiglu_large_shape_reaches_the_stride_loop():
    assert max(r * f for r, f in SWIGLU_SHAPES) > GRID_CAP


# ---------------------------------------------------------------------------------------------------------------------
# gate / residual: y = x * sigmoid(1 - gate[b]) + res, gate the [:, 2D:3D] slice of the (B, 6D) adaLN modulation
# ---------------------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(2, 9, 200), (1, 33, 300), (2, 130, 257), (1, 65, 1536), (3, 700, 1000)]


def _gate_case(ops, dev, dtype, b, n, d, seed):
    gen = torch.Generator().manual_seed(seed)
    mod = (1.5 * torch.randn(b, 6 * d, generator=gen)).to(dtype)
    x, res, dy = (torch.randn(b, n, d, generator=gen).to(dtype) for _ in range(3))
    gate_dev = mod.to(dev)[:, 2 * d:3 * d]
    assert gate_dev.stride(0) == 6 * d
    nch = ops.lib.sat_gate_residual_bwd_nchunks(n)
    assert nch == -(-n // 64), (n, nch)
    y = ops.gate_residual(x.to(dev), gate_dev, res.to(dev))
    dx, dgate = ops.gate_residual_bwd(dy.to(dev), x.to(dev), gate_dev)
    assert y.dtype == dtype and dx.dtype == dtype and dgate.dtype == torch.float32 and dgate.shape == (b, d)

    def formula(t):
        xr = leaf(x, t)
        gr = leaf(mod[:, 2 * d:3 * d], t)
        out = xr * torch.sigmoid(1 - gr[:, None, :]) + res.to(t)
        out.backward(dy.to(t))
        return out.detach(), xr.grad, gr.grad
    y64, dx64, dg64 = formula(torch.float64)
    y32, dx32, dg32 = formula(torch.float32)
    s = torch.sigmoid(1 - f64(mod[:, 2 * d:3 * d]))[:, None, :]
    tag = f"gate_residual[{b}x{n}x{d}]"
    check(tag + " fwd", y, y64, y32, smax((f64(x) * s).abs() + f64(res).abs()))
    check(tag + " dx", dx, dx64, dx32, smax(dx64.abs()))
    check(tag + " dgate", dgate, dg64, dg32, smax(((f64(dy) * f64(x)).abs() * (s * (1 - s))).sum(1)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_gate_residual_sim(emu, shape, dtype):
    _gate_case(emu, "cpu", dtype, *shape, seed=41)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_gate_residual_gpu(hip, shape, dtype):
    _gate_case(hip, "cuda", dtype, *shape, seed=42)


def test_gate_shapes_cover_the_chunks_and_the_stride_loop():
    assert sorted({-(-n // 64) for _, n, _ in GATE_SHAPES}) == [1, 2, 3, 11]
    assert max(b * n * d for b, n, d in GATE_SHAPES) > GRID_CAP


# ---------------------------------------------------------------------------------------------------------------------
# rotary tables and their application
# ---------------------------------------------------------------------------------------------------------------------
def _inv_freq(half):
    return 1.0 / (10000.0 ** (torch.arange(0, 2 * half, 2).float() / (2 * half)))       # RotaryEmbedding.__init__ :100-101


def _rope_tables_case(ops, dev, pos_scale):
    n, half = 1028, 16
    inv_freq = _inv_freq(half)
    cs = ops.rope_tables(inv_freq.to(dev), n, pos_scale)
    assert cs.shape == (n, half, 2)
    # the angle is formed in fp32 in the reference's order, (n * inv_freq) * pos_scale; cos / sin of THAT angle in float64
    ang = (torch.arange(n).float()[:, None] * inv_freq[None, :]) * torch.tensor(pos_scale, dtype=torch.float32)
    assert ang.dtype == torch.float32
    ref = torch.stack([torch.cos(ang.double()), torch.sin(ang.double())], dim=-1)
    f32 = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
    check(f"rope_tables[pos_scale={pos_scale}]", cs, ref, f32, 1.0)                       # |cos| reaches 1 at n = 0


@pytest.mark.parametrize("pos_scale", [1.0, 0.37])
def test_rope_tables_sim(emu, pos_scale):
    _rope_tables_case(emu, "cpu", pos_scale)


@pytest.mark.gpu
@pytest.mark.parametrize("pos_scale", [1.0, 0.37])
def test_rope_tables_gpu(hip, pos_scale):
    _rope_tables_case(hip, "cuda", pos_scale)


def _rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat([-x2, x1], dim=-1)


def _rope_formula(t, cs, off, sign):
    """apply_rotary_pos_emb (transformer.py:155-174) in t's dtype on a (B, N, H, dh) tensor: t * cos + rotate_half(t) * sin over the first
    2 * half dims with the table rows off + n (freqs[-seq_len:]); sign = -1: the transpose."""
    n, half = t.shape[1], cs.shape[1]
    c, s = cs[off:off + n, :, 0].to(t.dtype), sign * cs[off:off + n, :, 1].to(t.dtype)
    cos, sin = torch.cat([c, c], dim=-1)[None, :, None, :], torch.cat([s, s], dim=-1)[None, :, None, :]
    rot, rest = t[..., :2 * half], t[..., 2 * half:]
    return torch.cat([rot * cos + _rotate_half(rot) * sin, rest], dim=-1)


ROPE_KINDS = {
    # name: (shape of the buffer, how the rotated (B, N, H, dh) view is cut from it)
    "fused_qkv": ((2, 11, 3 * 3 * 64), lambda buf: buf[..., :2 * 3 * 64].view(2, 11, 2 * 3, 64)),       # q|k of a fused projection, v behind it
    "wide_heads": ((2, 17, 5, 96), lambda buf: buf),                                                   # 16 pairs in 96-wide heads
    "stride_loop": ((3, 1025, 48, 64), lambda buf: buf),                                               # 2 361 600 pairs
}
OFF = 3


def _rope_apply_case(ops, dev, dtype, kind, seed):
    shape, cut = ROPE_KINDS[kind]
    gen = torch.Generator().manual_seed(seed)
    buf0 = torch.randn(*shape, generator=gen).to(dtype)
    t0 = cut(buf0)
    b, n, h, dh = t0.shape
    half = 16
    cs = ops.rope_tables(_inv_freq(half).to(dev), n + OFF)
    csc = cs.cpu()
    x1, x2 = f64(t0[..., :half]), f64(t0[..., half:2 * half])
    c, s = csc[OFF:, :, 0].double()[None, :, None, :], csc[OFF:, :, 1].double()[None, :, None, :]
    scale = smax(torch.maximum((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()))
    for transpose in (False, True):
        sign = -1.0 if transpose else 1.0
        buf = buf0.clone().to(dev)
        t = cut(buf)
        if kind == "fused_qkv":
            assert not t.is_contiguous() and t.stride(1) == 3 * 3 * 64
        assert ops.rope_apply_(t, cs, transpose=transpose) is t
        ref64 = _rope_formula(f64(t0), csc.double(), OFF, sign)
        f32 = _rope_formula(t0.float(), csc, OFF, sign)
        check(f"rope_apply[{kind}{' T' if transpose else ''}]", t, ref64, f32, scale)
        assert torch.equal(t[..., 2 * half:].cpu(), t0[..., 2 * half:])               # columns past the rotary: bit-unchanged
        if kind == "fused_qkv":
            assert torch.equal(buf[..., 2 * 3 * 64:].cpu(), buf0[..., 2 * 3 * 64:])   # the v third: bit-unchanged
        if dtype == torch.float32 and not transpose:
            # forward then transpose: (c^2 + s^2) x.  Each rotation rounds two products and a sum, <= 2u (|x1| + |x2|) per pass with
            # u = 2^-24, the second pass on a vector no longer than sqrt(2) of that; table entries a few ulp off make |c^2 + s^2 - 1| <= 4u:
            # (2 + 2 sqrt(2) + 4) u < 12 u of the largest |x1| + |x2|.
            ops.rope_apply_(t, cs, transpose=True)
            back = float((f64(t) - f64(t0)).abs().max())
            bound = 12 * 2.0 ** -24 * float((x1.abs() + x2.abs()).max())
            print(f"FIGURE rope_apply[{kind}] round trip: {back:.3e} (bound {bound:.3e})")
            assert back <= bound, (kind, back, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(ROPE_KINDS))
def test_rope_apply_sim(emu, kind, dtype):
    _rope_apply_case(emu, "cpu", dtype, kind, seed=51)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(ROPE_KINDS))
def test_rope_apply_gpu(hip, kind, dtype):
    _rope_apply_case(hip, "cuda", dtype, kind, seed=52)


def test_rope_large_shape_reaches_the_stride_loop():
    b, n, h, _ = ROPE_KINDS["stride_loop"][0]
    assert b * n * h * 16 > GRID_CAP


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers hand raw pointers to kernels that assume contiguous tensors: other layouts are refused, not mis-read
# ---------------------------------------------------------------------------------------------------------------------
def _guards_case(ops, dev):
    xin = torch.randn(6, 8).to(dev)
    dout = torch.randn(6, 4).to(dev)
    ops.swiglu(xin), ops.swiglu_bwd(xin, dout)
    with pytest.raises(ValueError):
        ops.swiglu(torch.randn(8, 6).to(dev).t())                       # transposed view
    with pytest.raises(ValueError):
        ops.swiglu(torch.randn(6, 16).to(dev)[:, :8])                   # row stride != 2F
    with pytest.raises(ValueError):
        ops.swiglu_bwd(xin.t().contiguous().t(), dout)
    with pytest.raises(ValueError):
        ops.swiglu_bwd(xin, torch.randn(4, 6).to(dev).t())
    with pytest.raises(ValueError):
        ops.swiglu_bwd(xin, torch.randn(6, 3).to(dev))                  # another F
    b, n, d = 2, 5, 12
    x, res, dy = (torch.randn(b, n, d).to(dev) for _ in range(3))
    mod = torch.randn(b, 6 * d).to(dev)
    gate = mod[:, 2 * d:3 * d]
    ops.gate_residual(x, gate, res), ops.gate_residual_bwd(dy, x, gate)
    xt = torch.randn(b, d, n).to(dev).transpose(1, 2)                   # (B, N, D) view of a (B, D, N) tensor
    gt = torch.randn(d, b).to(dev).t()                                  # (B, D) with last stride B
    for bad in ((xt, gate, res), (x, gate, xt), (x, gt, res), (x, mod[:, :d + 1], res), (x, gate, res[:, :4])):
        with pytest.raises(ValueError):
            ops.gate_residual(*bad)
    for bad in ((xt, x, gate), (dy, xt, gate), (dy, x, gt), (dy[:1], x, gate)):
        with pytest.raises(ValueError):
            ops.gate_residual_bwd(*bad)


def test_wrapper_layout_guards_sim(emu):
    _guards_case(emu, "cpu")


@pytest.mark.gpu
def test_wrapper_layout_guards_gpu(hip):
    _guards_case(hip, "cuda")
