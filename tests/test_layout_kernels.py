"""The layout junction of the transformer autoencoder (csrc/layout.hip): ops.ct_to_tokens (fp32 (B, C, T) -> (B, T, C) tokens in fp32
or bf16) and ops.tokens_to_ct (the inverse, always fp32) against torch's transpose(1, 2).contiguous().  A transpose moves values and the
bf16 form rounds each once to nearest even, as torch's .to(torch.bfloat16) does, so every comparison is bit for bit — no tolerance.
Shapes: one element; the smallest vector-path shape; whole tiles; one column past a tile; odd sizes on the vector path's C but not its T;
C and T that are no multiple of 64 with several tiles each way; C < 8 (scalar path); and a base address that is not 16-byte aligned.
CPU: the simulator; `-m gpu`: the gfx950 library, plus one tensor above 2^31 bytes (element offsets past 2^31 bytes / tile ids past
65535 along one dim)."""
import pytest
import torch

SHAPES = [(1, 1, 1), (2, 8, 4), (1, 128, 64), (1, 128, 65), (3, 24, 63), (1, 136, 1043), (2, 7, 130), (1, 256, 521)]


def _input(shape, device, offset=0):
    b, c, t = shape
    g = torch.Generator().manual_seed(1000 + b + 7 * c + 13 * t)
    buf = torch.randn(b * c * t + offset, generator=g).to(device)
    x = buf[offset:].view(b, c, t)
    assert x.is_contiguous() and (offset == 0 or x.data_ptr() % 16 != 0)
    return x


def _check(ops, shape, device, offset=0):
    x = _input(shape, device, offset)
    want = x.transpose(1, 2).contiguous()
    tok = ops.ct_to_tokens(x)
    assert tok.dtype == torch.float32 and tok.shape == want.shape and torch.equal(tok, want)
    tok16 = ops.ct_to_tokens(x, torch.bfloat16)
    assert tok16.dtype == torch.bfloat16 and torch.equal(tok16, want.to(torch.bfloat16))
    # the inverse, from fp32 tokens (the round trip is the identity) and from bf16 tokens; token views with the same offset base
    assert torch.equal(ops.tokens_to_ct(tok), x)
    back16 = ops.tokens_to_ct(tok16)
    assert back16.dtype == torch.float32 and torch.equal(back16, tok16.float().transpose(1, 2).contiguous())
    if offset:
        tsrc = _input((shape[0], shape[2], shape[1]), device, offset)      # (B, T, C) tokens at a misaligned base
        assert torch.equal(ops.tokens_to_ct(tsrc), tsrc.transpose(1, 2).contiguous())
        t16 = torch.zeros(tsrc.numel() + 1, dtype=torch.bfloat16, device=device)
        t16[1:] = tsrc.reshape(-1).to(torch.bfloat16)
        t16 = t16[1:].view(tsrc.shape)
        assert t16.data_ptr() % 16 != 0
        assert torch.equal(ops.tokens_to_ct(t16), t16.float().transpose(1, 2).contiguous())


def _refusals(ops, device):
    x = torch.zeros(2, 8, 4, device=device)
    for bad in (x[:, :, :2], x.transpose(1, 2), x[0], x.double(), x.to(torch.bfloat16), torch.zeros(2, 0, 4, device=device)):
        with pytest.raises(ValueError, match="ct_to_tokens"):
            ops.ct_to_tokens(bad)
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            ops.ct_to_tokens(x, dt)
    for bad in (x[:, :, :2], x.transpose(1, 2), x[0], x.half(), torch.zeros(0, 8, 4, device=device)):
        with pytest.raises(ValueError, match="tokens_to_ct"):
            ops.tokens_to_ct(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_simulator(emu, shape):
    _check(emu, shape, "cpu")


def test_layout_misaligned_base_simulator(emu):
    _check(emu, (2, 8, 12), "cpu", offset=1)
    _check(emu, (1, 72, 68), "cpu", offset=3)


def test_layout_refusals_simulator(emu):
    _refusals(emu, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_gpu(hip, shape):
    _check(hip, shape, "cuda")


@pytest.mark.gpu
def test_layout_misaligned_base_gpu(hip):
    _check(hip, (2, 8, 12), "cuda", offset=1)
    _check(hip, (1, 72, 68), "cuda", offset=3)


@pytest.mark.gpu
def test_layout_refusals_gpu(hip):
    _refusals(hip, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.ct_to_tokens(torch.zeros(1, 8, 4))


@pytest.mark.gpu
def test_layout_graph_capture_gpu(hip):
    """one launch, no workspace: both directions replay from a HIP graph"""
    x = _input((1, 136, 1043), "cuda")
    hip.tokens_to_ct(hip.ct_to_tokens(x, torch.bfloat16))      # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tok = hip.ct_to_tokens(x, torch.bfloat16)
        back = hip.tokens_to_ct(tok)
    x.copy_(_input((1, 136, 1043), "cuda") * 2.0)
    g.replay()
    torch.cuda.synchronize()
    want = x.transpose(1, 2).contiguous().to(torch.bfloat16)
    assert torch.equal(tok, want) and torch.equal(back, want.float().transpose(1, 2).contiguous())


@pytest.mark.gpu
def test_layout_above_2g_gpu(hip):
    """(1, 128, 2^22 + 3): 2^31 + 1536 bytes per fp32 tensor, 65537 tiles along T; against torch on the device"""
    b, c, t = 1, 128, 2 ** 22 + 3
    x = torch.randn(b, c, t, device="cuda")
    assert x.numel() * 4 > 2 ** 31
    want = x.transpose(1, 2).contiguous()
    tok = hip.ct_to_tokens(x)
    assert torch.equal(tok, want)
    back = hip.tokens_to_ct(tok)
    assert torch.equal(back, x)
    del back, tok
    tok16 = hip.ct_to_tokens(x, torch.bfloat16)
    assert torch.equal(tok16, want.to(torch.bfloat16))
    del want
    assert torch.equal(hip.tokens_to_ct(tok16), tok16.float().transpose(1, 2).contiguous())
