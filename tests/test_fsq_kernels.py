"""The eval-mode dithered-FSQ quantiser (csrc/fsq.hip): ops.fsq_encode (fp32 (B, C, T) latents -> codes (B, C, T) and int64 token ids
(B, T, Q)) and ops.fsq_decode_tokens (token ids -> codes) against fixtures of the reference's DitheredFSQ (tools/gen_golden_fsq.py; cases
in tests/fsq_cases.py).  CPU: the simulator; `-m gpu`: the gfx950 library.

Token ids are integers and codes a finite set of fp32 values, so the comparison is bit for bit except where rounding is ill-conditioned:

  planted columns (x = 0: an exact tie for every even level count; +-20: tanh saturates; +-9): levels, codes and indices equal the
    fixture exactly.  roundf instead of rintf, a reciprocal multiply instead of the division, or an FMA'd code fail here.
  every other element: with li64 = (tanh(x.double()) + 1) * (L_d - 1) / 2, an element is NEAR A TIE if |li64 - floor(li64) - 0.5| < 1e-4.
    The band: fp32 spacing of li at its largest (L - 1 = 63) is 3.8e-6 and a few ulp of tanhf scaled by (L - 1) / 2 is of the same
    order; 1e-4 is about ten times their sum.  Away from a tie the level equals round(li64) and code and index equal the fixture bit
    for bit; near a tie the level is floor(li64) or ceil(li64).  Everywhere the code is exactly table[d][level] (the table torch computes
    on the host: arange(L) * half_l - 1) and the index is sum(level * basis) of the levels read back from the returned codes.
  cap: at most 1e-3 of a case's elements may be near a tie, else the test fails (the generator holds the fixtures to the same cap).

Decode: fsq_decode_tokens(indices) equals the codes bit for bit, no band; negative tokens and tokens >= codebook_size decode as the
reference decodes them (floor division, non-negative modulo); int32 tokens give what int64 tokens give.

Near-tie shares and the figures of the GPU runs: profiles/fsq/README.md."""
import pytest
import torch

import fsq_cases as cases
from golden_util import load_golden

IDS = list(range(len(cases.CASES)))
_GOLDEN = {}


def _golden(i):
    if i not in _GOLDEN:      # read once, shared, never written to
        _GOLDEN[i] = load_golden("fsq_" + cases.CASES[i])
    return _GOLDEN[i]


def _at_offset(x, offset):
    buf = torch.zeros(x.numel() + offset, dtype=x.dtype, device=x.device)
    buf[offset:] = x.reshape(-1)
    y = buf[offset:].view(x.shape)
    assert y.is_contiguous() and y.data_ptr() % 16 != 0
    return y


def _case(ops, i, device):
    g = _golden(i)
    shape, levels, q = cases.case(i)
    x = cases.inputs(i).to(device)
    if cases.CASES[i] == "offset":
        x = _at_offset(x, 1)
    codes, indices = ops.fsq_encode(x, levels, q)
    want_codes, want_indices = torch.from_numpy(g["codes"]), torch.from_numpy(g["indices"])
    cases.check_rule(cases.CASES[i], x, codes, indices, levels, q, want_codes, want_indices, cases.planted_columns(i))
    # decode: no band
    assert torch.equal(ops.fsq_decode_tokens(indices, levels), codes)
    tokens = want_indices.to(device)
    if cases.CASES[i] == "offset":
        tokens = _at_offset(tokens, 1)
    back = ops.fsq_decode_tokens(tokens, levels)
    assert back.dtype == torch.float32 and torch.equal(back, want_codes.to(device))
    if int(want_indices.max()) < 2 ** 31:
        assert torch.equal(ops.fsq_decode_tokens(tokens.to(torch.int32), levels), back)


def _odd_tokens(ops, device):
    i = cases.CASES.index(cases.ODD_CASE)
    levels = cases.case(i)[1]
    tokens = cases.odd_tokens().to(device)
    assert int(tokens.min()) == -2 ** 62 and int(tokens.max()) == 2 ** 40
    assert torch.equal(ops.fsq_decode_tokens(tokens, levels), torch.from_numpy(_golden(i)["odd_codes"]).to(device))
    small = tokens[:, :3, :1].contiguous()      # one codebook of -1, -361 and 360: just outside [0, 360) on either side
    assert torch.equal(ops.fsq_decode_tokens(small.to(torch.int32), levels), ops.fsq_decode_tokens(small, levels))


def _refusals(ops, device):
    x = torch.zeros(2, 8, 4, device=device)
    for bad in (x[:, :, :2], x.transpose(1, 2), x[0], x.double(), x.to(torch.bfloat16), torch.zeros(2, 0, 4, device=device)):
        with pytest.raises(ValueError, match="fsq_encode"):
            ops.fsq_encode(bad, [6, 5, 4, 3], 2)
    for levels, q in (([6, 5, 4, 3], 1), ([6, 5, 4], 2), ([6, 5, 4, 3], 3)):       # C != D * Q
        with pytest.raises(ValueError, match="fsq_encode"):
            ops.fsq_encode(x, levels, q)
    # L = 1, D = 17, sum L = 513, prod L > 2^63 - 1 ([64] * 11, whose sum passes 512 too, and [32] * 13, whose sum does not)
    for levels, c in (([1, 5], 2), ([3] * 17, 17), ([171, 171, 171], 3), ([64] * 11, 11), ([32] * 13, 13)):
        with pytest.raises(ValueError, match="fsq_encode"):
            ops.fsq_encode(torch.zeros(1, c, 4, device=device), levels, 1)
        with pytest.raises(ValueError, match="fsq_decode_tokens"):
            ops.fsq_decode_tokens(torch.zeros(1, 4, 1, dtype=torch.int64, device=device), levels)
    tok = torch.zeros(2, 4, 2, dtype=torch.int64, device=device)
    for bad in (tok[:, :, :1], tok.transpose(1, 2), tok[0], tok.float(), tok.bool(), torch.zeros(2, 0, 2, dtype=torch.int64, device=device)):
        with pytest.raises(ValueError, match="fsq_decode_tokens"):
            ops.fsq_decode_tokens(bad, [6, 5, 4, 3])
    # the C entry points refuse the same before any launch (null tensors: nothing could run)
    import ctypes
    null = ctypes.c_void_p(None)
    half = (ctypes.c_float * 17)(*([1.0] * 17))
    tab = (ctypes.c_float * 1024)()
    for levels, (b, c, t, d, q), msg in (([1, 5], (1, 2, 4, 2, 1), b">= 2"), ([3] * 17, (1, 17, 4, 17, 1), b"D <= 16"),
                                         ([171] * 3, (1, 3, 4, 3, 1), b"<= 512"), ([64] * 11, (1, 11, 4, 11, 1), b"<= 512"), ([32] * 13, (1, 13, 4, 13, 1), b"2^63"),
                                         ([5, 5], (1, 3, 4, 2, 1), b"D * Q"), ([5, 5], (1, 2, 0, 2, 1), b">= 1"), ([5, 5], (0, 2, 4, 2, 1), b">= 1")):
        lv = (ctypes.c_int * len(levels))(*levels)
        assert ops.lib.sat_fsq_encode(null, null, null, b, c, t, d, q, lv, half, tab, null) != 0
        assert msg in ops.lib.sat_last_error(), (levels, ops.lib.sat_last_error())
        assert ops.lib.sat_fsq_decode_tokens(null, null, b, c, t, d, q, lv, tab, null) != 0
        assert msg in ops.lib.sat_last_error(), (levels, ops.lib.sat_last_error())
    # at the limits nothing is refused
    for levels in ([3] * 16, [64] * 8, [512], [2] * 16, [30] * 12 + [15]):       # the last: 30^12 * 15 = 7.97e18 < 2^63 - 1
        ops._fsq_tables("fsq_encode", levels)


def _nan_stays_in_table(ops, device):
    x = torch.full((1, 4, 3), float("nan"), device=device)
    x[0, :, 1] = float("inf")
    x[0, :, 2] = -float("inf")
    codes, indices = ops.fsq_encode(x, [6, 5, 4, 3], 1)
    table = {round(-1.0 + 2.0 * r / (v - 1), 6) for v in (6, 5, 4, 3) for r in range(v)}
    assert all(round(float(v), 6) in table for v in codes.reshape(-1)) and bool(((indices >= 0) & (indices < 360)).all())
    assert torch.equal(codes[0, :, 1], torch.ones(4, device=device)) and torch.equal(codes[0, :, 2], -torch.ones(4, device=device))


@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_fsq_simulator(emu, i):
    _case(emu, i, "cpu")


def test_fsq_odd_tokens_simulator(emu):
    _odd_tokens(emu, "cpu")


def test_fsq_refusals_simulator(emu):
    _refusals(emu, "cpu")


def test_fsq_nan_simulator(emu):
    _nan_stays_in_table(emu, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_fsq_gpu(hip, i):
    _case(hip, i, "cuda")


@pytest.mark.gpu
def test_fsq_odd_tokens_gpu(hip):
    _odd_tokens(hip, "cuda")


@pytest.mark.gpu
def test_fsq_refusals_gpu(hip):
    _refusals(hip, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.fsq_encode(torch.zeros(1, 8, 4), [6, 5, 4, 3], 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.fsq_decode_tokens(torch.zeros(1, 4, 2, dtype=torch.int64), [6, 5, 4, 3])


@pytest.mark.gpu
def test_fsq_nan_gpu(hip):
    _nan_stays_in_table(hip, "cuda")


@pytest.mark.gpu
def test_fsq_graph_capture_gpu(hip):
    """one launch each, no workspace, tables in the kernel arguments: both ops replay from one captured HIP graph after the input changes"""
    i = cases.CASES.index("l6543x2")
    shape, levels, q = cases.case(i)
    x = cases.inputs(i).cuda()
    hip.fsq_decode_tokens(hip.fsq_encode(x, levels, q)[1], levels)      # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        codes, indices = hip.fsq_encode(x, levels, q)
        back = hip.fsq_decode_tokens(indices, levels)
    first = (codes.clone(), indices.clone())
    x.copy_(cases.inputs(i).cuda().flip(2) * 0.5 + 0.25)      # no column at 0: no planted ties in the replayed input
    g.replay()
    torch.cuda.synchronize()
    want_codes, want_indices = hip.fsq_encode(x, levels, q)
    assert not torch.equal(first[0], codes) and not torch.equal(first[1], indices)
    assert torch.equal(codes, want_codes) and torch.equal(indices, want_indices) and torch.equal(back, codes)
    cases.check_rule("graph replay", x, codes, indices, levels, q)


@pytest.mark.gpu
def test_fsq_past_65535_blocks_gpu(hip):
    """(1, 2, 2^24 + 3), [5, 5], one codebook: 65 537 blocks of 256 along blockIdx.x — past 65 535 — against the torch restatement of the
    eval quantiser on the device, under the same tie rule."""
    levels, q = [5, 5], 1
    t = 2 ** 24 + 3
    g = torch.Generator(device="cuda").manual_seed(1977)
    x = 1.5 * torch.randn(1, 2, t, device="cuda", generator=g)
    for col, v in enumerate(cases.PLANTED):
        x[:, :, col] = v
        x[:, :, t - 1 - col] = v       # and in the last block
    codes, indices = hip.fsq_encode(x, levels, q)
    want_codes, want_indices = cases.torch_fsq(x, levels, q)
    assert torch.equal(codes[:, :, t - 5:], want_codes[:, :, t - 5:]) and torch.equal(indices[:, t - 5:], want_indices[:, t - 5:])
    cases.check_rule("2^24 + 3", x, codes, indices, levels, q, want_codes, want_indices, len(cases.PLANTED))
    assert torch.equal(hip.fsq_decode_tokens(indices, levels), codes)
