"""Sliding-window self-attention forward (sat_attention_fwd_window: the WIN instantiations of sat_attn_fwd_kernel at head dims 64 and
128, fp32 two-plane and bf16) held to float64 per row.  Reference, yardstick and row scales are tests/attention_window_fp64.py's, the
assertion is attention_fp64.check_rows: every row within fp64_bounds.FACTOR x the yardstick's worst row — the bar of
tests/test_attention_fp64.py, nothing here comes from running a kernel; `pytest -s` shows every FIGURE line.

What the table reaches (128-query workgroups of four 32-query waves, 64-key tiles): bands that end on, one before and one after a tile
edge; a ragged last tile that is also a band edge, with its first 32 keys only and with both halves; a last tile of one key; workgroups
whose first staged tile is not tile 0, whose waves meet their first tile at different places, and rows that see no key in their wave's
first tile ((0, 0): queries 40..71 on keys 0..63); a GQA group; permuted storage.  Then: spikes inside and outside the band, the closed
form of (0, 0), bit-equality with the dense launch when the window hides nothing, the launch plans a windowed call must not take
(short-key, 64 queries per wave, 8 waves), the refusals, and on the GPU two sizes with several workgroups per head.

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import pytest
import torch

import attention_fp64 as A
import attention_window_fp64 as W

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
DIMS = [64, 128]

EDGE_WINDOWS = [(0, 0), (1, 0), (0, 1), (5, -1), (-1, 5)]
# ((B, H, Hkv, N), window, permuted)
TABLE = ([(c, w, False) for c in ((1, 2, 2, 64), (2, 2, 2, 65), (1, 2, 2, 20)) for w in EDGE_WINDOWS]
         + [((1, 2, 2, 130), (31, 32), False),        # ragged edge tile, its first 32 keys only (NKB = 1)
            ((1, 2, 2, 200), (31, 32), False),        # ragged edge tile, both halves (NKB = 2)
            ((1, 2, 2, 193), (63, 64), False), ((1, 2, 2, 193), (64, 0), False), ((1, 2, 2, 193), (0, 64), False),      # last tile of one key
            ((1, 4, 2, 300), (31, 32), False), ((1, 4, 2, 300), (0, 0), False),      # klo > 0; waves with different first tiles; GQA
            ((2, 2, 1, 130), (7, 9), True)])          # (B, N, H, D) storage
_IDS = [f"{'x'.join(map(str, c))}-w{w[0]}_{w[1]}" + ("-perm" if p else "") for c, w, p in TABLE]

_prepared = {}


def _prep(case, d, dtype, seed, window, spikes=(), permuted=False):
    """inputs, float64 reference, row scales and yardstick of one case: computed once, shared, never written"""
    key = (case, d, dtype, seed, window, spikes, permuted)
    if key not in _prepared:
        inp = W.make_inputs(case, d, dtype, seed, spikes, permuted)
        scale = d ** -0.5
        ref, srow = W.reference(*inp, scale, window)
        _prepared[key] = (inp, ref, srow, W.yardstick(*inp, scale, window))
    return _prepared[key]


def _run(ops, dev, inp, d, window):
    q, k, v = (t.to(dev) for t in inp)
    o, lse = ops.attention(q, k, v, d ** -0.5, need_lse=True, window=window)
    assert o.dtype == inp[0].dtype and lse.dtype == F32
    return {"o": o, "lse": lse}


def _check(label, got, ref, yard, srow):
    fails = []
    for n in W.NAMES:
        try:
            A.check_rows(f"{label} {n}", got[n], ref[n], yard[n], srow[n])
        except AssertionError as e:      # every tensor's figures are printed before the first failure is raised
            fails.append(str(e))
    assert not fails, "\n".join(fails)


def _case(ops, dev, case, d, dtype, seed, window, spikes=(), permuted=False):
    inp, ref, srow, yard = _prep(case, d, dtype, seed, window, spikes, permuted)
    got = _run(ops, dev, inp, d, window)
    leg = "gpu" if got["o"].is_cuda else "sim"
    _check(f"window {case} D {d} {window} {leg}", got, ref, yard, srow)
    return got


def _table(ops, dev, i, d, dtype):
    case, window, permuted = TABLE[i]
    _case(ops, dev, case, d, dtype, 300 + i, window, permuted=permuted)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("i", range(len(TABLE)), ids=_IDS)
def test_window_rows_sim(emu, i, d, dtype):
    _table(emu, "cpu", i, d, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("i", range(len(TABLE)), ids=_IDS)
def test_window_rows_gpu(hip, i, d, dtype):
    _table(hip, "cuda", i, d, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# spikes: k[j] = gain * q[i].  Three inside the band of their query; (100, 0) is outside query 100's band (keys 80..192) and inside
# that of queries 0..20: query 100 must not feel it — not in its max, not in its sums, not through a wave-wide rescale
# ---------------------------------------------------------------------------------------------------------------------
SPIKE_CASE, SPIKE_WINDOW = (1, 2, 2, 193), (20, 150)
SPIKES_IN = ((5, 150, 6.0), (41, 70, 3.0), (64, 192, 8.0))
SPIKE_OUT = (100, 0, 8.0)


def _spiked(ops, dev, d, dtype):
    vis = W.band(SPIKE_CASE[3], SPIKE_WINDOW)
    assert all(bool(vis[i, j]) for i, j, _ in SPIKES_IN) and not bool(vis[SPIKE_OUT[0], SPIKE_OUT[1]]) and bool(vis[:21, 0].all())
    got = _case(ops, dev, SPIKE_CASE, d, dtype, 340, SPIKE_WINDOW, spikes=SPIKES_IN + (SPIKE_OUT,))
    # the same inputs without the out-of-band spike: the rows that cannot see key 0 (queries 21 and up) are bit-identical
    calm = _run(ops, dev, W.make_inputs(SPIKE_CASE, d, dtype, 340, SPIKES_IN), d, SPIKE_WINDOW)
    assert torch.equal(got["o"][:, 21:], calm["o"][:, 21:]) and torch.equal(got["lse"][:, :, 21:], calm["lse"][:, :, 21:])
    assert not torch.equal(got["o"][:, :21], calm["o"][:, :21]), "key 0 moves nothing: the spike is not in the inputs"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_spiked_sim(emu, d, dtype):
    _spiked(emu, "cpu", d, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_spiked_gpu(hip, d, dtype):
    _spiked(hip, "cuda", d, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# closed form: under (0, 0) a query sees itself alone — o = v (bf16: P = 1 and l = 1 exactly, so bit for bit; fp32: v as hi + lo,
# 2^-17 each way), lse = scale * q . k
# ---------------------------------------------------------------------------------------------------------------------
def _closed_form(ops, dev, d, dtype):
    for case in ((1, 2, 2, 130), (2, 4, 2, 70)):
        got = _case(ops, dev, case, d, dtype, 350, (0, 0))
        b, h, hkv, n = case
        v = _prep(case, d, dtype, 350, (0, 0))[0][2]
        want = v.repeat_interleave(h // hkv, 1).permute(0, 2, 1, 3).reshape(b, n, h * d)
        o = got["o"].cpu()
        if dtype == BF16:
            assert torch.equal(o, want)
        else:
            assert bool(((o - want).abs() <= 2.0 ** -16 * want.abs()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_closed_form_sim(emu, d, dtype):
    _closed_form(emu, "cpu", d, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_closed_form_gpu(hip, d, dtype):
    _closed_form(hip, "cuda", d, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# a window that hides nothing is the dense launch, bit for bit — through ops and at the C entry
# ---------------------------------------------------------------------------------------------------------------------
def _c_entry(ops, dev, inp, d, dt_code, window=None, nk=None):
    """sat_attention_fwd (window None) or sat_attention_fwd_window on planes prepared from `inp`: (rc, o, lse)"""
    from stable_audio_tools_amd.ops import _ptr
    q, k, v = (t.to(dev) for t in inp)
    b, h, n, _ = q.shape
    hk = k.shape[1]
    nk = n if nk is None else nk
    qp, kp, vp = ops.attn_planes(q), ops.attn_planes(k), ops.attn_planes(v, row_major=False, transposed=True)
    o = torch.zeros(b, n, h * d, dtype=q.dtype, device=dev)
    lse = torch.zeros(b, h, n, dtype=F32, device=dev)
    args = (_ptr(qp["rm"][0]), _ptr(qp["rm"][1]), _ptr(kp["rm"][0]), _ptr(kp["rm"][1]), _ptr(vp["tr"][0]), _ptr(vp["tr"][1]), _ptr(o),
            _ptr(lse), b, h, hk, n, nk, qp["np"], kp["np"], d, d ** -0.5, dt_code, ops._stream(q))
    rc = ops.lib.sat_attention_fwd(*args) if window is None else ops.lib.sat_attention_fwd_window(*args, *window)
    return rc, o, lse


def _dense_equivalence(ops, dev, d, dtype):
    for case in ((1, 2, 2, 130), (1, 4, 2, 300)):
        n = case[3]
        inp = W.make_inputs(case, d, dtype, 360)
        q, k, v = (t.to(dev) for t in inp)
        dense = ops.attention(q, k, v, d ** -0.5, need_lse=True)
        for window in (None, (-1, -1), (n - 1, n - 1), (n + 5, -1)):
            got = ops.attention(q, k, v, d ** -0.5, need_lse=True, window=window)
            assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1]), window
        code = int(dtype == BF16)
        rc, o, lse = _c_entry(ops, dev, inp, d, code)
        assert rc == 0, ops.lib.sat_last_error()
        for window in ((-1, -1), (n - 1, n + 5), (-1, n - 1)):
            rc, ow, lw = _c_entry(ops, dev, inp, d, code, window)
            assert rc == 0, ops.lib.sat_last_error()
            assert torch.equal(ow, o) and torch.equal(lw, lse), window


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_dense_equivalence_sim(emu, d, dtype):
    _dense_equivalence(emu, "cpu", d, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_window_dense_equivalence_gpu(hip, d, dtype):
    _dense_equivalence(hip, "cuda", d, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# launch plans a windowed call must not take
# ---------------------------------------------------------------------------------------------------------------------
def _not_short_key(ops, dev):
    """N = 130 <= 256 in bf16: the dense call takes the short-key kernel, the windowed one must not (it has no window)"""
    case, window = (1, 4, 2, 130), (7, 9)
    assert ops.cross_kernels and ops.cross_ok(case[1], case[2], case[3], 64, 1)
    got = _case(ops, dev, case, 64, BF16, 370, window)
    inp, ref, srow, yard = _prep(case, 64, BF16, 370, window)
    q, k, v = (t.to(dev) for t in inp)
    dense = ops.attention(q, k, v, 64 ** -0.5, need_lse=True)
    with pytest.raises(AssertionError):      # what a short-key (dense) launch would have returned is not the windowed result
        A.check_rows("dense short-key against the windowed reference o", dense[0], ref["o"], yard["o"], srow["o"])
    pl = {n: ops.attn_planes(t, row_major=rm, transposed=not rm) for n, t, rm in (("q", q, True), ("k", k, True), ("v", v, False))}
    o = ops.attention_planes(pl["q"]["rm"][0], pl["k"]["rm"][0], pl["v"]["tr"][0], case[3], case[3], 64 ** -0.5, window=window)
    assert torch.equal(o, got["o"])


def _q64_ignored(ops, dev):
    saved = ops.attn_q64
    try:
        ops.attn_q64 = True
        got = _case(ops, dev, (1, 2, 2, 300), 64, BF16, 371, (31, 32))
        ops.attn_q64 = False
        again = _run(ops, dev, _prep((1, 2, 2, 300), 64, BF16, 371, (31, 32))[0], 64, (31, 32))
    finally:
        ops.attn_q64 = saved
    assert torch.equal(got["o"], again["o"]) and torch.equal(got["lse"], again["lse"])


def test_window_never_short_key_sim(emu):
    _not_short_key(emu, "cpu")


def test_window_ignores_q64_sim(emu):
    _q64_ignored(emu, "cpu")


def test_window_hd128_four_waves_sim(emu):
    """2 CUs: the dense bf16 head dim 128 call at this shape takes the 8-wave workgroup; the windowed call stays on 4 waves and passes"""
    case = (1, 2, 2, 300)
    assert -(-case[3] // 256) * case[1] * case[0] >= 2
    emu.lib.sat_emu_set_cu_count(2)
    try:
        _case(emu, "cpu", case, 128, BF16, 372, (31, 32))
    finally:
        emu.lib.sat_emu_set_cu_count(0)


@pytest.mark.gpu
def test_window_never_short_key_gpu(hip):
    _not_short_key(hip, "cuda")


@pytest.mark.gpu
def test_window_ignores_q64_gpu(hip):
    _q64_ignored(hip, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refusals(ops, dev):
    inp = W.make_inputs((1, 2, 2, 70), 64, BF16, 380)
    for kwargs, text in ((dict(window=(3, 3), nk=69), b"self-attention only"), (dict(window=(-2, 3)), b">= -1"),
                         (dict(window=(3, -2)), b">= -1"), (dict(window=(3, 3), dt_code=3), b"dtype 3")):
        rc, _, _ = _c_entry(ops, dev, inp, 64, kwargs.pop("dt_code", 1), **kwargs)
        assert rc != 0 and text in ops.lib.sat_last_error(), (kwargs, ops.lib.sat_last_error())
    q, k, v = (t.to(dev) for t in inp)
    with pytest.raises(NotImplementedError, match="inference-only"):
        ops.attention(q, k, v, 0.125, return_planes=True, window=(3, 3))
    for bad in ((-2, 3), (3, -2), (3,), (1.5, 2), "ab"):
        with pytest.raises(ValueError):
            ops.attention(q, k, v, 0.125, window=bad)
    with pytest.raises(NotImplementedError, match="self-attention"):
        ops.attention(q, k[:, :, :50], v[:, :, :50], 0.125, window=(3, 3))


def test_window_refusals_sim(emu):
    _refusals(emu, "cpu")


@pytest.mark.gpu
def test_window_refusals_gpu(hip):
    _refusals(hip, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# GPU only: several workgroups per head, interior tiles between the edges, the long-context row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("case", [(2, 8, 8, 1025), (1, 4, 4, 6145)], ids=["n1025", "n6145"])
def test_window_long_gpu(hip, case, d, dtype):
    _case(hip, "cuda", case, d, dtype, 390, (63, 64))
