"""Head dim 64 attention — the only attention that trains — held to float64 PER ROW, under every launch plan: the general forward (two
bf16 wave shapes and the two-plane fp32 mode), sat_attention_rowdot, the general backward, and the short-key forward / dQ / dK, dV kernels
of csrc/attention_cross.h.  Reference, yardstick, row scale and the assertion are tests/attention_fp64.py's (fp64_bounds.py's rule per
row: no bound here comes from running a kernel); `pytest -s` shows every FIGURE line.

What the per-tensor max-norm bound of tests/test_dit_kernels.py cannot see and this module does: a row that is small next to its
tensor's largest entry, the LSE (the backward recomputes P from it), and the launch plans no small shape reaches at the default CU
count — a wave's second block in the short-key forward / dQ (per_wg > 4), the dK / dV ring's third and later tiles, a ragged last
range, a range that crosses from one query head of a GQA group to the next, and the library's own choice of the 64-query forward.
Those run on the simulator with the CU count lowered (sat_emu_set_cu_count) and on the GPU at shapes that reach the same plans on a
full device; each asserts the plan before the values.  The last section pins that no forward kernel depends on the operand planes'
padding being zero (ops._head_planes(reuse=...) keeps planes by padded shape: a shorter sequence leaves the longer one's rows behind).

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import pytest
import torch

import attention_fp64 as A
import fp64_bounds as FB
from test_dit_kernels import SPIKES

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
# (B, H, Hkv, Nq, Nk): the tile edges, one past them, fewer than 32 / 64 keys, one key, one query, the short-key limit and one past it
EDGES = [(1, 2, 2, 64, 64), (2, 2, 2, 65, 65), (1, 4, 2, 130, 37), (1, 2, 1, 37, 200), (1, 4, 4, 1, 70), (1, 2, 2, 20, 20),
         (1, 2, 1, 70, 257), (1, 2, 2, 40, 256), (1, 2, 2, 33, 1), (1, 2, 2, 5, 17)]
GQA = [(2, 6, 2, 130, 130), (2, 6, 2, 70, 257), (2, 8, 2, 65, 96)]      # groups of 3 and 4 with B = 2
SCALED = [(1, 4, 2, 130, 37), (1, 2, 1, 70, 257)]                       # scale = 0.2
SPIKED = [((1, 2, 2, 130, 193), tuple(SPIKES)), ((1, 4, 2, 70, 200), tuple(SPIKES[:4]))]
PERMUTED = (2, 4, 2, 70, 130)

_prepared = {}


def _prep(case, dtype, seed, scale, spikes=(), permuted=False):
    """inputs, float64 reference, row scales and yardstick of one case: computed once, shared by every implementation, never written"""
    key = (case, dtype, seed, scale, spikes, permuted)
    if key not in _prepared:
        inp = A.make_inputs(case, dtype, seed, spikes, permuted)
        ref, srow = A.reference(*inp, scale)
        _prepared[key] = (inp, ref, srow, A.yardstick(*inp, scale))
    return _prepared[key]


def _launch(ops, dev, inp, scale, hkv, nk):
    q, k, v, do = (t.to(dev) for t in inp)
    o, lse, planes = ops.attention(q, k, v, scale, return_planes=True)
    dq, dk, dv = ops.attention_bwd(planes, o, do, lse, scale, hkv, nk)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _impls(ops, dtype, case):
    """(label, cross_kernels, attn_q64): bf16 with Nk <= 256 runs both implementations, the general bf16 forward both wave shapes"""
    if dtype == F32:
        return [("two-plane", True, None)]
    short = [("short-key", True, None)] if case[4] <= 256 else []
    return short + [("general-q32", False, False), ("general-q64", False, True)]


def _case(ops, dev, case, dtype, seed, scale=0.125, spikes=(), permuted=False, impls=None):
    b, h, hkv, nq, nk = case
    inp, ref, srow, yard = _prep(case, dtype, seed, scale, spikes, permuted)
    saved = ops.cross_kernels, ops.attn_q64
    outs = {}
    try:
        for label, cross, q64 in (impls or _impls(ops, dtype, case)):
            ops.cross_kernels, ops.attn_q64 = cross, q64
            assert ops.cross_ok(h, hkv, nk, 64, int(dtype == BF16)) == (dtype == BF16 and cross and nk <= 256)
            got = _launch(ops, dev, inp, scale, hkv, nk)
            leg = "gpu" if got["o"].is_cuda else "sim"
            fails = []
            for n in A.NAMES:
                assert got[n].dtype == (F32 if n == "lse" else dtype)
                try:
                    A.check_rows(f"attention {case} scale {scale:g} {label} {leg} {n}", got[n], ref[n], yard[n], srow[n])
                except AssertionError as e:      # every tensor's figures are printed before the first failure is raised
                    fails.append(str(e))
            assert not fails, "\n".join(fails)
            outs[label] = got
    finally:
        ops.cross_kernels, ops.attn_q64 = saved
    return outs


def _standard(ops, dev, which, i, dtype):
    if which == "edges":
        _case(ops, dev, EDGES[i], dtype, seed=100 + i)
    elif which == "gqa":
        _case(ops, dev, GQA[i], dtype, seed=120 + i)
    elif which == "scaled":
        _case(ops, dev, SCALED[i], dtype, seed=130 + i, scale=0.2)
    elif which == "spiked":
        _case(ops, dev, SPIKED[i][0], dtype, seed=140 + i, spikes=SPIKED[i][1])
    else:
        _case(ops, dev, PERMUTED, dtype, seed=150, permuted=True)


STANDARD = ([("edges", i) for i in range(len(EDGES))] + [("gqa", i) for i in range(len(GQA))] + [("scaled", i) for i in range(len(SCALED))]
            + [("spiked", i) for i in range(len(SPIKED))] + [("permuted", 0)])
_IDS = [f"{w}{i}" for w, i in STANDARD]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", STANDARD, ids=_IDS)
def test_attention_rows_sim(emu, which, dtype):
    _standard(emu, "cpu", *which, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", STANDARD, ids=_IDS)
def test_attention_rows_gpu(hip, which, dtype):
    _standard(hip, "cuda", *which, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# sat_attention_rowdot: D[b][h][q] = sum_d dO O, one wave per row, four rows per workgroup — B * H * Nq not multiples of 4
# ---------------------------------------------------------------------------------------------------------------------
def _rowdot_case(ops, dev, b, h, nq, dtype, seed):
    from stable_audio_tools_amd.ops import _ptr
    gen = torch.Generator().manual_seed(seed)
    do = torch.randn(b, nq, h * 64, generator=gen).to(dtype)
    o = torch.randn(b, nq, h * 64, generator=gen).to(dtype)
    prod64 = (FB.f64(do) * FB.f64(o)).view(b, nq, h, 64).permute(0, 2, 1, 3)
    f32 = (do.float() * o.float()).view(b, nq, h, 64).permute(0, 2, 1, 3).sum(-1)
    dod, od = do.to(dev), o.to(dev)
    dsum = torch.full((b, h, nq), float("nan"), dtype=F32, device=dev)
    ops._chk(ops.lib.sat_attention_rowdot(_ptr(dod), _ptr(od), _ptr(dsum), b, h, nq, int(dtype == BF16), ops._stream(dod)))
    FB.check(f"attention_rowdot ({b}, {h}, {nq}) {str(dtype)[6:]}-in", dsum, prod64.sum(-1), f32, FB.smax(prod64.abs().sum(-1)))


ROWDOT = [(1, 3, 37), (2, 5, 1), (1, 1, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_attention_rowdot_sim(emu, dtype):
    for i, (b, h, nq) in enumerate(ROWDOT):
        _rowdot_case(emu, "cpu", b, h, nq, dtype, seed=160 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_attention_rowdot_gpu(hip, dtype):
    for i, (b, h, nq) in enumerate(ROWDOT):
        _rowdot_case(hip, "cuda", b, h, nq, dtype, seed=160 + i)


# ---------------------------------------------------------------------------------------------------------------------
# launch plans: the simulator with the CU count lowered, the GPU at shapes that reach the same plans on a full device
# ---------------------------------------------------------------------------------------------------------------------
def _nsplit(ops, case):
    b, h, hkv, nq, nk = case
    nbytes = int(ops.lib.sat_attention_cross_bwd_ws(b, h, hkv, nq, nk))
    assert nbytes > 0 and nbytes % (2 * b * hkv * nk * 64 * 4) == 0
    return nbytes // (2 * b * hkv * nk * 64 * 4)


def _plans(ops, cus, case):
    """(forward / dQ per_wg, dK / dV tiles, tiles per range, ranges): the ranges from the library's workspace query, which must agree
    with the plan restated in attention_fp64"""
    b, h, hkv, nq, nk = case
    ntiles, per, nsplit = A.xatt_dkv_plan(cus, case)
    assert _nsplit(ops, case) == nsplit, "sat_xatt_dkv_plan changed: restate it in tests/attention_fp64.py"
    return A.xatt_per_wg(cus, b * hkv, (h // hkv) * -(-nq // 32)), ntiles, per, nsplit


SHORT = [("short-key", True, None)]


def _with_cus(emu, cus, fn):
    emu.lib.sat_emu_set_cu_count(cus)
    try:
        return fn()
    finally:
        emu.lib.sat_emu_set_cu_count(0)


def test_short_key_plan_head_crossing_ranges_sim(emu):
    """1 CU, a GQA group of 3 x 3 tiles: the dK / dV ranges are 5 and 4 tiles (ragged), each crosses a query-head boundary and walks the
    ring past its second tile.  (The forward's plan at this shape is per_wg = 4: ceil(15 / 4) wave blocks; per_wg = 8 is the next test's.)"""
    case = (1, 3, 1, 130, 130)

    def run():
        per_wg, ntiles, per, nsplit = _plans(emu, 1, case)
        nqt = -(-case[3] // 64)
        assert (ntiles, per, nsplit) == (9, 5, 2) and ntiles - per == 4, "not 9 tiles in ranges of 5 and 4: change the CU count or Nq"
        assert all(r * per // nqt != (min(ntiles, (r + 1) * per) - 1) // nqt for r in range(nsplit)), "a range stays inside one head"
        assert per_wg == 4
        _case(emu, "cpu", case, BF16, seed=170, impls=SHORT)
    _with_cus(emu, 1, run)


def test_short_key_plan_second_wave_block_sim(emu):
    """1 CU: forward and dQ workgroups of 8 wave blocks (every wave prefetches and runs a second block, the last workgroup is ragged and
    the blocks of a workgroup cross a head boundary); dK / dV in 2 ranges of 6 tiles (the ring's third to sixth tile)."""
    case = (1, 3, 1, 193, 70)

    def run():
        per_wg, ntiles, per, nsplit = _plans(emu, 1, case)
        assert per_wg == 8, "the forward / dQ workgroups no longer hold a second block per wave: raise Nq"
        assert (ntiles, per, nsplit) == (12, 6, 2) and per >= 3, "not 12 tiles in 2 ranges of 6: change the CU count or Nq"
        for dtype in DTYPES:
            _case(emu, "cpu", case, dtype, seed=171, impls=None if dtype == F32 else SHORT)
    _with_cus(emu, 1, run)


def test_short_key_plan_two_cus_sim(emu):
    case = (2, 4, 2, 100, 130)

    def run():
        print("FIGURE plan", case, "2 CUs: per_wg, tiles, per range, ranges =", _plans(emu, 2, case))
        for dtype in DTYPES:
            _case(emu, "cpu", case, dtype, seed=172, impls=None if dtype == F32 else SHORT)
    _with_cus(emu, 2, run)


def _auto_q64(ops, dev, case, seed):
    """attn_q64 = None must give the 64-query forward: bit-equal to the forced 64-query run, and not to the 32-query one"""
    auto, q64, q32 = (("auto", False, None),), (("q64", False, True),), (("q32", False, False),)
    o = {}
    for impl in (auto, q64, q32):
        o.update(_case(ops, dev, case, BF16, seed, impls=impl))
    for n in ("o", "lse"):
        assert torch.equal(o["auto"][n], o["q64"][n]), f"{n}: the library did not choose the 64-query forward"
    assert not torch.equal(o["auto"]["o"], o["q32"]["o"]), "the 32- and 64-query forwards are bit-equal here: the choice cannot be told"


def test_forward_q64_chosen_by_library_sim(emu):
    case = (1, 1, 1, 2049, 70)
    assert case[3] >= 2048 and -(-case[3] // 256) * case[1] * case[0] >= 2 * 1
    _with_cus(emu, 1, lambda: _auto_q64(emu, "cpu", case, seed=173))


@pytest.mark.gpu
def test_short_key_plans_gpu(hip):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = (16, 48, 16, 300, 130)
    per_wg, ntiles, per, nsplit = _plans(hip, cus, case)
    assert per_wg > 4, "the forward / dQ workgroups hold one block per wave on this device: raise B or Hkv"
    assert nsplit < ntiles and per >= 3, "one dK / dV tile per range on this device: raise B or Hkv"
    assert ntiles % per != 0, "no ragged last range on this device: change Nq"
    _case(hip, "cuda", case, BF16, seed=174, impls=SHORT)


@pytest.mark.gpu
def test_forward_q64_chosen_by_library_gpu(hip):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = (2, 32, 32, 2049, 257)
    assert case[3] >= 2048 and -(-case[3] // 256) * case[1] * case[0] >= 2 * cus, "the library no longer picks the 64-query forward: raise the head count"
    assert not hip.cross_ok(case[1], case[2], case[4], 64, 1)      # Nk = 257: the general backward
    _auto_q64(hip, "cuda", case, seed=175)


# ---------------------------------------------------------------------------------------------------------------------
# padding independence of the forward kernels (the no-grad path's persistent planes are zero-filled once, by PADDED shape)
# ---------------------------------------------------------------------------------------------------------------------
def _garbage(shape, gen):
    """finite bf16 garbage of magnitude ~1e4, both signs, as int16 bit patterns"""
    g = (torch.rand(shape, generator=gen) + 0.5) * 1.0e4 * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return g.bfloat16().view(torch.int16)


def _planes_pair(ops, dev, case, d, seed):
    b, h, hkv, nq, nk = case
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(b, hh, n, d, generator=gen).bfloat16().to(dev) for hh, n in ((h, nq), (hkv, nk), (hkv, nk)))
    clean = (ops.attn_planes(q)["rm"][0], ops.attn_planes(k)["rm"][0], ops.attn_planes(v, row_major=False, transposed=True)["tr"][0])
    npq, npk = clean[0].shape[2], clean[1].shape[2]
    assert npq > nq and npk > nk, "both lengths must be ragged"
    assert not bool(clean[0][:, :, nq:].any()) and not bool(clean[1][:, :, nk:].any()) and not bool(clean[2][:, :, :, nk:].any())
    dirty = tuple(t.clone() for t in clean)
    dirty[0][:, :, nq:] = _garbage((b, h, npq - nq, d), gen).to(dev)
    dirty[1][:, :, nk:] = _garbage((b, hkv, npk - nk, d), gen).to(dev)
    dirty[2][:, :, :, nk:] = _garbage((b, hkv, d, npk - nk), gen).to(dev)
    return clean, dirty


def _padding_case(ops, dev, case, d, seed, switches):
    nq, nk = case[3], case[4]
    clean, dirty = _planes_pair(ops, dev, case, d, seed)
    saved = ops.cross_kernels, ops.attn_q64
    try:
        for label, cross, q64 in switches:
            ops.cross_kernels, ops.attn_q64 = cross, q64
            assert ops.cross_ok(case[1], case[2], nk, d, 1) == (label == "short-key")
            want = ops.attention_planes(*clean, nq, nk, d ** -0.5)
            got = ops.attention_planes(*dirty, nq, nk, d ** -0.5)
            assert bool(torch.isfinite(want.float()).all()) and want.shape == (case[0], nq, case[1] * d)
            assert torch.equal(got, want), f"{label} forward at D = {d}, {case}: the output depends on the planes' padding"
    finally:
        ops.cross_kernels, ops.attn_q64 = saved


GENERAL = [("general-q32", False, False), ("general-q64", False, True)]
PAD_CASE_128 = (1, 2, 2, 70, 130)


def _padding_hd64(ops, dev):
    _padding_case(ops, dev, (1, 4, 2, 70, 100), 64, 180, SHORT + GENERAL)
    _padding_case(ops, dev, (1, 2, 2, 70, 300), 64, 181, GENERAL)


def test_forward_ignores_plane_padding_sim(emu):
    _padding_hd64(emu, "cpu")
    _padding_case(emu, "cpu", PAD_CASE_128, 128, 182, [("hd128-4-waves", True, False)])
    # 8 waves per workgroup once ceil(Nq / 256) * H * B reaches the CU count
    _with_cus(emu, 2, lambda: _padding_case(emu, "cpu", PAD_CASE_128, 128, 182, [("hd128-8-waves", True, None)]))


@pytest.mark.gpu
def test_forward_ignores_plane_padding_gpu(hip):
    _padding_hd64(hip, "cuda")
    _padding_case(hip, "cuda", PAD_CASE_128, 128, 182, [("hd128-4-waves", True, False)])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wide = (4, 64, 64, 70, 130)
    assert -(-wide[3] // 256) * wide[1] * wide[0] >= cus, "this shape no longer reaches the 8-wave kernel: raise the head count"
    _padding_case(hip, "cuda", wide, 128, 183, [("hd128-8-waves", True, None)])


def _module_reuse(ops_now, dev, make_fresh):
    """Attention in bf16 under no_grad: a shorter sequence after a longer one of the same padded length reads planes whose tail rows the
    longer call wrote; the result must be bit-equal to the same call on an ops object with an empty workspace cache."""
    from stable_audio_tools_amd import ops as ops_mod
    from stable_audio_tools_amd.transformer import Attention
    gen = torch.Generator().manual_seed(190)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).bfloat16().to(dev)
    self_attn = Attention(128, dim_heads=64, zero_init_output=False).to(dev).bfloat16()
    cross_attn = Attention(128, dim_heads=64, dim_context=64, zero_init_output=False).to(dev).bfloat16()
    x100, x70, xq = rnd(2, 100, 128), rnd(2, 70, 128), rnd(2, 50, 128)
    # context lengths: 130 then 100 (another padded length: new planes), 190 then 130 (the same padded length: the 190's rows stay)
    c130, c100, c190 = rnd(2, 130, 64), rnd(2, 100, 64), rnd(2, 190, 64)
    with torch.no_grad():
        self_attn(x100)
        y70 = self_attn(x70)
        cross_attn(xq, context=c130)
        z100 = cross_attn(xq, context=c100)
        cross_attn(xq, context=c190)
        z130 = cross_attn(xq, context=c130.clone())
        assert any(k[0] == "self" for k in ops_now._planes), "the no-grad path no longer keeps its planes in the workspace cache"
        current = ops_mod.get_ops
        fresh = make_fresh()
        assert not fresh._planes
        ops_mod.get_ops = lambda: fresh
        try:
            for a in (self_attn, cross_attn):
                a.__dict__.pop("_kv_ctx", None)
            y70_f = self_attn(x70)
            z100_f = cross_attn(xq, context=c100.clone())
            z130_f = cross_attn(xq, context=c130.clone())
        finally:
            ops_mod.get_ops = current
    for name, a, f in (("self 100 -> 70", y70, y70_f), ("cross 130 -> 100", z100, z100_f), ("cross 190 -> 130", z130, z130_f)):
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0.0
        assert torch.equal(a, f), f"{name}: the result depends on what an earlier, longer call left in the cached planes"


def test_no_grad_plane_reuse_sim(emu_modules):
    from stable_audio_tools_amd.ops import SatOps
    _module_reuse(emu_modules, "cpu", lambda: SatOps(emu_modules.lib))


@pytest.mark.gpu
def test_no_grad_plane_reuse_gpu(hip):
    from stable_audio_tools_amd.ops import SatOps
    _module_reuse(hip, "cuda", lambda: SatOps(hip.lib))
