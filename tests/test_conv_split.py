"""Split over input-channel chunks of the bf16x3 conv kernels (csrc/conv1d_bf16x3.hip, conv1d_bf16x3_k7q.h; SatOps.conv_split): n workgroups per
tile run 1 / n of the K loop each and store their raw accumulators, a finish launch of the same kernel sums the slabs in index order and runs the
ordinary epilogue.  The smallest shapes at which each mechanism can go wrong: 16 chunks, B = 2, a ragged last time tile, a half-empty channel
tile; forced splits 2 (8 / 8 chunks), 3 (6 / 6 / 4) and 16 (one chunk per split).

  * integer-valued operands, no SnakeBeta: every partial sum is exact in fp32, so the split result is BIT-equal to the unsplit kernel's and to
    the float64 formula;
  * random operands: relative L2 against float64 (tests/conv_fp64.py's references) no more than twice the unsplit kernel's own figure on the same
    operands, for the output and for both SnakeBeta gradient sums of a data-gradient call — both figures are printed (`pytest -s`);
  * a second run of the same split gives the same bits;
  * the rule (sat_conv_split_rule / sat_conv_bf16x3_split at 256 CUs) on the launches of the flagship step, and the refusal of a forced count a
    launch cannot have.

CPU: the simulator build of the same sources; `-m gpu`: the gfx950 library."""
import ctypes

import pytest
import torch

import conv_fp64 as C
from fp64_bounds import f64

SPLITS = (2, 3, 16)


class Cfg:
    """One conv call.  stride > 1: the strided plan <8, 4, true> (k = 2 stride); k = 3: plan <8, 2, false>; k = 7: the planes kernel, weights
    packed in data-gradient mode.  dsn: the data-gradient epilogue (dx and the two parameter sums), else SnakeBeta on the input + bias."""

    def __init__(self, name, cin, cout, tout, k, stride=1, dsn=False, q=False):
        self.name, self.b, self.cin, self.cout, self.tout, self.k, self.stride, self.dsn, self.q = name, 2, cin, cout, tout, k, stride, dsn, q
        self.pad = (stride + 1) // 2 if stride > 1 else (k - 1) // 2
        self.tin = (tout - 1) * stride + k - 2 * self.pad
        self.geom = C.Geom("conv", k, stride, 1, self.pad, tout)
        self.kind = 2 if q else 0
        self.nchunks = cin * stride // (16 if k in (3, 7) else 32)

    def __repr__(self):
        return self.name


CONFIGS = [Cfg(f"s8k16-64to{co}-{m}", 64, co, 132, 16, 8, dsn=(m == "dgrad")) for co in (64, 128) for m in ("fwd", "dgrad")]
CONFIGS += [Cfg(f"s2k4-256to64-{m}", 256, 64, 132, 4, 2, dsn=(m == "dgrad")) for m in ("fwd", "dgrad")]
CONFIGS += [Cfg(f"k3-256to{co}-fwd", 256, co, 136, 3) for co in (32, 128)]
CONFIGS += [Cfg("k7q-256to64-dgrad", 256, 64, 260, 7, dsn=True, q=True)]
assert all(c.nchunks == 16 for c in CONFIGS)

_cache = {}


def _data(cfg, ints):
    """CPU operands of one config, made once and never written.  w: the conv's own (Cout, Cin, K) weight."""
    key = ("data", cfg.name, ints)
    if key not in _cache:
        gen = torch.Generator().manual_seed(1000 + CONFIGS.index(cfg))
        if ints:
            ri = lambda lim, *shape: torch.randint(-lim, lim + 1, shape, generator=gen).float()
            _cache[key] = {"x": ri(4, cfg.b, cfg.cin, cfg.tin), "w": ri(2, cfg.cout, cfg.cin, cfg.k), "bias": ri(8, cfg.cout)}
        else:
            rn = lambda *shape, s=1.0: torch.randn(*shape, generator=gen) * s
            _cache[key] = {"x": rn(cfg.b, cfg.cin, cfg.tin), "w": rn(cfg.cout, cfg.cin, cfg.k, s=.2), "bias": rn(cfg.cout), "la": rn(cfg.cin, s=.3),
                           "lb": rn(cfg.cin, s=.3), "x2": rn(cfg.b, cfg.cout, cfg.tout), "la2": rn(cfg.cout, s=.3), "lb2": rn(cfg.cout, s=.3)}
    return _cache[key]


def _ref(cfg, ints):
    """float64, from the fp32 operands: (y,) or (dx, d log-alpha2, d log-beta2)"""
    key = ("ref", cfg.name, ints)
    if key not in _cache:
        d = _data(cfg, ints)
        x64 = f64(d["x"])
        if ints:
            _cache[key] = (cfg.geom.torch(x64, f64(d["w"])) + f64(d["bias"])[None, :, None],)
        elif cfg.dsn:
            acc = cfg.geom.torch(x64, f64(d["w"]))
            leaves = [f64(d[n]).clone().requires_grad_(True) for n in ("x2", "la2", "lb2")]
            _cache[key] = tuple(torch.autograd.grad(C._snake64(*leaves)[0], leaves, acc))
        else:
            _cache[key] = (cfg.geom.torch(C._snake64(x64, d["la"], d["lb"])[0], f64(d["w"])) + f64(d["bias"])[None, :, None],)
    return _cache[key]


def _weights(ops, dev, cfg, ints):
    w = _data(cfg, ints)["w"]
    if cfg.q:            # data-gradient mode: the planes are packed from the FORWARD conv's weight (Cin, Cout, K), taps flipped
        return ops.pack_bf16x3(w.flip(2).transpose(0, 1).contiguous().to(dev), 1, 1, q=True)
    return ops.pack_bf16x3(w.to(dev), 0, cfg.stride)


def _run(ops, dev, cfg, ints, split):
    """one call with ops.conv_split = split (0: the unsplit kernel) -> CPU tensors (y,) or (dx, da, db)"""
    d = {k: v.to(dev) for k, v in _data(cfg, ints).items()}
    kw = {"tout": cfg.tout}
    if ints:
        kw["bias"] = d["bias"]
    elif cfg.dsn:
        kw["dsnake"] = (d["x2"], d["la2"], d["lb2"])
    else:
        kw.update(bias=d["bias"], snake=(d["la"], d["lb"]))
    keep = ops.conv_split
    ops.conv_split = split
    try:
        got = ops.conv1d_bf16x3(d["x"], _weights(ops, dev, cfg, ints), cfg.cout, cfg.k, cfg.stride, 1, cfg.pad, **kw)
    finally:
        ops.conv_split = keep
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(_ref(cfg, ints))
    return tuple(g.detach().cpu().clone() for g in got)


def _unsplit(ops, dev, cfg, ints):
    key = ("unsplit", dev, cfg.name, ints)
    if key not in _cache:
        _cache[key] = _run(ops, dev, cfg, ints, 0)
    return _cache[key]


def _rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def _split_case(ops, dev, cfg, n):
    leg = "sim" if ops.simulator else "gpu"
    need = ctypes.c_longlong(0)
    shape = (cfg.kind, cfg.b, cfg.cin, cfg.cout, cfg.tout, cfg.k, cfg.stride, 1, cfg.pad)
    assert ops.lib.sat_conv_bf16x3_split(*shape, n, 0, ctypes.byref(need)) == n and need.value > 0       # the forced split is taken
    # integer-valued operands, no SnakeBeta: exact partial sums -> the same bits as the unsplit kernel and as float64
    got = _run(ops, dev, cfg, True, n)[0]
    assert torch.equal(got, _unsplit(ops, dev, cfg, True)[0]), f"{cfg} split {n}: integer result differs from the unsplit kernel's"
    assert torch.equal(got.double(), _ref(cfg, True)[0]), f"{cfg} split {n}: integer result differs from float64"
    # random operands: no worse than twice the unsplit kernel against float64; the same bits from a second run
    got = _run(ops, dev, cfg, False, n)
    again = _run(ops, dev, cfg, False, n)
    fails = []
    for name, g, g2, u, r in zip(("dx", "dla", "dlb") if cfg.dsn else ("y",), got, again, _unsplit(ops, dev, cfg, False), _ref(cfg, False)):
        e_split, e_unsplit = _rel_l2(g, r), _rel_l2(u, r)
        print(f"FIGURE {cfg} {name} {leg}: rel L2 vs float64 split {n} {e_split:.3e}  unsplit {e_unsplit:.3e}  ratio {e_split / e_unsplit:.3f}")
        if not e_split <= 2.0 * e_unsplit:
            fails.append(f"{cfg} {name}: split {n} {e_split:.3e} > 2 x unsplit {e_unsplit:.3e}")
        if not torch.equal(g, g2):
            fails.append(f"{cfg} {name}: two runs of split {n} differ")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", SPLITS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_split_sim(emu, cfg, n):
    _split_case(emu, "cpu", cfg, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SPLITS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=repr)
def test_split_gpu(hip, cfg, n):
    _split_case(hip, "cuda", cfg, n)


GRAPH_CONFIGS = [c for c in CONFIGS if c.name in ("s8k16-64to128-dgrad", "k3-256to32-fwd", "k7q-256to64-dgrad")]      # one per kernel path


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GRAPH_CONFIGS, ids=repr)
def test_split_graph_replay_equals_eager_gpu(hip, cfg):
    """split and finish launch captured into a HIP graph (the slabs come from the workspace cache of the capture's stream and keep their
    address): three replays on changing inputs, each bit-equal to the eager call on the same input"""
    d = {k: v.cuda() for k, v in _data(cfg, False).items()}
    wp = _weights(hip, "cuda", cfg, False)
    static = d["x"].clone()
    kw = {"tout": cfg.tout, "dsnake": (d["x2"], d["la2"], d["lb2"])} if cfg.dsn else {"tout": cfg.tout, "bias": d["bias"], "snake": (d["la"], d["lb"])}
    call = lambda: hip.conv1d_bf16x3(static, wp, cfg.cout, cfg.k, cfg.stride, 1, cfg.pad, **kw)
    keep = hip.conv_split
    hip.conv_split = 3
    try:
        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = call()
        outs = outs if isinstance(outs, tuple) else (outs,)
        for r in range(3):
            static.copy_(d["x"] * (1.0 + 0.25 * r))
            graph.replay()
            got = [o.clone() for o in outs]
            want = call()
            want = want if isinstance(want, tuple) else (want,)
            for g, w in zip(got, want):
                assert torch.equal(g, w), (cfg, r)
    finally:
        hip.conv_split = keep


# ---------------------------------------------------------------------------------------------------------------------
# the rule (host code only: the simulator library answers as the gfx950 one does)
# ---------------------------------------------------------------------------------------------------------------------
def _rule(lib, kind, cin, cout, tout, k, stride, pad, cus=256):
    return lib.sat_conv_bf16x3_split(kind, 1, cin, cout, tout, k, stride, 1, pad, -1, cus, None)


def test_rule_on_the_flagship_step(emu):
    """batch 1, 2097152 samples, channels 128 x (1, 2, 4, 8, 16), strides (2, 4, 4, 8, 8): the three launch shapes at the bottom of the U split
    4 / 16 / 16 ways at 256 CUs, every other conv launch of the step is left alone"""
    lib = emu.lib
    assert _rule(lib, 0, 1024, 2048, 1024, 16, 8, 4) == 4        # grid (8, 16, 1) of <8, 4, true>, 256 chunks: the last down conv, the first up conv's data-gradient
    assert _rule(lib, 0, 2048, 128, 1024, 3, 1, 1) == 16         # grid (8, 1, 1) of <8, 2, false>, 128 chunks: the encoder's final conv
    assert _rule(lib, 2, 2048, 64, 1024, 7, 1, 3) == 16          # grid (4, 1, 1) of the planes kernel, 128 chunks: the decoder's first conv's data-gradient
    levels = ((128, 128, 2, 1048576), (128, 256, 4, 262144), (256, 512, 4, 65536), (512, 1024, 8, 8192))      # (cin, cout, stride, tout) of the other down convs
    for cin, cout, s, tout in levels:
        assert _rule(lib, 0, cin, cout, tout, 2 * s, s, (s + 1) // 2) == 1, (cin, cout, s)                    # strided plan, e.g. grid (64, 8, 1) with 128 chunks
        assert _rule(lib, 1, cout, cin, tout * s, 2 * s, s, (s + 1) // 2) == 1, (cout, cin, s)                # the up convs / transposed plan, e.g. grid (9, 64, 1)
    assert _rule(lib, 1, 2048, 1024, 8192, 16, 8, 4) == 1
    for c, t in ((128, 2097152), (128, 1048576), (256, 262144), (512, 65536), (1024, 8192)):
        assert _rule(lib, 0, c, c, t, 1, 1, 0) == 1, (c, t)                                                   # the k = 1 plan, e.g. grid (64, 8, 1)
        assert _rule(lib, 2, c, c, t, 7, 1, 3) == 1, (c, t)                                                   # the ResidualUnits' k7 convs
    assert _rule(lib, 0, 128, 2048, 1024, 3, 1, 1) == 1          # grid (8, 16, 1) of <8, 2, false> with 8 chunks
    assert _rule(lib, 2, 64, 2048, 1024, 7, 1, 3) == 1           # grid (64, 1, 1) of the planes kernel with 4 chunks
    assert _rule(lib, 0, 2048, 128, 1024, 7, 1, 3) == 1          # the direct k7 kernel does not split


def test_rule_keeps_eight_chunks_per_split(emu):
    lib = emu.lib
    for tiles, nchunks, resident, cus in ((8, 128, 2, 256), (4, 128, 1, 256), (128, 256, 2, 256), (1, 1000, 3, 304), (3, 17, 2, 256), (1, 520, 3, 256)):
        n = lib.sat_conv_split_rule(tiles, nchunks, resident, cus)
        cps = -(-nchunks // n)
        assert n >= 2 and n * tiles <= cus * resident and nchunks // n >= 8 and (n - 1) * cps < nchunks, (tiles, nchunks, n)
    assert lib.sat_conv_split_rule(8, 15, 2, 256) == 1           # two splits would get 7 and 8 chunks
    assert lib.sat_conv_split_rule(8, 16, 2, 256) == 2
    assert lib.sat_conv_split_rule(128, 256, 2, 256) == 4 and lib.sat_conv_split_rule(512, 128, 2, 256) == 1 and lib.sat_conv_split_rule(257, 128, 2, 256) == 1
    assert _rule(lib, 0, 64, 64, 132, 16, 8, 4) == 2 and _rule(lib, 0, 64, 64, 132, 16, 8, 4, cus=1) == 1     # 16 chunks, 4 tiles


def _refusals(lib):
    null = ctypes.c_void_p(None)
    ws = ctypes.c_void_p(4096)          # never dereferenced: the count is refused before anything is launched
    for n in (5, 17, 1000):             # 16 chunks: five splits of 4 chunks leave the fifth empty; more splits than chunks
        assert lib.sat_conv_bf16x3_split(0, 2, 256, 32, 136, 3, 1, 1, 1, n, 256, None) == -1
        assert lib.sat_conv1d_bf16x3_ws(*([null] * 13), 2, 256, 32, 136, 136, 3, 1, 1, 1, 0, null, null, null, null, 0, ws, 1 << 40, n, null) == 1
        assert b"split" in lib.sat_last_error()
        assert lib.sat_conv1d_bf16x3_planesq_ws(ws, ws, lib.sat_conv1d_k7_plane_rows(260, 260, 3), *([null] * 10), 2, 256, 64, 260, 260, 7, 1, 3, 0, 1,
                                                ws, 1 << 40, n, null) == 1
        assert b"split" in lib.sat_last_error()
    # the direct k7 kernel (plain weights) does not split; a workspace smaller than asked for is refused as well
    assert lib.sat_conv1d_bf16x3_ws(*([null] * 13), 2, 256, 64, 260, 260, 7, 1, 1, 3, 0, null, null, null, null, 0, ws, 1 << 40, 2, null) == 1
    need = ctypes.c_longlong(0)
    assert lib.sat_conv_bf16x3_split(0, 2, 256, 32, 136, 3, 1, 1, 1, 2, 256, ctypes.byref(need)) == 2 and need.value == 4 * 2 * 128 * 128
    assert lib.sat_conv1d_bf16x3_ws(*([null] * 13), 2, 256, 32, 136, 136, 3, 1, 1, 1, 0, null, null, null, null, 0, ws, need.value - 1, 2, null) == 1
    assert b"workspace" in lib.sat_last_error()


def test_illegal_forced_split_is_refused_sim(emu):
    _refusals(emu.lib)


def test_illegal_forced_split_is_refused_gfx950():
    """the product library's host code, without a GPU: status 1 comes back before any launch"""
    from stable_audio_tools_amd import _lib
    _refusals(_lib.load())


def test_ops_knob_forces_only_where_legal(emu):
    """SatOps.conv_split = n is a plain launch where the launch cannot have n splits (here: 4 chunks)"""
    x = torch.randn(1, 64, 40)
    w = torch.randn(8, 64, 3) * .2
    wp = emu.pack_bf16x3(w)
    base = emu.conv1d_bf16x3(x, wp, 8, 3, 1, 1, 1)
    keep = emu.conv_split
    emu.conv_split = 16
    try:
        got = emu.conv1d_bf16x3(x, wp, 8, 3, 1, 1, 1)
    finally:
        emu.conv_split = keep
    assert torch.equal(got, base)
