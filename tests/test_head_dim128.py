"""Head dim 128 attention in the DiT, inference only (Attention(dim_heads=128): embed_dim // num_heads == 128, rotary on the first 64
dims) against fixtures of the reference's DiffusionTransformer (tools/gen_golden_head_dim128.py, cases in tests/head_dim128_cases.py):
module surface, the fp32 and bf16 no-grad forward with CFG, the v-DDIM sampler (eager; on the GPU also graphed), the error surface
(training, fp8 projections, other head dims) and a guard that the head dim 64 bf16 path still runs fused.  CPU: the simulator;
`-m gpu`: the gfx950 library.

Bars: 1e-3 is the bar of every DiT parity test here (tests/test_dit_parity.py TOL); 3e-2 is test_dit_bf16_*'s bar for the bf16 model
against the fp32 reference on bf16-rounded weights (the reference's own bf16 model sits 0.0082 / 0.0083 / 0.0082 from it)."""
import numpy as np
import pytest
import torch

import head_dim128_cases as cases
import refimport
import seeded
from golden_util import load_golden, rel_err
from test_qk_norm import _Counting

TOL = 1e-3
IDS = list(range(len(cases.CASES)))
_GOLDEN = {}


def _build(i, device, dtype=torch.float32):
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model.to(device=device, dtype=dtype).train(False)


def _inputs(i, device):
    inp = {k: v.to(device) for k, v in cases.inputs(i).items()}
    kw = dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], prepend_cond=inp.get("prepend_cond"),
              prepend_cond_mask=inp.get("prepend_cond_mask"))
    return inp, kw


def _golden(i):
    if i not in _GOLDEN:      # read once, shared, never written to
        _GOLDEN[i] = load_golden("dit_hd128_" + cases.case_id(i))
    return _GOLDEN[i]


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_head_dim128_surface():
    from stable_audio_tools_amd.transformer import Attention
    for kw, kvh in ((dict(), 2), (dict(dim_context=128), 1)):
        a = Attention(256, dim_heads=128, qk_norm="ln", **kw)
        assert (a.num_heads, a.kv_heads, a.dim_heads) == (2, kvh, 128) and a.scale == 128 ** -0.5
        sd = a.state_dict()
        for k, val in (("q_norm.weight", 1.0), ("q_norm.bias", 0.0), ("k_norm.weight", 1.0), ("k_norm.bias", 0.0)):
            assert tuple(sd[k].shape) == (128,) and bool((sd[k] == val).all())
        assert not any("norm" in k for k in Attention(256, dim_heads=128, qk_norm="l2", **kw).state_dict())
    for bad in (32, 96, 256):
        with pytest.raises(NotImplementedError):
            Attention(256, dim_heads=bad)
    for i in IDS:
        model = _build(i, "cpu")
        assert sorted(model.state_dict().keys()) == list(_golden(i)["keys"]), "state_dict keys differ from the reference"
        attn = model.transformer.layers[0]
        assert attn.self_attn.dim_heads == 128 and model.transformer.rotary_pos_emb.inv_freq.numel() == 32
        assert attn.cross_attn.kv_heads == (1 if i == 0 else 2)


# ---- error surface ---------------------------------------------------------------------------------------------------------------
def _error_surface(device):
    from stable_audio_tools_amd import linear
    from stable_audio_tools_amd.transformer import Attention
    for qk_norm in ("none", "ln"):
        for kw, ctx in ((dict(), None), (dict(dim_context=128), torch.zeros(1, 3, 128, device=device))):
            a = Attention(256, dim_heads=128, qk_norm=qk_norm, **kw).to(device)
            x = torch.zeros(1, 5, 256, device=device)
            with pytest.raises(NotImplementedError, match="inference"):      # grad mode is on: no backward kernels at this head dim
                a(x, context=ctx)
            with torch.no_grad():
                assert a(x, context=ctx).shape == (1, 5, 256)
            linear.set_fp8(a, True, min_features=1)
            with torch.no_grad(), pytest.raises(NotImplementedError, match="fp8"):
                a(x, context=ctx)
    model = _build(0, device)
    inp, kw = _inputs(0, device)
    with pytest.raises(NotImplementedError, match="inference"):
        model(inp["x"], inp["t"], cfg_scale=1.0, **kw)


def test_head_dim128_error_surface_simulator(emu_modules):
    _error_surface("cpu")


@pytest.mark.gpu
def test_head_dim128_error_surface_gpu(hip):
    _error_surface("cuda")


def _block_keeps_fp8_rows_away(device):
    """With the feed-forward and attention projections switched to fp8, the 128-dim attention must raise its own error — never be
    handed rows a LayerNorm quantised for it (fp8_for=)."""
    from stable_audio_tools_amd import linear
    from stable_audio_tools_amd.transformer import TransformerBlock
    blk = TransformerBlock(256, dim_heads=128).to(device=device, dtype=torch.bfloat16)
    x = torch.randn(1, 8, 256, device=device).bfloat16()
    linear.set_fp8(blk, True, min_features=1, policy="ff")      # feed-forward pair only: the block runs, attention in bf16
    with torch.no_grad():
        assert blk(x).shape == x.shape
    linear.set_fp8(blk, True, min_features=1, policy="all")
    with torch.no_grad(), pytest.raises(NotImplementedError, match="head dim 128 on an fp8"):
        blk(x)


def test_head_dim128_block_fp8_simulator(emu_modules):
    _block_keeps_fp8_rows_away("cpu")


@pytest.mark.gpu
def test_head_dim128_block_fp8_gpu(hip):
    _block_keeps_fp8_rows_away("cuda")


# ---- fp32 model against the reference fixtures -----------------------------------------------------------------------------------
def _forward_case(i, device):
    g = _golden(i)
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        plain = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
        guided = model(inp["x"], inp["t"], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw)
        _, info = model(inp["x"], inp["t"], return_info=True, **kw)
    errs = {"hidden_first": rel_err(info["hidden_states"][0], g["hidden_first"]), "hidden_last": rel_err(info["hidden_states"][-1], g["hidden_last"]),
            "plain": rel_err(plain, g["plain"]), "guided": rel_err(guided, g["guided"])}
    print("hd128 forward", cases.case_id(i), errs)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("i", IDS)
def test_head_dim128_matches_reference_simulator(emu_modules, i):
    _forward_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_head_dim128_matches_reference_gpu(hip, i):
    _forward_case(i, "cuda")


# ---- bf16 model ------------------------------------------------------------------------------------------------------------------
def _bf16_case(i, device):
    model = _build(i, device, torch.bfloat16)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        out = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
    assert out.dtype == torch.bfloat16
    e = rel_err(out.float(), _golden(i)["plain_bf16w"])
    print("hd128 bf16", cases.case_id(i), e)
    assert e < 3e-2, e


@pytest.mark.parametrize("i", IDS)
def test_head_dim128_bf16_simulator(emu_modules, i):
    _bf16_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_head_dim128_bf16_gpu(hip, i):
    _bf16_case(i, "cuda")


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
def _sampler_case(i, device, use_graph):
    from stable_audio_tools_amd.sampling import sample_v_ddim
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    out = sample_v_ddim(model, inp["x"], cases.SAMPLER_STEPS, cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, use_graph=use_graph, **kw)
    e = rel_err(out, _golden(i)["sampler"])
    print("hd128 sampler", cases.case_id(i), use_graph, e)
    assert e < TOL, e
    return out


@pytest.mark.parametrize("i", IDS)
def test_head_dim128_sampler_simulator(emu_modules, i):
    _sampler_case(i, "cpu", False)


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_head_dim128_sampler_gpu(hip, i):
    eager = _sampler_case(i, "cuda", False)
    graphed = _sampler_case(i, "cuda", True)
    assert torch.equal(eager, graphed)


# ---- guard: head dim 64 keeps its fused bf16 path ----------------------------------------------------------------------------------
def _hd64_stays_fused(device):
    from stable_audio_tools_amd import ops as ops_mod
    from stable_audio_tools_amd.transformer import Attention
    original = ops_mod.get_ops
    counting = _Counting(original())
    ops_mod.get_ops = lambda: counting
    try:
        for qk_norm in ("none", "ln"):
            for kw, ctx in ((dict(), None), (dict(dim_context=128), torch.randn(2, 11, 128, device=device).bfloat16())):
                a = Attention(256, qk_norm=qk_norm, zero_init_output=False, **kw).to(device=device, dtype=torch.bfloat16)
                assert a.dim_heads == 64
                with torch.no_grad():
                    a(torch.randn(2, 37, 256, device=device).bfloat16(), context=ctx)
        assert counting.calls.get("gemm_heads_bf16", 0) == 6 and counting.calls.get("attention_planes", 0) == 4, counting.calls
        assert not any(counting.calls.get(n, 0) for n in ("qk_norm", "attention", "attn_planes", "rope_apply_")), counting.calls
        # and 128 takes the standalone kernels
        counting.calls.clear()
        a = Attention(256, dim_heads=128, qk_norm="ln").to(device=device, dtype=torch.bfloat16)
        with torch.no_grad():
            a(torch.randn(2, 37, 256, device=device).bfloat16())
        assert counting.calls.get("qk_norm", 0) == 1 and counting.calls.get("attention", 0) == 1, counting.calls
        assert not any(counting.calls.get(n, 0) for n in ("gemm_heads_bf16", "attention_planes")), counting.calls
    finally:
        ops_mod.get_ops = original


def test_head_dim64_bf16_stays_fused_simulator(emu_modules):
    _hd64_stays_fused("cpu")


@pytest.mark.gpu
def test_head_dim64_bf16_stays_fused_gpu(hip):
    _hd64_stays_fused("cuda")


# ---- fixture pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_head_dim128_fixture_matches_reference():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_head_dim128
    finally:
        sys.path.remove(tools)
    i = 0
    fresh, g = gen_golden_head_dim128.generate(i), _golden(i)
    assert set(fresh) == set(g)
    assert list(fresh["keys"]) == list(g["keys"])
    for k in g:
        if k != "keys":
            assert rel_err(torch.from_numpy(np.asarray(fresh[k], dtype=np.float32)), np.asarray(g[k], dtype=np.float32)) < 1e-6, k
