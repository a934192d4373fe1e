"""Sliding-window self-attention in the DiT, inference only (ContinuousTransformer(sliding_window=[left, right]): flash-attn's
window_size on every layer's self-attention) against fixtures of the reference's DiffusionTransformer
(tools/gen_golden_sliding_window.py, whose docstring says how the reference applies the window; cases in
tests/sliding_window_cases.py): the fp32 and bf16 no-grad forward with CFG, the v-DDIM sampler (eager; on the GPU also graphed, bit-equal
— GraphedDenoiser and the samplers needed no change), a guard that the model without its window is far from the fixture, the module
surface (constructor, config JSON, validation) and the error surface (grad mode, fp8 projection, cross-attention window).
CPU: the simulator; `-m gpu`: the gfx950 library.

Bars: 1e-3 is the bar of every DiT parity test here (tests/test_dit_parity.py TOL); 3e-2 is test_dit_bf16_*'s bar for the bf16 model
against the fp32 reference on bf16-rounded weights."""
import json

import numpy as np
import pytest
import torch

import refimport
import seeded
import sliding_window_cases as cases
from golden_util import load_golden, rel_err

TOL = 1e-3
IDS = list(range(len(cases.CASES)))
_GOLDEN = {}


def _build(i, device, dtype=torch.float32, window=True):
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i, window=window))
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
        _GOLDEN[i] = load_golden("dit_window_" + cases.case_id(i))
    return _GOLDEN[i]


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_sliding_window_surface():
    from stable_audio_tools_amd.dit import DiffusionTransformer
    from stable_audio_tools_amd.transformer import ContinuousTransformer
    assert ContinuousTransformer(128, 1).sliding_window is None
    for w in ([5, 6], (0, 0), [-1, 8], [3, -1], [-1, -1]):
        assert ContinuousTransformer(128, 1, sliding_window=w).sliding_window == w
    for bad in ([5], [1, 2, 3], [-2, 3], [3, -2], [1.5, 2], ["a", 1], 7, "ab"):
        with pytest.raises(ValueError, match="sliding_window"):
            ContinuousTransformer(128, 1, sliding_window=bad)
    for i in IDS:
        cfg = json.loads(json.dumps(cases.case_config(i)))       # the model-config JSON route: plain kwargs, the window a list
        model = DiffusionTransformer(**cfg)
        assert model.transformer.sliding_window == cases.CONFIGS[cases.case_id(i)]["sliding_window"]
        assert sorted(model.state_dict().keys()) == list(_golden(i)["keys"]), "state_dict keys differ from the reference"
        assert DiffusionTransformer(**cases.case_config(i, window=False)).transformer.sliding_window is None
    assert [_build(i, "cpu").transformer.layers[0].self_attn.dim_heads for i in IDS] == [64, 128, 64]


# ---- error surface ---------------------------------------------------------------------------------------------------------------
def _error_surface(device):
    from stable_audio_tools_amd import linear
    from stable_audio_tools_amd.transformer import Attention, TransformerBlock
    for dh in (64, 128):
        for dtype in (torch.float32, torch.bfloat16):
            a = Attention(256, dim_heads=dh, zero_init_output=False).to(device=device, dtype=dtype)
            x = torch.randn(1, 9, 256, device=device).to(dtype)
            if dh == 64:
                with pytest.raises(NotImplementedError, match="inference-only"):      # grad mode is on: no windowed backward
                    a(x, flash_attn_sliding_window=(2, 2))
            with torch.no_grad():
                y, dense = a(x, flash_attn_sliding_window=(2, 2)), a(x)
                assert y.shape == (1, 9, 256) and not torch.equal(y, dense)
                assert torch.equal(a(x, flash_attn_sliding_window=(8, -1)), dense)      # hides nothing: the dense launch
                with pytest.raises(ValueError, match="sliding_window"):
                    a(x, flash_attn_sliding_window=(2, -3))
                linear.set_fp8(a, True, min_features=1)
                with pytest.raises(NotImplementedError, match="fp8"):
                    a(x, flash_attn_sliding_window=(2, 2))
        c = Attention(256, dim_heads=dh, dim_context=128).to(device)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="cross-attention"):
            c(torch.zeros(1, 5, 256, device=device), context=torch.zeros(1, 5, 128, device=device), flash_attn_sliding_window=(2, 2))
    blk = TransformerBlock(256, cross_attend=True, dim_context=128).to(device)
    x, ctx = torch.zeros(1, 5, 256, device=device), torch.zeros(1, 3, 128, device=device)
    with torch.no_grad():
        assert blk(x, context=ctx, self_attention_flash_sliding_window=[1, 1]).shape == x.shape
        with pytest.raises(NotImplementedError, match="cross_attention_flash_sliding_window"):
            blk(x, context=ctx, cross_attention_flash_sliding_window=[1, 1])
    model = _build(0, device)
    inp, kw = _inputs(0, device)
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(inp["x"], inp["t"], cfg_scale=1.0, **kw)


def test_sliding_window_error_surface_simulator(emu_modules):
    _error_surface("cpu")


@pytest.mark.gpu
def test_sliding_window_error_surface_gpu(hip):
    _error_surface("cuda")


# ---- fp32 model against the reference fixtures -----------------------------------------------------------------------------------
def _forward_case(i, device):
    g = _golden(i)
    assert rel_err(torch.from_numpy(np.asarray(g["plain"])), g["dense_plain"]) > 10 * TOL      # the fixture itself: the window matters
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        plain = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
        guided = model(inp["x"], inp["t"], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw)
        no_window = _build(i, device, window=False)(inp["x"], inp["t"], cfg_scale=1.0, **kw)
    errs = {"plain": rel_err(plain, g["plain"]), "guided": rel_err(guided, g["guided"])}
    far = rel_err(no_window, g["plain"])
    print("window forward", cases.case_id(i), errs, "without the window:", far, "dense fixture:", rel_err(no_window, g["dense_plain"]))
    assert max(errs.values()) < TOL, errs
    assert far > 10 * TOL, "the model without its window matches the windowed fixture: the fixture cannot tell a window ignored"
    assert rel_err(no_window, g["dense_plain"]) < TOL


@pytest.mark.parametrize("i", IDS)
def test_sliding_window_matches_reference_simulator(emu_modules, i):
    _forward_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_sliding_window_matches_reference_gpu(hip, i):
    _forward_case(i, "cuda")


# ---- bf16 model ------------------------------------------------------------------------------------------------------------------
def _bf16_case(i, device):
    model = _build(i, device, torch.bfloat16)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        out = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
    assert out.dtype == torch.bfloat16
    e = rel_err(out.float(), _golden(i)["plain_bf16w"])
    print("window bf16", cases.case_id(i), e)
    assert e < 3e-2, e


@pytest.mark.parametrize("i", IDS)
def test_sliding_window_bf16_simulator(emu_modules, i):
    _bf16_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_sliding_window_bf16_gpu(hip, i):
    _bf16_case(i, "cuda")


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
def _sampler_case(i, device, use_graph, dtype=torch.float32):
    from stable_audio_tools_amd.sampling import sample_v_ddim
    model = _build(i, device, dtype)
    inp, kw = _inputs(i, device)
    out = sample_v_ddim(model, inp["x"], cases.SAMPLER_STEPS, cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, use_graph=use_graph, **kw)
    if dtype == torch.float32:
        e = rel_err(out, _golden(i)["sampler"])
        print("window sampler", cases.case_id(i), use_graph, e)
        assert e < TOL, e
    return out


@pytest.mark.parametrize("i", IDS)
def test_sliding_window_sampler_simulator(emu_modules, i):
    _sampler_case(i, "cpu", False)


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_sliding_window_sampler_gpu(hip, i):
    """eager against the fixture, then GraphedDenoiser's replay bit-equal to eager, in fp32 and in bf16"""
    for dtype in (torch.float32, torch.bfloat16):
        eager = _sampler_case(i, "cuda", False, dtype)
        graphed = _sampler_case(i, "cuda", True, dtype)
        assert torch.equal(eager, graphed), dtype


# ---- fixture pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_sliding_window_fixture_matches_reference():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_sliding_window
    finally:
        sys.path.remove(tools)
    i = 2
    fresh, g = gen_golden_sliding_window.generate(i), _golden(i)
    assert set(fresh) == set(g)
    assert list(fresh["keys"]) == list(g["keys"])
    for k in g:
        if k not in ("keys", "window_gap"):
            assert rel_err(torch.from_numpy(np.asarray(fresh[k], dtype=np.float32)), np.asarray(g[k], dtype=np.float32)) < 1e-6, k
