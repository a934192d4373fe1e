"""The transformer autoencoder (autoencoders.TAAEBlock / TAAEEncoder / TAAEDecoder, factory type "taae") and the two block options it
needs (TransformerBlock(layer_scale=True), TransformerBlock(add_rope=True)), inference only, against fixtures of the reference
(tools/gen_golden_taae.py; cases in tests/taae_cases.py).  CPU: the simulator; `-m gpu`: the gfx950 library.

Bars: 1e-3 is the fp32 parity bar of test_vae_parity / test_dit_parity; 3e-2 is test_dit_bf16_*'s bar for a bf16 model, here for the
fp32-stored model under torch.autocast(bfloat16) against the fp32 fixture.  The generator holds every dense_* (no window) and
noscale_* (blocks switched off) fixture farther than 10 x 1e-3 from its counterpart; the tests hold the native outputs as far from them.

Measured bf16 figures (max |a - b| / max |b|), printed by the bf16 tests: recorded in profiles/taae/README.md."""
import json

import numpy as np
import pytest
import torch

import refimport
import taae_cases as cases
from golden_util import load_golden, rel_err

TOL = 1e-3
BF16_TOL = 3e-2
IDS = list(range(len(cases.CASES)))
_GOLDEN = {}


def _golden(i):
    if i not in _GOLDEN:      # read once, shared, never written to
        _GOLDEN[i] = load_golden("taae_" + cases.case_id(i))
    return _GOLDEN[i]


class _Pair(torch.nn.Module):
    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder


def _build(i, device, window=True):
    from stable_audio_tools_amd import autoencoders as ae
    if cases.case_id(i) == "vae":
        model = ae.create_autoencoder_from_config(json.loads(json.dumps(cases.model_config(i, window))))
    else:
        model = _Pair(ae.create_encoder_from_config({"type": "taae", "config": cases.case_config(i, "encoder", window)}),
                      ae.create_decoder_from_config({"type": "taae", "config": cases.case_config(i, "decoder", window)}))
    missing, unexpected = model.load_state_dict(cases.state_dict(model, cases.case_seed(i)), strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model.to(device).train(False)


def _outputs(i, model, device):
    inp = {k: v.to(device) for k, v in cases.inputs(i).items()}
    if cases.case_id(i) == "vae":
        _, info = model.encode(inp["audio"], return_info=True)
        enc = info["pre_bottleneck_latents"]
        dec = model.decode(enc.chunk(2, dim=1)[0])
    else:
        enc, dec = model.encoder(inp["audio"]), model.decoder(inp["latent"])
    block0 = model.encoder.layers[1](inp["block_input"])[:, ::cases.BLOCK0_STEP]
    return {"encoder": enc, "decoder": dec, "block0": block0}


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_taae_surface():
    from stable_audio_tools_amd import autoencoders as ae
    from stable_audio_tools_amd.transformer import ContinuousTransformer, LayerScale, RotaryEmbedding, TransformerBlock
    blk = ae.TAAEBlock(128, 256, 4)
    assert (blk.type, blk.sliding_window, blk.checkpointing, blk.use_snake, blk.use_dilated_conv) == ("encoder", [31, 32], False, False, False)
    stack = list(blk.layers[2])
    assert len(stack) == 5 and isinstance(stack[0], ae.Transpose) and isinstance(stack[4], ae.Transpose)
    t = stack[1]
    assert isinstance(t, TransformerBlock) and t.dim == 256 and t.dim_heads == 128 and t.layer_scale and t.add_rope
    assert t.self_attn.qk_norm == "ln" and t.pre_norm.eps == 1e-2 and t.ff.ff[2].bias is not None and t.ff.ff[2].in_features == 1024
    assert isinstance(t.self_attn_scale, LayerScale) and torch.equal(t.ff_scale.scale, torch.full([256], 1e-5))
    assert isinstance(t.rope, RotaryEmbedding) and t.rope.inv_freq.shape == (32,)
    assert t.self_attn.to_out.weight.abs().max() > 0, "layer_scale forces zero_init_branch_outputs=False"
    assert isinstance(ae.TAAEBlock(128, 128, 1).layers[1], torch.nn.Identity)
    enc, dec = ae.TAAEEncoder(), ae.TAAEDecoder()
    assert [b.sliding_window for b in list(enc.layers)[1:-2]] == [[63, 64]] * 4 and len(list(dec.layers)[1:-2]) == 4
    assert [len(b.layers[2]) - 2 for b in list(enc.layers)[1:-2]] == [3, 3, 3, 3]
    # the block options on their own, through ContinuousTransformer(**kwargs)
    ct = ContinuousTransformer(128, 2, layer_scale=True, add_rope=True)
    assert sorted(k for k in ct.layers[1].state_dict() if "scale." in k or "rope" in k) == ["ff_scale.scale", "rope.inv_freq", "self_attn_scale.scale"]
    assert "cross_attn_scale.scale" in TransformerBlock(128, cross_attend=True, layer_scale=True).state_dict()
    assert TransformerBlock(128).rope is None and isinstance(TransformerBlock(128).self_attn_scale, torch.nn.Identity)
    # ... and through the DiT's config JSON
    from stable_audio_tools_amd.dit import DiffusionTransformer
    dit = DiffusionTransformer(**json.loads(json.dumps(dict(io_channels=4, embed_dim=128, depth=1, num_heads=2, cond_token_dim=64, global_cond_dim=64,
                                                            layer_scale=True, add_rope=True))))
    assert dit.transformer.layers[0].layer_scale and dit.transformer.layers[0].rope.inv_freq.shape == (16,)
    assert "transformer.layers.0.cross_attn_scale.scale" in dit.state_dict()
    for i in IDS:
        model = _build(i, "cpu")
        assert sorted(model.state_dict().keys()) == list(_golden(i)["keys"]), "state_dict keys differ from the reference"
        sd = cases.state_dict(model, 1)
        sd.update({k: v for k, v in model.state_dict().items() if k.endswith("inv_freq")})
        model.load_state_dict(sd, strict=True)
    keys = list(_golden(0)["keys"])
    assert "encoder.layers.1.layers.2.1.pre_norm.gamma" in keys and "encoder.layers.1.layers.2.1.self_attn_scale.scale" in keys
    frozen = ae.create_encoder_from_config({"type": "taae", "requires_grad": False, "config": cases.case_config(0, "encoder")})
    assert not any(p.requires_grad for p in frozen.parameters())


def test_taae_refusals():
    from stable_audio_tools_amd import autoencoders as ae
    from stable_audio_tools_amd.transformer import Attention, TransformerBlock
    with pytest.raises(NotImplementedError, match="[Cc]onformer"):
        ae.TAAEBlock(64, 64, 2, conformer=True)
    with pytest.raises(NotImplementedError, match="ELU"):
        ae.TAAEBlock(64, 64, 2, use_dilated_conv=True, use_snake=False)
    with pytest.raises(ValueError, match="in_channels == out_channels"):
        ae.TAAEBlock(128, 64, 2, type="decoder", use_snake=True)
    with pytest.raises(ValueError, match="in_channels == out_channels"):
        ae.TAAEDecoder(channels=64, c_mults=[1, 2], strides=[2, 4], transformer_depths=[1, 1], use_snake=True)
    with pytest.raises(ValueError, match="Unknown type"):
        ae.TAAEBlock(64, 64, 2, type="middle")
    with pytest.raises(ValueError, match="sliding_window"):
        ae.TAAEBlock(64, 64, 2, sliding_window=[1])
    for make in (ae.create_encoder_from_config, ae.create_decoder_from_config):
        for kind in ("dac", "seanet", "local_attn", None):
            with pytest.raises(NotImplementedError, match="out of scope"):
                make({"type": kind, "config": {}})
    # what raised before for its own reasons still does
    for kw in (dict(conformer=True), dict(remove_norms=True), dict(causal=True)):
        with pytest.raises(NotImplementedError):
            TransformerBlock(128, **kw)
    with pytest.raises(NotImplementedError, match="dyt"):
        Attention(128, qk_norm="dyt")


def _forward_refusals(device):
    from stable_audio_tools_amd import autoencoders as ae
    from stable_audio_tools_amd.pretransforms import AutoencoderPretransform
    from stable_audio_tools_amd.transformer import TransformerBlock
    enc = ae.TAAEEncoder(**cases.case_config(0, "encoder")).to(device)
    x = torch.zeros(1, 2, 64, device=device)
    with pytest.raises(NotImplementedError, match="inference-only"):
        enc(x)
    blk = TransformerBlock(128, layer_scale=True).to(device)
    with pytest.raises(NotImplementedError, match="inference-only"):
        blk(torch.zeros(1, 8, 128, device=device))
    # grad mode with a window or head dim 128 keeps raising, with or without the new options
    plain = TransformerBlock(128, add_rope=True).to(device)
    with pytest.raises(NotImplementedError, match="inference-only"):
        plain(torch.zeros(1, 8, 128, device=device), self_attention_flash_sliding_window=[1, 1])
    with pytest.raises(NotImplementedError, match="inference-only"):
        TransformerBlock(128, dim_heads=128, add_rope=True).to(device)(torch.zeros(1, 8, 128, device=device))
    pre = AutoencoderPretransform(_build(3, device), model_half=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp32 and bf16 only"):
        pre.encode(torch.zeros(1, 2, 64, device=device))


def test_taae_forward_refusals_simulator(emu_modules):
    _forward_refusals("cpu")


@pytest.mark.gpu
def test_taae_forward_refusals_gpu(hip):
    _forward_refusals("cuda")


# ---- fp32 parity -----------------------------------------------------------------------------------------------------------------
def _parity_case(i, device):
    g = _golden(i)
    model = _build(i, device)
    with torch.no_grad():
        out = _outputs(i, model, device)
    errs = {k: rel_err(out[k], g[k]) for k in cases.OUTPUTS}
    far_dense = {k: rel_err(out[k], g["dense_" + k]) for k in cases.OUTPUTS}
    far_noscale = {k: rel_err(out[k], g["noscale_" + k]) for k in cases.OUTPUTS} if cases.has_scale(i) else {}
    print("taae fp32", cases.case_id(i), errs, "to dense:", far_dense, "to noscale:", far_noscale)
    assert all(tuple(out[k].shape) == g[k].shape for k in cases.OUTPUTS)
    assert max(errs.values()) < TOL, errs
    assert min(far_dense.values()) > 10 * TOL, far_dense
    assert not far_noscale or min(far_noscale.values()) > 10 * TOL, far_noscale


@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_taae_matches_reference_simulator(emu_modules, i):
    _parity_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_taae_matches_reference_gpu(hip, i):
    _parity_case(i, "cuda")


# ---- bf16 autocast ---------------------------------------------------------------------------------------------------------------
def _bf16_case(i, device):
    g = _golden(i)
    model = _build(i, device)
    with torch.no_grad(), torch.autocast(device, torch.bfloat16):
        out = _outputs(i, model, device)
    errs = {k: rel_err(out[k].float(), g[k]) for k in cases.OUTPUTS}
    print("taae bf16", cases.case_id(i), errs)
    assert all(out[k].dtype == torch.float32 for k in cases.OUTPUTS), "the conv stack stays fp32; only the tokens are bf16"
    assert max(errs.values()) < BF16_TOL, errs


@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_taae_bf16_simulator(emu_modules, i):
    _bf16_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS, ids=cases.CASES)
def test_taae_bf16_gpu(hip, i):
    _bf16_case(i, "cuda")


# ---- junction A/B ----------------------------------------------------------------------------------------------------------------
def _junction_ab(ops, device):
    """one model, fp32 through its decoder and bf16 through its encoder: both junction directions in both token dtypes"""
    i = 0
    model = _build(i, device)
    inp = {k: v.to(device) for k, v in cases.inputs(i).items()}
    for lowp in (False, True):
        outs = []
        for fused in (True, False):
            ops.taae_junction_fused = fused
            try:
                with torch.no_grad(), torch.autocast(device, torch.bfloat16, enabled=lowp):
                    outs.append(model.encoder(inp["audio"]) if lowp else model.decoder(inp["latent"]))
            finally:
                del ops.taae_junction_fused      # back to the class default
        assert ops.taae_junction_fused is True
        assert torch.equal(outs[0], outs[1]), lowp


def test_taae_junction_ab_simulator(emu_modules):
    _junction_ab(emu_modules, "cpu")


@pytest.mark.gpu
def test_taae_junction_ab_gpu(hip):
    _junction_ab(hip, "cuda")


# ---- scale folding ---------------------------------------------------------------------------------------------------------------
def _scale_folding(device):
    from stable_audio_tools_amd.transformer import TransformerBlock
    torch.manual_seed(7)
    kw = dict(dim_heads=64, cross_attend=True, dim_context=64, attn_kwargs={"qk_norm": "ln"}, ff_kwargs={"mult": 4, "no_bias": False})
    for gdim in (None, 128):
        blk = TransformerBlock(128, layer_scale=True, global_cond_dim=gdim, **kw).to(device)
        ref = TransformerBlock(128, layer_scale=False, zero_init_branch_outputs=False, global_cond_dim=gdim, **kw).to(device)
        with torch.no_grad():
            for name in ("self_attn_scale", "cross_attn_scale", "ff_scale"):
                getattr(blk, name).scale.copy_(torch.randn(128, device=device))
            ref.load_state_dict({k: v for k, v in blk.state_dict().items() if ".scale" not in k or "to_scale" in k}, strict=True)
            ref.self_attn.to_out.weight.mul_(blk.self_attn_scale.scale[:, None])
            ref.cross_attn.to_out.weight.mul_(blk.cross_attn_scale.scale[:, None])
            ref.ff.ff[2].weight.mul_(blk.ff_scale.scale[:, None])
            ref.ff.ff[2].bias.mul_(blk.ff_scale.scale)
            x, ctx = torch.randn(2, 70, 128, device=device), torch.randn(2, 5, 64, device=device)
            cond = torch.randn(2, 6 * 128, device=device) if gdim else None
            y, want = blk(x, context=ctx, global_cond=cond), ref(x, context=ctx, global_cond=cond)
            e = rel_err(y, want)
            print("scale folding", gdim, e)
            assert e < 1e-6, e
            assert rel_err(y, x) > 1e-2, "the branches contribute"
            # the folded copy follows in-place changes of the scale AND of the weight (and bias)
            cached = blk.ff.ff[2]._cache.items["scaled"][1][0]
            assert blk(x, context=ctx, global_cond=cond) is not None and blk.ff.ff[2]._cache.items["scaled"][1][0] is cached
            blk.ff_scale.scale.mul_(2.0)
            y2 = blk(x, context=ctx, global_cond=cond)
            assert not torch.equal(y2, y) and blk.ff.ff[2]._cache.items["scaled"][1][0] is not cached
            ref.ff.ff[2].weight.mul_(2.0)
            ref.ff.ff[2].bias.mul_(2.0)
            assert rel_err(y2, ref(x, context=ctx, global_cond=cond)) < 1e-6
            blk.self_attn.to_out.weight.mul_(0.5)
            ref.self_attn.to_out.weight.mul_(0.5)
            y3 = blk(x, context=ctx, global_cond=cond)
            assert not torch.equal(y3, y2) and rel_err(y3, ref(x, context=ctx, global_cond=cond)) < 1e-6
            blk.ff.ff[2].bias.add_(1.0)
            ref.ff.ff[2].bias.add_(blk.ff_scale.scale)
            assert rel_err(blk(x, context=ctx, global_cond=cond), ref(x, context=ctx, global_cond=cond)) < 1e-6
            # zero scales: the block is the identity on the residual stream
            for name in ("self_attn_scale", "cross_attn_scale", "ff_scale"):
                getattr(blk, name).scale.zero_()
            assert torch.equal(blk(x, context=ctx, global_cond=cond), x)


def test_taae_scale_folding_simulator(emu_modules):
    _scale_folding("cpu")


@pytest.mark.gpu
def test_taae_scale_folding_gpu(hip):
    _scale_folding("cuda")


# ---- add_rope --------------------------------------------------------------------------------------------------------------------
def _add_rope(device):
    from stable_audio_tools_amd.transformer import TransformerBlock
    torch.manual_seed(11)
    n = 70
    blk = TransformerBlock(128, dim_heads=64, add_rope=True, zero_init_branch_outputs=False).to(device)
    bare = TransformerBlock(128, dim_heads=64, zero_init_branch_outputs=False).to(device)
    bare.load_state_dict({k: v for k, v in blk.state_dict().items() if not k.startswith("rope.")}, strict=True)
    x = torch.randn(2, n, 128, device=device)
    with torch.no_grad():
        own = blk(x)
        assert torch.equal(own, blk(x, rotary_pos_emb=blk.rope.forward_from_seq_len(n)))
        assert torch.equal(own, bare(x, rotary_pos_emb=blk.rope.forward_from_seq_len(n)))
        assert not torch.equal(own, bare(x)), "the rotary table is applied"
    grads = []
    for explicit in (False, True):
        blk.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = blk(xg, rotary_pos_emb=blk.rope.forward_from_seq_len(n)) if explicit else blk(xg)
        assert torch.equal(y.detach(), own)
        y.square().sum().backward()
        grads.append([xg.grad.clone()] + [p.grad.clone() for p in blk.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_add_rope_simulator(emu_modules):
    _add_rope("cpu")


@pytest.mark.gpu
def test_add_rope_gpu(hip):
    _add_rope("cuda")


# ---- one block at the workload's length (GPU only) -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
def test_taae_block_at_workload_length_gpu(hip, lowp):
    """The first TAAE stage of an Oobleck-length item: N = 2^20 + 1 tokens of width 128 through one block.  Everything but attention is per
    token and attention is banded ([63, 64]), so rows [s, e) of the full output depend on rows [s - 63, e + 64) of the input alone: they
    must equal the block run on rows [s - 64, e + 64) with the matching rows of the full rotary table.  Three slices of 256 rows: the
    start, one straddling row 2^19, the end.  A 32-bit offset in the norm, projection, plane-preparation or attention launch at 1 M rows
    shows as a mismatch in the middle or at the end.  Bars: the fp32 / bf16 parity bars of this file, against the slice run."""
    from stable_audio_tools_amd.transformer import TransformerBlock
    n, w = 2 ** 20 + 1, [63, 64]
    torch.manual_seed(5)
    blk = TransformerBlock(128, dim_heads=128, layer_scale=True, add_rope=True, attn_kwargs={"qk_norm": "ln"}, norm_kwargs={"eps": 1e-2}).cuda()
    with torch.no_grad():
        for name in ("self_attn_scale", "ff_scale"):      # 1e-5 at construction: the branches would not show
            getattr(blk, name).scale.copy_(1.0 + 0.25 * torch.randn(128, device="cuda"))
        x = torch.randn(1, n, 128, device="cuda")
        if lowp:
            x = x.to(torch.bfloat16)
        with torch.autocast("cuda", torch.bfloat16, enabled=lowp):
            full = blk(x, self_attention_flash_sliding_window=w)
            table = blk.rope.forward_from_seq_len(n)[0]
            errs = {}
            for s, e in ((0, 256), (2 ** 19 - 128, 2 ** 19 + 128), (n - 256, n)):
                lo, hi = max(s - 64, 0), min(e + 64, n)
                part = blk(x[:, lo:hi].contiguous(), rotary_pos_emb=(table[lo:hi], 1.0), self_attention_flash_sliding_window=w)
                want = part[:, s - lo:e - lo]
                errs[(s, e)] = rel_err(full[:, s:e].float(), want.float())
                assert rel_err(full[:, s:e].float(), x[:, s:e].float()) > 1e-2, "the branches contribute"
        assert full.shape == x.shape and full.dtype == x.dtype and bool(torch.isfinite(full.float()).all())
    print("taae block at N = 2^20 + 1", "bf16" if lowp else "fp32", errs)
    assert max(errs.values()) < (BF16_TOL if lowp else TOL), errs


# ---- fixture pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_taae_fixture_matches_reference():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_taae
    finally:
        sys.path.remove(tools)
    i = 1
    fresh, g = gen_golden_taae.generate(i), _golden(i)
    assert set(fresh) == set(g)
    assert list(fresh["keys"]) == list(g["keys"])
    for k in g:
        if k not in ("keys", "window_gap", "block_gap"):
            assert rel_err(torch.from_numpy(np.asarray(fresh[k], dtype=np.float32)), np.asarray(g[k], dtype=np.float32)) < 1e-6, k
