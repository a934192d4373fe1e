"""The dithered-FSQ bottleneck around a transformer autoencoder — the codec: audio -> token ids -> audio through
create_autoencoder_from_config, AudioAutoencoder.decode_tokens and AutoencoderPretransform.tokenize / decode_tokens, inference only,
against a fixture of the reference (tools/gen_golden_fsq.py; the case is in tests/fsq_cases.py).  CPU: the simulator; `-m gpu`: the
gfx950 library.

What can be exact is held exactly: the native bottleneck on the reference's STORED latents obeys the kernel rule of
tests/test_fsq_kernels.py (bit for bit away from rounding ties).  What goes through the encoder carries the encoder's error: its latents
are within test_taae.py's TOL = 1e-3 of the fixture, and with E the largest elementwise latent error of that run every digit whose
reference li64 lies farther than (L_d - 1) / 2 * E + 1e-4 from a tie equals the reference's digit (tanh is 1-Lipschitz, so li moves by at
most (L_d - 1) / 2 * E).  A transposed index tensor or swapped codebooks fail that on almost every digit.  At most 5 % of the digits may lie
inside the band, else the test fails: that would be a finding about the encoder's error, not a reason to move the cap.

Measured E and band shares: profiles/fsq/README.md."""
import json

import numpy as np
import pytest
import torch

import fsq_cases as cases
import refimport
import taae_cases
from golden_util import load_golden, rel_err

TOL = 1e-3      # test_taae.py's fp32 parity bar
LEVELS = cases.BOTTLENECK["config"]["levels"]
Q = cases.BOTTLENECK["config"]["num_codebooks"]
_GOLDEN = {}


def _golden(name="codec"):
    if name not in _GOLDEN:      # read once, shared, never written to
        _GOLDEN[name] = load_golden("fsq_" + name)
    return _GOLDEN[name]


def _build(device):
    from stable_audio_tools_amd import autoencoders as ae
    model = ae.create_autoencoder_from_config(json.loads(json.dumps(cases.codec_config())))
    missing, unexpected = model.load_state_dict(cases.codec_state_dict(model), strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model.to(device).train(False)


def _digits(tokens):
    """(B, T, Q) tokens -> (B, T, Q, D) digits"""
    basis = torch.tensor(cases.basis(LEVELS), dtype=torch.int64, device=tokens.device)
    return (tokens[..., None] // basis) % torch.tensor(LEVELS, dtype=torch.int64, device=tokens.device)


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_fsq_codec_surface():
    from stable_audio_tools_amd import autoencoders as ae
    from stable_audio_tools_amd import bottleneck as bn
    from stable_audio_tools_amd.pretransforms import AutoencoderPretransform
    model = _build("cpu")
    b = model.bottleneck
    assert isinstance(b, bn.DitheredFSQBottleneck) and isinstance(b, bn.DiscreteBottleneck) and isinstance(b, bn.Bottleneck)
    assert model.is_discrete and b.is_discrete and b.num_quantizers == 2 and b.codebook_size == 360 and b.tokens_id == "quantizer_indices"
    assert len(b.state_dict()) == 0 and sorted(model.state_dict().keys()) == list(_golden()["keys"])
    q = b.quantizer
    assert isinstance(q, bn.DitheredFSQ)
    assert (q.levels, q.codebook_dim, q.codebook_size, q.num_codebooks, q.dim, q.dither_inference, q.noise_dropout) == ([6, 5, 4, 3], 4, 360, 2, 8, True, 0.05)
    assert torch.equal(q._levels, torch.tensor([6, 5, 4, 3])) and q._levels.dtype == torch.int64
    assert torch.equal(q._basis, torch.tensor([1, 6, 30, 120])) and q._basis.dtype == torch.int64
    assert q.half_l.dtype == torch.float32 and torch.equal(q.half_l, 2.0 / torch.tensor([5.0, 4.0, 3.0, 2.0]))
    plain = bn.DitheredFSQ([5, 5])
    assert (plain.dither_inference, plain.num_codebooks, plain.noise_dropout, plain.codebook_size, plain.dim) == (False, 1, 0.5, 25, 2)
    assert float(b.norm_std_loss(torch.tensor([0.0, 2.0]))) == pytest.approx((2.0 ** 0.5 - 1.0) ** 2)
    x = torch.zeros(1, 8, 3)
    assert b.decode(x) is x
    pre = AutoencoderPretransform(model)
    assert pre.is_discrete and pre.num_quantizers == 2 and pre.codebook_size == 360
    with pytest.raises(NotImplementedError):
        bn.DiscreteBottleneck(1, 2, "x").decode_tokens(None)
    # levels as an int and as a list; the reference's errors
    assert bn.DitheredFSQBottleneck(3, 5).codebook_size == 125 and bn.DitheredFSQBottleneck(3, 5).quantizer.levels == [5, 5, 5]
    assert bn.DitheredFSQBottleneck(6, 17).codebook_size == 17 ** 6
    assert bn.DitheredFSQBottleneck(2, [4, 3], num_codebooks=3).num_quantizers == 3
    with pytest.raises(ValueError, match=r"Length of levels list \(3\) must match dim \(4\)"):
        bn.DitheredFSQBottleneck(4, [5, 5, 5])
    with pytest.raises(TypeError, match="either an int or a list"):
        bn.DitheredFSQBottleneck(2, (5, 5))
    with pytest.raises(NotImplementedError, match="scale"):
        bn.DitheredFSQ([5, 5], scale=2.0)
    made = ae.create_bottleneck_from_config({"type": "dithered_fsq", "config": {"dim": 2, "levels": 5}})
    assert isinstance(made, bn.DitheredFSQBottleneck) and isinstance(ae.create_bottleneck_from_config({"type": "vae"}), bn.VAEBottleneck)
    for kind in ("fsq", "rvq", "dac_rvq", "dac_rvq_vae", "rvq_vae", "tanh", "l2_norm", "wasserstein", "softnorm"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            ae.create_bottleneck_from_config({"type": kind, "config": {"levels": [5, 5]}})
    cfg = cases.codec_config()
    cfg["model"]["bottleneck"] = {"type": "fsq", "config": {"levels": [5, 5, 5, 5]}}
    with pytest.raises(NotImplementedError):
        ae.create_autoencoder_from_config(cfg)
    # a continuous model keeps the reference's assertions
    vae = ae.create_autoencoder_from_config(taae_cases.model_config(taae_cases.CASES.index("vae")))
    vpre = AutoencoderPretransform(vae)
    assert not vpre.is_discrete and vpre.num_quantizers is None and vpre.codebook_size is None
    with pytest.raises(AssertionError, match="Cannot tokenize with a continuous model"):
        vpre.tokenize(torch.zeros(1, 2, 64))
    with pytest.raises(AssertionError, match="Cannot decode tokens with a continuous model"):
        vpre.decode_tokens(torch.zeros(1, 8, 2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="only works with discrete autoencoders"):
        vae.decode_tokens(torch.zeros(1, 8, 2, dtype=torch.int64))


def _forward_refusals(device):
    from stable_audio_tools_amd import bottleneck as bn
    b = bn.DitheredFSQBottleneck(4, [6, 5, 4, 3], num_codebooks=2).to(device)
    x = torch.zeros(1, 8, 6, device=device)
    assert b.training
    with pytest.raises(NotImplementedError, match=r"call \.eval\(\)"):
        b.encode(x)
    with pytest.raises(NotImplementedError, match=r"call \.eval\(\)"):
        b.quantizer(x.transpose(1, 2))
    b.train(False)
    for bad in (x.double(), x.to(torch.bfloat16), x.half()):
        with pytest.raises(NotImplementedError, match="float32"):
            b.encode(bad)
    with pytest.raises(NotImplementedError, match="skip_tanh"):
        b.quantizer(x.transpose(1, 2), skip_tanh=True)
    with pytest.raises(NotImplementedError, match="inference-only"):      # no straight-through gradient: a graph must not end here silently
        b.encode(x.clone().requires_grad_(True))
    with torch.no_grad():
        assert b.encode(x.clone().requires_grad_(True)).shape == x.shape
    with pytest.raises(ValueError, match="fsq_encode"):
        b.encode(torch.zeros(1, 6, 6, device=device))
    with pytest.raises(AssertionError, match="expected last dimension of 2"):
        b.decode_tokens(torch.zeros(1, 6, 3, dtype=torch.int64, device=device))
    # the token-major wrappers of the quantiser agree with the (B, C, T) path, and a non-contiguous (B, C, T) view is taken
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 8, 37, generator=g).to(device)
    codes, info = b.encode(z, return_info=True)
    assert torch.equal(b.encode(z), codes) and info["quantizer_indices"].shape == (2, 37, 2) and info["quantizer_indices"].dtype == torch.int64
    c2, i2 = b.quantizer(z.transpose(1, 2))
    assert c2.shape == (2, 37, 8) and torch.equal(c2.transpose(1, 2), codes) and torch.equal(i2, info["quantizer_indices"])
    assert torch.equal(b.quantizer.indices_to_codes(i2), c2) and torch.equal(b.decode_tokens(i2), codes)
    assert torch.equal(b.encode(z.transpose(1, 2).contiguous().transpose(1, 2)), codes)


def test_fsq_codec_forward_refusals_simulator(emu_modules):
    _forward_refusals("cpu")


@pytest.mark.gpu
def test_fsq_codec_forward_refusals_gpu(hip):
    _forward_refusals("cuda")


# ---- the bottleneck on the reference's stored latents: the kernel rule -----------------------------------------------------------
def _stored_latents(device):
    g = _golden()
    model = _build(device)
    pre = torch.from_numpy(g["pre_bottleneck_latents"]).to(device)
    with torch.no_grad():
        codes, info = model.bottleneck.encode(pre, return_info=True)
        cases.check_rule("codec, stored latents", pre, codes, info["quantizer_indices"], LEVELS, Q,
                   torch.from_numpy(g["latents"]), torch.from_numpy(g["quantizer_indices"]))
        assert torch.equal(model.bottleneck.decode_tokens(torch.from_numpy(g["quantizer_indices"]).to(device)), torch.from_numpy(g["latents"]).to(device))


def test_fsq_codec_stored_latents_simulator(emu_modules):
    _stored_latents("cpu")


@pytest.mark.gpu
def test_fsq_codec_stored_latents_gpu(hip):
    _stored_latents("cuda")


# ---- audio -> tokens -> audio ----------------------------------------------------------------------------------------------------
def _codec(device):
    from stable_audio_tools_amd.pretransforms import AutoencoderPretransform
    g = _golden()
    model = _build(device)
    audio = cases.codec_audio().to(device)
    ref_pre = torch.from_numpy(g["pre_bottleneck_latents"]).to(device)
    ref_tokens = torch.from_numpy(g["quantizer_indices"]).to(device)
    with torch.no_grad():
        latents, info = model.encode(audio, return_info=True)
        pre, tokens = info["pre_bottleneck_latents"], info["quantizer_indices"]
        assert tokens.shape == ref_tokens.shape and tokens.dtype == torch.int64 and latents.shape == ref_pre.shape
        err = rel_err(pre, ref_pre)
        e = float((pre.double() - ref_pre.double()).abs().max())
        # digits outside the band the encoder's error opens around a tie equal the reference's
        d = len(LEVELS)
        lm1 = torch.tensor([LEVELS[c % d] - 1 for c in range(ref_pre.shape[1])], dtype=torch.float64, device=device)[None, :, None]
        li64 = (torch.tanh(ref_pre.double()) + 1.0) * lm1 / 2.0
        inside = (li64 - li64.floor() - 0.5).abs() <= lm1 / 2.0 * e + cases.TIE_BAND                          # (B, C, T)
        inside = inside.view(1, Q, d, -1).permute(0, 3, 1, 2)                                                    # (B, T, Q, D)
        share = float(inside.sum()) / inside.numel()
        same = _digits(tokens) == _digits(ref_tokens)
        print(f"fsq codec: latent rel err {err:.2e}, E {e:.2e}, band share {share:.4f}, digits equal {float(same.sum()) / same.numel():.4f}, "
              f"tokens equal {float((tokens == ref_tokens).sum()) / tokens.numel():.4f}")
        assert err < TOL, err
        assert bool(same[~inside].all()), "a digit outside the band differs from the reference's"
        assert share <= cases.CODEC_BAND_CAP, f"{share:.3f} of the digits lie inside the band: the encoder's error E = {e:.2e} is too large for this check"
        assert bool(((tokens >= 0) & (tokens < model.bottleneck.codebook_size)).all())
        # tokens -> audio, from the reference's tokens
        dec = model.decode_tokens(ref_tokens)
        derr = rel_err(dec, g["decoded"])
        print(f"fsq codec: decode_tokens rel err {derr:.2e}")
        assert dec.shape == g["decoded"].shape and derr < TOL, derr
        # the pretransform: audio -> tokens -> audio is decode() of the quantised latents, bit for bit
        pt = AutoencoderPretransform(model)
        ptok = pt.tokenize(audio)
        assert torch.equal(ptok, tokens)
        assert torch.equal(pt.decode_tokens(ptok), model.decode(latents))
        assert torch.equal(model.bottleneck.decode_tokens(tokens), latents)


def test_fsq_codec_simulator(emu_modules):
    _codec("cpu")


@pytest.mark.gpu
def test_fsq_codec_gpu(hip):
    _codec("cuda")


def _codec_bf16(device):
    from stable_audio_tools_amd.pretransforms import AutoencoderPretransform
    model = _build(device)
    pt = AutoencoderPretransform(model)
    audio = cases.codec_audio().to(device)
    with torch.no_grad(), torch.autocast(device, torch.bfloat16):
        codes, info = model.encode(audio, return_info=True)
        tokens = pt.tokenize(audio)
        assert codes.dtype == torch.float32 and info["pre_bottleneck_latents"].dtype == torch.float32, "the bottleneck runs in fp32 under autocast"
        assert tokens.dtype == torch.int64 and tokens.shape == (1, 130, 2) and torch.equal(tokens, info["quantizer_indices"])
        assert bool(((tokens >= 0) & (tokens < pt.codebook_size)).all())
        assert torch.equal(model.bottleneck.decode_tokens(tokens), codes)
        out = pt.decode_tokens(tokens)
        assert out.shape == audio.shape and bool(torch.isfinite(out).all())
    ref_tokens = torch.from_numpy(_golden()["quantizer_indices"]).to(device)
    print(f"fsq codec bf16: tokens equal to the fp32 reference's {float((tokens == ref_tokens).sum()) / tokens.numel():.4f}")


def test_fsq_codec_bf16_simulator(emu_modules):
    _codec_bf16("cpu")


@pytest.mark.gpu
def test_fsq_codec_bf16_gpu(hip):
    _codec_bf16("cuda")


# ---- fixture pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_fsq_fixtures_match_reference():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_fsq
    finally:
        sys.path.remove(tools)
    # integers and a finite set of fp32 values: exactly, except that another host's tanh may round an element near a tie the other way
    # — the rule of test_fsq_kernels.py, with the stored fixture as the reference
    for i, name in enumerate(cases.CASES):
        fresh, g = gen_golden_fsq.generate_kernel_case(i), _golden(name)
        assert set(fresh) == set(g), name
        levels, q = cases.case(i)[1:]
        cases.check_rule("fixture " + name, cases.inputs(i), torch.from_numpy(fresh["codes"]), torch.from_numpy(fresh["indices"]), levels, q,
                         torch.from_numpy(g["codes"]), torch.from_numpy(g["indices"]), cases.planted_columns(i))
        if "odd_codes" in g:
            assert np.array_equal(fresh["odd_codes"], g["odd_codes"])
    fresh, g = gen_golden_fsq.generate_codec(), _golden()
    assert set(fresh) == set(g) and list(fresh["keys"]) == list(g["keys"])
    for k in ("pre_bottleneck_latents", "decoded"):
        assert rel_err(torch.from_numpy(fresh[k]), g[k]) < 1e-6, k
    cases.check_rule("fixture codec", torch.from_numpy(g["pre_bottleneck_latents"]), torch.from_numpy(fresh["latents"]),
                     torch.from_numpy(fresh["quantizer_indices"]), LEVELS, Q, torch.from_numpy(g["latents"]), torch.from_numpy(g["quantizer_indices"]))
