"""Attention(qk_norm="ln" | "l2") in the DiT (attn_kwargs: {"qk_norm": ...}; reference transformer.py:336, :369-379, :397-403, :485-489)
against fixtures of the reference's DiffusionTransformer (tools/gen_golden_qk_norm.py, cases in tests/qk_norm_cases.py): module
surface, fp32 forward / gradients on every execution path, the bf16 inference path (norm inside the projection GEMM's epilogue),
the sampler, the cross-attention K / V plane cache, and the train step.  CPU: the simulator; `-m gpu`: the gfx950 library.
There is no graphed DiT train step in the library to compare with the eager one (GraphedTrainStep is the autoencoder's): the GPU
comparison is made on a captured forward + backward pass instead (test_qk_norm_graphed_training_pass_equals_eager_gpu).

Bars: 1e-3 is the BASELINE bar of every DiT parity test here (tests/test_dit_parity.py TOL); 3e-2 is test_dit_bf16_*'s bar for the
bf16 model against the fp32 reference on bf16-rounded weights (the reference's own bf16 distance with qk_norm is <= 0.011).
cross_attn.k_norm.bias has a mathematically zero gradient (without rotary a constant added to every key shifts all of a query's
scores equally): it is held to 1e-3 of the same layer's cross_attn.q_norm.bias gradient instead of to a relative error."""
import math

import numpy as np
import pytest
import torch

import qk_norm_cases as cases
import refimport
import seeded
from gen_golden import dit_inputs
from golden_util import load_golden, rel_err

TOL = 1e-3
IDS = list(range(len(cases.CASES)))


def _build(i, device, dtype=torch.float32):
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model.to(device=device, dtype=dtype).train(False)


def _inputs(i, device):
    inp = {k: v.to(device) for k, v in dit_inputs(cases.CASES[i][0]).items()}
    kw = dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], prepend_cond=inp.get("prepend_cond"),
              prepend_cond_mask=inp.get("prepend_cond_mask"))
    return inp, kw


def _golden(i):
    return load_golden("dit_qknorm_" + cases.case_id(i))


# ---- 1. surface --------------------------------------------------------------------------------------------------------------
def test_qk_norm_surface():
    from stable_audio_tools_amd import linear
    from stable_audio_tools_amd.transformer import Attention
    for kw in (dict(), dict(dim_context=64)):
        a = Attention(256, qk_norm="ln", **kw)
        sd = a.state_dict()
        for k, val in (("q_norm.weight", 1.0), ("q_norm.bias", 0.0), ("k_norm.weight", 1.0), ("k_norm.bias", 0.0)):
            assert tuple(sd[k].shape) == (64,) and bool((sd[k] == val).all())
        assert not any("norm" in k for k in Attention(256, qk_norm="l2", **kw).state_dict())
        assert not any("norm" in k for k in Attention(256, **kw).state_dict())
    with pytest.raises(NotImplementedError, match="dyt"):
        Attention(256, qk_norm="dyt")
    with pytest.raises(ValueError):
        Attention(256, qk_norm="rms")
    for bad in (dict(causal=True), dict(differential=True), dict(feat_scale=True)):
        with pytest.raises(NotImplementedError):
            Attention(256, qk_norm="ln", **bad)
    for i in IDS:
        assert sorted(_build(i, "cpu").state_dict().keys()) == list(_golden(i)["keys"]), "state_dict keys differ from the reference"
    # an fp8-switched input projection has no norm epilogue
    for kw, ctx in ((dict(), None), (dict(dim_context=64), torch.zeros(1, 3, 64))):
        a = Attention(256, qk_norm="l2", **kw)
        linear.set_fp8(a, True, min_features=1)
        with pytest.raises(NotImplementedError, match="fp8"):
            a(torch.zeros(1, 5, 256), context=ctx)


# ---- 3. (model part) the no-grad bf16 forward never launches a standalone norm kernel -------------------------------------------
class _Counting:
    """Forwards everything to the ops object, counting calls per name."""

    def __init__(self, ops):
        self.__dict__["_ops"], self.__dict__["calls"] = ops, {}

    def __getattr__(self, name):
        val = getattr(self._ops, name)
        if not callable(val):
            return val

        def wrapped(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return val(*a, **k)
        return wrapped

    def __setattr__(self, name, val):
        setattr(self._ops, name, val)


def _no_standalone_norm(device):
    from stable_audio_tools_amd import ops as ops_mod
    original = ops_mod.get_ops
    counting = _Counting(original())
    ops_mod.get_ops = lambda: counting
    try:
        for i in (0, 1):
            model = _build(i, device, torch.bfloat16)
            inp, kw = _inputs(i, device)
            with torch.no_grad():
                model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
        assert counting.calls.get("gemm_heads_bf16", 0) > 0
        assert counting.calls.get("qk_norm", 0) == 0 and counting.calls.get("layernorm_fp8", 0) == 0, counting.calls
    finally:
        ops_mod.get_ops = original


def test_qk_norm_bf16_forward_is_fused_simulator(emu_modules):
    _no_standalone_norm("cpu")


@pytest.mark.gpu
def test_qk_norm_bf16_forward_is_fused_gpu(hip):
    _no_standalone_norm("cuda")


# ---- 4. fp32 model against the reference fixtures --------------------------------------------------------------------------------
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
    print("qk_norm forward", cases.case_id(i), errs)
    assert max(errs.values()) < TOL, errs


def _gradient_case(i, device, ops, fused):
    g = _golden(i)
    model = _build(i, device)
    model.train(True)
    inp, kw = _inputs(i, device)
    x0, t = inp["x"], inp["t"]
    noise = torch.from_numpy(seeded.seeded_array(tuple(x0.shape), cases.NOISE_SEED)).to(device)
    alpha, sigma = torch.cos(t * math.pi / 2)[:, None, None], torch.sin(t * math.pi / 2)[:, None, None]
    noised, target = x0 * alpha + noise * sigma, noise * alpha - x0 * sigma
    xin = noised.clone().requires_grad_(True)
    before = ops.train_fused_nodes
    ops.train_fused_nodes = fused
    try:
        loss = torch.nn.functional.mse_loss(model(xin, t, **kw), target)
        names = [n for n, _ in model.named_parameters()]
        grads = dict(zip(["<input>"] + names, torch.autograd.grad(loss, [xin] + list(model.parameters()))))
    finally:
        ops.train_fused_nodes = before
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    stored = {k[len("grad/"):] for k in g if k.startswith("grad/")}
    assert stored == set(grads), stored ^ set(grads)
    worst = ("", 0.0)
    for n, got in grads.items():
        want = torch.from_numpy(g["grad/" + n])
        got = got.detach().cpu().reshape(-1)
        if got.numel() > seeded.FULL_KEEP_NUMEL:
            got = got[torch.from_numpy(seeded.probe_index(n, got.numel()))]
        if n.endswith("cross_attn.k_norm.bias"):
            ref_scale = float(torch.from_numpy(g["grad/" + n.replace("k_norm", "q_norm")]).abs().max())
            assert float(got.abs().max()) <= 1e-3 * ref_scale, (n, float(got.abs().max()), ref_scale)
            continue
        e = rel_err(got, want)
        if e > worst[1]:
            worst = (n, e)
    print("qk_norm gradients", cases.case_id(i), "fused" if fused else "unfused", worst)
    assert worst[1] < TOL, worst


@pytest.mark.parametrize("i", IDS)
def test_qk_norm_matches_reference_simulator(emu_modules, i):
    _forward_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_qk_norm_matches_reference_gpu(hip, i):
    _forward_case(i, "cuda")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", IDS)
def test_qk_norm_gradients_simulator(emu_modules, i, fused):
    _gradient_case(i, "cpu", emu_modules, fused)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", IDS)
def test_qk_norm_gradients_gpu(hip, i, fused):
    _gradient_case(i, "cuda", hip, fused)


# ---- 5. bf16 model ---------------------------------------------------------------------------------------------------------------
def _bf16_case(i, device):
    model = _build(i, device, torch.bfloat16)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        out = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
    assert out.dtype == torch.bfloat16
    e = rel_err(out.float(), _golden(i)["plain_bf16w"])
    print("qk_norm bf16", cases.case_id(i), e)
    assert e < 3e-2, e


@pytest.mark.parametrize("i", IDS)
def test_qk_norm_bf16_simulator(emu_modules, i):
    _bf16_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_qk_norm_bf16_gpu(hip, i):
    _bf16_case(i, "cuda")


# ---- 6. sampler ------------------------------------------------------------------------------------------------------------------
def _sampler_case(i, device, use_graph):
    from stable_audio_tools_amd.sampling import sample_v_ddim
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    out = sample_v_ddim(model, inp["x"], cases.SAMPLER_STEPS, cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, use_graph=use_graph, **kw)
    e = rel_err(out, _golden(i)["sampler"])
    print("qk_norm sampler", cases.case_id(i), use_graph, e)
    assert e < TOL, e
    return out


@pytest.mark.parametrize("i", [0, 1])
def test_qk_norm_sampler_simulator(emu_modules, i):
    _sampler_case(i, "cpu", False)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_qk_norm_sampler_gpu(hip, i):
    eager = _sampler_case(i, "cuda", False)
    graphed = _sampler_case(i, "cuda", True)
    assert torch.equal(eager, graphed)


# ---- 7. cross-attention K / V plane cache ----------------------------------------------------------------------------------------
def _cache_case(device):
    from stable_audio_tools_amd.dit import clear_inference_caches
    from stable_audio_tools_amd.transformer import Attention
    model = _build(0, device, torch.bfloat16)
    inp, _ = _inputs(0, device)
    cond = inp["cross_attn_cond"].to(torch.bfloat16)
    cross = [m for m in model.modules() if isinstance(m, Attention) and hasattr(m, "to_q")]
    assert cross and all(m.qk_norm == "ln" for m in cross)

    def run(fresh=False):
        if fresh:
            clear_inference_caches(model)
        with torch.no_grad():
            return model(inp["x"], inp["t"], cross_attn_cond=cond, global_embed=inp["global_embed"], cfg_scale=4.0, scale_phi=0.5).float().clone()

    a = run(fresh=True)
    ctx0 = cross[0]._kv_ctx
    assert torch.equal(a, run()) and cross[0]._kv_ctx is ctx0            # same conditioning object, same parameters: the planes are reused
    for name in ("weight", "bias"):
        with torch.no_grad():
            getattr(cross[0].k_norm, name).mul_(0.5).add_(0.25)            # in-place edit of a norm parameter: the planes are stale
        c = run()
        assert not torch.equal(a, c)
        assert torch.equal(c, run(fresh=True))
        a = c


def test_qk_norm_kv_cache_simulator(emu_modules):
    _cache_case("cpu")


@pytest.mark.gpu
def test_qk_norm_kv_cache_gpu(hip):
    _cache_case("cuda")


# ---- 8. train step ---------------------------------------------------------------------------------------------------------------
def _train_step_case(device):
    from stable_audio_tools_amd.training import DiTTrainStep
    model = _build(0, device)
    model.train(True)
    stepper = DiTTrainStep(model, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-3, cfg_dropout_prob=0.0, use_ema=True)
    normed = {n: p for n, p in model.named_parameters() if ".q_norm." in n or ".k_norm." in n}
    assert len(normed) == 4 * 2 * cases.case_config(0)["depth"]
    flat = stepper.flat.data
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()
    before = {n: p.detach().clone() for n, p in normed.items()}
    inp, _ = _inputs(0, device)
    noise = torch.from_numpy(seeded.seeded_array(tuple(inp["x"].shape), 2000)).to(device)
    out = stepper(inp["x"], cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], t=inp["t"], noise=noise)
    assert math.isfinite(float(out["loss"]))
    for n, p in normed.items():
        assert lo <= p.data_ptr() < hi, f"{n} is outside the flat parameter buffer"
        if n.endswith("cross_attn.k_norm.bias"):
            continue                                   # zero gradient (see the module docstring): AdamW leaves only the weight decay
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"


def test_qk_norm_train_step_simulator(emu_modules):
    _train_step_case("cpu")


@pytest.mark.gpu
def test_qk_norm_train_step_gpu(hip):
    _train_step_case("cuda")


def _train_batch(i, device, seed):
    inp, kw = _inputs(i, device)
    kw = {k: v for k, v in kw.items() if v is not None}
    x0 = torch.from_numpy(seeded.seeded_array(tuple(inp["x"].shape), seed)).to(device)
    noise = torch.from_numpy(seeded.seeded_array(tuple(inp["x"].shape), seed + 1)).to(device)
    t = inp["t"]
    alpha, sigma = torch.cos(t * math.pi / 2)[:, None, None], torch.sin(t * math.pi / 2)[:, None, None]
    return x0 * alpha + noise * sigma, noise * alpha - x0 * sigma, t, kw


@pytest.mark.gpu
def test_qk_norm_graphed_training_pass_equals_eager_gpu(hip):
    """The library has no graphed DiT train step (training.GraphedTrainStep wraps the autoencoder's step only), so the graphed / eager
    comparison is made on what qk_norm adds to a step: forward + loss + backward of the "ln" model, captured once with torch.cuda.graph
    and replayed on two batches, must give the gradients — input and every parameter, q_norm / k_norm included — of the eager pass
    bit for bit (same kernels, same order, no host-side value inside the capture)."""
    model = _build(0, "cuda")
    model.train(True)
    params = list(model.parameters())
    noised, target, t, kw = _train_batch(0, "cuda", 3000)
    xin = noised.clone().requires_grad_(True)
    tgt = target.clone()

    def pass_():
        loss = torch.nn.functional.mse_loss(model(xin, t, **kw), tgt)
        return torch.autograd.grad(loss, [xin] + params)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pass_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = pass_()
    for seed in (3000, 3100):
        noised, target, _, _ = _train_batch(0, "cuda", seed)
        with torch.no_grad():
            xin.copy_(noised)
            tgt.copy_(target)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [g.clone() for g in static]
        eager = pass_()
        torch.cuda.synchronize()
        for n, a, b in zip(["<input>"] + [n for n, _ in model.named_parameters()], replayed, eager):
            assert torch.equal(a, b), (seed, n, rel_err(a, b))


# ---- 9. fixture pin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_qk_norm_fixture_matches_reference():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_qk_norm
    finally:
        sys.path.remove(tools)
    i = 2
    fresh, g = gen_golden_qk_norm.generate(i), _golden(i)
    assert set(fresh) == set(g)
    assert list(fresh["keys"]) == list(g["keys"])
    for k in g:
        if k != "keys":
            assert rel_err(torch.from_numpy(np.asarray(fresh[k], dtype=np.float32)), np.asarray(g[k], dtype=np.float32)) < 1e-6, k
