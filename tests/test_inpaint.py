"""Inpainting for the DiT (`diffusion_cond_inpaint`): training.random_inpaint_segments, the inpainting / input_concat_cond /
gradient_clip_val options of training.DiTTrainStep and the model's input_concat_cond path, against fixtures of the reference's
DiffusionTransformer and random_inpaint_mask (tools/gen_golden_inpaint.py, cases in tests/inpaint_cases.py).  Both cases have
dim_in = 4 + 5 = 9, the padded-K path of project_in and the 1x1 pre-conv.  CPU: the simulator; `-m gpu`: the gfx950 library.

Bars.  1e-3 (golden_util.rel_err) is the bar of every DiT parity test here (tests/test_qk_norm.py TOL); 3e-2 is
tests/test_head_dim128.py::_bf16_case's bar for the bf16 model against the fp32 reference on bf16-rounded weights; train steps:
losses within 1e-3 relative and worst relative parameter-update error < 2e-2, the bounds of tests/test_dit_step_options.py.
cross_attn.k_norm.bias (case adaln_rf) has a mathematically zero gradient (tests/test_qk_norm.py says why): its gradient is held
to 1e-3 of the same layer's cross_attn.q_norm.bias gradient, and its AdamW update — rounding noise divided by its own magnitude —
only to the most AdamW can move a parameter, lr * (1 + weight_decay * |p|) per step.  The same holds for the dims of
self_attn.k_norm.bias that the rotary embedding leaves alone (the last 32 of the 64: RotaryEmbedding(max(64 // 2, 32)) rotates the
first 32; the reference's own gradient there is <= 3e-8 against 1e-2 in the rotated dims): a gradient comparison in the max norm
does not see them, AdamW's elementwise normalisation does, so the update is compared on the rotated dims and bounded on the rest.

The mask draw relies on CPython's `random.choices` / `random.randint` streams being what they were when the fixtures were written: on
another stream the mask comparison fails first, loudly."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

import inpaint_cases as cases
import refimport
import seeded
from golden_util import load_golden, rel_err

TOL = 1e-3
ROTARY_DIMS = 32                # of the 64 dims of a head
IDS = list(range(len(cases.CASES)))
_GOLDEN = {}


def _golden(i):
    if i not in _GOLDEN:
        _GOLDEN[i] = load_golden("dit_inpaint_" + cases.case_id(i))
    return _GOLDEN[i]


def _build(i, device, dtype=torch.float32):
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**cases.case_config(i))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    sd = {k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, cases.case_seed(i)).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing)
    return model.to(device=device, dtype=dtype).train(False)


def _inputs(i, device):
    """(inputs, model keywords with the inpaint conditioning of the recorded draw cases.COND_DRAW)."""
    inp = cases.inputs(i)
    cond = cases.concat_cond(i, inp["x"], torch.from_numpy(_golden(i)["mask/" + cases.COND_DRAW]))
    inp = {k: v.to(device) for k, v in inp.items()}
    return inp, dict(cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], input_concat_cond=cond.to(device))


def _noise_targets(objective, x0, noise, t):
    if objective == "v":
        alpha, sigma = torch.cos(t * math.pi / 2)[:, None, None], torch.sin(t * math.pi / 2)[:, None, None]
        return x0 * alpha + noise * sigma, noise * alpha - x0 * sigma
    alpha, sigma = (1 - t)[:, None, None], t[:, None, None]
    return x0 * alpha + noise * sigma, noise - x0


def _stepper(i, device, **kw):
    from stable_audio_tools_amd.training import DiTTrainStep
    model = _build(i, device)
    model.train(True)
    args = dict(cases.OPT, cfg_dropout_prob=0.0, use_ema=True)
    args.update(kw)
    return DiTTrainStep(model, **args), model


# ---- 1. the mask draw --------------------------------------------------------------------------------------------------------
def _mask_draw(device):
    from stable_audio_tools_amd.training import expand_inpaint_segments, random_inpaint_segments
    g = _golden(0)
    for name, (seed, kwargs) in cases.MASK_DRAWS.items():
        random.seed(seed)
        table = random_inpaint_segments(cases.LENGTHS, cases.LENGTH, **kwargs)
        after = random.random()
        assert table.dtype == torch.int32 and table.device.type == "cpu"
        assert tuple(table.shape) == (cases.BATCH, max(1, kwargs.get("max_mask_segments", 10)), 2)
        want = torch.from_numpy(g["mask/" + name])
        got = expand_inpaint_segments(table.to(device), cases.LENGTH).to(torch.float32).cpu()
        assert torch.equal(got, want), (name, table.tolist())
        assert after == float(g["next/" + name]), (name, "the stream of `random` is not where the reference leaves it")
        assert torch.equal(torch.from_numpy(_golden(1)["mask/" + name]), want)
        used = (table[:, :, 1] > table[:, :, 0]).sum(dim=1).tolist()
        if not kwargs:
            assert max(used) >= 8 and min(used) == 0, (name, used)          # many segments on one item, an unmasked item
    # the reference's argument checks
    with pytest.raises(ValueError, match="must have 3 elements"):
        random_inpaint_segments([3], 5, mask_type_probabilities=[0.5, 0.5])
    with pytest.raises(ValueError, match="must sum to 1.0"):
        random_inpaint_segments([3], 5, mask_type_probabilities=[0.5, 0.5, 0.5])
    # FULL_MASK covers the padding too; a real length of 0 stays unmasked for the other two types
    random.seed(0)
    assert random_inpaint_segments([2, 0], 5, mask_type_probabilities=[0.0, 1.0, 0.0])[:, 0].tolist() == [[0, 5], [0, 5]]
    for probs in ([1.0, 0.0, 0.0], [0.0, 0.0, 1.0]):
        table = random_inpaint_segments([0, 0], 5, mask_type_probabilities=probs)
        assert bool(expand_inpaint_segments(table, 5).all())


def test_mask_draw_matches_reference():
    _mask_draw("cpu")


@pytest.mark.gpu
def test_mask_draw_matches_reference_gpu(hip):
    _mask_draw("cuda")


# ---- 2. surface --------------------------------------------------------------------------------------------------------------
def _surface(device, device_mask):
    from stable_audio_tools_amd.training import DiTTrainStep
    for i in IDS:
        assert sorted(_build(i, "cpu").state_dict().keys()) == list(_golden(i)["keys"]), "state_dict keys differ from the reference"
    model = _build(0, device)
    model.train(True)
    assert DiTTrainStep(model, inpainting_config={}).inpaint_mask_first is True
    assert DiTTrainStep(model, inpainting_config={"mask_kwargs": {"max_mask_segments": 3}},
                        input_concat_ids=["inpaint_masked_input", "inpaint_mask"]).inpaint_mask_first is False
    for bad in (("inpaint_mask",), ("inpaint_mask", "inpaint_mask"), ("inpaint_mask", "inpaint_masked_input", "x"), ("mask", "masked_input"), ()):
        with pytest.raises(ValueError, match="input_concat_ids"):
            DiTTrainStep(model, inpainting_config={}, input_concat_ids=bad)
    inp, kw = _inputs(0, device)
    stepper = DiTTrainStep(model, inpainting_config={}, cfg_dropout_prob=0.0)
    with pytest.raises(ValueError, match="input_concat_cond"):
        stepper(inp["x"], t=inp["t"], **kw)
    kw.pop("input_concat_cond")
    with pytest.raises(ValueError, match="inpaint_lengths"):
        stepper(inp["x"], t=inp["t"], padding_mask=device_mask, **kw)
    with pytest.raises(ValueError, match="inpaint_lengths"):
        stepper(inp["x"], t=inp["t"], inpaint_lengths=[1, 2], **kw)
    # a CPU mask at twice the latent length is resized as :375 does before its rows are summed
    assert stepper._inpaint_lengths(None, cases.padding_mask().repeat_interleave(2, dim=1), cases.BATCH, cases.LENGTH) == cases.LENGTHS
    assert stepper._inpaint_lengths(None, None, 2, 9) == [9, 9]
    assert math.isfinite(float(stepper(inp["x"], t=inp["t"], inpaint_lengths=cases.LENGTHS, **kw)["loss"]))


def test_inpaint_surface_simulator(emu_modules):
    _surface("cpu", torch.ones(cases.BATCH, cases.LENGTH, dtype=torch.bool, device="meta"))


@pytest.mark.gpu
def test_inpaint_surface_gpu(hip):
    _surface("cuda", cases.padding_mask().cuda())


# ---- 3. forward parity -------------------------------------------------------------------------------------------------------
def _forward_case(i, device):
    g = _golden(i)
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        plain = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
        guided = model(inp["x"], inp["t"], cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, **kw)
    errs = {"plain": rel_err(plain, g["plain"]), "guided": rel_err(guided, g["guided"])}
    print("inpaint forward", cases.case_id(i), errs)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("i", IDS)
def test_inpaint_forward_simulator(emu_modules, i):
    _forward_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_inpaint_forward_gpu(hip, i):
    _forward_case(i, "cuda")


def _bf16_case(i, device):
    model = _build(i, device, torch.bfloat16)
    inp, kw = _inputs(i, device)
    with torch.no_grad():
        out = model(inp["x"], inp["t"], cfg_scale=1.0, **kw)
    assert out.dtype == torch.bfloat16
    e = rel_err(out.float(), _golden(i)["plain_bf16w"])
    print("inpaint bf16", cases.case_id(i), e)
    assert e < 3e-2, e


@pytest.mark.parametrize("i", IDS)
def test_inpaint_bf16_simulator(emu_modules, i):
    _bf16_case(i, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("i", IDS)
def test_inpaint_bf16_gpu(hip, i):
    _bf16_case(i, "cuda")


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------
def _gradient_case(i, device, ops, fused):
    g = _golden(i)
    model = _build(i, device)
    model.train(True)
    inp, kw = _inputs(i, device)
    noise = torch.from_numpy(seeded.seeded_array(tuple(inp["x"].shape), cases.NOISE_SEED)).to(device)
    noised, target = _noise_targets(cases.objective(i), inp["x"], noise, inp["t"])
    xin = noised.clone().requires_grad_(True)
    before = ops.train_fused_nodes
    ops.train_fused_nodes = fused
    try:
        loss = torch.nn.functional.mse_loss(model(xin, inp["t"], **kw), target)
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
    print("inpaint gradients", cases.case_id(i), "fused" if fused else "unfused", worst)
    assert worst[1] < TOL, worst


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", IDS)
def test_inpaint_gradients_simulator(emu_modules, i, fused):
    _gradient_case(i, "cpu", emu_modules, fused)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", IDS)
def test_inpaint_gradients_gpu(hip, i, fused):
    _gradient_case(i, "cuda", hip, fused)


# ---- 5. two train steps ------------------------------------------------------------------------------------------------------
def _update_errors(i, model, before, g, nsteps):
    """Worst relative parameter-update error against the fixture's upd/<name> (the module docstring on cross_attn.k_norm.bias)."""
    worst = ("", 0.0)
    names = [n for n, _ in model.named_parameters()]
    assert {k[len("upd/"):] for k in g if k.startswith("upd/")} == set(names)
    for n, p in model.named_parameters():
        got = (p.detach().cpu() - before[n]).reshape(-1)
        if got.numel() > seeded.FULL_KEEP_NUMEL:
            got = got[torch.from_numpy(seeded.probe_index(n, got.numel()))]
        want = torch.from_numpy(g["upd/" + n])
        if n.endswith("k_norm.bias"):
            rotated = 0 if ".cross_attn." in n else ROTARY_DIMS
            most = nsteps * cases.OPT["lr"] * (1 + cases.OPT["weight_decay"] * float(before[n].abs().max())) * (1 + 1e-3)
            assert float(got[rotated:].abs().max()) <= most, (n, float(got[rotated:].abs().max()), most)
            if not rotated:
                continue
            got, want = got[:rotated], want[:rotated]
        e = float((got - want).norm() / want.norm().clamp_min(1e-12))
        if e > worst[1]:
            worst = (n, e)
    return worst


def _train_steps(i, device, by_lengths):
    g = _golden(i)
    stepper, model = _stepper(i, device, inpainting_config={}, input_concat_ids=cases.CONCAT_IDS[cases.case_id(i)])
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    inp = {k: v.to(device) for k, v in cases.inputs(i).items()}
    if by_lengths:
        extra = dict(inpaint_lengths=cases.LENGTHS, padding_mask=cases.padding_mask().to(device))
    else:
        extra = dict(padding_mask=cases.padding_mask())
    random.seed(cases.TRAIN_SEED)
    for s in range(cases.TRAIN_STEPS):
        x0, noise, t = cases.train_data(i, s)
        out = stepper(x0.to(device), t=t.to(device), noise=noise.to(device), cross_attn_cond=inp["cross_attn_cond"],
                      global_embed=inp["global_embed"], **extra)
        got, want = float(out["loss"]), float(g["train_loss"][s])
        print(f"inpaint train {cases.case_id(i)} by_lengths {by_lengths} step {s}: loss {got:.6f} reference {want:.6f}")
        assert abs(got - want) <= 1e-3 * abs(want), (s, got, want)
    worst = _update_errors(i, model, before, g, cases.TRAIN_STEPS)
    print(f"inpaint train {cases.case_id(i)}: worst relative parameter-update error {worst}")
    assert worst[1] < 2e-2, worst


@pytest.mark.parametrize("by_lengths", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_inpaint_train_steps_simulator(emu_modules, i, by_lengths):
    _train_steps(i, "cpu", by_lengths)


@pytest.mark.gpu
@pytest.mark.parametrize("by_lengths", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_inpaint_train_steps_gpu(hip, i, by_lengths):
    _train_steps(i, "cuda", by_lengths)


def _train_masks_are_the_reference_draws():
    """The masks the two reference train steps drew are what random_inpaint_segments draws from the same stream."""
    from stable_audio_tools_amd.training import expand_inpaint_segments, random_inpaint_segments
    random.seed(cases.TRAIN_SEED)
    for s in range(cases.TRAIN_STEPS):
        table = random_inpaint_segments(cases.LENGTHS, cases.LENGTH)
        assert torch.equal(expand_inpaint_segments(table, cases.LENGTH).float(), torch.from_numpy(_golden(0)["train_mask"][s]))


def test_inpaint_train_masks_are_the_reference_draws():
    _train_masks_are_the_reference_draws()


# ---- 6. gradient clipping ------------------------------------------------------------------------------------------------------
def _clipping(device):
    """gradient_clip_val against a torch restatement of the step's tail — torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW on a
    second copy of the model, the loss written out — on a caller-made input_concat_cond (the non-inpainting concat path)."""
    i, clip, nsteps = 0, 0.05, 2
    inp, kw = _inputs(i, device)
    ref = _build(i, device)
    ref.train(True)
    start = {n: p.detach().cpu().clone() for n, p in ref.named_parameters()}
    opt = torch.optim.AdamW(ref.parameters(), **cases.OPT)
    ref_losses, norms = [], []
    for s in range(nsteps):
        x0, noise, t = (a.to(device) for a in cases.train_data(i, s))
        noised, targets = _noise_targets(cases.objective(i), x0, noise, t)
        loss = torch.nn.functional.mse_loss(ref(noised, t, **kw), targets)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)))
        opt.step()
        ref_losses.append(float(loss.detach()))
    assert min(norms) > 2 * clip, norms                      # the clip is active at every step
    ref_upd = {n: p.detach().cpu() - start[n] for n, p in ref.named_parameters()}
    final = {}
    for value in (clip, 0.0):
        stepper, model = _stepper(i, device, gradient_clip_val=value)
        for s in range(nsteps):
            x0, noise, t = (a.to(device) for a in cases.train_data(i, s))
            out = stepper(x0, t=t, noise=noise, **kw)
            if value:
                assert abs(float(out["loss"]) - ref_losses[s]) <= 1e-3 * abs(ref_losses[s]), (s, float(out["loss"]), ref_losses[s])
        gnorm = float(stepper.flat.grad.double().norm())
        if value:
            assert gnorm <= clip * (1 + 1e-4), gnorm
            worst = max(float((p.detach().cpu() - start[n] - ref_upd[n]).norm() / ref_upd[n].norm().clamp_min(1e-12)) for n, p in model.named_parameters())
            print(f"clipping: grad norms {norms} -> {gnorm:.6f}, worst relative parameter-update error {worst:.3e}")
            assert worst < 2e-2, worst
        else:
            assert gnorm > 2 * clip, gnorm                       # the unclipped run keeps its gradient as it is
        final[value] = stepper.flat.data.detach().cpu().clone()
    assert not torch.equal(final[clip], final[0.0])


def test_gradient_clipping_simulator(emu_modules):
    _clipping("cpu")


@pytest.mark.gpu
def test_gradient_clipping_gpu(hip):
    _clipping("cuda")


# ---- 7. sampler ----------------------------------------------------------------------------------------------------------------
def _sampler_case(i, device, use_graph):
    from stable_audio_tools_amd.sampling import sample_v_ddim
    model = _build(i, device)
    inp, kw = _inputs(i, device)
    out = sample_v_ddim(model, inp["x"], cases.SAMPLER_STEPS, cfg_scale=cases.CFG_SCALE, scale_phi=cases.SCALE_PHI, use_graph=use_graph, **kw)
    e = rel_err(out, _golden(i)["sampler"])
    print("inpaint sampler", cases.case_id(i), use_graph, e)
    assert e < TOL, e


@pytest.mark.parametrize("i", IDS)
def test_inpaint_sampler_simulator(emu_modules, i):
    _sampler_case(i, "cpu", False)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_inpaint_sampler_gpu(hip, i, use_graph):
    _sampler_case(i, "cuda", use_graph)


# ---- 8. capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_inpaint_graphed_training_pass_equals_eager_gpu(hip):
    """Forward + loss + backward of the inpainting step front (ops.diffusion_noise_inpaint) and the model, captured once with
    torch.cuda.graph on a single stream and replayed with the interval tables of random.seed(58) and random.seed(90) copied into the
    static table: the gradients — input and every parameter — equal the eager pass bit for bit both times, and differ between the two
    tables, so the table is read from device memory at replay and nothing of it was frozen into the capture."""
    from stable_audio_tools_amd.training import random_inpaint_segments
    i = 0
    stepper, model = _stepper(i, "cuda", inpainting_config={}, input_concat_ids=cases.CONCAT_IDS[cases.case_id(i)], use_ema=False)
    params = list(model.parameters())
    inp = {k: v.cuda() for k, v in cases.inputs(i).items()}
    x0, noise, t = (a.cuda() for a in cases.train_data(i, 0))
    seg = torch.zeros(cases.BATCH, 10, 2, dtype=torch.int32, device="cuda")

    def pass_():
        noised, targets, cond = stepper._inpaint_front(x0, noise, t, seg)
        xin = noised.requires_grad_(True)
        out = stepper._model(xin, t, cross_attn_cond=inp["cross_attn_cond"], global_embed=inp["global_embed"], cfg_dropout_prob=0.0,
                             input_concat_cond=cond)
        return torch.autograd.grad(stepper._loss(out, targets, None), [xin] + params)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pass_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = pass_()
    seen = []
    for seed in (58, 90):
        random.seed(seed)
        seg.copy_(random_inpaint_segments(cases.LENGTHS, cases.LENGTH))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [a.clone() for a in static]
        eager = pass_()
        torch.cuda.synchronize()
        for n, a, b in zip(["<input>"] + [n for n, _ in model.named_parameters()], replayed, eager):
            assert torch.equal(a, b), (seed, n, rel_err(a, b))
        seen.append(replayed)
    assert not torch.equal(seen[0][0], seen[1][0])


# ---- 9. fixture pin ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not refimport.available(), reason="needs the reference checkout (build container only)")
def test_inpaint_fixture_matches_reference():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_golden_inpaint
    finally:
        sys.path.remove(tools)
    i = 0
    state = random.getstate()
    try:
        fresh, g = gen_golden_inpaint.generate(i), _golden(i)
    finally:
        random.setstate(state)
    assert set(fresh) == set(g)
    assert list(fresh["keys"]) == list(g["keys"])
    for k in g:
        if k.startswith("mask/") or k.startswith("next/") or k == "train_mask":
            assert np.array_equal(np.asarray(fresh[k]), g[k]), k
        elif k != "keys":
            assert rel_err(torch.from_numpy(np.asarray(fresh[k], dtype=np.float32)), np.asarray(g[k], dtype=np.float32)) < 1e-6, k
