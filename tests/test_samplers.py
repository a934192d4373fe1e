"""the native samplers (stable_audio_tools_amd/sampling.py) around the native DiT against golden vectors produced
by the REFERENCE's own sampler functions around the REFERENCE's DiffusionTransformer (oracle/gen_golden_samplers.py ->
tests/golden/samplers.npz): v-DDIM (eta 0 / eta > 0 / cfg_pp / dist_shift / sample_k dispatch), rectified-flow Euler (steps /
dist_shift / explicit sigmas), RK4, DPM-Solver++ (steps / sigmas), ping-pong, and the sample_rf schedule + dispatch.

Three executions of every case: the FUSED step (guidance + update in csrc/dit_ops.hip sat_sampler_step), the plain step (the model
wrapped so that it does not advertise the fused extension: the torch arithmetic of the reference), and — GPU only — the fused
step replayed from a HIP graph.  Final samples AND the per-step `denoised` handed to the callback are compared at the 1e-3 bar of
BASELINE.json (fp32).  When a reference tree is importable (build container: /root/reference; GPU box: oracle/_ref staged by
oracle/stage_ref.py) the reference's sampler functions are additionally run LIVE around the native model.
"""
import contextlib
import sys

import pytest
import torch

import gen_golden_samplers as gs
import refimport
import seeded
from golden_util import load_golden, rel_err

TOL = 1e-3
CASES = list(gs.CASES)


def _build(name, seed, device):
    from stable_audio_tools_amd.dit import DiffusionTransformer
    model = DiffusionTransformer(**seeded.DIT_CONFIGS[name])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded.seeded_state_dict(shapes, seed).items()}, strict=False)
    return model.to(device).train(False)


class _Plain(torch.nn.Module):
    """The native model without the `supports_fused_update` advertisement: the samplers take their plain-torch branch."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *a, **kw):
        return self.model(*a, **kw)


class _OnDevice:
    """Runs gen_golden_samplers.run_case (CPU inputs, CPU noise stream) against a model living on `device`."""

    def __init__(self, sampling, device, **native_kw):
        self.sampling, self.device, self.native_kw = sampling, device, native_kw
        self.DistributionShift = sampling.DistributionShift

    def __getattr__(self, fn_name):
        fn = getattr(self.sampling, fn_name)
        dev = self.device

        def call(model, x, *args, **kw):
            args = tuple(a.to(dev) if isinstance(a, torch.Tensor) else a for a in args)
            kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) and k != "sigmas" else v) for k, v in kw.items()}
            if "device" in kw:
                kw["device"] = dev
            if self.native_kw:
                g = torch.Generator().manual_seed(gs.NOISE_SEED)       # the reference drew from the global CPU stream after manual_seed
                kw.update(self.native_kw)
                if fn_name in ("sample", "sample_flow_pingpong"):
                    kw["noise_fn"] = lambda t: torch.randn(t.shape, generator=g).to(t.device)
            return fn(model, x.to(dev), *args, **kw).cpu()
        return call


def _check(case, device, mode):
    from stable_audio_tools_amd import sampling as native
    g = load_golden("samplers")
    name, seed, fn_name, kw, _ = gs.CASES[case]
    model = _build(name, seed, device)
    native_kw = {"use_graph": True} if mode == "graph" else {"use_graph": False}
    if mode == "plain":
        model = _Plain(model)
    with torch.no_grad():
        out, den = gs.run_case(_OnDevice(native, device, **native_kw), model, case)
    assert rel_err(out, g[case]) < TOL, (case, mode)
    assert den.shape == g[case + "/denoised"].shape and rel_err(den, g[case + "/denoised"]) < TOL, (case, mode, "denoised")


# the simulator runs a DiT evaluation in seconds: the CPU suite takes one case per update rule / operand (u-term, noise operand, third
# operand + separate base, previous-denoised operand, schedule + init data); the GPU suite runs all 15 cases in all three modes
SIM_FUSED = ["ddim_cfgpp", "ddim_eta", "euler_shift", "rk4", "dpmpp", "pingpong", "rf_dpmpp"]


@pytest.mark.parametrize("case", SIM_FUSED)
def test_native_samplers_match_reference_golden_fused_simulator(emu_modules, case):
    _check(case, "cpu", "fused")


@pytest.mark.parametrize("case", ["dpmpp", "pingpong"])
def test_native_samplers_match_reference_golden_plain_simulator(emu_modules, case):
    _check(case, "cpu", "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fused", "plain", "graph"])
@pytest.mark.parametrize("case", CASES)
def test_native_samplers_match_reference_golden_gpu(hip, case, mode):
    _check(case, "cuda", mode)


def _live(case, device):
    """The reference's OWN sampler function around the native model vs the native sampler around the same model: isolates the
    sampler arithmetic (the model evaluations are the same kernels on both sides)."""
    from stable_audio_tools_amd import sampling as native
    with contextlib.redirect_stdout(sys.stderr):
        refimport.import_reference()
    import stable_audio_tools.inference.sampling as ref_sampling
    name, seed, *_ = gs.CASES[case]
    model = _build(name, seed, device)

    class _RefOnDevice(_OnDevice):
        def __getattr__(self, fn_name):
            fn = getattr(self.sampling, fn_name)
            dev = self.device

            def call(m, x, *args, **kw):
                args = tuple(a.to(dev) if isinstance(a, torch.Tensor) else a for a in args)
                kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) and k != "sigmas" else v) for k, v in kw.items()}
                if "device" in kw:
                    kw["device"] = dev
                return fn(m, x.to(dev), *args, **kw).cpu()
            return call
    with torch.no_grad():
        ref_out, ref_den = gs.run_case(_RefOnDevice(ref_sampling, device), model, case)
        nat_out, nat_den = gs.run_case(_OnDevice(native, device, use_graph=False), model, case)
    # not tighter than the model's own noise floor: the fp32 model's attention runs the bf16x3 split (about 1e-5 per evaluation, and
    # not continuous in its input: a 6e-8 difference in x after step 0 moves step 1's output by 1e-4 — measured), so two arithmetically
    # equivalent update orders separate to a few 1e-4 over the steps; the bar is the fp32 bar of BASELINE.json
    assert rel_err(nat_out, ref_out) < TOL and rel_err(nat_den, ref_den) < TOL, case


LIVE = ["ddim", "ddim_cfgpp", "euler_shift", "rk4", "dpmpp", "rf_dpmpp"]       # deterministic cases (no device-side noise stream)


@pytest.mark.skipif(not refimport.available(), reason="no reference tree (/root/reference or oracle/_ref)")
@pytest.mark.parametrize("case", ["rk4", "rf_dpmpp"])
def test_reference_sampler_functions_on_native_model_simulator(emu_modules, case):
    _live(case, "cpu")


@pytest.mark.gpu
@pytest.mark.skipif(not refimport.available(), reason="no reference tree (oracle/_ref is staged by __graft_entry__.build())")
@pytest.mark.parametrize("case", LIVE)
def test_reference_sampler_functions_on_native_model_gpu(hip, case):
    _live(case, "cuda")


def test_distribution_shift_and_schedule_match_reference():
    """DistributionShift.time_shift, bit for bit against the reference's: its outputs stored by oracle/gen_golden_samplers.py
    (tests/golden/sampler_shift.npz), and the reference itself when its tree is importable (CPU only)."""
    from stable_audio_tools_amd import sampling as native
    got = gs.shift_table(native)
    want = load_golden("sampler_shift")
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        assert torch.equal(v, torch.from_numpy(want[k])), k
    if not refimport.available():
        return
    with contextlib.redirect_stdout(sys.stderr):
        refimport.import_reference()
    import stable_audio_tools.inference.sampling as ref_sampling
    ref = gs.shift_table(ref_sampling)
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k
