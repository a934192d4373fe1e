"""The k = 7 weight gradient from bf16 planes (csrc/conv_wgrad7_planes.h): the transposed LDS read it is built on, the kernel against a
float64 evaluation of  dW[co][ci][tap] = sum_{b,t} dy[co][t] * act[ci][t + tap*dil - pad]  (bound: twice the pipelined fp32-input
kernel's own relative L2 error on the same inputs — same bf16 bits, another summation order), exact integer data (a permuted k order),
ResidualUnitFn end to end with the knobs on and off, the fallbacks (stale kept planes, recompute, a shape outside the contract), and a
captured generator step of a 128-channel model against eager steps."""
import ctypes

import numpy as np
import pytest
import torch

from stable_audio_tools_amd import functional as F_


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- the primitive
def _tr_probe(ops, dev):
    img = torch.arange(1024, dtype=torch.int32).mul(37).add(11).remainder(65536).to(torch.int16).to(dev)     # distinct 16-bit patterns
    g = torch.Generator().manual_seed(5)
    for trial in range(4):
        # per 16-lane group: a base + 4 rows (stride a multiple of 8 bytes) x 4 pieces of 8 bytes anywhere (8-byte aligned)
        off = torch.zeros(64, dtype=torch.int32)
        for grp in range(4):
            for q in range(4):
                for p in range(4):
                    off[16 * grp + 4 * q + p] = 8 * int(torch.randint(0, 256, (1,), generator=g)) if trial else 512 * grp + 64 * q + 8 * p
        out = torch.zeros(256, dtype=torch.int16, device=dev)
        assert ops.lib.sat_lds_read_tr16_probe(_p(img), _p(off.to(dev)), _p(out), None) == 0
        if dev != "cpu":
            torch.cuda.synchronize()
        out = out.cpu().view(64, 4)
        imgc = img.cpu()
        for lane in range(64):
            g0, i = lane & ~15, lane & 15
            for q in range(4):
                src = int(off[g0 + 4 * q + (i >> 2)]) // 2 + (i & 3)
                assert int(out[lane, q]) == int(imgc[src]), (trial, lane, q)


def test_lds_read_tr16_sim(emu):
    _tr_probe(emu, "cpu")


@pytest.mark.gpu
def test_lds_read_tr16_gpu(hip):
    _tr_probe(hip, "cuda")


# ---------------------------------------------------------------- the kernel
def _planes(ops, x, snake):
    b, c, t = x.shape
    rows = ops.lib.sat_conv1d_k7_plane_rows(t, t, 0)
    n = b * ((c + 7) // 8) * rows * 8
    hi = torch.zeros(n, dtype=torch.int16, device=x.device)
    lo = torch.zeros(n, dtype=torch.int16, device=x.device)
    sa = sib = None
    if snake is not None:
        sa, sib = ops.snake_consts(snake[0], snake[1])
    assert ops.lib.sat_conv1d_k7_planes(_p(x), _p(sa) if sa is not None else None, _p(sib) if sib is not None else None, _p(hi), _p(lo),
                                        b, c, t, rows, None) == 0
    return hi, lo, rows


def _ref64(dy, act, dil, pad):
    b, m, t = dy.shape
    n = act.shape[1]
    dy64, a64 = dy.double().cpu(), act.double().cpu()
    ap = torch.nn.functional.pad(a64, (pad, 6 * dil - pad))
    out = torch.zeros(m, n, 7, dtype=torch.float64)
    for k in range(7):
        out[:, :, k] = torch.einsum("bmt,bnt->mn", dy64, ap[:, :, k * dil:k * dil + t])
    return out


def _snake64(x, la, lb):
    x64 = x.double().cpu()
    a = la.double().cpu().exp()[None, :, None]
    ib = 1.0 / (lb.double().cpu().exp()[None, :, None] + 1e-9)
    return x64 + ib * torch.sin(x64 * a) ** 2


def _rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def _kernel_case(ops, dev, c, t, dil, bsz=2, integer=False, raw=False):
    g = torch.Generator().manual_seed(c + t + dil)
    pad = 3 * dil
    if integer:
        dy = torch.randint(-3, 4, (bsz, c, t), generator=g).float().to(dev)
        x = torch.randint(-3, 4, (bsz, c, t), generator=g).float().to(dev)
        snake = None
        act64 = x.double().cpu()
    else:
        dy = torch.randn(bsz, c, t, generator=g).to(dev)
        x = torch.randn(bsz, c, t, generator=g).to(dev)
        snake = (0.3 * torch.randn(c, generator=g).to(dev), 0.3 * torch.randn(c, generator=g).to(dev))
        act64 = _snake64(x, *snake)
    ref = _ref64(dy, act64, dil, pad)
    dyp, actp = _planes(ops, dy, None), _planes(ops, x, snake)
    assert ops.conv_wgrad7_planes_ok(bsz, c, c, t, dil, pad, dyp[2], actp[2])
    new = ops.conv_wgrad7_planes(dyp, actp, bsz, c, c, t, dil, pad, raw=raw)
    if raw:
        new = new.reduce(ops)
    if integer:
        assert torch.equal(new.double().cpu(), ref), "integer data: dW must be exact (k order / fragment map)"
        return
    old = ops.conv_wgrad7_bf16x3(dy, x, dil, pad, snake=snake)
    e_old, e_new = _rel(old, ref), _rel(new, ref)
    print(f"wgrad7 C={c} T={t} dil={dil} B={bsz}: rel L2 vs float64  pipelined {e_old:.3e}  planes {e_new:.3e}")
    assert e_new <= 2 * e_old, f"planes kernel {e_new:.3e} > 2 x pipelined kernel {e_old:.3e} (C={c}, T={t}, dil={dil})"


# (256, 2112) at batch 2: 66 stages over 8 tiles -> 33 splits of TWO stages (the double-buffered loop); the others: one stage per split
@pytest.mark.parametrize("c,t,dil", [(64, 64, 1), (128, 200, 3), (64, 448, 9), (256, 136, 9), (256, 2112, 9)])
def test_wgrad7_planes_kernel_sim(emu, c, t, dil):
    _kernel_case(emu, "cpu", c, t, dil, raw=(dil == 3))


@pytest.mark.parametrize("c,t,dil", [(64, 192, 1), (64, 192, 3), (64, 192, 9), (256, 2112, 3)])
def test_wgrad7_planes_integer_sim(emu, c, t, dil):
    if t > 192:
        assert emu.lib.sat_conv_wgrad7_planes_nsplit(2, c, c, t) < 2 * ((t + 63) // 64)      # several stages per split
    _kernel_case(emu, "cpu", c, t, dil, integer=True)


_GPU_SHAPES = [(128, 1 << 18, 1), (128, 1 << 18, 9), (256, 1 << 16, 3), (64, 1 << 18, 9), (256, 8192, 1), (64, 64, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("c,t,dil", _GPU_SHAPES)
def test_wgrad7_planes_kernel_gpu(hip, c, t, dil):
    _kernel_case(hip, "cuda", c, t, dil, bsz=2 if t <= (1 << 16) else 1, raw=(dil == 3))


@pytest.mark.gpu
@pytest.mark.parametrize("dil", [1, 3, 9])
def test_wgrad7_planes_integer_gpu(hip, dil):
    assert hip.lib.sat_conv_wgrad7_planes_nsplit(2, 256, 256, 16384) == 64                       # 512 stages: 8 per split
    _kernel_case(hip, "cuda", 256, 16384, dil, integer=True)


def test_wgrad7_planes_contract(emu):
    lib = emu.lib
    assert lib.sat_conv_wgrad7_planes_ok(1, 128, 128, 4096, 9, 27, 32 + 4096 + 320, 32 + 4096 + 320) == 1
    assert lib.sat_conv_wgrad7_planes_ok(1, 128, 32, 4096, 9, 27, 32 + 4096 + 320, 32 + 4096 + 320) == 0      # narrow input: 4-wave kernel
    assert lib.sat_conv_wgrad7_planes_ok(1, 128, 128, 4096, 2, 6, 32 + 4096 + 320, 32 + 4096 + 320) == 0      # dilation
    assert lib.sat_conv_wgrad7_planes_ok(1, 128, 128, 4096, 9, 27, 32 + 4096, 32 + 4096) == 0                 # no trailing halo rows
    assert lib.sat_conv_wgrad7_planes(None, None, 0, None, None, 0, None, 1, 1, 1, 1, 128, 128, 64, 1, 3, None) != 0


# ---------------------------------------------------------------- ResidualUnitFn end to end
def _unit(ops, dev, c, t, dil, steps=2, recompute=False, stale=None, on_forward=None):
    """Gradients of `steps` forward / backward passes of one unit (the second one finds the owned plane buffer in place).
    stale (last pass only): "gen" — the same unit runs a second forward before the backward (its owned buffer is rewritten);
    "ver" / "snake" — the kept handle's record of x's version / of the SnakeBeta parameters no longer matches (what an in-place edit
    between forward and backward leaves behind; autograd itself refuses such an edit of a saved tensor, so the guard is driven directly).
    on_forward(y): called after every forward."""
    g = torch.Generator().manual_seed(3)
    mk = lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g)).to(dev).requires_grad_(True)
    x = mk(2, c, t)
    a1, b1, a2, b2 = (mk(c, sc=0.3) for _ in range(4))
    w1, w2 = mk(c, c, 7, sc=0.05), mk(c, c, 1, sc=0.1)
    bias1, bias2 = mk(c, sc=0.1), mk(c, sc=0.1)
    dy = torch.randn(2, c, t, generator=g).to(dev)
    leaves = (x, a1, b1, w1, bias1, a2, b2, w2, bias2)
    out = None
    for _ in range(steps):
        for p in leaves:
            p.grad = None
        y = F_.ResidualUnitFn.apply(x, a1, b1, w1, bias1, a2, b2, w2, bias2, dil, ops, recompute)
        if on_forward is not None:
            on_forward(y)
        if stale is not None and _ == steps - 1:
            kp = y.grad_fn.k7_planes
            assert kp is not None, "nothing was kept: the guard is not exercised"
            if stale == "gen":
                with torch.no_grad():
                    F_.ResidualUnitFn.apply(x.detach().flip(2).requires_grad_(True), a1, b1, w1, bias1, a2, b2, w2, bias2, dil, ops, recompute)
                assert kp.gen != kp.own.gen
            elif stale == "ver":
                kp.ver -= 1
            else:
                kp.snake = kp.snake[:2] + (kp.snake[2] - 1,) + kp.snake[3:]
        y.backward(dy)
        out = [p.grad.clone() for p in leaves]
    return out


def _unit_case(ops, dev, c, t, dil):
    saved = (ops.wgrad7_planes, ops.ru_k1_bwd_skip_dh)
    try:
        ops.wgrad7_planes, ops.ru_k1_bwd_skip_dh = False, False
        ref = _unit(ops, dev, c, t, dil)
        ops.wgrad7_planes, ops.ru_k1_bwd_skip_dh = True, False
        calls, skips = [], []
        orig, orig_k1 = ops.conv_wgrad7_planes, ops.ru_k1_bwd
        ops.conv_wgrad7_planes = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        ops.ru_k1_bwd = lambda *a, **k: (skips.append(bool(k.get("skip_dh"))), orig_k1(*a, **k))[1]
        try:
            on = _unit(ops, dev, c, t, dil)
            assert calls, "the planes kernel did not run"
            assert not any(skips), "ru_k1_bwd_skip_dh is off"
            del skips[:]
            ops.ru_k1_bwd_skip_dh = True
            skip = _unit(ops, dev, c, t, dil)
            # C = 128: sat_ru_k1_bwd runs and skips the dh store in both passes (nobody emits this x: the conv owns its planes from the first); C = 256: it never runs
            assert skips == ([True, True] if c == 128 else []), skips
            # stale kept planes: the fp32 kernel's result, bit for bit, and no planes launch in that backward
            for why in ("gen", "ver", "snake"):
                n = len(calls)
                st = _unit(ops, dev, c, t, dil, stale=why)
                assert len(calls) == n + 1, (why, "only the first, valid pass may use the planes kernel")
                for a, b in zip(st, ref):
                    assert torch.equal(a, b), why
            n = len(calls)
            rec = _unit(ops, dev, c, t, dil, recompute=True)
            assert len(calls) == n, "recompute=True must keep the fp32 path"
        finally:
            del ops.conv_wgrad7_planes
            del ops.ru_k1_bwd
        for a, b in zip(on, skip):
            assert torch.equal(a, b), "ru_k1_bwd_skip_dh changes a gradient"
        for i, (a, b) in enumerate(zip(on, ref)):
            if i == 3:      # dW1: another summation order over the same bf16 products.  2e-6: both kernels sit at 4.4e-6 ... 4.5e-6 of the float64
                            # result (the kernel tests above, which hold the measured 2x bound); two results that close to a third differ by
                            # less than half of it when their errors share the bf16 split, which is all but the fp32 summation order
                assert _rel(a, b.double().cpu()) < 2e-6, _rel(a, b.double().cpu())
            else:           # nothing else reads the weight gradient
                assert torch.equal(a, b), i
        for a, b in zip(rec, ref):
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)
    finally:
        ops.wgrad7_planes, ops.ru_k1_bwd_skip_dh = saved


def test_residual_unit_planes_sim(emu):
    _unit_case(emu, "cpu", 128, 128, 3)        # C = 128: sat_ru_k1_bwd emits dh's planes (and may skip dh)


def test_residual_unit_planes_c256_sim(emu):
    _unit_case(emu, "cpu", 256, 128, 9)        # C = 256: the generic k1 data-gradient emits them


def test_residual_unit_outside_contract_sim(emu):
    """C = 64 is not served by the plane-fed k7 convs: nothing is kept, the fp32 kernel runs, the knob changes nothing."""
    saved = emu.wgrad7_planes
    try:
        emu.wgrad7_planes = False
        ref = _unit(emu, "cpu", 64, 192, 9)
        emu.wgrad7_planes = True
        on = _unit(emu, "cpu", 64, 192, 9)
    finally:
        emu.wgrad7_planes = saved
    for a, b in zip(on, ref):
        assert torch.equal(a, b)


def test_residual_unit_planes_budget_spent_sim(emu):
    """wgrad7_planes_budget_gib = 0: no conv comes to own a plane buffer — nothing is kept, the planes kernel never runs and every
    gradient is the fp32 kernel's, bit for bit."""
    saved = (emu.wgrad7_planes, emu.wgrad7_planes_budget_gib)
    calls, kept = [], []
    orig = emu.conv_wgrad7_planes
    emu.conv_wgrad7_planes = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        emu.wgrad7_planes = False
        ref = _unit(emu, "cpu", 128, 128, 3)
        emu.wgrad7_planes, emu.wgrad7_planes_budget_gib = True, 0
        emu.release_owned_planes()
        on = _unit(emu, "cpu", 128, 128, 3, on_forward=lambda y: kept.append(y.grad_fn.k7_planes))
    finally:
        del emu.conv_wgrad7_planes
        emu.wgrad7_planes, emu.wgrad7_planes_budget_gib = saved
    assert kept == [None, None], kept
    assert not calls, "conv_wgrad7_planes ran although no conv owns a buffer"
    for a, b in zip(on, ref):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("c,t,dil", [(128, 8192, 9), (512, 1024, 1), (256, 2048, 3)])
def test_residual_unit_planes_gpu(hip, c, t, dil):
    _unit_case(hip, "cuda", c, t, dil)


# ---------------------------------------------------------------- a captured generator step
def _graph_config():
    """Two levels of 128 and 256 channels: C = 128 units (sat_ru_k1_bwd, dh skipped) and C = 256 units (generic k1 data-gradient)."""
    enc = {"in_channels": 2, "channels": 128, "c_mults": [1, 2], "strides": [2, 4], "latent_dim": 8, "use_snake": True}
    dec = {"out_channels": 2, "channels": 128, "c_mults": [1, 2], "strides": [2, 4], "latent_dim": 4, "use_snake": True, "final_tanh": False}
    return {"model_type": "autoencoder", "sample_size": 2048, "sample_rate": 16000, "audio_channels": 2,
            "model": {"encoder": {"type": "oobleck", "config": enc}, "decoder": {"type": "oobleck", "config": dec},
                      "bottleneck": {"type": "vae"}, "latent_dim": 4, "downsampling_ratio": 8, "io_channels": 2},
            "training": {"learning_rate": 1e-3, "use_ema": True,
                         "optimizer_configs": {"autoencoder": {
                             "optimizer": {"type": "AdamW", "config": {"betas": [0.8, 0.99], "lr": 1e-3, "weight_decay": 1e-3, "eps": 1e-3}},
                             "scheduler": {"type": "InverseLR", "config": {"inv_gamma": 200000, "power": 0.5, "warmup": 0.9}}}},
                         "loss_configs": {"spectral": {"type": "mrstft", "config": {"fft_sizes": [256, 128, 64, 32], "hop_sizes": [64, 32, 16, 8],
                                                                                    "win_lengths": [256, 128, 64, 32], "perceptual_weighting": True},
                                                       "weights": {"mrstft": 1.0}},
                                          "bottleneck": {"type": "kl", "weights": {"kl": 1e-4}}}}}


@pytest.mark.gpu
def test_graphed_generator_step_with_planes_equals_eager_gpu(hip):
    """One eager warm-up step (the k7 convs come to own their plane buffers), the second step captured and replayed, the third replayed:
    losses and parameters equal three eager steps bit for bit, and the captured backward contains the planes kernel (the capture found
    the buffers the warm-up created, on its own stream, and created none)."""
    from stable_audio_tools_amd import ops as ops_mod
    from stable_audio_tools_amd.autoencoders import create_autoencoder_from_config
    from stable_audio_tools_amd.training import AutoencoderTrainStep, GraphedTrainStep
    ops = ops_mod.get_ops()
    assert ops.wgrad7_planes and ops.ru_k1_bwd_skip_dh
    cfg = _graph_config()
    g = torch.Generator().manual_seed(11)
    batches = [(0.3 * torch.randn(2, 2, 2048, generator=g), torch.randn(2, 4, 256, generator=g)) for _ in range(3)]
    torch.manual_seed(5)
    init = {k: v.clone() for k, v in create_autoencoder_from_config(cfg).state_dict().items()}
    seen = []
    orig = ops.conv_wgrad7_planes
    ops.conv_wgrad7_planes = lambda *a, **k: (seen.append(torch.cuda.is_current_stream_capturing()), orig(*a, **k))[1]

    def run(graphed):
        model = create_autoencoder_from_config(cfg)
        model.load_state_dict(init)
        model = model.to("cuda")
        stepper = AutoencoderTrainStep(model, cfg)
        step = GraphedTrainStep(stepper, eager_steps=1) if graphed else stepper
        losses = []
        for a, n in batches:
            out = step(a.to("cuda"), noise=n.to("cuda"))
            losses.append({k: float(v) for k, v in out.items()})
        torch.cuda.synchronize()
        extra = (step.replays, dict(step.fallback), len(step.graphs)) if graphed else None
        return stepper.flat.data.clone(), stepper.opt.ema.clone(), losses, extra

    try:
        pe, ee, le, _ = run(False)
        n_eager = len(seen)
        assert n_eager > 0 and not any(seen), "the eager steps must reach the planes kernel"
        ops.release_owned_planes()                      # the graphed run starts where a fresh process does
        pg, eg, lg, (replays, fallback, ngraphs) = run(True)
    finally:
        del ops.conv_wgrad7_planes
    assert not fallback, fallback
    assert replays == 2 and ngraphs == 1
    assert any(seen[n_eager:]), "the captured step did not contain the planes kernel"
    print("graphed vs eager: max |dparam|", float((pe - pg).abs().max()), "max |dema|", float((ee - eg).abs().max()), le, lg)
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(ee, eg), (float((pe - pg).abs().max()), float((ee - eg).abs().max()))
