"""bench.py's command line: a plain run is the headline alone, `--full` brings back every other leg of the line."""
import json
import os
import subprocess
import sys
import time

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# keys of the line that only a `--full` run may carry (top level / under `config`)
FULL_ONLY_TOP = ("cpu_baseline", "parity", "secondary", "long_context", "dit_train", "real_step_samples_per_s", "real_step_ms",
                 "real_step_dominant_discriminator_kernel")
FULL_ONLY_CONFIG = ("batch_sweep", "real_step")
# a plain run's budget outside its warm-up and timed steps: whole process, start to exit, less (steps + warmup) x ms_per_step
PLAIN_OVERHEAD_BOUND_S = 30.0


def _parse(argv):
    import bench
    return bench.parse(argv)


def test_full_is_off_by_default_and_plain_run_has_no_extra_leg():
    import bench
    args = _parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert args.full is False
    assert (args.steps, args.warmup, args.gpus, args.workload) == (3, 1, 1, "vae_train")
    for leg in bench.FULL_ONLY_LEGS:
        assert getattr(args, "no_" + leg) is True, leg
    assert args.no_graph is False            # the HIP-graph replay of the steps is part of the headline (`value` = the faster mode)
    assert args.dump_outputs is None


def test_full_runs_every_leg_unless_dropped_one_by_one():
    import bench
    args = _parse(["--full"])
    assert args.full is True
    for leg in bench.FULL_ONLY_LEGS:
        assert getattr(args, "no_" + leg) is False, leg
    args = _parse(["--full", "--no-parity", "--no-dit-train"])
    dropped = {leg for leg in bench.FULL_ONLY_LEGS if getattr(args, "no_" + leg)}
    assert dropped == {"parity", "dit_train"}


@pytest.mark.parametrize("workload", ["dit_sample", "dit_train", "long_context"])
def test_other_workloads_keep_their_cpu_legs_behind_full(workload):
    assert _parse(["--workload", workload]).no_cpu_baseline is True
    assert _parse(["--workload", workload, "--full"]).no_cpu_baseline is False
    assert _parse(["--workload", workload, "--full", "--no-cpu-baseline"]).no_cpu_baseline is True


@pytest.mark.gpu
def test_plain_run_is_lean_gpu(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` in a fresh process: one JSON line with the headline fields, the dumped arrays of both
    launch modes, none of the `--full` legs, and at most 30 s spent outside the (N + W) steps."""
    steps, warmup = 2, 1
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(_REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(dump)]
    t0 = time.perf_counter()
    res = subprocess.run(cmd, cwd=_REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["metric"] == "train-step samples/sec (47s@44.1kHz)" and line["unit"] == "samples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32(bf16x3)"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (steps, warmup, 1)
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 1.0) < 1e-9      # batch 1: value = 1 / step time
    assert line["config"]["full"] is False
    assert set(line["config"]["launch"]["ms_per_step"]) == {"eager", "hip_graph"}
    assert line["roofline"]["kernel"]
    for k in FULL_ONLY_TOP:
        assert k not in line, k
    for k in FULL_ONLY_CONFIG:
        assert k not in line["config"], k
    files = line["config"]["dump_outputs"]["files"]
    assert "eager_params.npy" in files and "hip_graph_params.npy" in files and "eager_loss.npy" in files
    assert sorted(os.listdir(dump)) == files
    overhead = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    print(f"plain run: wall {wall:.1f} s, ms_per_step {line['ms_per_step']:.1f}, outside the steps {overhead:.1f} s")
    assert overhead <= PLAIN_OVERHEAD_BOUND_S, (wall, line["ms_per_step"], overhead)
