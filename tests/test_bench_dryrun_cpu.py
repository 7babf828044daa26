"""`python bench.py --gpus N` without GPUs: launcher, sharded step, timing, rc and the one-JSON-line contract (gloo, toy
model, kernel shims: tests/bench_dryrun.py).  The driver runs the same code with RCCL on 8 MI355X at round end."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def run(gpus, env_extra=None, timeout=600, extra=("--full",), steps=1):
    env = dict(os.environ, **(env_extra or {}))
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, str(ROOT / "tests" / "bench_dryrun.py"), "--gpus", str(gpus), "--steps",
                           str(steps), "--warmup", "0", "--frames", "12", *extra], capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=str(ROOT))


def result_line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    # the collective library may print its own banner through C stdio (gloo here, RCCL with GPUs: bench.py drains
    # it on every rank before the last barrier): exactly ONE line is a JSON object, and it is the LAST line of stdout
    js = [l for l in lines if l.lstrip().startswith("{")]
    assert len(js) == 1 and lines[-1] == js[0], lines
    return json.loads(js[0])


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_job_prints_exactly_one_json_line(gpus):
    d = result_line(run(gpus))
    assert d["n_gpus"] == gpus and d["steps"] == 1 and d["unit"] == "frames/s" and d["value"] > 0
    assert d["metric"].startswith("video frames/sec fwd")
    assert d["config"]["parallelism"] == ("single GPU" if gpus == 1 else "sequence-sharded x2 (RCCL)")
    for key in ("ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "roofline", "rooflines"):
        assert key in d
    # every HBM companion of the scan is event-timed inside the timed step
    kinds = " | ".join(e["kernel"] for e in d["rooflines"])
    for name in ("ssd_scan", "conv1d_xbc", "rmsnorm_gated", "Mamba mixer trio", "rmsnorm_kernel", "layernorm"):
        assert name in kinds, (name, kinds)


def test_bench_job_propagates_a_failing_rank():
    r = run(2, {"TV_BENCH_DRYRUN_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.strip().startswith("{")], "a failed job must not print a result line"


def test_plain_bench_times_the_steps_only():
    """Without --full the line carries the headline figure and nothing that needs timers or runs of its own."""
    d = result_line(run(1, extra=(), steps=2))
    assert d["steps"] == 2 and d["warmup"] == 0 and d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype", "scaling", "vs_baseline", "data", "config"):
        assert key in d
    for key in ("roofline", "rooflines", "timed_ms_per_step", "cpu_baseline"):
        assert key not in d


def test_dump_outputs_is_the_same_from_run_to_run(tmp_path):
    """--dump-outputs writes the last timed step's logits as float32; the same arguments give the same arrays, with
    and without --full."""
    import numpy as np
    outs = []
    for i, extra in enumerate([(), (), ("--full",)]):
        d = tmp_path / f"run{i}"
        result_line(run(1, extra=("--dump-outputs", str(d), *extra)))
        assert sorted(p.name for p in d.iterdir()) == ["logits.npy"]
        outs.append(np.load(d / "logits.npy"))
    a = outs[0]
    assert a.dtype == np.float32 and a.ndim == 3 and a.shape[:2] == (1, 1) and np.isfinite(a).all()
    for b in outs[1:]:
        assert b.shape == a.shape and np.array_equal(a, b)
