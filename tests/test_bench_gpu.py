"""`python bench.py --gpus N` as the driver calls it without a launcher: the parent process starts the N ranks itself
(the reference's one-command launch is `accelerate launch ... finetune_asr_model.py`,
R/src/scripts/finetune_asr_model.py:9-12) and relays their exit code; the JSON line reports the real number of ranks
and the gradient wire format (fp32 = what the reference's DDP reduces).  The GPU box has one device, so the two ranks
share it through the gloo backend (CA_BENCH_SHARE_GPU=1): everything but the RCCL transport is the production path."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("zero", [None, 0, 2])
def test_bench_spawns_its_ranks_and_reports_them(zero):
    """zero = None: the N > 1 --full run - the headline is BASELINE configs[2]'s replicated DDP (gradient all-reduce) and the
    sharded optimiser (the reference's `--zero-stage 2` launch) follows in the same run as config.also_zero2; 0 / 2: one
    of them alone."""
    env = dict(os.environ, CA_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--backend", "gloo", "--model", "wav2vec2-small",
           "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--check-replicas", "--full"] + ([] if zero is None else ["--zero-stage", str(zero)])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    main = [d for d in lines if "metric" in d]
    assert len(main) == 1, r.stdout[-1500:]              # rank 0 prints ONE line
    d = main[0]
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["backend"] == "gloo" and d["grad_wire"] == "fp32" and d["scaling"] == "weak"
    assert d["rccl_ranks"] == 1  # (no RCCL rank ran: the field counts ranks of backend "nccl" only)
    assert d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert ("sharded optimiser" in d["config"]["workload"]) == (zero == 2)
    assert ("gradient all-reduce" in d["config"]["workload"]) == (zero != 2)
    z2 = d["config"].get("also_zero2")
    assert (z2 is not None) == (zero is None)
    if z2 is not None:
        assert z2["value"] > 0 and z2["zero_stage_in_effect"] == 2
    spread = [x for x in lines if "replica_param_spread" in x]
    assert len(spread) == (2 if zero is None else 1)
    for sp_line in spread:  # DDP invariant: identical replicas - parameters, bf16 copy AND the AdamW moments
        assert sp_line["replica_param_spread"] == 0.0
        sp = sp_line["replica_spreads"]
        assert set(sp) >= {"p32", "p16", "m", "v"} and all(x == 0.0 for x in sp.values()), sp
    assert ("p16_vs_master" in spread[-1]["replica_spreads"]) == (zero != 0)


def test_the_headline_line_survives_a_secondary_run_that_does_not_finish():
    """N > 1 --full: the zero_stage 2 run follows the headline in the same process group.  If it does not finish
    (CA_BENCH_ZERO2_TIMEOUT; here: at once) rank 0 still prints the ONE line, with the headline and an error field."""
    env = dict(os.environ, CA_BENCH_SHARE_GPU="1", CA_BENCH_ZERO2_TIMEOUT="0.001")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--backend", "gloo", "--model", "wav2vec2-small",
           "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    main = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "metric" in l]
    assert len(main) == 1, r.stdout[-1500:] + r.stderr[-1500:]
    assert main[0]["value"] > 0 and main[0]["ranks"] == 2
    assert "error" in main[0]["config"]["also_zero2"]


def test_two_ranks_at_the_full_xlsr_2b_shape_with_the_sharded_optimizer():
    """BASELINE configs[2]'s model (wav2vec2-large = XLS-R-2B, 8 x 10 s per rank) on two ranks with the N > 1 default
    (reduce-scatter of the 48 layers' 44 M-element matrix parts, AdamW on 1/2, bf16 all-gather): the real bucket
    sizes, offsets and slice alignments; after three steps both ranks hold the same bf16 compute copy bit for bit.
    (Two processes share the one GPU over gloo: ~82 GB of device memory, ~40 s.)"""
    env = dict(os.environ, CA_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-also", "--no-fwd-bwd", "--check-replicas", "--zero-stage", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    d = [x for x in lines if "metric" in x][0]
    assert d["n_gpus"] == 2 and "sharded optimiser" in d["config"]["workload"] and "wav2vec2-large" in d["metric"]
    assert d["config"]["loss"] > 0 and d["config"]["loss"] == d["config"]["loss"]  # finite
    spread = [x for x in lines if "replica_param_spread" in x]
    assert spread and spread[0]["replica_param_spread"] == 0.0


def test_bench_refuses_more_ranks_than_devices():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("CA_BENCH_SHARE_GPU", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "64"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode != 0 and "only" in r.stderr   # never a silent 1-GPU run


def test_bench_line_of_a_single_rank_and_the_one_rank_rccl_diagnostic():
    """The N = 1 line: every field the contract names, the forward+backward-only time beside the whole step, the
    roofline object; and the labelled diagnostic that runs the N > 1 exchange path over an RCCL group of one rank."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    base = [sys.executable, str(ROOT / "bench.py"), "--model", "wav2vec2-small", "--steps", "2", "--warmup", "1",
            "--no-cpu-baseline", "--full"]
    r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["grad_wire"] is None and d["vs_baseline"] is None
    fb = d["config"]["fwd_bwd"]
    assert 0 < fb["ms_per_step"] < d["ms_per_step"] and fb["value"] > d["value"]   # the optimiser is inside `value`
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    r = subprocess.run(base + ["--one-rank-exchange", "--no-fwd-bwd"], env=env, capture_output=True, text=True,
                       timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    e = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert "DIAGNOSTIC" in e["config"]["workload"] and e["n_gpus"] == 1 and e["value"] > 0
    assert abs(e["config"]["loss"] - d["config"]["loss"]) <= 1e-3 * abs(d["config"]["loss"])  # identity exchange


def test_a_plain_run_times_the_headline_alone_and_dumps_what_its_last_step_computed(tmp_path):
    """Without --full the line carries the headline only (no roofline, no fwd_bwd, no secondary workloads, no CPU
    baseline); --dump-outputs writes the last timed step's loss, logits and gradient norm and a seeded sample of the
    updated fp32 master weights, float32 / float64, 64 MB at most.  Two runs with the same arguments see the same inputs:
    their outputs agree.  A run with more --steps starts its timed steps from the same weights and moves them further
    (the learning rate warms up linearly: 5 timed steps after one warm-up step take 1 + ... + 5 = 15 learning-rate units,
    3 take 6)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    runs = []
    for k, steps in enumerate((3, 3, 5)):
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--model", "wav2vec2-small", "--steps", str(steps),
               "--warmup", "1", "--dump-outputs", str(tmp_path / f"run{k}")]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-1500:]
        d = lines[0]
        for k_ in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k_ in d, k_
        assert d["steps"] == steps and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "bf16"
        assert "roofline" not in d and "cpu_baseline" not in d
        assert not any(k_ == "fwd_bwd" or k_.startswith("also") for k_ in d["config"])
        out = {f.stem: np.load(f) for f in (tmp_path / f"run{k}").glob("*.npy")}
        assert set(out) == {"loss", "logits", "grad_norm", "params_sample", "params_update_sample"}, sorted(out)
        assert all(a.dtype in (np.float32, np.float64) for a in out.values())
        assert sum(a.nbytes for a in out.values()) <= 64 << 20
        assert out["logits"].shape[0] == 8 and np.isfinite(out["logits"]).all()
        assert abs(float(out["loss"]) - d["config"]["loss"]) <= 1e-3 * abs(d["config"]["loss"]) + 1e-3
        assert np.isfinite(out["grad_norm"]).all() and float(out["grad_norm"][0]) > 0
        assert np.abs(out["params_update_sample"]).max() > 0   # the timed steps moved the weights
        runs.append(out)
    a, b, c = runs
    # same arguments: the same outputs, the final weights and the clipped-by norm included
    np.testing.assert_allclose(a["params_sample"], b["params_sample"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["params_update_sample"], b["params_update_sample"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a["grad_norm"], b["grad_norm"], rtol=1e-4)
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-4)
    np.testing.assert_allclose(a["logits"], b["logits"], rtol=1e-3, atol=1e-3)
    # --steps 5: the same weights before the timed steps (same warm-up), a larger update after them
    np.testing.assert_allclose(a["params_sample"] - a["params_update_sample"], c["params_sample"] - c["params_update_sample"],
                               rtol=0, atol=1e-6)
    ratio = float(np.abs(c["params_update_sample"]).mean() / np.abs(a["params_update_sample"]).mean())
    assert 1.5 < ratio < 4.0, ratio
