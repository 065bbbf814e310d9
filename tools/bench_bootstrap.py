#!/usr/bin/env python3
"""Time of the bootstrap kernel (ca_bootstrap_sums) and of `score_table(bootstrap=...)` around it (not bench.py: a side
measurement).  The workload is a score table: `--examples` examples of synthetic counts at about 150 characters each,
three categories of 3 x 2 x 10 values, `--resamples` replicates of every kept combination and of the whole set.

  kernel      HIP-event median over `--iters` launches after warm-up, on buffers uploaded once; draws per second from it
  end to end  `score_table(bootstrap=...)`: the table, one upload, the launch, the copy back and the float64 figures, by a
              host clock (the call ends in the copy back, which synchronises)
  baseline    the same groups and replicates on this machine's CPU in vectorised NumPy: `Generator.integers` for the
              draws and fancy-index sums (its own generator, so other draws: a timing baseline, not the restatement)
The kernel's sums are checked against tests/bootstrap_ref.py on the first two groups and on the whole set.  One JSON
line at the end.

    python tools/bench_bootstrap.py [--iters 20] [--examples 10000] [--resamples 1000]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bootstrap_ref  # noqa: E402
from coral_amd import _lib, error_rates  # noqa: E402


def event_median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def synthetic_counts(rng, n, rate):
    length = rng.randint(120, 181, n)
    s, d, i = (rng.binomial(length, rate / 3) for _ in range(3))
    return np.stack([length - s - d, s, d, i], axis=1).astype(np.int64)


def numpy_baseline(rows, groups, R, seed):
    gen = np.random.default_rng(seed)
    out = np.empty((len(groups), R, rows.shape[1]), dtype=np.int64)
    for g, members in enumerate(groups):
        n = len(members)
        step = max(1, (1 << 21) // n)
        for r0 in range(0, R, step):
            k = gen.integers(0, n, size=(min(R, r0 + step) - r0, n))
            out[g, r0:r0 + len(k)] = rows[members[k]].sum(axis=1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--examples", type=int, default=10_000)
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap.py measures on the GPU; none is visible")
    rng = np.random.RandomState(0)
    n, R = args.examples, args.resamples
    cats = ["age_group", "gender", "dialect"]
    rows = [dict(age_group=int(rng.randint(3)), gender=int(rng.randint(2)), dialect=int(rng.randint(10))) for _ in range(n)]
    cc, wc = synthetic_counts(rng, n, 0.1), synthetic_counts(rng, n, 0.3)
    plain = error_rates.score_table(rows, cats, cc, wc)
    system = error_rates._system_rows(cc, wc, True)
    groups = [np.flatnonzero([all(rec[c] is None or row[c] == rec[c] for c in cats) for row in rows]) for rec in plain]
    G, draws = len(groups), R * int(sum(len(g) for g in groups))
    out = dict(examples=n, resamples=R, groups=G, draws=draws, iters=args.iters)

    # the kernel alone, on buffers uploaded once
    goff = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int64)
    members = np.concatenate(groups).astype(np.int32)
    d_vals, d_mem, d_off = (torch.from_numpy(a).cuda() for a in (system.astype(np.int32), members, goff))
    d_sums = torch.empty(G, R, 4, dtype=torch.int64, device="cuda")
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.ca_bootstrap_sums(d_vals.data_ptr(), n, 4, d_mem.data_ptr(), len(members), d_off.data_ptr(), G, R,
                                         args.seed, d_sums.data_ptr(), stream), "ca_bootstrap_sums")

    launch()
    got = d_sums.cpu().numpy()
    checked = (0, 1, G - 1)
    want = bootstrap_ref.sums(system, members, goff, R, args.seed, only=checked)
    for g in checked:
        assert np.array_equal(got[g], want[g]), f"group {g} differs from the restatement"
    out["kernel_ms"] = event_median_ms(launch, args.iters)
    out["draws_per_s"] = draws / (out["kernel_ms"][0] * 1e-3)

    # end to end
    boot = dict(n_resamples=R, seed=args.seed, device="cuda")
    e2e = []
    for _ in range(5):
        t0 = time.perf_counter()
        table = error_rates.score_table(rows, cats, cc, wc, bootstrap=boot)
        e2e.append(time.perf_counter() - t0)
    out["score_table_bootstrap_ms"] = tuple(1e3 * v for v in (statistics.median(e2e[1:]), min(e2e[1:]), max(e2e[1:])))
    t0 = time.perf_counter()
    error_rates.score_table(rows, cats, cc, wc)
    out["score_table_plain_ms"] = 1e3 * (time.perf_counter() - t0)
    assert [{k: t[k] for k in p} for t, p in zip(table, plain)] == plain

    # the CPU baseline
    t0 = time.perf_counter()
    base = numpy_baseline(system, groups, R, args.seed)
    out["numpy_baseline_ms"] = 1e3 * (time.perf_counter() - t0)
    out["numpy_over_kernel"] = out["numpy_baseline_ms"] / out["kernel_ms"][0]
    # (other draws, the same estimator: the two standard deviations of the whole set's CER agree within resampling noise)
    ours = error_rates.intervals_from_sums(got[-1][:, 0], got[-1][:, 1], plain[-1]["cer"])
    theirs = error_rates.intervals_from_sums(base[-1][:, 0], base[-1][:, 1], plain[-1]["cer"])
    out["whole_set_cer_std_kernel"], out["whole_set_cer_std_numpy"] = ours["std"], theirs["std"]
    assert abs(ours["std"] / theirs["std"] - 1) <= 5 * (2 / (2 * (R - 1))) ** 0.5, (ours["std"], theirs["std"])

    for k, v in out.items():
        if isinstance(v, tuple):
            print(f"{k:32s} median {v[0]:10.3f} ms   min {v[1]:10.3f}   max {v[2]:10.3f}")
            out[k] = round(v[0], 4)
        else:
            print(f"{k:32s} {v}")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
