#!/usr/bin/env python3
"""Time of the alignment-count kernel (ca_edit_counts) and of coral_amd/error_rates.py around it (not bench.py: a side
measurement).  Kernel times are HIP-event medians over `--iters` launches after warm-up; end-to-end and host times are a
host clock around work that ends in a device synchronise (the copy of the counts back).

  (a) a batch of clips: `--pairs` pairs of about 150 characters with 10 % random edits - the kernel alone, `error_counts`
      end to end (tokenisation, packing, one upload, the kernel, the copy back), and coral_amd.metrics.cer on the same
      pairs on this machine's CPU (`--host-pairs` of them, default all; the per-pair time is what is compared);
  (b) one pair of `--long` x `--long` characters on the workgroup route, in cells per second;
  (c) 16 short pairs on the wave route; the same 15 pairs with one `--long`-character pair, launched largest first and
      with the long pair last; and the batch of (a) with that pair, both ways.
Every timed result is checked: (a) against the host metric's total distance, the others against the invariants of the
counts and the number of edits made.  One JSON line at the end.

    python tools/bench_error_rates.py [--iters 20] [--pairs 10000] [--long 60000]
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

from coral_amd import _lib, error_rates, metrics, ops  # noqa: E402

ALPHABET = list("abcdefghijklmnopqrstuvwxyzæøå") + [" "] * 6


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


def edited(rng, tokens, share=0.10):
    """tokens with share * len random edits (a third each: substitution, deletion, insertion).  -> (array, edits)"""
    t = tokens.tolist()
    k = max(1, int(len(t) * share))
    for _ in range(k):
        op, at = rng.randint(3), rng.randint(len(t))
        if op == 0:
            t[at] = int(rng.randint(len(ALPHABET)))
        elif op == 1:
            del t[at]
        else:
            t.insert(at, int(rng.randint(len(ALPHABET))))
    return np.asarray(t, dtype=np.int32), k


def text(tokens):
    return "".join(ALPHABET[i] for i in tokens)


def plan_of(refs, hyps, route=0, order=None):
    ref_off = np.concatenate(([0], np.cumsum([len(r) for r in refs])))
    hyp_off = np.concatenate(([0], np.cumsum([len(h) for h in hyps])))
    return ops.edit_counts_plan(np.concatenate(refs), ref_off, np.concatenate(hyps), hyp_off, "cuda:0", route, order)


def check_invariants(counts, refs, hyps, edits):
    c = counts.cpu().numpy().astype(np.int64)
    n, m = np.array([len(r) for r in refs]), np.array([len(h) for h in hyps])
    assert (c >= 0).all() and (c[:, 0] + c[:, 1] + c[:, 2] == n).all() and (c[:, 0] + c[:, 1] + c[:, 3] == m).all()
    assert (c[:, 1] + c[:, 2] + c[:, 3] <= np.asarray(edits)).all()
    return c


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--host-pairs", type=int, default=0, help="pairs the host metric is timed on (0 = all)")
    ap.add_argument("--long", type=int, default=60_000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_error_rates.py measures on the GPU; none is visible")
    rng = np.random.RandomState(0)
    out = dict(pairs=args.pairs, long=args.long, iters=args.iters, wave_max=_lib.EDIT_WAVE_MAX, panel=_lib.EDIT_PANEL)

    # (a) a batch of clips
    refs = [rng.randint(0, len(ALPHABET), rng.randint(120, 181)).astype(np.int32) for _ in range(args.pairs)]
    pairs = [edited(rng, r) for r in refs]
    hyps, edits = [p[0] for p in pairs], [p[1] for p in pairs]
    plan = plan_of(refs, hyps)
    check_invariants(ops.edit_counts_launch(plan), refs, hyps, edits)
    cells = int(sum(len(r) * len(h) for r, h in zip(refs, hyps)))
    out["a_kernel_ms"] = event_median_ms(lambda: ops.edit_counts_launch(plan), args.iters)
    out["a_cells"] = cells
    labels, preds = [text(r) for r in refs], [text(h) for h in hyps]
    # (texts with inner double spaces or outer spaces tokenise differently on the two sides of the comparison; the
    # character counts below are taken on the stripped texts both ways)
    labels, preds = [x.strip() for x in labels], [x.strip() for x in preds]
    e2e = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = error_rates.error_counts(preds, labels, "char", "cuda:0")
        e2e.append(time.perf_counter() - t0)
    out["a_end_to_end_ms"] = tuple(1e3 * v for v in (statistics.median(e2e[1:]), min(e2e[1:]), max(e2e[1:])))
    nh = args.host_pairs or args.pairs
    t0 = time.perf_counter()
    host_cer = metrics.cer(preds[:nh], labels[:nh])
    host_s = time.perf_counter() - t0
    out["a_host_metric_s"] = host_s
    out["a_host_metric_pairs"] = nh
    out["a_host_ms_per_pair"] = 1e3 * host_s / nh
    out["a_device_end_to_end_ms_per_pair"] = out["a_end_to_end_ms"][0] / args.pairs
    out["a_ratio_host_over_device_per_pair"] = out["a_host_ms_per_pair"] / out["a_device_end_to_end_ms_per_pair"]
    assert error_rates._rate(got[:nh], False) == host_cer, (error_rates._rate(got[:nh], False), host_cer)

    # (b) one long pair on the workgroup route
    lr = rng.randint(0, len(ALPHABET), args.long).astype(np.int32)
    lh, ledits = edited(rng, lr)
    lplan = plan_of([lr], [lh], route=2)
    check_invariants(ops.edit_counts_launch(lplan), [lr], [lh], [ledits])
    out["b_long_pair_ms"] = event_median_ms(lambda: ops.edit_counts_launch(lplan), max(3, args.iters // 5), warmup=1)
    out["b_cells"] = len(lr) * len(lh)
    out["b_cells_per_s"] = out["b_cells"] / (out["b_long_pair_ms"][0] * 1e-3)

    # (c) small batches, and what the launch order does
    srefs, shyps, sedits = refs[:16], hyps[:16], edits[:16]
    splan = plan_of(srefs, shyps, route=1)
    check_invariants(ops.edit_counts_launch(splan), srefs, shyps, sedits)
    out["c_16_pairs_wave_ms"] = event_median_ms(lambda: ops.edit_counts_launch(splan), args.iters)
    few = max(3, args.iters // 5)
    for name, base_r, base_h, base_e in (("16", refs[:15], hyps[:15], edits[:15]), ("batch", refs, hyps, edits)):
        mr, mh, me = base_r + [lr], base_h + [lh], base_e + [ledits]
        first = plan_of(mr, mh)  # largest first: the wrapper's own order
        last = plan_of(mr, mh, order=np.arange(len(mr)))  # as given: the long pair at the end
        for tag, p in (("largest_first", first), ("long_pair_last", last)):
            check_invariants(ops.edit_counts_launch(p), mr, mh, me)
            out[f"c_{name}_with_long_pair_{tag}_ms"] = event_median_ms(lambda: ops.edit_counts_launch(p), few, warmup=1)

    for k, v in out.items():
        if isinstance(v, tuple):
            print(f"{k:44s} median {v[0]:10.3f} ms   min {v[1]:10.3f}   max {v[2]:10.3f}")
            out[k] = round(v[0], 4)
        else:
            print(f"{k:44s} {v}")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
