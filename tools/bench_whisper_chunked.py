#!/usr/bin/env python3
"""Chunked Whisper long-form decoding beside the sequential loop, and the merge launch alone (not bench.py: a side
measurement).  whisper-medium shape, seeded random weights, one synthetic recording of `--seconds` of noise.

  long form   `transcribe_whisper(long_form="chunked")` (30 s chunks, default stride, batch 16 and 64) beside
              `transcribe_whisper()` - the sequential window loop - on the same recording and max_length; a host clock
              around calls that end in a copy back; medians of `--iters` runs after one warm-up run each, the three
              variants alternating.  Random weights seldom emit EOS, so every window and every chunk decodes to
              max_length; the number of windows the sequential loop takes depends on where the model puts its last
              timestamp, so it is counted and printed (a trained checkpoint closes segments near the window's end and
              takes about seconds / 28 windows; the loop is then `windows` decodes of one row each)
  merge       ca_overlap_merge on buffers uploaded once, HIP-event median over `--launches` launches: one group of 180
              rows of about 200 tokens (an hour of audio), and 64 groups of 30 rows (a batch of 10-minute recordings);
              the second also through the float64 restatement (tests/whisper_chunk_ref.py) on this machine's CPU, whose
              result the kernel's must equal
One JSON line at the end; the partial results are printed as they come.

    python tools/bench_whisper_chunked.py [--iters 5] [--seconds 600] [--max-length 64] [--skip-sequential]
"""
import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import whisper_chunk_ref as C  # noqa: E402
from coral_amd import ops  # noqa: E402


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


def stream_groups(rng, n_groups, n_rows, length, vocab=5000, noise=0.05):
    """Rows cut from one token stream per group, neighbours overlapping by about a third of a row (two strides of a sixth)."""
    groups = []
    for _ in range(n_groups):
        step = length - length // 3
        stream = [rng.randrange(vocab) for _ in range(n_rows * step + length)]
        groups.append([[t if rng.random() > noise else rng.randrange(vocab) for t in stream[j * step:j * step + length + rng.randint(-8, 8)]]
                       for j in range(n_rows)])
    return groups


def merge_plan(groups, dev):
    rows = [r for g in groups for r in g]
    ld = max(len(r) for r in rows)
    table = np.zeros((len(rows), ld), dtype=np.int32)
    for i, r in enumerate(rows):
        table[i, :len(r)] = r
    return torch.from_numpy(table).to(dev), [len(r) for r in rows], np.concatenate([[0], np.cumsum([len(g) for g in groups])])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--max-length", type=int, default=64)
    ap.add_argument("--model", default="openai/whisper-medium")
    ap.add_argument("--skip-sequential", action="store_true")
    ap.add_argument("--skip-long-form", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_chunked.py measures on the GPU; none is visible")
    dev = "cuda:0"
    out = dict(model=args.model, seconds=args.seconds, max_length=args.max_length, iters=args.iters)

    # ---- the merge launch alone ----
    rng = random.Random(1)
    for name, groups in (("merge_1x180", stream_groups(rng, 1, 180, 200)), ("merge_64x30", stream_groups(rng, 64, 30, 200))):
        ids, row_len, group_off = merge_plan(groups, dev)
        res = ops.overlap_merge(ids, row_len, group_off)
        got = ops.overlap_merge_read(res)[0]
        if name == "merge_64x30":
            t0 = time.perf_counter()
            want = [C.merge_sequences(g)[0] for g in groups]
            out["restatement_64x30_cpu_s"] = round(time.perf_counter() - t0, 3)
            assert got == want, "the kernel's merge differs from the restatement"
        else:
            assert got == [C.merge_sequences(groups[0])[0]], "the kernel's merge differs from the restatement"
        # every launch of the wrapper uploads its offsets and allocates its output: the launch alone is timed on those of `res`
        args_dev = torch.from_numpy(np.concatenate([np.zeros(len(row_len)), row_len, group_off, res["out_off"]]).astype(np.int32)).to(dev)
        rows, G, buf, cap = len(row_len), len(group_off) - 1, res["buf"], res["cap"]
        lib, stream, pa, pb = ops.lib(), torch.cuda.current_stream().cuda_stream, args_dev.data_ptr(), buf.data_ptr()

        def launch():
            rc = lib.ca_overlap_merge(ids.data_ptr(), ids.shape[1], pa, pa + 4 * rows, rows, max(row_len), None, 0,
                                      pa + 8 * rows, pa + 8 * rows + 4 * (G + 1), G, pb, cap, pb + 4 * cap, None, stream)
            assert rc == 0

        out[name + "_us"] = tuple(round(1e3 * v, 1) for v in event_median_ms(launch, args.launches))
        out[name + "_tokens"] = int(sum(row_len))
        print(name, out[name + "_us"], "us (median, min, max);", out[name + "_tokens"], "tokens in", G, "groups", flush=True)
    if "restatement_64x30_cpu_s" in out:
        out["restatement_over_kernel_64x30"] = round(out["restatement_64x30_cpu_s"] * 1e6 / out["merge_64x30_us"][0])
        print("restatement on the CPU, 64 x 30:", out["restatement_64x30_cpu_s"], "s", flush=True)

    # ---- long form ----
    if not args.skip_long_form:
        from coral_amd.evaluate import transcribe_whisper
        from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

        model = WhisperForConditionalGeneration.from_pretrained(args.model, device=dev).eval()
        proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
        g = np.random.RandomState(3)
        wave = np.clip(0.1 * g.randn(int(args.seconds * 16000)), -1, 1).astype(np.float32)
        calls = []
        real = model.generate

        def counted(feats, *a, **kw):
            calls.append(int(feats.shape[0]))
            return real(feats, *a, **kw)

        model.generate = counted
        variants = {"chunked_b16": lambda: transcribe_whisper(model, proc, [wave], 16, args.max_length, long_form="chunked"),
                    "chunked_b64": lambda: transcribe_whisper(model, proc, [wave], 64, args.max_length, long_form="chunked")}
        if not args.skip_sequential:
            variants["sequential"] = lambda: transcribe_whisper(model, proc, [wave], 16, args.max_length)
        times = {k: [] for k in variants}
        for it in range(args.iters + 1):  # (run 0 warms every shape up and is not counted)
            for name, fn in variants.items():
                calls.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if it:
                    times[name].append(dt)
                out[name + "_generate_calls"], out[name + "_rows_decoded"] = len(calls), sum(calls)
                print(f"run {it} {name}: {dt:.3f} s, {len(calls)} generate calls, {sum(calls)} rows", flush=True)
        for name, ts in times.items():
            out[name + "_s"] = (round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4))
            out[name + "_audio_s_per_s"] = round(args.seconds / statistics.median(ts), 1)
        if "sequential" in times:
            for name in ("chunked_b16", "chunked_b64"):
                out["sequential_over_" + name] = round(out["sequential_s"][0] / out[name + "_s"][0], 2)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
