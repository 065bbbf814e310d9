#!/usr/bin/env python3
"""What a left-padded prompt in front of the forced prefix costs the decoder (not bench.py: a side measurement).

whisper-medium shape, seeded random weights, 16 clips of noise features, decoding with timestamps as a graph-replayed
launch sequence.  Mean over `--iters` (20) repetitions between device events after 3 warm-ups:
  (a) per decoded token without a prefix row (the greedy pick of generate(return_timestamps=True) as it was - the figure
      of tools/measure_whisper_fallback.py) and from a `--prefix` (228) token left-padded prefix_rows (rows padded by 0,
      1, 64, ... positions: CaAttnDesc.kstart in every token step, the keys of a step 228 more): the time of
      `WhisperEngine.generate` to P + 3 + tokens minus the same call to P + 3, over the tokens in between;
  (b) the prefill: `decode_step` over the forced prefix alone, over the 228-token rows without a first key (nothing
      padded, kstart=None) and with the rows' first keys (the causal 128-query kernel's km instantiation).
The cross K|V are computed once in front and passed in, so no variant runs the encoder.  One JSON line at the end.

    python tools/measure_whisper_prompt.py [--iters 20] [--tokens 64] [--clips 16] [--prefix 228]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from coral_amd.whisper import CORAL_WHISPER_SHAPES, WhisperEngine, WhisperShape  # noqa: E402
from coral_amd.whisper_setup import prefix_ids  # noqa: E402


def event_mean_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
    return total / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--prefix", type=int, default=228)
    ap.add_argument("--model", default="whisper-medium")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("measure_whisper_prompt.py measures on the GPU; none is visible")
    dev = "cuda:0"
    shape = WhisperShape(**CORAL_WHISPER_SHAPES[args.model])
    eng = WhisperEngine(shape, dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        eng.store.p32.copy_((torch.randn(eng.store.numel, generator=g) * 0.02).to(dev))
    eng.refresh_compute_weights()
    prefix = prefix_ids(shape)[:-1]  # with timestamps: no <|notimestamps|>
    tb = prefix_ids(shape)[-1] + 1
    P, B, Pp = len(prefix), args.clips, args.prefix
    sup = [shape.eos_token_id]  # random weights: no row may end early, every run decodes `tokens` tokens between the lengths
    feats = torch.randn(B, shape.num_mel_bins, 3000, generator=g) * 0.5
    kv = eng.cross_kv(eng.encode(feats))
    kw = dict(suppress_tokens=sup, return_timestamps=True, timestamp_begin=tb, max_initial_timestamp_index=50)
    # left-padded rows: previous text of different lengths in front of the forced prefix
    start = torch.tensor([(0, 1, 64, 100, 163, 7, 200, 31)[b % 8] for b in range(B)], dtype=torch.int32)
    rows = torch.randint(1000, 20000, (B, Pp), generator=g)
    rows[:, Pp - P:] = torch.tensor(prefix)
    rows[torch.arange(Pp)[None, :] < start[:, None]] = shape.pad_token_id

    def per_token(p_len, **extra):
        short, long = p_len + 3, p_len + 3 + args.tokens
        pre = None if extra else prefix
        run = lambda n: (lambda: eng.generate(None, pre, n, cross_kv=kv, **kw, **extra))  # noqa: E731
        return (event_mean_ms(run(long), args.iters) - event_mean_ms(run(short), args.iters)) / args.tokens

    res = dict(model=args.model, clips=B, tokens=args.tokens, iters=args.iters, prefix=Pp)
    res["plain_ms_per_token"] = per_token(P)
    res["prompt_ms_per_token"] = per_token(Pp, prefix_rows=rows, prefix_start=start)
    res["prompt_over_plain"] = res["prompt_ms_per_token"] / res["plain_ms_per_token"]

    def prefill(ids, kstart):
        def run():
            cache = eng.new_decode_cache(B, ids.shape[1] + 1)
            eng.decode_step(ids, kv, cache, kstart=kstart)
        return event_mean_ms(run, args.iters)

    res["prefill_forced_prefix_ms"] = prefill(torch.tensor([prefix] * B), None)
    full = torch.randint(1000, 20000, (B, Pp), generator=g)
    res["prefill_prompt_unmasked_ms"] = prefill(full, None)
    res["prefill_prompt_masked_ms"] = prefill(rows, start.to(dev))
    for k, v in res.items():
        if isinstance(v, float):
            print(f"{k:32s} {v:9.4f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
