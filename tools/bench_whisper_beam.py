#!/usr/bin/env python3
"""Time per decoded token of Whisper beam search beside greedy decoding (not bench.py: a side measurement).

whisper-medium shape, seeded random weights, 8 clips of noise features.  Prints, per decoded token (wall time of
`WhisperEngine.generate` minus the same call stopped right after the forced prefix, over the tokens in between;
median of `--iters` runs after a warm-up):
  (a) beam search, 8 clips x 5 beams;
  (b) greedy, 8 clips and 40 clips, as a launch sequence (the one-launch kernel switched off): 40 greedy rows are the
      GEMM and self-attention work of 8 x 5 beam rows without the selection;
  (c) the two new launches alone (ca_beam_select, ca_beam_advance) at 8 x 5 over V = 51865, as HIP-event medians.
One JSON line at the end.  `--tokens N` sets the decoded length (default 64).

    python tools/bench_whisper_beam.py [--iters 5] [--tokens 64] [--clips 8] [--beams 5]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from coral_amd import _lib, ops  # noqa: E402
from coral_amd.whisper import CORAL_WHISPER_SHAPES, WhisperEngine, WhisperShape  # noqa: E402
from coral_amd.whisper_setup import prefix_ids  # noqa: E402


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
    return statistics.median(times)


def wall_ms(fn, iters):
    fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--model", default="whisper-medium")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_beam.py measures on the GPU; none is visible")
    dev = "cuda:0"
    shape = WhisperShape(**CORAL_WHISPER_SHAPES[args.model])
    eng = WhisperEngine(shape, dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        eng.store.p32.copy_((torch.randn(eng.store.numel, generator=g) * 0.02).to(dev))
    eng.refresh_compute_weights()
    eng._persistent_off = True  # greedy as a launch sequence: the form the beam step extends
    prefix = prefix_ids(shape)
    P, B, k = len(prefix), args.clips, args.beams
    short, long = P + 3, P + 3 + args.tokens
    # random weights seldom emit EOS, and a finished greedy row keeps decoding pad anyway; EOS is suppressed so that neither
    # search ends early and every run decodes exactly `tokens` tokens between the two lengths
    sup = [shape.eos_token_id]

    def per_token(feats, **kw):
        def run(n):
            return lambda: eng.generate(feats, prefix, n, suppress_tokens=sup, **kw)
        return (wall_ms(run(long), args.iters) - wall_ms(run(short), args.iters)) / args.tokens

    feats = {n: torch.randn(n, shape.num_mel_bins, 3000, generator=g) * 0.5 for n in (B, B * k)}
    res = dict(model=args.model, clips=B, beams=k, tokens=args.tokens)
    res["beam_ms_per_token"] = per_token(feats[B], num_beams=k)
    res["greedy_ms_per_token"] = per_token(feats[B])
    res[f"greedy{B * k}_ms_per_token"] = per_token(feats[B * k])
    res["beam_over_greedy_rows"] = res["beam_ms_per_token"] / res[f"greedy{B * k}_ms_per_token"]

    # the two new launches alone
    V, Vp, R, L = shape.vocab_size, (shape.vocab_size + 7) // 8 * 8, B * k, long
    logits = torch.randn(R, Vp, generator=g).to(dev)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    cs, cp, ct = z(B, 2 * k, dt=torch.float32), z(B, 2 * k), z(B, 2 * k)
    run = z(R, dt=torch.float32)
    ws = z(ops.beam_select_workspace_bytes(B, k, V), dt=torch.uint8)
    supm = z(V, dt=torch.uint8)
    res["select_us"] = 1e3 * event_median_ms(lambda: ops.beam_select(logits, supm, run, B, k, V, Vp, cs, cp, ct, ws), 50)
    t = dict(len_pen=torch.ones(L + 1, device=dev), cand_score=cs, cand_parent=cp, cand_token=ct, run_score=run, tok=z(R),
             pos=z(R), klen=z(R), anc_in=z(R, L), anc_out=z(R, L), ids_in=z(R, L), ids_out=z(R, L),
             fin_score=z(R, dt=torch.float32), fin_len=z(R), fin_seq=z(R), fin_ids=z(R, L), fin_count=z(B), heur=z(B) + 1,
             done=z(B, dt=torch.bool), tr_parent=z(L, B, k), tr_token=z(L, B, k), tr_score=z(L, B, k, dt=torch.float32))
    d = _lib.CaBeamDesc()
    d.B, d.k, d.max_len, d.prompt_len, d.max_length, d.eos_id, d.early_stopping = B, k, L, P, L, shape.eos_token_id, 0

    def advance():
        t["pos"].fill_(L // 2)  # (the launch moves the cursor: put it back so every timed launch copies L / 2 columns)
        for n, v in t.items():
            setattr(d, n, v.data_ptr())
        ops.beam_advance(d)

    fill_ms = event_median_ms(lambda: t["pos"].fill_(L // 2), 50)
    res["advance_us"] = 1e3 * (event_median_ms(advance, 50) - fill_ms)
    print(json.dumps({n: (round(v, 4) if isinstance(v, float) else v) for n, v in res.items()}))
    return res


if __name__ == "__main__":
    main()
