"""What word timestamps add to a 16-clip Whisper window batch, in milliseconds.

For each of two shapes - the timestamp fixture's model at its own length (64 tokens) and whisper-medium's shape at
Lw = 224 / F = 1500 - with seeded random weights and 16 clips: the teacher-forced alignment pass, the three cost
launches, the DTW, and beside them the greedy decode of the same batch on the existing path (EOS suppressed, so every row
runs to max_length).  Each figure is the mean over `--reps` repetitions between two device events, after `--warmup`
untimed ones.

usage: python tools/measure_whisper_word.py [--reps 20] [--warmup 3] [--only fixture|medium]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(name, shape_kw, heads, prefix, max_length, ts_begin, reps, warmup, B=16):
    from coral_amd import ops
    from coral_amd.whisper import WhisperEngine, WhisperShape
    from oracle import whisper_ref as w

    dev = "cuda:0"
    eng = WhisperEngine(WhisperShape(**shape_kw), dev)
    eng.load_state_dict(w.synth_params(w.WhisperConfig(**shape_kw), seed=7))
    s = eng.s
    feats = torch.randn(B, s.num_mel_bins, 3000, generator=torch.Generator().manual_seed(3)) * 0.5
    gen = lambda: eng.generate(feats, prefix, max_length, suppress_tokens=[s.eos_token_id], return_timestamps=True,  # noqa: E731
                               timestamp_begin=ts_begin)
    rows = gen()
    assert all(len(r) == max_length for r in rows)
    P, Ltot = len(prefix), max_length
    Lw = Ltot - 1 - P
    d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
    hd = d // H
    kv = eng.cross_kv(eng.encode(feats))
    ids = torch.tensor(rows)[:, :Ltot - 1]
    frames = torch.full((B,), Te, dtype=torch.int32, device=dev)
    q = eng.alignment_queries(ids, kv, heads, P)
    cost_fn = lambda: ops.whisper_align_cost(q, kv, heads, B, Lw, Te, H, hd, 2 * d, Te * 2 * d, frames, Te, hd ** -0.5, 7)  # noqa: E731
    cost = cost_fn()
    out = dict(shape=name, clips=B, Lw=Lw, F=Te, heads=len(heads),
               decode_ms=timed(gen, reps, warmup),
               align_pass_ms=timed(lambda: eng.alignment_queries(ids, kv, heads, P), reps, warmup),
               cost_ms=timed(cost_fn, reps, warmup),
               dtw_ms=timed(lambda: ops.dtw_token_times(cost, frames), reps, warmup),
               whole_ms=timed(lambda: eng.token_timestamps(rows, kv, P, heads), reps, warmup))
    print(json.dumps(out), flush=True)
    return out


def main():
    import whisper_ts_ref as R

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["fixture", "medium"])
    a = ap.parse_args()
    if a.only in (None, "fixture"):
        measure("fixture", dict(R.CONFIG), [(0, 1), (1, 0), (1, 3), (0, 2)], R.PREFIX, R.MAX_LENGTH, R.TIMESTAMP_BEGIN, a.reps, a.warmup)
    if a.only in (None, "medium"):
        kw = dict(d_model=1024, encoder_layers=24, decoder_layers=24, encoder_attention_heads=16, decoder_attention_heads=16,
                  encoder_ffn_dim=4096, decoder_ffn_dim=4096, num_mel_bins=80, vocab_size=51865, max_target_positions=448,
                  pad_token_id=50257, decoder_start_token_id=50258, eos_token_id=50257)
        heads = [(13, 15), (15, 4), (15, 15), (16, 1), (20, 0), (23, 4)]  # openai/whisper-medium's alignment_heads
        measure("whisper-medium", kw, heads, [50258, 50285, 50359], 3 + 225, 50364, a.reps, a.warmup)


if __name__ == "__main__":
    main()
