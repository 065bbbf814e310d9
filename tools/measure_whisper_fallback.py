#!/usr/bin/env python3
"""What the scored pick of the temperature fallback costs per decoded token (not bench.py: a side measurement).

whisper-medium shape, seeded random weights, 16 clips of noise features, decoding with timestamps as a graph-replayed
launch sequence.  Mean over `--iters` (20) repetitions between device events after 3 warm-ups, per decoded token (the
time of `WhisperEngine.generate` to P + 3 + tokens minus the same call to P + 3, over the tokens in between; the cross
K|V are computed once in front and passed in, so no variant runs the encoder):
  (a) the greedy pick of generate(return_timestamps=True) as it was (ca_argmax_timestamps_advance);
  (b) the scored pick at temperature 0 (return_stats=True) and (c) at temperature 0.4 (ca_pick_scored_advance);
  (d) the four pick launches alone at 16 x V (ca_argmax_advance, ca_argmax_timestamps_advance, the scored pick twice);
  (e) one fallback attempt over 4 of the 16 clips: with a gather of the cross K|V against encoder + projection again.
One JSON line at the end.

    python tools/measure_whisper_fallback.py [--iters 20] [--tokens 64] [--clips 16]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from coral_amd import ops  # noqa: E402
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
    ap.add_argument("--model", default="whisper-medium")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("measure_whisper_fallback.py measures on the GPU; none is visible")
    dev = "cuda:0"
    shape = WhisperShape(**CORAL_WHISPER_SHAPES[args.model])
    eng = WhisperEngine(shape, dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        eng.store.p32.copy_((torch.randn(eng.store.numel, generator=g) * 0.02).to(dev))
    eng.refresh_compute_weights()
    prefix = prefix_ids(shape)[:-1]  # with timestamps: no <|notimestamps|>
    tb = prefix_ids(shape)[-1] + 1
    P, B, V = len(prefix), args.clips, shape.vocab_size
    short, long = P + 3, P + 3 + args.tokens
    sup = [shape.eos_token_id]  # random weights: no row may end early, every run decodes `tokens` tokens between the lengths
    feats = torch.randn(B, shape.num_mel_bins, 3000, generator=g) * 0.5
    kv = eng.cross_kv(eng.encode(feats))
    u = torch.rand(B, long, generator=g)
    kw = dict(suppress_tokens=sup, return_timestamps=True, timestamp_begin=tb, max_initial_timestamp_index=50)

    def per_token(cross, **extra):
        run = lambda n: (lambda: eng.generate(None, prefix, n, cross_kv=cross, **kw, **extra))  # noqa: E731
        return (event_mean_ms(run(long), args.iters) - event_mean_ms(run(short), args.iters)) / args.tokens

    res = dict(model=args.model, clips=B, tokens=args.tokens, iters=args.iters)
    res["greedy_ms_per_token"] = per_token(kv)
    res["scored_t0_ms_per_token"] = per_token(kv, return_stats=True)
    res["scored_t04_ms_per_token"] = per_token(kv, return_stats=True, temperature=0.4, sample_uniforms=u)
    res["scored_t0_over_greedy"] = res["scored_t0_ms_per_token"] / res["greedy_ms_per_token"]
    res["scored_t04_over_greedy"] = res["scored_t04_ms_per_token"] / res["greedy_ms_per_token"]

    # the pick launches alone
    Vp, L = (V + 7) // 8 * 8, long
    logits = torch.randn(B, Vp, generator=g).to(dev)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    st = dict(out=z(B), done=z(B, dt=torch.bool), ids=z(B, L, dt=torch.int64), tok=z(B), pos=z(B), klen=z(B),
              slp=z(B, dt=torch.float32), ns=z(B))
    st["ids"][:, P] = tb + 3
    supm, ud = z(V, dt=torch.uint8), u.to(dev)

    def reset():
        st["pos"].fill_(P + 1)

    def plain():
        reset()
        ops.argmax_advance(logits, supm, st["out"], B, V, Vp, st["done"], st["ids"], st["tok"], st["pos"], st["klen"],
                           shape.pad_token_id, shape.eos_token_id)

    def greedy():
        reset()
        ops.argmax_timestamps_advance(logits, supm, st["out"], B, V, Vp, st["done"], st["ids"], st["tok"], st["pos"], st["klen"],
                                      shape.pad_token_id, shape.eos_token_id, P, tb, 50)

    def scored(inv_t):
        def run():
            reset()
            ops.pick_scored_advance(logits, supm, st["out"], B, V, Vp, inv_t, ud if inv_t else None, st["slp"], st["ns"],
                                    st["done"], st["ids"], st["tok"], st["pos"], st["klen"], shape.pad_token_id,
                                    shape.eos_token_id, timestamps=(P, tb, 50))
        return run

    fill = event_mean_ms(reset, 50)
    res["argmax_advance_us"] = 1e3 * (event_mean_ms(plain, 50) - fill)
    res["argmax_timestamps_us"] =1e3 * (event_mean_ms(greedy, 50) - fill)
    res["pick_scored_t0_us"] = 1e3 * (event_mean_ms(scored(0.0), 50) - fill)
    res["pick_scored_t04_us"] = 1e3 * (event_mean_ms(scored(2.5), 50) - fill)

    # one fallback attempt over a quarter of the clips
    rows = list(range(0, B, 4))
    extra = dict(return_stats=True, temperature=0.4, sample_uniforms=u[rows].contiguous())
    res["attempt_rows"] = len(rows)
    res["attempt_reused_kv_ms"] = event_mean_ms(
        lambda: eng.generate(None, prefix, long, cross_kv=eng.gather_cross_kv(kv, rows), **kw, **extra), args.iters)
    res["attempt_encoded_again_ms"] = event_mean_ms(lambda: eng.generate(feats[rows], prefix, long, **kw, **extra), args.iters)
    print(json.dumps({n: (round(v, 4) if isinstance(v, float) else v) for n, v in res.items()}))
    return res


if __name__ == "__main__":
    main()
