#!/usr/bin/env python3
"""Time of the LM-fused CTC beam search beside what an evaluation already pays (not bench.py: a side measurement).

XLS-R-300M shape at 16 x 10 s (T = 499, V = 46), confident and flat logits (the regimes of tests/test_ctc_beam_gpu.py),
beam 100, with the fixture LM of tests/golden/lm_tiny and without.  Prints, as HIP-event medians over `--iters` launches
after warm-up: (a) the encoder forward of that batch, (b) ca_ctc_greedy_decode, (c) ca_ctc_beam_decode per regime and
LM setting, and (d) the host time of the test-side Python search for one utterance, for scale.  One JSON line at the
end.  `--decode-only N` runs N beam launches and nothing else (for a kernel trace).

    python tools/bench_ctc_beam.py [--iters 20] [--batch 16]
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

import ctc_beam_ref as ref  # noqa: E402
from coral_amd import ops  # noqa: E402
from coral_amd.ngram import NGramLM  # noqa: E402
from coral_amd.processor import CTCTokenizer  # noqa: E402

CHARS = "abcdefghijklmnopqrstuvwxyzæøå0123456789éü"
V, BLANK, DELIM, T = 46, 45, 36, 499
ARPA = ROOT / "tests" / "golden" / "lm_tiny" / "3gram.arpa"


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--decode-only", type=int, default=0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_beam.py measures on the GPU; none is visible")
    dev = "cuda:0"
    B = args.batch
    tok = CTCTokenizer({c: i for i, c in enumerate(sorted(set(CHARS + "|")))})
    lm = NGramLM.from_arpa(ARPA)
    tables = lm.device_tables(tok, dev)
    words = [w for w in lm.words if not w.startswith("<")]
    lex = [[tok.vocab[c] for c in w] for w in sorted(words)]
    forb = torch.zeros(V, dtype=torch.uint8)
    forb[[tok.bos_token_id, tok.eos_token_id, tok.unk_token_id]] = 1
    forb = forb.to(dev)
    ids = torch.empty(B, T, dtype=torch.int32, device=dev)
    raw = torch.empty(B, T, dtype=torch.int32, device=dev)
    olen = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, V, args.beam), dtype=torch.uint8, device=dev)
    logits = {k: torch.from_numpy(ref.regime_logits(k, 1, B, T, V, BLANK, lex, DELIM)).to(dev) for k in ("confident", "flat")}

    def beam(kind, with_lm):
        ops.ctc_beam_decode(logits[kind], None, ids, olen, score, ws, B, T, V, V, BLANK, DELIM, forb,
                            tables if with_lm else None, beam_width=args.beam)

    if args.decode_only:
        for kind in ("confident", "flat"):
            for with_lm in (True, False):
                for _ in range(args.decode_only):
                    beam(kind, with_lm)
        torch.cuda.synchronize()
        return None

    out = dict(B=B, T=T, V=V, beam_width=args.beam, iters=args.iters)
    from bench import init_random_
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape

    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(), dev)
    init_random_(eng, 4242)
    eng.eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 160_000, generator=g).to(dev)  # 10 s -> 499 frames
    with torch.no_grad():
        eng(x)
    assert eng._saved["w"]["T"] == T
    out["encoder_forward_ms"] = event_median_ms(lambda: eng(x), args.iters)
    out["greedy_decode_ms"] = event_median_ms(
        lambda: ops.ctc_greedy_decode(logits["confident"], None, raw, ids, olen, B, T, V, V, BLANK), args.iters)
    for kind in ("confident", "flat"):
        for with_lm in (True, False):
            out[f"beam_{kind}_{'lm' if with_lm else 'nolm'}_ms"] = event_median_ms(lambda: beam(kind, with_lm), args.iters)
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    rlm = ref.RefLM(ARPA)
    for kind in ("confident", "flat"):
        x0 = logits[kind][0].cpu().numpy()
        t0 = time.perf_counter()
        ref.prefix_beam_search(x0, BLANK, DELIM, id2char, rlm, (42, 43, 44), beam_width=args.beam)
        out[f"host_python_one_utterance_{kind}_s"] = time.perf_counter() - t0
    for k, v in out.items():
        if isinstance(v, tuple):
            print(f"{k:36s} median {v[0]:9.3f} ms   min {v[1]:9.3f}   max {v[2]:9.3f}")
            out[k] = round(v[0], 4)
        else:
            print(f"{k:36s} {v}")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
