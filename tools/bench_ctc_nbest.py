#!/usr/bin/env python3
"""Time of the extended CTC beam search (`ca_ctc_beam_decode_ex`: n-best output, hotwords) beside the plain entry, and
of the plain entry beside another build of the library (not bench.py: a side measurement).

16 rows x 499 frames with about 100 labels each (the "noisy" regime of tests/test_ctc_beam_gpu.py), V = 46, beam 100,
the fixture LM of tests/golden/lm_tiny.  HIP-event medians over `--iters` launches after warm-up, the variants taken in
alternation round by round so that drift on a shared box hits all of them alike:
  (a) `ca_ctc_beam_decode` of this build and, with `--other-lib PATH` (a libcoral_amd.so of another commit, loaded beside
      this one in the same process), of that build - same logits, and the outputs are compared bit for bit;
  (b) `ca_ctc_beam_decode_ex` with n_best = 1 / 10 / 100 without hotwords, and n_best = 1 with 10 and with 1000 hotwords
      (seeded random words of 3..10 letters);
  (c) `--long`: one row x 30 000 frames, the plain entry and n_best = 100 (the parallel trace-back).
One JSON line at the end.

    python tools/bench_ctc_nbest.py [--iters 20] [--other-lib /path/to/libcoral_amd.so] [--long]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ctc_beam_ref as ref  # noqa: E402
from coral_amd import _lib, ngram, ops  # noqa: E402
from coral_amd.processor import CTCTokenizer  # noqa: E402

CHARS = "abcdefghijklmnopqrstuvwxyzæøå0123456789éü"
V, BLANK, DELIM = 46, 45, 36
ARPA = ROOT / "tests" / "golden" / "lm_tiny" / "3gram.arpa"


def alternating_medians_ms(fns: dict, iters: int, warmup: int = 3) -> dict:
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def random_words(n, seed):
    rng = np.random.RandomState(seed)
    letters = "abcdefghijklmnopqrstuvwxyzæøå"
    out = set()
    while len(out) < n:
        out.add("".join(letters[i] for i in rng.randint(len(letters), size=rng.randint(3, 11))))
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--long", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_nbest.py measures on the GPU; none is visible")
    dev = "cuda:0"
    tok = CTCTokenizer({c: i for i, c in enumerate(sorted(set(CHARS + "|")))})
    lm = ngram.NGramLM.from_arpa(ARPA)
    tables = lm.device_tables(tok, dev)
    lex = [[tok.vocab[c] for c in w] for w in sorted(w for w in lm.words if not w.startswith("<"))]
    forb = torch.zeros(V, dtype=torch.uint8)
    forb[[tok.bos_token_id, tok.eos_token_id, tok.unk_token_id]] = 1
    forb = forb.to(dev)
    other = None
    if args.other_lib:
        other = C.CDLL(str(args.other_lib))
        other.ca_ctc_beam_decode.restype = C.c_int
        other.ca_ctc_beam_decode.argtypes = [C.POINTER(_lib.CaCtcBeamDesc), C.c_void_p]

    def setup(B, T):
        x = torch.from_numpy(ref.regime_logits("noisy", 1, B, T, V, BLANK, lex, DELIM)).to(dev)
        ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, V, args.beam), dtype=torch.uint8, device=dev)
        plain = [(torch.empty(B, T, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                  torch.empty(B, dtype=torch.float32, device=dev)) for _ in range(2)]

        def run_plain(which=0):
            ids, olen, score = plain[which]
            ops.ctc_beam_decode(x, None, ids, olen, score, ws, B, T, V, V, BLANK, DELIM, forb, tables, beam_width=args.beam)

        def run_other():
            ids, olen, score = plain[1]
            d = ops._ctc_beam_desc(x, None, ids, olen, score, ws, B, T, V, V, BLANK, DELIM, forb, tables, args.beam,
                                   0.5, 1.5, -10.0, -5.0, -10.0, True)
            rc = other.ca_ctc_beam_decode(C.byref(d), ops._stream())
            assert rc == 0, rc

        def make_ex(n_best, hotwords=None):
            ids = torch.empty(B, n_best, T, dtype=torch.int32, device=dev)
            olen = torch.empty(B, n_best, dtype=torch.int32, device=dev)
            split = torch.empty(3, B, n_best, dtype=torch.float32, device=dev)
            n_out = torch.empty(B, dtype=torch.int32, device=dev)
            hot = None if hotwords is None else ngram.hotword_tables(hotwords, tok, dev)

            def run():
                ops.ctc_beam_decode_ex(x, None, ids, olen, split[0], split[1], split[2], n_out, ws, B, T, V, V, BLANK, DELIM,
                                       forb, tables, n_best=n_best, hotwords=hot, hotword_weight=10.0, beam_width=args.beam)
            return run

        return plain, run_plain, run_other, make_ex

    out = dict(B=args.batch, T=499, V=V, beam_width=args.beam, iters=args.iters, regime="noisy", lm="lm_tiny")
    plain, run_plain, run_other, make_ex = setup(args.batch, 499)
    fns = {"plain_ms": run_plain}
    if other is not None:
        fns["plain_other_lib_ms"] = run_other
    for n in (1, 10, 100):
        fns[f"ex_nbest{n}_ms"] = make_ex(n)
    for n in (10, 1000):
        fns[f"ex_nbest1_hot{n}_ms"] = make_ex(1, random_words(n, n))
    res = alternating_medians_ms(fns, args.iters)
    if other is not None:  # the two builds on the same logits: the same bits
        run_plain(0)
        run_other()
        torch.cuda.synchronize()
        out["other_lib_same_bits"] = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(*plain))
        out["plain_over_other_lib"] = round(res["plain_ms"][0] / res["plain_other_lib_ms"][0], 4)
    if args.long:
        _, run_plain1, _, make_ex1 = setup(1, 30_000)
        long = alternating_medians_ms({"long_plain_ms": run_plain1, "long_ex_nbest100_ms": make_ex1(100)}, max(3, args.iters // 4), 1)
        res.update(long)
    for k, v in res.items():
        print(f"{k:28s} median {v[0]:10.3f} ms   min {v[1]:10.3f}   max {v[2]:10.3f}")
        out[k] = round(v[0], 4)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
