"""Stage times of n-gram training on the GPU (coral_amd/ngram_train.py) on a seeded Zipf corpus; not a test.

  python tools/measure_ngram_train.py [--tokens 100000000] [--types 1000000] [--order 3] [--table-capacity 268435456]
                                      [--slice 1000000 (0: skip the Python restatement)] [--out ngram_train_measure.json] [--no-arpa]

Device events around each stage after a warm-up run on a small corpus (tokenise, vocabulary, count, adjust, statistics,
probabilities, prune, export), host wall-clock for the vocabulary extraction and for building and writing the ARPA file,
tokens/s, and for each stage the bytes it has to move at the least (computed from the counts, not measured) with the time
those bytes take at the measured HBM copy rate.  No target is fixed (lmplz is not available to this project): the
yardsticks are that floor and the float64 Python restatement of the estimator (tests/kn_ref.py) timed on a slice of the
same corpus.  Figures and command: DESIGN.md §8."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate of the MI355X (79 % of the 8 TB/s peak)
WIDTH = 5                   # letters per word: 26^5 = 11.9 M spellings


def zipf_chunks(n_tokens, n_types, seed, block=10_000_000, exponent=1.1, mean_len=12):
    """Seeded corpus as byte blocks ending at a line end: word i is spelt in WIDTH letters, Zipf frequencies."""
    rng = np.random.RandomState(seed)
    cdf = np.cumsum(1.0 / np.arange(1, n_types + 1) ** exponent)
    cdf /= cdf[-1]
    perm = rng.permutation(26 ** WIDTH)[:n_types]          # spellings in no particular order
    done = 0
    while done < n_tokens:
        m = min(block, n_tokens - done)
        ids = perm[np.searchsorted(cdf, rng.rand(m))]
        out = np.empty((m, WIDTH + 1), dtype=np.uint8)
        for k in range(WIDTH):
            out[:, k] = 97 + (ids // 26 ** k) % 26
        out[:, WIDTH] = np.where(rng.rand(m) < 1.0 / mean_len, 10, 32)
        out[-1, WIDTH] = 10
        done += m
        yield out.tobytes()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=100_000_000)
    ap.add_argument("--types", type=int, default=1_000_000)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--table-capacity", type=int, default=1 << 28)
    ap.add_argument("--slice", type=int, default=1_000_000)
    ap.add_argument("--out", default="ngram_train_measure.json")
    ap.add_argument("--no-arpa", action="store_true")
    a = ap.parse_args(argv)

    import torch

    import kn_ref
    from coral_amd.ngram_train import NGramTrainer, default_prune, lm_from_export, train_ngram

    if not torch.cuda.is_available():
        raise SystemExit("measure_ngram_train needs the GPU: there is no CPU path and no CPU figure")
    res = dict(tokens=a.tokens, types=a.types, order=a.order, table_capacity=a.table_capacity)
    out_path = Path(a.out)

    def save():
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1))
        print(json.dumps(res), flush=True)

    train_ngram(kn_ref.zipf_corpus(20_000, 500, seed=1), order=a.order)     # warm-up: every kernel once
    t0 = time.time()
    chunks = list(zipf_chunks(a.tokens, a.types, seed=7))
    res["corpus_bytes"] = size = sum(len(c) for c in chunks)
    res["host_generate_s"] = time.time() - t0

    # the float64 Python restatement on a slice of the same corpus
    if a.slice > 0:
        head = chunks[0][: a.slice * (WIDTH + 1)].decode("ascii").split("\n")
        t0 = time.time()
        ref = kn_ref.KNRef(head, a.order)
        ref.rows()
        res["python_reference"] = dict(tokens=ref.tokens, seconds=time.time() - t0)
        res["python_reference"]["tokens_per_s"] = ref.tokens / res["python_reference"]["seconds"]
        del ref
        save()

    caps = [a.table_capacity] * (a.order + 1)
    tr = NGramTrainer(a.order, caps[0], caps[1:], a.types * 16, "cuda")
    tr.time_stages()
    torch.cuda.synchronize()
    t0 = time.time()
    for c in chunks:
        tr.feed(c)
    torch.cuda.synchronize()
    res["host_feed_wall_s"] = time.time() - t0          # uploads, status reads and id assignment included
    t0 = time.time()
    words = tr.words()
    res["host_vocabulary_s"] = time.time() - t0
    tr.finalize()
    res["word_types"] = len(words)
    res["count_of_counts"], res["discounts"], res["fallback"] = tr.count_of_counts, tr.discounts, tr.discount_fallback
    distinct = [int((k != 0).sum().item()) for k in tr.arrays["key"]]
    res["distinct_ngrams"] = distinct
    res["stage_ms"] = tr.stage_ms()
    save()

    t0 = time.time()
    rows = tr.export(default_prune(a.order))
    torch.cuda.synchronize()
    res["host_export_s"] = time.time() - t0                # prune + export launches, copies to the host, lexsort
    res["written_ngrams"] = [len(r["ids"]) for r in rows]
    res["stage_ms"] = ms = tr.stage_ms()
    # least bytes per stage, from the counts (T tokens, S = T + sentences positions, G_n distinct n-grams, C_n slots):
    T, N = tr.tokens, a.order
    C = a.table_capacity
    G = distinct
    least = dict(
        tokenise=2 * size + 20 * T,                                   # the text twice (count, emit), 20-byte records out
        vocabulary=T * (20 + 16),                                    # records in, one key and one representative probed
        count=T * 8 + sum(T * (8 + 8 * ((n + 2) // 2) + 4) for n in range(1, N + 1)),   # per gram: key, id words, count
        adjust=sum(C * 8 + G[m - 1] * (24 + 2 * 32 + 8 + 4) for m in range(2, N + 1)) + sum(C * 8 + G[n] * 12 for n in range(N)),
        statistics=sum(C * 8 + G[n] * (4 + 4 + 8) for n in range(N)),
        probabilities=sum(C * 8 + G[n] * (4 + 8 + 16 + 8 + 8) for n in range(N)),
        prune=sum(C * (8 + 1) + G[n] * 9 for n in range(N)),
        export=sum(C * 1 + len(rows[n]["ids"]) * (24 + 16 + 4 * (n + 1) + 24 + 16) for n in range(N)),
    )
    res["least_bytes"] = least
    res["hbm_floor_ms"] = {k: 1e3 * v / HBM_BYTES_PER_S for k, v in least.items()}
    res["tokens_per_s_by_stage"] = {k: T / (v / 1e3) for k, v in ms.items() if v > 0}
    res["device_ms_total"] = sum(ms.values())
    res["tokens_per_s_device"] = T / (res["device_ms_total"] / 1e3)
    save()

    if not a.no_arpa:
        t0 = time.time()
        lm = lm_from_export(words, rows)
        res["host_build_lm_s"] = time.time() - t0
        t0 = time.time()
        lm.write_arpa(out_path.with_suffix(".arpa"))
        res["host_write_arpa_s"] = time.time() - t0
        res["arpa_bytes"] = out_path.with_suffix(".arpa").stat().st_size
        out_path.with_suffix(".arpa").unlink()
        save()


if __name__ == "__main__":
    main()
