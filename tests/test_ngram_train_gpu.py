"""n-gram training on the GPU (coral_amd/ngram_train.py over coral_amd/csrc/ngram_train.hip) against the float64
restatement of the estimator in tests/kn_ref.py: the tokeniser against `str.split` per line, every integer statistic
exactly, every log10 value within a derived bound, determinism, chunking, the table-overflow refusal, and end to end
through the processor, the beam search, `finetune` and `evaluate`.

Bound on a log10 value: p_n is at most 4 n + 4 correctly rounded fp64 operations on positive terms, and a log10 follows:
|d log10 p| <= (4 N + 8) * 2^-53 / ln 10 + 2 ulp(log10 p) < 4e-15 at N = 5 and |log10 p| < 8.  Asserted: 1e-13."""
import functools
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref  # noqa: E402
import kn_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CAP = 1 << 16
TOL = 1e-13
_WORD = re.compile(rb"[^ \t\r\n]+")


# ---------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def corpus(kind):
    """"main": about 20 000 tokens over about 500 types, every count-of-counts positive at N = 5 (asserted below);
    "fallback": the same size with a unigram order that falls back to the fixed discounts."""
    return tuple(kn_ref.zipf_corpus(20_000, 500, seed=1, exponent=dict(main=1.3, fallback=1.1)[kind]))


@functools.lru_cache(maxsize=None)
def reference(kind, order):
    return kn_ref.KNRef(corpus(kind), order)


def run_trainer(lines, order, chunk_bytes=1 << 26, caps=None, hash_bits=64):
    from coral_amd.ngram_train import NGramTrainer, iter_chunks

    chunks = list(iter_chunks(lines, chunk_bytes))
    caps = caps or [CAP] * (order + 1)
    tr = NGramTrainer(order, caps[0], caps[1:], sum(len(c) for c in chunks), "cuda", hash_bits)
    for c in chunks:
        tr.feed(c)
    words = tr.words()
    tr.finalize()
    return tr, words, len(chunks)


@functools.lru_cache(maxsize=None)
def trained(kind, order):
    tr, words, _ = run_trainer(corpus(kind), order)
    return tr, words, tr.export([0] * order)


def same_rows(a, b):
    return all(np.array_equal(x[k], y[k]) if x[k].dtype != np.float64 else np.array_equal(x[k].view(np.int64), y[k].view(np.int64))
               for x, y in zip(a, b) for k in x)


def expected_tokens(data: bytes):
    from coral_amd.ngram_train import word_hash

    out = []
    for m in _WORD.finditer(data):
        out.append((m.start(), m.end() - m.start(), data.count(b"\n", 0, m.start()), word_hash(m.group())))
    # the same words as `str.split` gives per line
    per_line = [[w for w in line.decode("utf-8").split()] for line in data.split(b"\n")]
    mine = [[] for _ in per_line]
    for s, n, line, _ in out:
        mine[line].append(data[s:s + n].decode("utf-8"))
    assert mine == per_line
    return out


def device_tokens(tr, data: bytes):
    tok = tr.tokenize(data)
    nw = tok["nw"]
    cols = [tok[k][:nw].cpu().numpy() for k in ("start", "length", "line")]
    h = tok["hash"][:nw].cpu().numpy().view(np.uint64)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*cols, h)], tok


def small_trainer(order=1, hash_bits=64, cap=1 << 12):
    from coral_amd.ngram_train import NGramTrainer

    return NGramTrainer(order, cap, [cap] * order, 1 << 16, "cuda", hash_bits)


def span_buffer(length: int, seed: int) -> bytes:
    """`length` bytes of short words; a word straddles every multiple of the workgroup span inside the buffer."""
    from coral_amd._lib import NGT_TOK_SPAN

    rng = np.random.RandomState(seed)
    parts, size = [], 0
    while size < length + 16:
        w = bytes(rng.randint(97, 123, size=rng.randint(1, 10)).astype(np.uint8)) + (b"\n" if rng.rand() < 0.15 else b" ")
        parts.append(w)
        size += len(w)
    buf = bytearray(b"".join(parts)[:length])
    for edge in range(NGT_TOK_SPAN, length, NGT_TOK_SPAN):
        buf[edge - 2:edge + 2] = b"qrst"[:min(4, length - edge + 2)]
    buf[-1:] = b"z"
    assert len(buf) == length
    return bytes(buf)


# ---------------------------------------------------------------------------------------------- tokeniser
def test_tokeniser_matches_split_on_awkward_buffers():
    tr = small_trainer()
    buffers = [
        b"\n\n  hej \t\tmed  dig\r\n\r\n\t\xc3\xa6ble \xc3\xb8 \xc3\xa5\n x\n\n\nenkelt\n   \nsidste linje uden",
        b"ord\n",
        b"x",
        b" \t\r\n",
        b"a " + b"y" * 255 + b" b\n",               # a word at the byte limit
    ]
    for data in buffers:
        got, _ = device_tokens(tr, data)
        assert got == expected_tokens(data), data[:40]
    assert "æble" in buffers[0].decode("utf-8").split()


def test_tokeniser_refuses_a_word_above_the_byte_limit():
    tr = small_trainer()
    data = b"kort ord\n" + b"og " + b"y" * 256 + b" efter\n"
    with pytest.raises(ValueError, match=r"above 255 bytes, the first at byte 12 of the corpus: 'yyyy"):
        tr.tokenize(data)


@pytest.mark.parametrize("spans,extra", [(1, 0), (2, 0), (2, 1)])
def test_tokeniser_at_workgroup_span_boundaries(spans, extra):
    from coral_amd._lib import NGT_TOK_SPAN

    length = spans * NGT_TOK_SPAN + extra
    data = span_buffer(length, seed=spans * 10 + extra)
    want = expected_tokens(data)
    for edge in range(NGT_TOK_SPAN, length, NGT_TOK_SPAN):   # a word straddles every boundary
        assert any(s < edge < s + n for s, n, _, _ in want)
    got, _ = device_tokens(small_trainer(), data)
    assert got == want


@pytest.mark.parametrize("hash_bits", [64, 4], ids=["hash64", "hash4"])
def test_vocabulary_order_over_two_chunks_and_words_that_share_a_hash(hash_bits):
    """Word ids follow the first occurrence (byte offset), over two chunks fed in sequence.  Planting two words with one
    64-bit hash is impractical, so the compare-on-probe path is driven through the debug hash width: with 4 bits 60 word
    types share 15 hash values, and every one of them must still get its own id and its own counts."""
    lines = kn_ref.zipf_corpus(600, 60, seed=4)
    half = len(lines) // 2
    chunks = [("\n".join(part) + "\n").encode("utf-8") for part in (lines[:half], lines[half:])]
    r = kn_ref.KNRef(lines, 2)
    assert len(set(lines[half:]) - set(lines[:half])) and len(r.words) > 40
    tr = small_trainer(order=2, hash_bits=hash_bits)
    if hash_bits == 4:
        tok = device_tokens(tr, chunks[0])[0]
        assert len({h for _, _, _, h in tok}) <= 15 < len({chunks[0][s:s + n] for s, n, _, _ in tok})
    for c in chunks:
        tr.feed(c)
    assert tr.words() == r.words
    tr.finalize()
    rows = tr.export([0, 0])
    for n in (1, 2):
        keys = sorted(r.c[n])
        assert rows[n - 1]["ids"].tolist() == [list(g) for g in keys]
        assert rows[n - 1]["count"].tolist() == [r.c[n][g] for g in keys]


# ---------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("order", [1, 3, 5])
def test_every_integer_statistic_equals_the_reference(order):
    r = reference("main", order)
    assert all(min(t) > 0 for t in r.t[1:]), r.t    # the corpus is large enough for every count-of-counts
    assert 15_000 < r.tokens < 25_000 and 400 < len(r.words) < 520
    tr, words, rows = trained("main", order)
    assert words == r.words and tr.tokens == r.tokens
    assert tr.count_of_counts == r.t[1:]
    assert tr.discount_fallback == r.fallback[1:] and not any(tr.discount_fallback)
    g = tr.gstat.cpu().numpy()
    assert [int(x) for x in g[20:24]] == [r.Z[1][()]] + r.Nk[1][()]
    for n in range(1, order + 1):
        keys = sorted(r.c[n])
        row = rows[n - 1]
        assert row["ids"].tolist() == [list(k) for k in keys]
        assert row["count"].tolist() == [r.c[n][k] for k in keys]
        assert row["adj"].tolist() == [r.a[n][k] for k in keys]
        Z = r.Z[n + 1] if n < order else {}
        Nk = r.Nk[n + 1] if n < order else {}
        assert row["Z"].tolist() == [Z.get(k, 0) for k in keys]
        for i, name in enumerate(("N1", "N2", "N3")):
            assert row[name].tolist() == [Nk.get(k, [0, 0, 0])[i] for k in keys]


def test_bit_identical_from_run_to_run_and_under_chunking():
    _, words, rows = trained("main", 3)
    tr2, words2, nchunks = run_trainer(corpus("main"), 3)
    assert nchunks == 1 and words2 == words and same_rows(rows, tr2.export([0, 0, 0]))
    tr3, words3, nchunks = run_trainer(corpus("main"), 3, chunk_bytes=2048)
    assert nchunks > 20 and words3 == words and same_rows(rows, tr3.export([0, 0, 0]))
    assert tr3.count_of_counts == tr2.count_of_counts and tr3.discounts == tr2.discounts


def test_a_full_table_is_an_error_naming_the_capacity():
    from coral_amd.ngram_train import CoralAmdError, train_ngram

    lines = corpus("main")
    assert len(reference("main", 3).c[2]) > 64
    with pytest.raises(CoralAmdError, match=r"the 2-gram table \(64 slots\)"):
        run_trainer(lines, 3, caps=[CAP, CAP, 64, CAP])
    with pytest.raises(CoralAmdError, match=r"the vocabulary table \(64 slots\)"):
        train_ngram(lines, order=3, table_capacity=64)
    with pytest.raises(ValueError, match="power of two"):
        train_ngram(lines, order=3, table_capacity=1000)


# ---------------------------------------------------------------------------------------------- probabilities
@pytest.mark.parametrize("kind,order", [("main", 1), ("main", 3), ("main", 5), ("fallback", 3)])
def test_every_log10_value_within_the_derived_bound(kind, order):
    r = reference(kind, order)
    tr, _, rows = trained(kind, order)
    assert tr.discount_fallback == r.fallback[1:] and any(r.fallback[1:]) == (kind == "fallback")
    for n in range(order):
        assert all(abs(a - b) <= 1e-15 for a, b in zip(tr.discounts[n], r.D[n + 1][1:]))
    worst_p = worst_b = 0.0
    for n, want in enumerate(r.rows([0] * order)):
        assert rows[n]["ids"].tolist() == [list(g) for g, _, _ in want]
        worst_p = max(worst_p, float(np.abs(rows[n]["logp"] - np.array([lp for _, lp, _ in want])).max()))
        worst_b = max(worst_b, float(np.abs(rows[n]["backoff"] - np.array([bo for _, _, bo in want])).max()))
    print(f"{kind} N={order}: largest |d log10 p| = {worst_p:.3e}, largest |d log10 back-off| = {worst_b:.3e}")
    assert worst_p <= TOL and worst_b <= TOL


def test_written_arpa_equals_the_reference_estimators(tmp_path):
    from coral_amd.ngram import NGramLM
    from coral_amd.ngram_train import train_ngram

    r = reference("main", 3)
    path = tmp_path / "corpus.txt"
    path.write_text("\n".join(corpus("main")), encoding="utf-8")    # a last line without a line feed
    lm = train_ngram(path, order=3, chunk_bytes=1 << 15)             # the default prune 0 1 1, several chunks
    want = r.rows([0, 1, 1])
    assert lm.prune == [0, 1, 1] and lm.words == r.words and lm.order == 3
    assert lm.count_of_counts == r.t[1:] and lm.discount_fallback == r.fallback[1:] and lm.tokens == r.tokens
    assert len(want[1]) < len(r.c[2]) and len(want[2]) < len(r.c[3])
    for n in range(3):
        assert list(lm.grams[n]) == [g for g, _, _ in want[n]]       # entry for entry, in order
        for g, lp, bo in want[n]:
            assert abs(lm.grams[n][g][0] - lp) <= TOL and abs(lm.grams[n][g][1] - bo) <= TOL
    lm.write_arpa(tmp_path / "3gram.arpa")
    back = NGramLM.from_arpa(tmp_path / "3gram.arpa")
    assert back.words == lm.words and back.grams == lm.grams


# ---------------------------------------------------------------------------------------------- end to end
def test_trained_model_through_the_processor_and_the_beam_search(tmp_path):
    from test_ctc_beam_gpu import TinyTok, gpu_decode
    from test_ctc_beam_host import EXHAUSTIVE, TINY, coral_tokenizer, tiny_cases

    from coral_amd.ngram_train import train_ngram
    from coral_amd.processor import Wav2Vec2ProcessorWithLM, WaveformFeatureExtractor

    lines = kn_ref.zipf_corpus(1500, 80, seed=9)
    r = kn_ref.KNRef(lines, 3)
    lm = train_ngram(lines, order=3)
    Wav2Vec2ProcessorWithLM(WaveformFeatureExtractor(), coral_tokenizer(), lm).save_pretrained(tmp_path / "m")
    proc = Wav2Vec2ProcessorWithLM.from_pretrained(tmp_path / "m")
    assert (tmp_path / "m" / "language_model" / "3gram.arpa").exists() and proc.lm.words == r.words
    want_lm = r.to_lm()
    held_out = [["w0", "w1", "ø3"], ["w2"], ["aldrig", "set", "w0"], ["w5", "w0", "w0", "w1", "w4"]]
    for words in held_out:
        for boundary in (True, False):
            assert abs(proc.lm.score(words, boundary) - want_lm.score(words, boundary)) <= TOL * (len(words) + 1)
    # the beam search with tables built from a trained model: words over the tiny alphabet {a, b}
    rng = np.random.RandomState(0)
    vocab = ["a", "b", "ab", "ba", "aa", "bb", "aba"]
    tiny_lines = [" ".join(vocab[i] for i in rng.randint(0, len(vocab), size=rng.randint(1, 5))) for _ in range(60)]
    tiny_lm = train_ngram(tiny_lines, order=3, prune=[0, 0, 0])
    tiny_lm.write_arpa(tmp_path / "tiny.arpa")
    rlm = ctc_beam_ref.RefLM(tmp_path / "tiny.arpa")
    done = 0
    for logits in tiny_cases():
        exact = ctc_beam_ref.brute_force(logits, lm=rlm, **TINY)
        order = sorted(exact, key=exact.get, reverse=True)
        if exact[order[0]] - exact[order[1]] < 1e-3:   # (ten times the fp32 tolerance of the kernel's score)
            continue
        ids, score = gpu_decode(logits[None], lm=tiny_lm, tok=TinyTok(), blank=0, delim=3, forbidden=(), **EXHAUSTIVE)
        assert ids[0] == order[0] and abs(float(score[0]) - exact[order[0]]) <= 1e-4
        done += 1
        if done == 2:
            break
    assert done >= 1


def test_finetune_trains_and_stores_the_language_model_and_evaluate_uses_it(tmp_path, monkeypatch, caplog):
    sys.path.insert(0, str(ROOT / "scripts"))
    import finetune_asr_model

    from coral_amd import modeling
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.ngram import NGramLM
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine

    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(modeling.HUB_SHAPES, "facebook/wav2vec2-xls-r-300m",
                        dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=4))
    sentences = ["det er en test", "en test er det", "det var en anden test", "er det en test", "en anden en"]
    (tmp_path / "corpus.txt").write_text("\n".join(sentences * 3) + "\n", encoding="utf-8")
    common = ["model=test-wav2vec2", "datasets=synthetic", f"models_dir={tmp_path}", "max_steps=1", "total_batch_size=2",
              "per_device_batch_size=2", "max_seconds_per_example=2.0", "min_seconds_per_example=1.0", "logging_steps=1",
              "eval_steps=1", "model.use_decoder=true"]
    with caplog.at_level("INFO", logger="coral_amd"):
        finetune_asr_model.main(common + ["model_id=plain"])
    assert not (tmp_path / "plain" / "language_model").exists()        # no corpus: as before, and one line says so
    assert sum("decoder_corpus_path is not" in rec.getMessage() for rec in caplog.records) == 1

    (tmp_path / "withlm" / "language_model").mkdir(parents=True)
    (tmp_path / "withlm" / "language_model" / "stale.arpa").write_text("stale")
    finetune_asr_model.main(common + ["model_id=withlm", f"decoder_corpus_path={tmp_path / 'corpus.txt'}"])
    lm_dir = tmp_path / "withlm" / "language_model"
    assert sorted(p.name for p in lm_dir.iterdir()) == ["3gram.arpa", "attrs.json"]
    assert not list((tmp_path / "withlm").glob("*.arpa"))
    r = kn_ref.KNRef(sentences * 3, 3)
    lm = NGramLM.from_arpa(lm_dir / "3gram.arpa")
    assert lm.words == r.words and lm.order == 3 and lm.counts[0] == len(r.words) + 1   # the added </s> line
    want = r.to_lm()
    assert list(lm.grams[2]) == list(want.grams[2])
    assert all(abs(lm.grams[2][g][0] - want.grams[2][g][0]) <= TOL for g in want.grams[2])

    calls = []
    real = Wav2Vec2CTCEngine.beam_decode
    monkeypatch.setattr(Wav2Vec2CTCEngine, "beam_decode", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    rng = np.random.RandomState(3)
    examples = [dict(audio=(0.1 * rng.randn(int(16_000 * s))).astype(np.float32), text="det er") for s in (1.0, 1.4)]
    for no_lm, used in (("false", True), ("true", False)):
        calls.clear()
        cfg = load_config("evaluation", [f"model_id={tmp_path / 'withlm'}", "batch_size=2", "dataset=synthetic",
                                         f"no_lm={no_lm}"])
        scores = evaluate(cfg, examples)
        assert bool(calls) == used and math.isfinite(float(scores["wer"]))
