"""Host side of n-gram training (coral_amd/ngram_train.py) and the float64 restatement of the estimator the GPU tests
compare against (tests/kn_ref.py): a hand-worked corpus with literal values, the discount formula and every fallback
trigger, exact normalisation of the written model under the ARPA back-off rule, the pruning rule, the ARPA round trip
with the reference's </s> line, the refusals, and the C ABI additions."""
import math
import re
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kn_ref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
UNK, BOS, EOS = 0, 1, 2


def test_hand_worked_corpus():
    """Corpus: "a b a" / "a b", N = 2.  Ids: <unk> 0, <s> 1, </s> 2, a 3, b 4; padded: <s> a b a </s>, <s> a b </s>.
    Raw counts: <s> 2, a 3, b 2, </s> 2;  (<s>,a) 2, (a,b) 2, (b,a) 1, (a,</s>) 1, (b,</s>) 1.
    Adjusted: a_2 = c_2;  a_1(a) = |{<s>, b}| = 2, a_1(b) = |{a}| = 1, a_1(</s>) = |{a, b}| = 2, a_1(<s>) = a_1(<unk>) = 0.
    Count-of-counts: order 1 (1, 2, 0, 0), order 2 (3, 2, 0, 0): t_3 = 0, both orders fall back to D = (0.5, 1, 1.5).
    Order 1: Z = 5, N = (1, 2, 0), gamma = (0.5 + 2) / 5 = 0.5, |W| = 5, gamma / (|W| - 1) = 0.125:
      p(a) = 1/5 + 0.125 = 0.325, p(b) = 0.5/5 + 0.125 = 0.225, p(</s>) = 0.325, p(<unk>) = 0.125 (sum 1).
    Order 2: <s>: Z 2, N (0,1,0), gamma 0.5, p(a|<s>) = 1/2 + 0.5 * 0.325 = 0.6625;
      a: Z 3, N (1,1,0), gamma 0.5, p(b|a) = 1/3 + 0.5 * 0.225, p(</s>|a) = 0.5/3 + 0.5 * 0.325;
      b: Z 2, N (2,0,0), gamma 0.5, p(a|b) = p(</s>|b) = 0.25 + 0.5 * 0.325 = 0.4125."""
    r = kn_ref.KNRef(["a b a", "a b"], 2)
    a, b = 3, 4
    assert r.words == ["<unk>", "<s>", "</s>", "a", "b"]
    assert r.c[1] == {(BOS,): 2, (a,): 3, (b,): 2, (EOS,): 2, (UNK,): 0}
    assert r.c[2] == {(BOS, a): 2, (a, b): 2, (b, a): 1, (a, EOS): 1, (b, EOS): 1}
    assert r.a[1] == {(BOS,): 0, (UNK,): 0, (a,): 2, (b,): 1, (EOS,): 2} and r.a[2] == r.c[2]
    assert r.t[1] == [1, 2, 0, 0] and r.t[2] == [3, 2, 0, 0]
    assert r.fallback[1:] == [True, True] and r.D[1] == r.D[2] == (0.0, 0.5, 1.0, 1.5)
    assert r.Z[1] == {(): 5} and r.Nk[1] == {(): [1, 2, 0]} and r.gamma[1] == {(): 0.5}
    want1 = {(a,): 0.325, (b,): 0.225, (EOS,): 0.325, (UNK,): 0.125}
    assert set(r.p[1]) == set(want1) and all(abs(r.p[1][g] - v) <= 1e-15 for g, v in want1.items())
    assert r.Z[2] == {(BOS,): 2, (a,): 3, (b,): 2} and r.Nk[2] == {(BOS,): [0, 1, 0], (a,): [1, 1, 0], (b,): [2, 0, 0]}
    assert all(abs(v - 0.5) <= 1e-15 for v in r.gamma[2].values())
    want2 = {(BOS, a): 0.6625, (a, b): 1 / 3 + 0.1125, (a, EOS): 0.5 / 3 + 0.1625, (b, a): 0.4125, (b, EOS): 0.4125}
    assert set(r.p[2]) == set(want2) and all(abs(r.p[2][g] - v) <= 1e-15 for g, v in want2.items())
    rows = r.rows([0, 0])
    assert [g for g, _, _ in rows[0]] == [(0,), (1,), (2,), (3,), (4,)]          # unigrams in id order
    assert [g for g, _, _ in rows[1]] == sorted(want2)                            # higher orders: lexicographic
    assert rows[0][1] == ((BOS,), 0.0, math.log10(0.5)) and rows[0][0][2] == 0.0  # <s>: log10 p = 0 and its back-off


def test_discount_formula_and_every_fallback_trigger():
    from coral_amd.ngram_train import FALLBACK_DISCOUNTS, kn_discounts

    # t = (100, 40, 20, 10): Y = 100 / 180 = 5/9; D1 = 1 - 2 (5/9) 40/100 = 5/9; D2 = 2 - 3 (5/9) 20/40 = 7/6;
    # D3 = 3 - 4 (5/9) 10/20 = 17/9
    for fn in (kn_discounts, kn_ref.discounts):
        d, fb = fn([100, 40, 20, 10])
        assert not fb and all(abs(x - y) <= 1e-15 for x, y in zip(d, (5 / 9, 7 / 6, 17 / 9)))
        for k in range(4):   # any zero count-of-counts
            t = [100, 40, 20, 10]
            t[k] = 0
            assert fn(t) == (FALLBACK_DISCOUNTS, True)
        # D1 = 1 - 2 Y t2 / t1 = t1 / (t1 + 2 t2) lies in (0, 1) for positive counts, and no D(k) reaches k (the
        # subtrahend is positive): the remaining triggers are D2 <= 0 (t3 large) and D3 <= 0 (t4 large).
        assert fn([100, 40, 400, 10]) == (FALLBACK_DISCOUNTS, True)    # D2 = 2 - 3 (5/9) 10 < 0
        assert fn([100, 40, 20, 400]) == (FALLBACK_DISCOUNTS, True)    # D3 = 3 - 4 (5/9) 20 < 0
        d, fb = fn([100, 40, 47, 10])                                   # D2 = 2 - (5/3)(47/40) = 0.0417 > 0: kept
        assert not fb and 0 < d[1] < 0.05
        assert fn([100, 40, 48, 10]) == (FALLBACK_DISCOUNTS, True)     # D2 = 2 - (5/3)(48/40) = 0 exactly: outside (0, 2)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_written_model_normalises_in_every_context(order):
    """Unpruned, every context h of every order (the empty one and <s> included): the sum over every word but <s> of
    P(w | h) under `NGramLM.logp`'s back-off rule is 1 - by induction over the order,
    (Z - sum D) / Z + (sum D / Z) * 1.  Within 1e-12 (a few hundred float64 terms of 10 ** log10 p)."""
    r = kn_ref.KNRef(kn_ref.zipf_corpus(3000, 120, seed=order), order)
    lm = r.to_lm([0] * order)
    targets = [w for w in range(len(r.words)) if w != BOS]
    contexts = {()} | {h for n in range(2, order + 1) for h in r.Z[n]}
    assert (BOS,) in contexts or order == 1
    worst = 0.0
    for h in contexts:
        total = math.fsum(10.0 ** lm.logp(h, w) for w in targets)
        worst = max(worst, abs(total - 1.0))
    print(f"order {order}: {len(contexts)} contexts, largest |sum - 1| = {worst:.3e}")
    assert worst <= 1e-12


def test_pruning_drops_exactly_the_rare_grams_without_written_extension():
    r = kn_ref.KNRef(kn_ref.zipf_corpus(3000, 120, seed=11), 3)
    full = r.rows([0, 0, 0])
    for prune in ([0, 1, 1], [0, 0, 2], [0, 3, 1]):
        rows = r.rows(prune)
        assert [g for g, _, _ in rows[0]] == [g for g, _, _ in full[0]]
        written3 = {g for g, _, _ in rows[2]}
        assert written3 == {g for g, c in r.c[3].items() if c > prune[2]}
        prefixes = {g[:-1] for g in written3}
        assert {g for g, _, _ in rows[1]} == {g for g, c in r.c[2].items() if c > prune[1] or g in prefixes}
        assert len(rows[2]) < len(full[2]) and (len(rows[1]) < len(full[1]) or prune[1] == 0)
        for n in range(3):   # what is written keeps its unpruned values, bit for bit
            values = {g: (lp, bo) for g, lp, bo in full[n]}
            assert all(values[g] == (lp, bo) for g, lp, bo in rows[n])


def test_arpa_round_trip_and_the_added_eos_line(tmp_path):
    from coral_amd.ngram import NGramLM
    from coral_amd.ngram_train import add_eos_line

    r = kn_ref.KNRef(kn_ref.zipf_corpus(1500, 80, seed=5), 3)
    lm = r.to_lm()
    lm.write_arpa(tmp_path / "raw.arpa")
    back = NGramLM.from_arpa(tmp_path / "raw.arpa")
    assert back.words == lm.words and back.grams == lm.grams and [list(g) for g in back.grams] == [list(g) for g in lm.grams]
    add_eos_line(tmp_path / "raw.arpa", tmp_path / "3gram.arpa")
    text = (tmp_path / "3gram.arpa").read_text(encoding="utf-8").splitlines()
    raw = (tmp_path / "raw.arpa").read_text(encoding="utf-8").splitlines()
    assert len(text) == len(raw) + 1 and f"ngram 1={len(lm.words) + 1}" in text and f"ngram 1={len(lm.words)}" in raw
    at = next(i for i, line in enumerate(text) if "<s>" in line)
    assert text[at + 1] == text[at].replace("<s>", "</s>") and text[at + 2].split("\t")[1] == "</s>"
    fixed = NGramLM.from_arpa(tmp_path / "3gram.arpa")    # the first </s> line wins; everything else is unchanged
    assert fixed.words == lm.words and fixed.counts[0] == len(lm.words) + 1
    assert fixed.grams[1] == lm.grams[1] and fixed.grams[2] == lm.grams[2]
    assert {g: v for g, v in fixed.grams[0].items() if g != (EOS,)} == {g: v for g, v in lm.grams[0].items() if g != (EOS,)}
    assert fixed.grams[0][(EOS,)] == (0.0, lm.grams[0][(BOS,)][1])


def test_refusals(tmp_path):
    from coral_amd.ngram_train import train_ngram

    for word in ("<s>", "</s>", "<unk>"):
        with pytest.raises(ValueError, match="reserved word"):
            train_ngram(["et ord", f"her er {word} midt i"], order=2)
        with pytest.raises(ValueError, match="reserved word"):
            kn_ref.KNRef([f"{word} først"], 2)
    with pytest.raises(ValueError, match="prune\\[0\\] must be 0"):
        train_ngram(["a b"], order=3, prune=[1, 1, 1])
    with pytest.raises(ValueError, match="one threshold per order"):
        train_ngram(["a b"], order=3, prune=[0, 1])
    with pytest.raises(ValueError, match="outside 1..5"):
        train_ngram(["a b"], order=6)
    with pytest.raises(ValueError, match="outside 1..5"):
        train_ngram(["a b"], order=0)
    with pytest.raises(ValueError, match="empty"):
        train_ngram([], order=3)
    (tmp_path / "empty.txt").write_bytes(b"")
    with pytest.raises(ValueError, match="empty"):
        train_ngram(tmp_path / "empty.txt", order=3)
    with pytest.raises(ValueError, match="empty"):
        kn_ref.KNRef(["", "  \t "], 3)


def test_chunks_end_at_line_ends_and_the_capacity_rule(tmp_path):
    from coral_amd.ngram_train import corpus_size, iter_chunks, table_capacity_rule, word_hash

    lines = kn_ref.zipf_corpus(400, 50, seed=2)
    data = ("\n".join(lines)).encode("utf-8")           # the last line has no line feed
    (tmp_path / "c.txt").write_bytes(data)
    for size in (16, 100, 1 << 20):
        chunks = list(iter_chunks(tmp_path / "c.txt", size))
        assert b"".join(chunks) == data and all(c.endswith(b"\n") for c in chunks[:-1])
        assert b"".join(iter_chunks(lines, size)) == data + b"\n"
    n, ws, lf = corpus_size([data])
    words = sum(len(kn_ref.split_line(l)) for l in lines)
    assert n == len(data) and lf == len(lines) - 1 and ws + lf + 4 >= words + len(lines) + 2
    cap = table_capacity_rule(ws, lf)
    assert cap & (cap - 1) == 0 and cap >= 2 * (words + len(lines) + 2) and cap < 4 * (ws + lf + 4)
    assert word_hash(b"a") != word_hash(b"b") and 0 < word_hash("ø".encode()) < 1 << 64


def test_abi_declares_the_training_entries(tmp_path):
    from coral_amd import _lib, ops

    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "coral_amd.h").read_text(), flags=re.S)
    names = ["ca_ngt_tokenize_blocks", "ca_ngt_tokenize", "ca_ngt_vocab_round", "ca_ngt_vocab_commit", "ca_ngt_count",
             "ca_ngt_adjust", "ca_ngt_stats", "ca_ngt_probs", "ca_ngt_prune", "ca_ngt_export"]
    for sym in names:
        m = re.search(rf"\b{sym}\s*\(([^)]*)\)", hdr)
        assert m and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[sym][1]), sym
        assert hasattr(ops, sym[3:])
    assert lib.ca_ngt_tokenize_blocks(1) == 1 and lib.ca_ngt_tokenize_blocks(_lib.NGT_TOK_SPAN + 1) == 2
    for macro, value in (("CA_NGT_MAX_ORDER", _lib.NGT_MAX_ORDER), ("CA_NGT_MAX_WORD_BYTES", _lib.NGT_MAX_WORD_BYTES),
                         ("CA_NGT_TOK_SPAN", _lib.NGT_TOK_SPAN), ("CA_NGT_ST_WORDS_N", _lib.NGT_ST_WORDS_N)):
        assert re.search(rf"#define {macro} {value}\b", hdr)
    # argument validation needs no GPU
    assert lib.ca_ngt_tokenize(None, 4, 0, 64, None, None, None, None, None, 4, None, None) == -1
    assert b"ca_ngt_tokenize" in lib.ca_last_error()
    # the descriptor is laid out as g++ lays the header out
    import ctypes
    import subprocess

    exe = tmp_path / "layout"
    (exe.parent / "layout.cpp").write_text('#include <cstddef>\n#include <cstdio>\n#include "coral_amd.h"\nint main() {\n'
                                           '  printf("%zu %zu %zu %zu\\n", sizeof(CaNgramTables), offsetof(CaNgramTables, key), '
                                           'offsetof(CaNgramTables, ext), offsetof(CaNgramTables, status));\n  return 0;\n}\n')
    subprocess.run(["g++", "-I", str(ROOT / "include"), str(exe.parent / "layout.cpp"), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.CaNgramTables
    assert got == [ctypes.sizeof(T), T.key.offset, T.ext.offset, T.status.offset]


def test_config_key_and_finetune_docstrings():
    from coral_amd import finetune, ngram
    from coral_amd.config import load_config

    base = ["model=test-wav2vec2", "datasets=synthetic"]
    assert load_config("asr_finetuning", base).decoder_corpus_path is None
    assert load_config("asr_finetuning", base + ["decoder_corpus_path=/tmp/c.txt"]).decoder_corpus_path == "/tmp/c.txt"
    for key in ("wav2vec2-small", "wav2vec2-medium", "wav2vec2-large"):
        m = load_config("asr_finetuning", [f"model={key}"]).model
        assert m.use_decoder is True and m.decoder_num_ngrams == 3
    assert "out of scope" not in ngram.__doc__ and "ngram_train" in ngram.__doc__
    assert "decoder_corpus_path" in finetune.finetune.__doc__
