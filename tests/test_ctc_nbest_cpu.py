"""Host side of n-best output and hotword boosting in the CTC beam search (no GPU): the float64 restatement
(tests/ctc_hotword_ref.py) against brute force over every alignment, the host hotword tables, the oracle choice among
n-best hypotheses, and what is refused by name."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref as ref  # noqa: E402
import ctc_hotword_ref as href  # noqa: E402
from test_ctc_beam_host import ARPA, ARPA_NOUNK, EXHAUSTIVE, TINY, coral_tokenizer, tiny_cases  # noqa: E402

# the three hotword settings of the tiny cases: (hotwords, hotword_weight)
HOT_SETTINGS = {"none": ((), 10.0), "ab": (("ab",), 1.5), "b_abb": (("b", "abb"), 2.5)}
N_TINY = 8


def tiny_lm(mode):
    return dict(lm=ref.RefLM(ARPA), lm_nounk=ref.RefLM(ARPA_NOUNK), plain=None)[mode]


@pytest.mark.parametrize("hot", list(HOT_SETTINGS))
@pytest.mark.parametrize("mode", ["lm", "lm_nounk", "plain"])
def test_restatement_returns_the_brute_force_top_8_in_order(mode, hot):
    lm = tiny_lm(mode)
    params = dict(alpha=0.0, beta=0.0) if mode == "plain" else {}
    words, weight = HOT_SETTINGS[hot]
    for logits in tiny_cases():
        exact = href.brute_force(logits, lm=lm, hotwords=words, hotword_weight=weight, **TINY, **params)
        order = href.ranked(exact)
        got = href.prefix_beam_search_nbest(logits, lm=lm, hotwords=words, hotword_weight=weight, **TINY, **EXHAUSTIVE,
                                            **params)
        assert [g[0] for g in got] == order  # exhaustive: every string, in the brute force's order
        for y, s, logit, lms in got[:N_TINY]:
            assert abs(s - exact[y]) < 1e-9 and abs(logit + lms - s) < 1e-12
        if not words:  # without hotwords: the objective and the winner of the existing helper
            plain = ref.brute_force(logits, lm=lm, **TINY, **params)
            assert all(abs(plain[y] - exact[y]) < 1e-12 for y in plain)
            assert got[0][0] == ref.prefix_beam_search(logits, lm=lm, **TINY, **EXHAUSTIVE, **params)[0]


def test_hotword_term_counts_closed_words_and_the_provisional_bonus_is_no_part_of_S():
    lm = ref.RefLM(ARPA)
    logits = tiny_cases()[2]
    base = ref.brute_force(logits, lm=lm, **TINY)
    hot = href.brute_force(logits, lm=lm, hotwords=["AB b", "ab"], hotword_weight=2.0, **TINY)
    for y, s in base.items():
        words = href.words_of(y, TINY["delimiter"], TINY["id2char"])
        assert abs(hot[y] - s - 2.0 * sum(w in ("ab", "b") for w in words)) < 1e-12
    assert href.hot_set(["AB b", "ab"]) == ["ab", "b"]
    assert href.hot_prefixes(["b", "abb", "ab"]) == {"b": 1, "a": 2, "ab": 2, "abb": 3}
    # weight 0 and an empty list are both "no hotwords"
    a = href.prefix_beam_search_nbest(logits, lm=lm, hotwords=["ab"], hotword_weight=0.0, **TINY, **EXHAUSTIVE)
    b = href.prefix_beam_search_nbest(logits, lm=lm, hotwords=[], **TINY, **EXHAUSTIVE)
    assert a == b


def test_host_hotword_tables_hold_every_prefix_with_fraction_and_flag():
    from coral_amd import ngram

    tok = coral_tokenizer()
    tb = ngram.hotword_tables(["Århus by", "år", "århundrede", "by"], tok, "cpu")
    keys = tb["hot_keys"].numpy().view(np.uint64)
    assert (keys[1:] > keys[:-1]).all()
    assert tb["hot_frac"].dtype.is_floating_point and tb["hot_frac"].numpy().dtype == np.float32
    assert tb["hot_word"].numpy().dtype == np.uint8
    look = {int(k): (float(f), int(w)) for k, f, w in zip(keys, tb["hot_frac"].numpy(), tb["hot_word"].numpy())}

    def h(word):
        return ngram.hash_ids([tok.vocab[c] for c in word], ngram.WORD_SEED)

    words = ["århus", "by", "år", "århundrede"]
    assert ngram.hotword_set(["Århus by", "år", "århundrede", "by"]) == words
    prefixes = {w[:n] for w in words for n in range(1, len(w) + 1)}
    assert len(look) == len(prefixes)
    for p in prefixes:
        len_min = min(len(w) for w in words if w.startswith(p))
        frac, flag = look[h(p)]
        assert frac == float(np.float32(len(p)) / np.float32(len_min)), p
        assert flag == (p in words), p
    assert look[h("å")] == (0.5, 0) and look[h("år")] == (1.0, 1) and look[h("århu")][0] == float(np.float32(4) / np.float32(5))
    assert h("b") in look and h("a") not in look and h("byen") not in look
    for none in ([], None, ["  "]):
        assert ngram.hotword_tables(none, tok, "cpu")["hot_keys"].numel() == 0
    with pytest.raises(ValueError, match=r"hotword 'sankt-hans'.*'-'"):
        ngram.hotword_tables(["by", "Sankt-Hans aften"], tok, "cpu")
    with pytest.raises(ValueError, match=r"hotword 'a\|b'.*'\|'"):
        ngram.hotword_tables(["a|b"], tok, "cpu")
    with pytest.raises(TypeError, match="list of strings"):
        ngram.hotword_tables("by", tok, "cpu")


def test_processor_caches_the_hotword_tables_per_word_list():
    from coral_amd.ngram import NGramLM
    from coral_amd.processor import Wav2Vec2ProcessorWithLM, WaveformFeatureExtractor

    proc = Wav2Vec2ProcessorWithLM(WaveformFeatureExtractor(), coral_tokenizer(), NGramLM.from_arpa(ARPA))
    a = proc.hotword_tables(["ab", "ba"], "cpu")
    assert proc.hotword_tables(["AB ba"], "cpu") is a  # the same word set
    assert proc.hotword_tables(["ab"], "cpu") is not a
    assert proc.hotword_tables([], "cpu") is None and proc.hotword_tables(None, "cpu") is None
    assert proc.device_tables("cpu") is proc.device_tables("cpu")  # the LM tables' cache is undisturbed


def test_oracle_choice_takes_the_fewest_errors_and_the_better_rank_on_ties():
    from coral_amd.error_rates import oracle_choice

    #          H  S  D  I
    counts = [[3, 1, 0, 1],   # example 0: 2 errors
              [4, 0, 0, 1],   #            1 error   <- first minimum
              [3, 0, 1, 0],   #            1 error (tie, worse rank)
              [2, 0, 0, 0],   # example 1: 0 errors  <- rank 0 already best
              [1, 1, 0, 0],
              [0, 2, 1, 0],   # example 2: 3 errors
              [0, 1, 1, 1],   #            3 errors (tie)
              [1, 1, 0, 0],   #            1 error   <- last
              [0, 0, 3, 0]]   # example 3: its only hypothesis
    assert oracle_choice(counts, [3, 2, 3, 1]).tolist() == [1, 0, 2, 0]
    with pytest.raises(ValueError, match="oracle_choice"):
        oracle_choice(counts, [3, 2, 3])
    with pytest.raises(ValueError, match="oracle_choice"):
        oracle_choice(counts, [9, 0])


def test_oracle_counts_sends_all_pairs_through_one_launch(monkeypatch):
    from coral_amd import error_rates

    calls = []
    table = {("ab", "ab"): [2, 0, 0, 0], ("ax", "ab"): [1, 1, 0, 0], ("b", "ab"): [1, 0, 1, 0], ("", "cd"): [0, 0, 2, 0],
             ("cd", "cd"): [2, 0, 0, 0], ("c", "cd"): [1, 0, 1, 0], ("d", "cd"): [1, 0, 1, 0]}

    def fake(preds, labels, unit="char", device="cuda", **kw):
        calls.append((list(preds), list(labels), unit))
        return np.array([table[(p, l)] for p, l in zip(preds, labels)], dtype=np.int64)

    monkeypatch.setattr(error_rates, "error_counts", fake)
    res = error_rates.oracle_counts([["ax", "b", "ab"], [], ["c", "d", "cd"]], ["ab", "cd", "cd"], "char", "cpu")
    assert len(calls) == 1 and calls[0][0] == ["ax", "b", "ab", "", "c", "d", "cd"]
    assert calls[0][1] == ["ab"] * 3 + ["cd"] * 4
    assert res["index"].tolist() == [2, -1, 2]
    assert res["counts"].tolist() == [[2, 0, 0, 0], [0, 0, 2, 0], [2, 0, 0, 0]]
    res = error_rates.oracle_counts([["ax", "b"], ["c", "d"]], ["ab", "cd"], "char", "cpu")
    assert res["index"].tolist() == [0, 0]  # equal error counts: the better-ranked hypothesis
    with pytest.raises(ValueError, match="1 n-best lists for 2 labels"):
        error_rates.oracle_counts([["a"]], ["a", "b"])


def test_extended_entry_validates_its_arguments_without_a_gpu():
    from coral_amd import _lib

    lib = _lib.load()
    d, x = _lib.CaCtcBeamDesc(), _lib.CaCtcBeamExt()
    buf = (C.c_char * 64)()
    assert lib.ca_ctc_beam_decode_ex(C.byref(d), None, None) == -1 and b"null extension" in lib.ca_last_error()
    assert lib.ca_ctc_beam_decode_ex(None, C.byref(x), None) == -1 and b"null descriptor" in lib.ca_last_error()
    d.logits = d.ws = C.addressof(buf)  # ids_out / out_len / score_out are not used by this entry
    d.B, d.T, d.V, d.ldv, d.blank, d.delimiter, d.beam_width = 1, 4, 46, 46, 45, 36, 100
    d.beam_prune_logp, d.ws_bytes = -10.0, lib.ca_ctc_beam_workspace_bytes(1, 4, 46, 100)

    def err():
        assert lib.ca_ctc_beam_decode_ex(C.byref(d), C.byref(x), None) == -1
        return lib.ca_last_error()

    for n in (0, 101, -3):
        x.n_best = n
        assert b"n_best %d outside 1..beam_width = 100" % n in err()
    x.n_best = 100
    assert b"null output pointer" in err()
    for name in ("ids_n", "len_n", "score_n", "logit_n", "lm_n"):
        setattr(x, name, C.addressof(buf))
    assert b"null output pointer" in err()  # n_out still missing
    x.n_out = C.addressof(buf)
    x.hot_keys = C.addressof(buf)
    assert b"hotword table pointers without a count" in err()
    x.n_hot = 3
    assert b"3 hotword prefixes without their tables" in err()
    x.n_hot = -1
    assert b"negative hotword table size" in err()
    x.hot_keys, x.n_hot = None, 0
    for bad in (math.inf, -math.inf, math.nan):
        x.hotword_weight = bad
        assert b"hotword_weight must be a finite number" in err()
    # the shared checks still speak for this entry
    x.hotword_weight, d.beam_width = 1.0, 129
    assert b"beam_width 129 outside 1..128" in err()


class _Greedy:
    lm = None


class _WithLM:
    lm = object()
    decoder_params = {}


def test_transcription_arguments_are_refused_by_name():
    from coral_amd.evaluate import transcribe
    from coral_amd.longform import transcribe_long
    from coral_amd.nbest import check_nbest_arguments, nbest_records

    with pytest.raises(ValueError, match="n_best needs the LM-fused beam search.*no LM decoder"):
        transcribe(None, _Greedy(), [], n_best=3)
    with pytest.raises(ValueError, match="hotwords needs the LM-fused beam search.*no LM decoder"):
        transcribe(None, _Greedy(), [], hotwords=["by"])
    with pytest.raises(ValueError, match="n_best=101 is larger than beam_width=100"):
        transcribe(None, _WithLM(), [], n_best=101)
    with pytest.raises(ValueError, match="n_best must be a positive integer"):
        transcribe(None, _WithLM(), [], n_best=0)
    with pytest.raises(ValueError, match="hotword_weight must be a finite number"):
        transcribe(None, _WithLM(), [], hotwords=["by"], hotword_weight=math.inf)
    with pytest.raises(ValueError, match="hotwords is a list"):
        transcribe(None, _WithLM(), [], hotwords="by")
    assert check_nbest_arguments(_WithLM(), None, None, 10.0) is False
    assert check_nbest_arguments(_Greedy(), None, None, 10.0) is False
    assert check_nbest_arguments(_WithLM(), 100, ["by"], 2) is True
    narrow = _WithLM()
    narrow.decoder_params = dict(beam_width=16)
    with pytest.raises(ValueError, match="n_best=17 is larger than beam_width=16"):
        check_nbest_arguments(narrow, 17, None, 10.0)

    class _Model:
        engine = None

    with pytest.raises(ValueError, match="wav2vec2"):  # the chunked path's own refusal comes first, as before
        transcribe_long(_Model(), _Greedy(), [np.zeros(4, dtype=np.float32)], 1.0, n_best=2)

    class _Tok:
        @staticmethod
        def decode(ids, group_tokens=False):
            return "".join("ab|"[i] for i in ids).replace("|", " ")

    rec = nbest_records([dict(ids=[0, 1], score=-1.0, logit_score=-3.0, lm_score=2.0),
                         dict(ids=[1], score=-1.0 + math.log(0.5), logit_score=-2.0, lm_score=1.0 + math.log(0.5))], _Tok())
    assert [r["text"] for r in rec] == ["ab", "b"]
    assert abs(rec[0]["posterior"] - 2 / 3) < 1e-12 and abs(rec[1]["posterior"] - 1 / 3) < 1e-12
    assert nbest_records([], _Tok()) == []


def test_engine_beam_decode_signature_keeps_its_defaults():
    import inspect

    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine

    sig = inspect.signature(Wav2Vec2CTCEngine.beam_decode).parameters
    assert sig["n_best"].default == 1 and sig["hotwords"].default is None and sig["hotword_weight"].default == 10.0
    assert [p for p in sig][:6] == ["self", "lm", "beam_width", "in_len", "tokenizer", "logits"]
