"""Host side of the LM-fused CTC beam search (no GPU): the ARPA reader and its float64 scoring against hand-computed
values, the device tables and their rolling hash, the test-side prefix beam search against brute force over every
alignment, and the processor round trip."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref as ref  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
ARPA = GOLD / "lm_tiny" / "3gram.arpa"
ARPA_NOUNK = GOLD / "lm_tiny_nounk" / "3gram.arpa"
CHARS = "abcdefghijklmnopqrstuvwxyzæøå0123456789éü"


def coral_tokenizer():
    from coral_amd.processor import CTCTokenizer

    return CTCTokenizer({c: i for i, c in enumerate(sorted(set(CHARS + "|")))})


def tiny_cases():
    """20 seeded cases over {blank = 0, a, b, |}: (logits [T, 4], T)."""
    out = []
    for seed in range(20):
        rng = np.random.RandomState(1000 + seed)
        T = 2 + seed % 3
        out.append((2.0 * rng.randn(T, 4)).astype(np.float32))
    return out


TINY = dict(blank=0, delimiter=3, id2char={1: "a", 2: "b", 3: "|"})
EXHAUSTIVE = dict(beam_width=128, token_min_logp=-math.inf, beam_prune_logp=-math.inf)


def test_arpa_reader_counts_and_hand_computed_probabilities():
    from coral_amd.ngram import NGramLM

    lm = NGramLM.from_arpa(ARPA)
    assert lm.order == 3 and lm.counts == [15, 10, 5] and [len(g) for g in lm.grams] == [15, 10, 5]
    assert {"bæ", "æ", "cæb", "<unk>", "<s>", "</s>"} <= set(lm.words)
    wid = lm.word_id
    s = (wid["<s>"],)
    # stored trigram
    assert abs(lm.logp(s + (wid["a"],), wid["ab"]) - (-0.3)) < 1e-12
    # bigram through the trigram context's back-off: bo(<s> ab) + P(ba | ab)
    assert abs(lm.logp(s + (wid["ab"],), wid["ba"]) - (-0.1 + -0.8)) < 1e-12
    # unigram through two back-offs: bo(<s> a) + bo(a) + P(ba)
    assert abs(lm.logp(s + (wid["a"],), wid["ba"]) - (-0.2 + -0.30 + -1.3)) < 1e-12
    # a context that is no stored n-gram backs off at no cost; a unigram line without a back-off column has 0
    assert abs(lm.logp((wid["bab"], wid["cæb"]), wid["æ"]) - (-1.8)) < 1e-12
    # sentence: <s> a ab </s> = P(a|<s>) + P(ab|<s> a) + P(</s>|a ab)
    assert abs(lm.score(["a", "ab"], True) - (-0.5 + -0.3 + -0.2)) < 1e-12
    assert abs(lm.score(["a", "ab"], False) - (-0.5 + -0.3)) < 1e-12
    # OOV with <unk>: bo(<s>) + P(<unk>), then the context continues as <unk>: P(a | <unk>)
    assert abs(lm.score(["zz", "a"], False) - ((-0.5 + -1.2) + -0.85)) < 1e-12
    # OOV without <unk>: log10 P = 0 and an empty context, then P(a)
    lm2 = NGramLM.from_arpa(ARPA_NOUNK)
    assert lm2.counts == [14, 9, 5] and lm2.unk_id == -1
    assert abs(lm2.score(["zz", "a"], False) - (0.0 + -1.0)) < 1e-12
    # the helper's own reader agrees
    r = ref.RefLM(ARPA)
    assert abs(r.logp(("<s>", "a"), "ba") - (-1.8)) < 1e-12


def test_arpa_reader_accepts_the_reference_eos_line_and_refuses_binaries(tmp_path):
    from coral_amd.ngram import NGramLM

    # what R/src/coral/ngram.py:147-169 writes: the <s> line repeated as </s>, the 1-gram count raised by one
    text = ARPA_NOUNK.read_text(encoding="utf-8").replace("ngram 1=14", "ngram 1=15")
    text = text.replace("-99\t<s>\t-0.5\n", "-99\t<s>\t-0.5\n-99\t</s>\t-0.5\n")
    p = tmp_path / "3gram.arpa"
    p.write_text(text, encoding="utf-8")
    lm = NGramLM.from_arpa(p)
    assert lm.counts[0] == 15 and lm.grams[0][(lm.eos_id,)] == (-99.0, -0.5)
    bad = tmp_path / "short.arpa"
    bad.write_text(text.replace("ngram 2=9", "ngram 2=8"), encoding="utf-8")
    with pytest.raises(ValueError, match="announces 8 2-grams"):
        NGramLM.from_arpa(bad)
    with pytest.raises(ValueError, match="KenLM binary language models cannot be read without KenLM"):
        NGramLM.from_arpa(tmp_path / "3gram.bin")


def test_attrs_json_overrides_defaults_and_anything_else_means_defaults(tmp_path):
    from coral_amd.ngram import DEFAULT_PARAMS, load_attrs

    a = load_attrs(GOLD / "lm_tiny")
    assert a == dict(alpha=0.6, beta=1.2, unk_score_offset=-8.0, score_boundary=True)
    dflt = {k: DEFAULT_PARAMS[k] for k in a}
    assert load_attrs(tmp_path) == dflt
    (tmp_path / "attrs.json").write_text("[1, 2")
    assert load_attrs(tmp_path) == dflt
    (tmp_path / "attrs.json").write_text(json.dumps({"alpha": "x", "beta": 2.0}))
    assert load_attrs(tmp_path) == dict(dflt, beta=2.0)


def test_device_tables_rolling_hash_finds_words_and_prefixes():
    from coral_amd import ngram

    lm = ngram.NGramLM.from_arpa(ARPA)
    tok = coral_tokenizer()
    tb = lm.device_tables(tok, "cpu")
    keys = tb["pfx_keys"].numpy().view(np.uint64)
    wids = tb["pfx_wid"].numpy()
    assert (keys[1:] > keys[:-1]).all()
    look = dict(zip(keys.tolist(), wids.tolist()))

    def h(word):
        return ngram.hash_ids([tok.vocab[c] for c in word], ngram.WORD_SEED)

    spelled = [w for w in lm.words if w not in ("<s>", "</s>", "<unk>")]
    assert len(spelled) == 12
    for w in spelled:
        assert look[h(w)] == lm.word_id[w]
        for n in range(1, len(w)):
            if w[:n] not in spelled:
                assert look[h(w[:n])] == -1, w[:n]
    for non_prefix in ("d", "aa", "abca", "æb", "bb"):
        assert h(non_prefix) not in look
    assert len(look) == len({w[:n] for w in spelled for n in range(1, len(w) + 1)})
    # n-gram segments: sorted inside each order, every stored n-gram found with its values
    nk = tb["ng_keys"].numpy().view(np.uint64)
    assert tb["ng_count"] == [15, 10, 5] and tb["order"] == 3
    off = 0
    for k, g in enumerate(lm.grams):
        seg = nk[off:off + len(g)]
        assert (seg[1:] > seg[:-1]).all()
        for ids, (lp, bo) in g.items():
            i = off + int(np.searchsorted(seg, np.uint64(ngram.hash_ids(ids, ngram.NGRAM_SEED))))
            assert nk[i] == ngram.hash_ids(ids, ngram.NGRAM_SEED)
            assert tb["ng_logp"][i].item() == np.float32(lp) and tb["ng_backoff"][i].item() == np.float32(bo)
        off += len(g)
    assert (tb["bos_wid"], tb["eos_wid"], tb["unk_wid"]) == (lm.word_id["<s>"], lm.word_id["</s>"], lm.word_id["<unk>"])
    # a word with a character the tokenizer cannot spell is left out of the prefix table
    lm.words.append("a-b")
    lm.word_id["a-b"] = len(lm.words) - 1
    assert lm.device_tables(tok, "cpu")["pfx_keys"].numel() == len(look)
    assert ngram.mix64(ngram.WORD_SEED, 3) == ref.mix64(ngram.WORD_SEED, 3)


@pytest.mark.parametrize("mode", ["lm", "lm_nounk", "plain"])
def test_reference_beam_search_is_exhaustive_against_brute_force(mode):
    lm = dict(lm=ref.RefLM(ARPA), lm_nounk=ref.RefLM(ARPA_NOUNK), plain=None)[mode]
    params = dict(alpha=0.0, beta=0.0) if mode == "plain" else {}
    for logits in tiny_cases():
        exact = ref.brute_force(logits, lm=lm, **TINY, **params)
        ids, score, finals = ref.prefix_beam_search(logits, lm=lm, **TINY, **EXHAUSTIVE, **params)
        assert set(finals) == set(exact)
        best = max(exact, key=exact.get)
        assert ids == best and abs(score - exact[best]) < 1e-9
        for y, s in finals.items():
            assert abs(s - exact[y]) < 1e-9


def test_processor_round_trip_and_load_saved_types(tmp_path, caplog):
    from coral_amd.config import DictConfig
    from coral_amd.model_setup import Wav2Vec2ModelSetup
    from coral_amd.ngram import NGramLM
    from coral_amd.processor import (Wav2Vec2Processor, Wav2Vec2ProcessorWithLM, WaveformFeatureExtractor)

    tok = coral_tokenizer()
    proc = Wav2Vec2ProcessorWithLM(WaveformFeatureExtractor(), tok, NGramLM.from_arpa(ARPA), dict(alpha=0.7))
    proc.save_pretrained(tmp_path / "m")
    assert (tmp_path / "m" / "language_model" / "3gram.arpa").exists()
    back = Wav2Vec2ProcessorWithLM.from_pretrained(tmp_path / "m")
    assert back.decoder_params == proc.decoder_params and back.decoder_params["alpha"] == 0.7
    assert back.lm.words == proc.lm.words and back.lm.grams == proc.lm.grams
    ta, tb = proc.device_tables("cpu"), back.device_tables("cpu")
    for k, v in ta.items():
        assert (v.equal(tb[k]) if hasattr(v, "equal") else v == tb[k]), k

    # load_saved: the processor type follows language_model/ and no_lm (the model itself needs the GPU library's engine,
    # so only the processor selection is exercised here)
    import coral_amd.modeling as modeling

    class _NoModel:
        @staticmethod
        def from_pretrained(path):
            return None

    real = modeling.Wav2Vec2ForCTC
    modeling.Wav2Vec2ForCTC = _NoModel
    try:
        def load(d, **kw):
            cfg = DictConfig(model=DictConfig(type="wav2vec2", sampling_rate=16_000), model_dir=str(d), padding="longest",
                             max_seconds_per_example=10)
            return Wav2Vec2ModelSetup(cfg).load_saved(**kw).processor

        assert type(load(tmp_path / "m")) is Wav2Vec2ProcessorWithLM
        assert type(load(tmp_path / "m", no_lm=True)) is Wav2Vec2Processor
        Wav2Vec2Processor(WaveformFeatureExtractor(), tok).save_pretrained(tmp_path / "plain")
        assert type(load(tmp_path / "plain")) is Wav2Vec2Processor
        (tmp_path / "plain" / "language_model").mkdir()
        (tmp_path / "plain" / "language_model" / "3gram.bin").write_bytes(b"mmap lm http://kheafield.com/code format version 5\n")
        with caplog.at_level("WARNING"):
            assert type(load(tmp_path / "plain")) is Wav2Vec2Processor
        assert sum("ARPA" in r.getMessage() for r in caplog.records) == 1
    finally:
        modeling.Wav2Vec2ForCTC = real


def test_beam_decode_validates_arguments_without_a_gpu():
    import ctypes as C

    from coral_amd import _lib

    lib = _lib.load()
    assert lib.ca_ctc_beam_decode(None, None) == -1 and b"null descriptor" in lib.ca_last_error()
    d = _lib.CaCtcBeamDesc()
    buf = (C.c_char * 64)()
    for name in ("logits", "ids_out", "out_len", "score_out", "ws"):
        setattr(d, name, C.addressof(buf))
    d.B, d.T, d.V, d.ldv, d.blank, d.delimiter, d.beam_width = 1, 4, 46, 46, 45, 36, 129
    assert lib.ca_ctc_beam_decode(C.byref(d), None) == -1 and b"beam_width 129 outside 1..128" in lib.ca_last_error()
    d.beam_width, d.V, d.ldv, d.blank = 128, 80, 80, 79
    assert lib.ca_ctc_beam_decode(C.byref(d), None) == -1 and b"LDS layout holds" in lib.ca_last_error()
    d.beam_width, d.V, d.ldv, d.blank, d.order = 100, 46, 46, 45, 3
    assert lib.ca_ctc_beam_decode(C.byref(d), None) == -1 and b"without its tables" in lib.ca_last_error()
    d.order, d.beam_prune_logp, d.ws_bytes = 0, -10.0, 8
    assert lib.ca_ctc_beam_decode(C.byref(d), None) == -1 and b"workspace too small" in lib.ca_last_error()
    assert lib.ca_ctc_beam_workspace_bytes(16, 499, 46, 100) == 16 * 499 * 100 * 8
