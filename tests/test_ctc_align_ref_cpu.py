"""CTC forced alignment without a GPU: the float64 Viterbi reference (tests/ctc_align_ref.py) against a brute force over
every alignment, the tie rule, the C ABI's presence and argument checks, the timestamp_source argument, tokenisation."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_align_ref as aref  # noqa: E402
import longform_ref as lref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
V, BLANK = 3, 2


def _label_strings(max_len):
    out = [[]]
    for n in range(1, max_len + 1):
        out += [list(c) for c in np.ndindex(*([2] * n))]  # ids 0 / 1: every string, repeated labels included
    return out


@pytest.mark.parametrize("quantised", [False, True])
def test_viterbi_equals_the_brute_force_over_every_alignment(quantised):
    rng = np.random.RandomState(5)
    strings = _label_strings(3)
    seen_infeasible = seen_repeat = 0
    for T in range(1, 8):
        x = rng.randn(T, V)
        if quantised:  # many exact ties: the score is still the optimum
            x = np.round(x)
        lp = aref.log_softmax64(x) if not quantised else -np.abs(x) - 1.0
        best = {}
        for frames in np.ndindex(*([V] * T)):
            key = tuple(aref.collapse(frames, BLANK))
            sc = aref.path_score(lp, frames)
            if sc > best.get(key, -np.inf):
                best[key] = sc
        for labels in strings:
            want = best.get(tuple(labels), -np.inf)
            score, start, end = aref.viterbi(lp, labels, BLANK)
            repeats = sum(a == b for a, b in zip(labels, labels[1:]))
            seen_repeat += repeats > 0
            if len(labels) + repeats > T:
                seen_infeasible += 1
                assert want == -np.inf and score == -np.inf and start == end == [-1] * len(labels)
                continue
            assert abs(score - want) <= 1e-12 * max(1.0, abs(want)), (T, labels, score, want)
            aref.check_valid_alignment(start, end, labels, T)
            frames = aref.path_of(start, end, labels, T, BLANK)
            assert aref.collapse(frames, BLANK) == labels
            assert abs(aref.path_score(lp, frames) - score) <= 1e-12 * max(1.0, abs(score))
            if T <= 5:
                assert abs(aref.brute_force(lp, labels, BLANK) - want) <= 1e-12 * max(1.0, abs(want))
    assert seen_infeasible > 0 and seen_repeat > 0
    assert aref.viterbi(np.zeros((0, V)), [0], BLANK)[0] == -np.inf


def test_tie_rule():
    # every frame and symbol equally probable: stay beats s-1 beats s-2, and the final tie takes the last blank state,
    # so the token sits as early as it can and stays one frame
    lp = np.full((3, V), -1.0)
    assert aref.viterbi(lp, [0], BLANK) == (-3.0, [0], [1])
    assert aref.viterbi(lp, [0, 1], BLANK) == (-3.0, [0, 1], [1, 2])
    assert aref.viterbi(lp, [], BLANK) == (-3.0, [], [])


def test_c_abi_and_argument_checks():
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym in ("ca_ctc_align", "ca_ctc_align_workspace_bytes"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    assert int(re.search(r"#define CA_CTC_ALIGN_MAX_LABELS (\d+)", hdr).group(1)) == _lib.CTC_ALIGN_MAX_LABELS == 4095
    assert callable(ops.ctc_align) and callable(ops.ctc_align_workspace_bytes)
    # argument validation needs no GPU
    assert lib.ca_ctc_align(None, 48, None, None, None, None, None, None, None, None, 0, 1, 8, 46, 4, 45, None) == -1
    assert b"ca_ctc_align" in lib.ca_last_error()
    # 2 bits per state and frame, packed, beside one float per frame
    B, T, L = 3, 1000, 4095
    need = lib.ca_ctc_align_workspace_bytes(B, T, L)
    assert B * T * (4 + (2 * L + 1) / 4) <= need <= B * T * (4 + (2 * L + 1) / 4 + 64) + 1024
    assert lib.ca_ctc_align_workspace_bytes(1, 30000, 4000) > 0  # int64 sizes


def test_check_timestamp_mode_takes_the_source():
    from coral_amd import longform as lf

    lf.check_timestamp_mode("word", True, "alignment")
    lf.check_timestamp_mode("char", True, "alignment")
    lf.check_timestamp_mode("word", False, "alignment")
    lf.check_timestamp_mode(None, True, "alignment")
    lf.check_timestamp_mode("char", False, "emission")
    with pytest.raises(ValueError, match="return_timestamps.*LM"):
        lf.check_timestamp_mode("word", True, "emission")
    with pytest.raises(ValueError, match="return_timestamps.*LM.*timestamp_source"):
        lf.check_timestamp_mode("word", True)
    with pytest.raises(ValueError, match="timestamp_source.*'viterbi'"):
        lf.check_timestamp_mode("word", False, "viterbi")
    with pytest.raises(ValueError, match="timestamp_source"):
        lf.check_timestamp_mode(None, False, None)
    with pytest.raises(ValueError, match="return_timestamps"):
        lf.check_timestamp_mode("words", False, "alignment")


def test_align_tokenises_as_the_tokenizer_does():
    from coral_amd import ctc_align as ca
    from coral_amd.processor import CTCTokenizer

    tok = CTCTokenizer(lref.load_fixture()[0]["vocab"])
    texts = ["hej med dig", "", "a  b", "x?y"]
    rows = ca.tokenize(tok, texts)
    assert rows == [tok.encode(t, truncation=False) for t in texts]
    delim = tok.vocab[tok.word_delimiter_token]
    assert rows[0].count(delim) == 2 and rows[2][1:3] == [delim, delim] and rows[1] == []
    assert tok.pad_token_id not in [i for r in rows for i in r]
    long_text = "ab " * 1365  # 4095 tokens: the limit itself passes (no truncation at model_max_length)
    assert len(ca.tokenize(tok, [long_text])[0]) == 4095
    with pytest.raises(ValueError, match="4095"):
        ca.tokenize(tok, [long_text + "a"])
    # word grouping follows longform.word_offsets
    from coral_amd import longform as lf

    ids = rows[2]
    offs = lf.char_offsets(ids, list(range(len(ids))), list(range(1, len(ids) + 1)), tok)
    assert [[offs[i]["char"] for i in g] for g in ca.word_groups(offs)] == [[c for c in w["word"]] for w in lf.word_offsets(offs)]
    chunks = ca.chunks_of(ids, list(range(len(ids))), list(range(1, len(ids) + 1)), [-1.0, -2.0, -3.0, -5.0], tok, "word",
                          320, 16000)
    assert chunks == [{"text": "a", "timestamp": (0.0, 0.02), "score": -1.0},
                      {"text": "b", "timestamp": (0.06, 0.08), "score": -5.0}]
