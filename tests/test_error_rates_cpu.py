"""The alignment-count rule of ca_edit_counts and the host side of coral_amd/error_rates.py, without a GPU: the
lexicographic recurrence of tests/edit_ref.py against an enumeration of all optimal alignments, hand cases, tokenisation,
the rate arithmetic, the score table, the refusals and the C ABI's argument check."""
import random
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edit_ref as eref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def test_recurrence_against_all_optimal_alignments():
    from coral_amd.metrics import _edit_distance

    rnd = random.Random(1)
    n_pairs, ambiguous = 3000, 0
    for _ in range(n_pairs):
        r = [rnd.choice("abc") for _ in range(rnd.randint(0, 7))]
        h = [rnd.choice("abc") for _ in range(rnd.randint(0, 7))]
        every = eref.optimal_alignments(r, h)
        H, S, D, I = eref.counts(r, h)
        assert (S, D, I) in every, (r, h, every, (S, D, I))
        assert I == min(x[2] for x in every), (r, h, every, I)
        assert S + D + I == _edit_distance(r, h) and H + S + D == len(r) and H + S + I == len(h), (r, h)
        assert eref.counts_numpy([ord(c) for c in r], [ord(c) for c in h]) == (H, S, D, I), (r, h)
        ambiguous += len({x[2] for x in every}) > 1
    # the rule must be visible: pairs whose optimal alignments differ in their insertion count
    assert ambiguous >= 0.05 * n_pairs, ambiguous


def test_hand_cases():
    assert eref.counts("ab", "ba") == (0, 2, 0, 0)  # two substitutions, not a deletion and an insertion
    assert eref.counts("abc", "") == (0, 0, 3, 0)
    assert eref.counts("", "abc") == (0, 0, 0, 3)
    assert eref.counts("", "") == (0, 0, 0, 0)
    assert eref.counts("hej med dig", "hej med dig") == (11, 0, 0, 0)
    assert eref.counts("abcd", "xabcdyy") == (4, 0, 0, 3)
    assert eref.counts("xabcdyy", "abcd") == (4, 0, 3, 0)
    for r, h in (("ab", "ba"), ("abc", ""), ("", "abc"), ("kitten", "sitting")):
        assert eref.counts_numpy([ord(c) for c in r], [ord(c) for c in h]) == eref.counts(r, h)


def test_anti_diagonal_form_on_larger_pairs():
    rng = np.random.RandomState(5)
    for n, m in ((1, 40), (40, 1), (33, 57), (64, 64), (90, 31)):
        r, h = rng.randint(0, 3, n).tolist(), rng.randint(0, 3, m).tolist()
        assert eref.counts_numpy(r, h) == eref.counts(r, h), (n, m)


def test_tokenisation():
    from coral_amd import error_rates as er

    assert er.tokenise("  hej   med\tdig ", "word") == ["hej", "med\tdig"]  # a single tab is no run of white space
    assert er.tokenise("  hej   med \t dig ", "word") == ["hej", "med", "dig"]
    assert er.tokenise("", "word") == [] and er.tokenise("   ", "word") == []
    assert er.tokenise("  hæj på ", "char") == list("hæj på")
    with pytest.raises(ValueError, match="unit"):
        er.tokenise("a", "byte")
    ids = {}
    toks, off = er._pack(["a b a", "", "c  b"], "word", ids, "label")
    assert toks.tolist() == [0, 1, 0, 2, 1] and off.tolist() == [0, 3, 3, 5] and toks.dtype == np.int32 and off.dtype == np.int64
    toks, off = er._pack([" æb", ""], "char", ids, "label")
    assert toks.tolist() == [ord("æ"), ord("b")] and off.tolist() == [0, 2, 2]


def test_rates_from_counts():
    from coral_amd import error_rates as er

    counts = np.array([[3, 1, 0, 1], [0, 0, 0, 2], [0, 0, 0, 0], [2, 1, 1, 0], [0, 0, 3, 0]])
    assert er.per_example_rates(counts, normalise=True).tolist() == [2 / 5, 1.0, 0.0, 2 / 4, 1.0]
    assert er.per_example_rates(counts, normalise=False).tolist() == [2 / 4, float("inf"), 0.0, 2 / 4, 1.0]
    assert er.per_example_rates(counts).dtype == np.float64
    assert er._rate(counts, True) == 9 / (11 + 3) and er._rate(counts, False) == 9 / 11
    assert er._rate(np.zeros((0, 4)), True) == 0.0


def test_score_table_and_its_skip_rules():
    from coral_amd import error_rates as er

    rows = [dict(age="young", gender="f", dialect="x"), dict(age="old", gender="f", dialect="x"),
            dict(age="young", gender="m", dialect="x"), dict(age="old", gender="f", dialect="x")]
    cc = np.array([[8, 1, 1, 0], [5, 0, 0, 5], [9, 1, 0, 0], [10, 0, 0, 0]])
    wc = np.array([[2, 1, 0, 0], [1, 0, 0, 1], [3, 0, 0, 0], [2, 0, 1, 0]])
    table = er.score_table(rows, ["age", "gender", "dialect"], cc, wc, normalise=True)
    keys = [(t["age"], t["gender"], t["dialect"]) for t in table]
    # dialect = x removes nothing (skipped everywhere); old + m leaves nothing; old + f removes nothing from old
    assert keys == [("young", "f", None), ("young", "m", None), ("young", None, None), ("old", None, None),
                    (None, "f", None), (None, "m", None), (None, None, None)]
    by = dict(zip(keys, table))

    def rate(c, sel, normalise=True):
        return eref.rate(c[sel], normalise)

    assert by[("young", "f", None)]["cer"] == rate(cc, [0]) == 2 / 10
    assert by[("old", None, None)]["cer"] == rate(cc, [1, 3]) == 5 / 20
    assert by[(None, "f", None)]["wer"] == rate(wc, [0, 1, 3]) == 3 / 8
    assert by[(None, None, None)]["cer"] == rate(cc, [0, 1, 2, 3]) and by[(None, None, None)]["wer"] == rate(wc, [0, 1, 2, 3])
    plain = er.score_table(rows, ["age"], cc, wc, normalise=False)
    assert [(t["age"], t["cer"]) for t in plain] == [("young", 3 / 20), ("old", 5 / 15), (None, 8 / 35)]
    assert set(plain[0]) == {"age", "cer", "wer"}
    with pytest.raises(ValueError, match="example 1 has no 'age'"):
        er.score_table([dict(age=1), dict(gender=2)], ["age"], cc[:2], wc[:2])
    with pytest.raises(ValueError, match="2 rows"):
        er.score_table(rows[:2], ["age"], cc, wc)


def test_refusals_need_no_gpu():
    from coral_amd import error_rates as er
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate

    with pytest.raises(ValueError, match="label 1 is empty"):
        er.cer(["a", "b"], ["a", "  "])
    with pytest.raises(ValueError, match="label 0 is empty"):
        er.wer(["a"], [""], normalise=False)
    long_text = "a" * (er.MAX_TOKENS + 1)
    with pytest.raises(ValueError, match=rf"prediction 1 has {er.MAX_TOKENS + 1} char tokens"):
        er.error_counts(["a", long_text], ["a", "b"])
    with pytest.raises(ValueError, match="label 0 has"):
        er.error_counts(["a"], [long_text])
    with pytest.raises(ValueError, match="2 predictions for 1 labels"):
        er.error_counts(["a", "b"], ["a"])
    assert er.error_counts([], []).shape == (0, 4)
    with pytest.raises(ValueError, match="normalise_error_rates"):
        er.check_options("host", True)
    with pytest.raises(ValueError, match="score_categories"):
        er.check_options("host", False, ["age"])
    with pytest.raises(ValueError, match="error_rates must be"):
        er.check_options("gpu", False)
    assert er.check_options("host", False) is False and er.check_options("device", True, ["age"]) is True
    with pytest.raises(ValueError, match="normalise_error_rates"):
        er.text_rates(["a"], ["a"], "host", True)
    assert er.text_rates(["ab c"], ["ab d"], "host", False) == dict(cer=1 / 4, wer=1 / 2)
    # evaluate refuses by name before it loads anything
    ex = [dict(audio=np.zeros(16000, dtype=np.float32), text="a", age="young"), dict(audio=np.zeros(16000, dtype=np.float32), text="b")]
    with pytest.raises(ValueError, match="normalise_error_rates"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "normalise_error_rates=true"]), ex)
    with pytest.raises(ValueError, match="score_categories"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "score_categories=[age]"]), ex)
    with pytest.raises(ValueError, match="example 1 has no 'age'"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "error_rates=device", "score_categories=[age]"]), ex)


def test_config_keys_default_to_the_host_metric():
    from coral_amd.config import load_config

    ev = load_config("evaluation")
    assert ev.error_rates == "host" and ev.normalise_error_rates is False and ev.score_categories is None
    ft = load_config("asr_finetuning", ["model=test-wav2vec2", "datasets=synthetic"])
    assert ft.error_rates == "host" and ft.normalise_error_rates is False


def test_c_abi():
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym in ("ca_edit_counts", "ca_edit_counts_workspace_bytes"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    assert "#define CA_EDIT_MAX_TOKENS ((1 << 20) - 1)" in hdr and _lib.EDIT_MAX_TOKENS == (1 << 20) - 1
    assert int(re.search(r"#define CA_EDIT_WAVE_MAX (\d+)", hdr).group(1)) == _lib.EDIT_WAVE_MAX
    assert int(re.search(r"#define CA_EDIT_PANEL (\d+)", hdr).group(1)) == _lib.EDIT_PANEL
    assert lib.ca_edit_counts(None, None, None, None, None, 1, None, 0, None, 0, None) == -1
    assert b"ca_edit_counts" in lib.ca_last_error()
    # the bound: two boundary columns of 8-byte keys per pair
    assert lib.ca_edit_counts_workspace_bytes(3, 100, 7) == 3 * 2 * 101 * 8
    assert lib.ca_edit_counts_workspace_bytes(1, _lib.EDIT_MAX_TOKENS, _lib.EDIT_MAX_TOKENS) == 2 * (1 << 20) * 8
    assert lib.ca_edit_counts_workspace_bytes(0, 5, 5) == 0
    # the wrapper's host checks come before any device work
    one = np.array([0, 1], dtype=np.int64)
    with pytest.raises(ValueError, match="tokens must be >= 0"):
        ops.edit_counts_plan([-1], one, [1], one)
    with pytest.raises(ValueError, match="ref_off must start at 0"):
        ops.edit_counts_plan([1, 2], one, [1], one)
    with pytest.raises(ValueError, match="permutation"):
        ops.edit_counts_plan([1], one, [1], one, order=[1])
    with pytest.raises(ops.CoralAmdError, match="CA_ERR_ARG.*route 1"):
        ops.edit_counts_plan(np.zeros(_lib.EDIT_WAVE_MAX + 1), [0, _lib.EDIT_WAVE_MAX + 1], [1], one, route=1)
