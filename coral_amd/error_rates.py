"""Error rates from alignment counts computed on the GPU (ca_edit_counts, coral_amd/csrc/edit.hip).

For every (prediction, label) pair the kernel returns hits H, substitutions S, deletions D and insertions I of a
minimum-edit-distance alignment; every figure here is arithmetic on those four integers:

    rate = (S + D + I) / (S + D + H)          normalise=False: the reference length, what coral_amd.metrics divides by
    rate = (S + D + I) / (S + D + H + I)      normalise=True: the reference's default (R/src/coral/metrics.py:8-61),
                                              always within 0 .. 1

Optimal alignments are not unique in these counts (two substitutions cost what a deletion plus an insertion cost), and
the normalised denominator depends on the choice.  The rule here: among the minimum-distance alignments, the one with
the fewest insertions (equivalently the fewest deletions and the most substitutions).  jiwer takes its counts from
rapidfuzz's edit operations; neither is available offline, so parity with their own choice among equal-cost alignments
is unpinned, and so are the tokenisations below (jiwer's default transforms as documented).  S + D + I is the edit
distance under any rule, so the unnormalised rates do not depend on it.

`coral_amd.metrics` stays the project's default metric (the reference's normalise=False); this module is opt-in
(`error_rates: device` in the configurations)."""

from __future__ import annotations

import re

import numpy as np

from . import _lib

MAX_TOKENS = _lib.EDIT_MAX_TOKENS

_SPACES = re.compile(r"\s\s+")


def tokenise(text: str, unit: str) -> list:
    """"char": the code points of text.strip().  "word": runs of white space reduced to one space, stripped, split at
    spaces, no empty strings (jiwer's default transforms as documented; unpinned)."""
    if unit == "char":
        return list(text.strip())
    if unit == "word":
        return [w for w in _SPACES.sub(" ", text).strip().split(" ") if w]
    raise ValueError(f"unit must be \"char\" or \"word\", got {unit!r}")


def _pack(texts: list, unit: str, ids: dict, what: str):
    """-> (tokens int32, offsets int64 [n + 1]); words get their ids from `ids`, shared by both sides of the batch."""
    if unit == "char":  # the code points of every stripped text, through one UTF-32 encode of the batch
        rows = [t.strip() for t in texts]
        lens = [len(t) for t in rows]
        toks = np.frombuffer("".join(rows).encode("utf-32-le", "surrogatepass"), dtype="<i4").astype(np.int32)
    else:
        rows = [tokenise(t, unit) for t in texts]
        lens = [len(t) for t in rows]
        toks = np.fromiter((ids.setdefault(w, len(ids)) for r in rows for w in r), dtype=np.int32, count=sum(lens))
    for i, n in enumerate(lens):
        if n > MAX_TOKENS:
            raise ValueError(f"{what} {i} has {n} {unit} tokens, the limit is {MAX_TOKENS} (CA_EDIT_MAX_TOKENS)")
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return toks, off


def error_counts(predictions: list, labels: list, unit: str = "char", device="cuda", *, refuse_empty_labels: bool = False) -> np.ndarray:
    """-> int64 [n, 4]: hits, substitutions, deletions, insertions of every (prediction, label) pair, the label being the
    reference.  Tokenised on the host (`tokenise`), packed into ragged int32 arrays, uploaded in one copy, aligned by
    ca_edit_counts in one launch (largest pairs first), the counts copied back once.  A text of more than
    CA_EDIT_MAX_TOKENS tokens raises ValueError naming its index; so does, with refuse_empty_labels, a label without
    tokens (before anything is uploaded)."""
    from . import ops

    if len(predictions) != len(labels):
        raise ValueError(f"{len(predictions)} predictions for {len(labels)} labels")
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be \"char\" or \"word\", got {unit!r}")
    if not len(labels):
        return np.zeros((0, 4), dtype=np.int64)
    ids: dict = {}
    ref, ref_off = _pack(list(labels), unit, ids, "label")
    empty = np.flatnonzero(np.diff(ref_off) == 0)
    if refuse_empty_labels and len(empty):
        raise ValueError(f"label {int(empty[0])} is empty: an error rate needs a non-empty reference")
    hyp, hyp_off = _pack(list(predictions), unit, ids, "prediction")
    counts = ops.edit_counts(ref, ref_off, hyp, hyp_off, device).cpu().numpy().astype(np.int64)
    if (counts < 0).any():  # the kernel's mark of a pair it could not serve; the host checks above leave none
        raise _lib.CoralAmdError(f"ca_edit_counts left pair {int(np.argwhere(counts < 0)[0, 0])} without a result")
    return counts


def _rate(counts: np.ndarray, normalise: bool) -> float:
    """(S + D + I) / (S + D + H [+ I]) of summed counts; a zero denominator divides by 1 (as coral_amd.metrics does)."""
    h, s, d, i = (int(v) for v in np.asarray(counts, dtype=np.int64).reshape(-1, 4).sum(0))
    return (s + d + i) / max(1, s + d + h + (i if normalise else 0))


def cer(predictions: list, labels: list, normalise: bool = True, device="cuda") -> float:
    """Character error rate over the batch, the reference's signature and default (R/src/coral/metrics.py:8-33):
    (S + D + I) / (S + D + H + I) summed over the pairs, or without the I below with normalise=False.  An empty label
    raises ValueError naming its index: jiwer refuses empty references, and we follow it."""
    return _rate(error_counts(predictions, labels, "char", device, refuse_empty_labels=True), normalise)


def wer(predictions: list, labels: list, normalise: bool = True, device="cuda") -> float:
    """Word error rate over the batch (R/src/coral/metrics.py:36-61); see `cer`."""
    return _rate(error_counts(predictions, labels, "word", device, refuse_empty_labels=True), normalise)


def per_example_rates(counts, normalise: bool = True) -> np.ndarray:
    """-> float64 [n]: every pair's own rate from its counts [n, 4], the per-sample figure a CER filter works on
    (R/src/coral/validation.py:136-159).  A pair whose denominator is 0 (empty reference; with normalise=True also an
    empty prediction) has rate 0 if it has no errors and inf otherwise."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    err = (c[:, 1] + c[:, 2] + c[:, 3]).astype(np.float64)
    den = (c[:, 0] + c[:, 1] + c[:, 2] + (c[:, 3] if normalise else 0)).astype(np.float64)
    out = np.where(err > 0, np.inf, 0.0)
    np.divide(err, den, out=out, where=den > 0)
    return out


def score_table(rows: list, categories: list, char_counts, word_counts, normalise: bool = True) -> list:
    """The behaviour of the reference's per-category score table (R/src/coral/evaluate.py:161-216) without pandas.
    rows: one plain dict per example carrying every category; char_counts / word_counts: int [n, 4] from `error_counts`.
    Every category takes each of its values (in order of first appearance) and then None, meaning all; the combinations
    come in product order, the all-None one (the whole set) last.  A combination is skipped if one of its filters removes
    nothing from what the filters before it left, or leaves nothing; otherwise it is one record {category: value | None,
    ..., "cer": ..., "wer": ...}, each rate a masked sum of the counts."""
    import itertools

    cc = np.asarray(char_counts, dtype=np.int64).reshape(-1, 4)
    wc = np.asarray(word_counts, dtype=np.int64).reshape(-1, 4)
    if not (len(rows) == len(cc) == len(wc)):
        raise ValueError(f"{len(rows)} rows for {len(cc)} character and {len(wc)} word counts")
    categories = list(categories)
    for i, row in enumerate(rows):
        for c in categories:
            if c not in row:
                raise ValueError(f"score_table: example {i} has no {c!r}")
    values = []
    for c in categories:
        seen: dict = {}
        for row in rows:
            seen.setdefault(row[c], None)
        values.append(list(seen) + [None])
    columns = {c: np.array([row[c] for row in rows], dtype=object) for c in categories}
    records = []
    for combo in itertools.product(*values):
        mask = np.ones(len(rows), dtype=bool)
        skip = False
        for c, v in zip(categories, combo):
            if v is None:
                continue
            new = mask & (columns[c] == v)
            if new.sum() == mask.sum() or not new.any():
                skip = True
                break
            mask = new
        if skip:
            continue
        rec = dict(zip(categories, combo))
        rec["cer"], rec["wer"] = _rate(cc[mask], normalise), _rate(wc[mask], normalise)
        records.append(rec)
    return records


def check_options(error_rates, normalise_error_rates, score_categories=None) -> bool:
    """The opt-in keys of the configurations.  -> True when the counts come from the device."""
    mode = "host" if error_rates is None else str(error_rates)
    if mode not in ("host", "device"):
        raise ValueError(f"error_rates must be \"host\" or \"device\", got {error_rates!r}")
    if normalise_error_rates and mode != "device":
        raise ValueError("normalise_error_rates: true needs error_rates: device (the host metric has no alignment counts)")
    if score_categories and mode != "device":
        raise ValueError("score_categories needs error_rates: device (the score table is summed from alignment counts)")
    return mode == "device"


def text_rates(predictions: list, labels: list, error_rates="host", normalise_error_rates=False, device="cuda") -> dict:
    """{"cer", "wer"} of normalised texts, by the `error_rates` / `normalise_error_rates` keys of the finetuning
    configuration: "host" is coral_amd.metrics, as before; "device" takes the same rates from alignment counts."""
    if check_options(error_rates, normalise_error_rates):
        res = batch_scores(predictions, labels, bool(normalise_error_rates), device)
        return dict(cer=res["cer"], wer=res["wer"])
    from .metrics import cer as host_cer, wer as host_wer

    return dict(cer=host_cer(predictions, labels), wer=host_wer(predictions, labels))


def batch_scores(predictions: list, labels: list, normalise: bool = False, device="cuda") -> dict:
    """What the evaluation paths use under `error_rates: device`: {"cer", "wer", "char_counts", "word_counts"}.  With
    normalise=False the two rates are the floats coral_amd.metrics returns for the same texts: the same integers, the
    same division (an empty label adds its errors and no length, as there)."""
    cc = error_counts(predictions, labels, "char", device)
    wc = error_counts(predictions, labels, "word", device)
    return dict(cer=_rate(cc, normalise), wer=_rate(wc, normalise), char_counts=cc, word_counts=wc)
