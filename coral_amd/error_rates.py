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


def score_table(rows: list, categories: list, char_counts, word_counts, normalise: bool = True, *, bootstrap=None) -> list:
    """The behaviour of the reference's per-category score table (R/src/coral/evaluate.py:161-216) without pandas.
    rows: one plain dict per example carrying every category; char_counts / word_counts: int [n, 4] from `error_counts`.
    Every category takes each of its values (in order of first appearance) and then None, meaning all; the combinations
    come in product order, the all-None one (the whole set) last.  A combination is skipped if one of its filters removes
    nothing from what the filters before it left, or leaves nothing; otherwise it is one record {category: value | None,
    ..., "cer": ..., "wer": ...}, each rate a masked sum of the counts.
    bootstrap = dict(n_resamples=1000, seed=0, confidence=0.95, clusters=None, device="cuda") resamples every kept
    combination in one launch of ca_bootstrap_sums, each combination's examples (or, with clusters, its clusters' sums
    inside the combination) one group, and adds BOOTSTRAP_FIELDS to every record (`n`: its examples; the figures of
    `intervals_from_sums` under cer_ / wer_); "cer" / "wer" stay the plug-in rates."""
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
    if bootstrap is not None:  # refused before the table is built
        bootstrap = _bootstrap_options(**bootstrap)
    records, masks = [], []
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
        masks.append(mask)
    if bootstrap is not None:
        system = _system_rows(cc, wc, normalise)
        vals, groups = _resampling_units(system, masks, bootstrap["clusters"])
        sums = bootstrap_sums(vals, groups, bootstrap["n_resamples"], bootstrap["seed"], bootstrap["device"])
        for rec, mask, s in zip(records, masks, sums):
            rec["n"] = int(mask.sum())
            for name, col in (("cer", 0), ("wer", 2)):
                iv = intervals_from_sums(s[:, col], s[:, col + 1], rec[name], bootstrap["confidence"])
                rec.update({f"{name}_{k}": iv[k] for k in INTERVAL_FIELDS})
    return records


def check_options(error_rates, normalise_error_rates, score_categories=None, bootstrap_samples=None,
                  bootstrap_confidence=None, bootstrap_cluster=None) -> bool:
    """The opt-in keys of the configurations.  -> True when the counts come from the device."""
    mode = "host" if error_rates is None else str(error_rates)
    if mode not in ("host", "device"):
        raise ValueError(f"error_rates must be \"host\" or \"device\", got {error_rates!r}")
    if normalise_error_rates and mode != "device":
        raise ValueError("normalise_error_rates: true needs error_rates: device (the host metric has no alignment counts)")
    if score_categories and mode != "device":
        raise ValueError("score_categories needs error_rates: device (the score table is summed from alignment counts)")
    if bootstrap_samples is not None:
        if mode != "device":
            raise ValueError("bootstrap_samples needs error_rates: device (the resampled sums are taken from alignment counts)")
        _check_resampling(bootstrap_samples, 0.95 if bootstrap_confidence is None else bootstrap_confidence)
    elif bootstrap_cluster is not None:
        raise ValueError("bootstrap_cluster needs bootstrap_samples (it names the units that are resampled)")
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


def oracle_choice(counts, sizes) -> np.ndarray:
    """counts int [sum(sizes), 4] (H, S, D, I) of every example's hypotheses in rank order, sizes[i] >= 1 of them for
    example i -> int64 [n]: per example the position (inside its list) of the hypothesis with the fewest errors
    S + D + I; ties go to the better-ranked one."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    sizes = np.asarray(sizes, dtype=np.int64)
    if (sizes < 1).any() or int(sizes.sum()) != len(c):
        raise ValueError(f"oracle_choice: {len(c)} counts for lists of {sizes.tolist()} hypotheses (each at least one)")
    err = c[:, 1] + c[:, 2] + c[:, 3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.array([int(np.argmin(err[a:b])) for a, b in zip(off[:-1], off[1:])], dtype=np.int64)  # argmin: first minimum


def oracle_counts(nbest_texts: list, labels: list, unit: str = "char", device="cuda") -> dict:
    """The oracle error counts of n-best lists: how good the best hypothesis in each list is.  nbest_texts: per example
    its hypotheses, best-ranked first (an empty list counts as the one hypothesis ""); all the (hypothesis, label) pairs
    of the batch go through one ca_edit_counts launch.  -> {"counts": int64 [n, 4] of the chosen hypotheses, "index":
    int64 [n] their positions (-1 for an empty list)}; the choice is `oracle_choice`."""
    if len(nbest_texts) != len(labels):
        raise ValueError(f"{len(nbest_texts)} n-best lists for {len(labels)} labels")
    lists = [list(h) or [""] for h in nbest_texts]
    sizes = [len(h) for h in lists]
    flat = [t for h in lists for t in h]
    counts = error_counts(flat, [l for l, n in zip(labels, sizes) for _ in range(n)], unit, device)
    pick = oracle_choice(counts, sizes) if len(lists) else np.zeros(0, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.int64)
    index = np.where(np.array([len(h) > 0 for h in nbest_texts], dtype=bool), pick, -1) if len(lists) else pick
    return dict(counts=counts[off + pick] if len(lists) else counts, index=index)


# ---- bootstrapped rates (ca_bootstrap_sums, coral_amd/csrc/bootstrap.hip) ----
# The reference's model cards publish every CER / WER as "the mean of 1000 bootstrap resamples ± a 95 % confidence
# interval"; the procedure itself is not in the reference tree, so parity with it is unpinned.  This project's reading:
# a replicate draws n examples with replacement from the n of the set (or of a score-table cell), its rate is the pooled
# rate of the drawn examples (summed errors over summed denominators, the division of `_rate`), and the published form
# is  mean ± z * std  over the replicates.  The sums come from the kernel as exact integers; everything behind them is
# float64 NumPy on the host.

MAX_SYSTEMS = _lib.BOOTSTRAP_MAX_COLUMNS // 4  # systems side by side in one launch: four columns each
INTERVAL_FIELDS = ("mean", "std", "half_width", "low", "high")
BOOTSTRAP_FIELDS = ("n",) + tuple(f"{rate}_{k}" for rate in ("cer", "wer") for k in INTERVAL_FIELDS)


def _check_resampling(n_resamples, confidence) -> None:
    if int(n_resamples) < 2:
        raise ValueError(f"n_resamples must be at least 2 (a standard deviation needs two replicates), got {n_resamples!r}")
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence must lie inside (0, 1), got {confidence!r}")


def _bootstrap_options(n_resamples=1000, seed=0, confidence=0.95, clusters=None, device="cuda") -> dict:
    _check_resampling(n_resamples, confidence)
    return dict(n_resamples=int(n_resamples), seed=int(seed), confidence=float(confidence), clusters=clusters, device=device)


def _system_rows(char_counts, word_counts, normalise: bool) -> np.ndarray:
    """-> int64 [n, 4]: character errors, character denominator, word errors, word denominator of every example, the
    integers `_rate` sums: S + D + I over S + D + H (+ I with normalise)."""
    cc = np.asarray(char_counts, dtype=np.int64).reshape(-1, 4)
    wc = np.asarray(word_counts, dtype=np.int64).reshape(-1, 4)
    if len(cc) != len(wc):
        raise ValueError(f"{len(cc)} character counts for {len(wc)} word counts")
    out = np.empty((len(cc), 4), dtype=np.int64)
    for at, c in ((0, cc), (2, wc)):
        out[:, at] = c[:, 1] + c[:, 2] + c[:, 3]
        out[:, at + 1] = c[:, 0] + c[:, 1] + c[:, 2] + (c[:, 3] if normalise else 0)
    return out


def _cluster_codes(clusters, n: int) -> np.ndarray:
    """-> int64 [n]: every example's cluster, numbered in order of first appearance."""
    clusters = list(clusters)
    if len(clusters) != n:
        raise ValueError(f"{len(clusters)} cluster keys for {n} examples")
    seen: dict = {}
    return np.fromiter((seen.setdefault(k, len(seen)) for k in clusters), dtype=np.int64, count=n)


def cluster_sums(values, clusters) -> np.ndarray:
    """values int [n, C] summed per cluster -> int64 [clusters, C], the clusters in order of first appearance.
    clusters: one hashable key per example (the speaker id, say).  The cluster bootstrap resamples these rows: utterances
    of one speaker are not independent, whole speakers are drawn."""
    values = np.asarray(values, dtype=np.int64)
    codes = _cluster_codes(clusters, len(values))
    out = np.zeros((int(codes.max()) + 1 if len(codes) else 0, values.shape[1]), dtype=np.int64)
    np.add.at(out, codes, values)
    return out


def _resampling_units(rows: np.ndarray, masks: list, clusters):
    """The table and the groups of one launch for several subsets (boolean masks) of the examples.  Without clusters the
    examples' own rows, each subset's indices one group; with clusters every subset gets rows of its own behind the
    others: the sums of each of its clusters over the subset's examples."""
    if clusters is None:
        return rows, [np.flatnonzero(m) for m in masks]
    codes = _cluster_codes(clusters, len(rows))
    parts, groups, pos = [], [], 0
    for m in masks:
        at = np.flatnonzero(m)
        part = cluster_sums(rows[at], codes[at].tolist())
        parts.append(part)
        groups.append(np.arange(pos, pos + len(part)))
        pos += len(part)
    return np.concatenate(parts), groups


def bootstrap_sums(values, groups=None, n_resamples: int = 1000, seed: int = 0, device="cuda") -> np.ndarray:
    """-> int64 [G, n_resamples, C]: for every group and replicate the column sums of as many rows of `values`
    (int [N, C] >= 0, C at most CA_BOOTSTRAP_MAX_COLUMNS) as the group has members, drawn from it with replacement by
    ca_bootstrap_sums (the draw rule: include/coral_amd.h).  groups: a list of index arrays, which may overlap; None =
    one group holding every example.  The columns are padded to a multiple of 4 here; one upload, one launch, one copy
    back (`ops.bootstrap_sums`, which also checks the values and the indices)."""
    from . import ops

    values = np.asarray(values)
    if values.ndim != 2:
        raise ValueError(f"bootstrap_sums: values must be [N, C], got {list(values.shape)}")
    N, Cn = values.shape
    if groups is None:
        groups = [np.arange(N)]
    groups = [np.asarray(g).reshape(-1) for g in groups]
    goff = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    members = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
    if Cn % 4:
        values = np.concatenate([values, np.zeros((N, 4 - Cn % 4), dtype=values.dtype)], axis=1)
    return ops.bootstrap_sums(values, members, goff, n_resamples, seed, device)[:, :, :Cn]


def _replicate_rates(err_sums, den_sums) -> np.ndarray:
    """Every replicate's pooled rate, float64: err / max(1, den), the division of `_rate`."""
    err, den = np.asarray(err_sums, dtype=np.int64).reshape(-1), np.asarray(den_sums, dtype=np.int64).reshape(-1)
    if len(err) != len(den):
        raise ValueError(f"{len(err)} error sums for {len(den)} denominator sums")
    return err.astype(np.float64) / np.maximum(1, den).astype(np.float64)


def _interval(values: np.ndarray, point: float, confidence: float) -> dict:
    from statistics import NormalDist

    _check_resampling(len(values), confidence)
    z = NormalDist().inv_cdf((1.0 + confidence) / 2.0)
    std = float(values.std(ddof=1))
    low, high = np.quantile(values, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
    return dict(point=float(point), mean=float(values.mean()), std=std, half_width=z * std, low=float(low), high=float(high))


def intervals_from_sums(err_sums, den_sums, point: float, confidence: float = 0.95) -> dict:
    """One rate's bootstrap figures from its replicates' integer sums (int [R] each), float64 NumPy throughout:
    {"point": the plug-in rate as given, "mean", "std" (ddof = 1), "half_width" = z * std with z =
    NormalDist().inv_cdf((1 + confidence) / 2), "low" / "high": the percentile interval (np.quantile, linear)}.  The
    published form is mean ± half_width.  Fewer than 2 replicates, or a confidence outside (0, 1), raise ValueError."""
    return _interval(_replicate_rates(err_sums, den_sums), point, confidence)


def bootstrap_rates(char_counts, word_counts, normalise: bool = True, n_resamples: int = 1000, seed: int = 0,
                    confidence: float = 0.95, clusters=None, device="cuda") -> dict:
    """{"cer": interval, "wer": interval} (`intervals_from_sums`) of the whole set from counts [n, 4] (`error_counts`).
    clusters: one key per example (e.g. the speaker id): the counts are summed per cluster first and whole clusters are
    resampled (the cluster bootstrap, for utterances that are not independent); the same kernel on fewer rows."""
    _check_resampling(n_resamples, confidence)
    rows = _system_rows(char_counts, word_counts, normalise)
    point = rows.sum(0)
    if clusters is not None:
        rows = cluster_sums(rows, clusters)
    s = bootstrap_sums(rows, None, n_resamples, seed, device)[0]
    return {name: intervals_from_sums(s[:, col], s[:, col + 1], int(point[col]) / max(1, int(point[col + 1])), confidence)
            for name, col in (("cer", 0), ("wer", 2))}


def compare_systems(systems: dict, normalise: bool = True, n_resamples: int = 1000, seed: int = 0,
                    confidence: float = 0.95, clusters=None, device="cuda") -> dict:
    """Several systems on the same examples, compared on the same resamples.  systems: {name: (char_counts,
    word_counts)}, at most MAX_SYSTEMS of them, every count array over the same examples in the same order.  Their
    columns are stacked side by side and go through one launch, so every replicate draws the same examples for all of
    them (a paired comparison).
    -> {"systems": {name: {"cer": interval, "wer": interval}},
        "pairs": {(a, b): {"cer": d, "wer": d}} for every ordered pair a != b, d the interval of rate(a) - rate(b) per
        replicate plus "p_better": the share of replicates in which a has the lower rate, ties counting half,
        "n_resamples", "seed", "confidence"}."""
    _check_resampling(n_resamples, confidence)
    names = list(systems)
    if not 1 <= len(names) <= MAX_SYSTEMS:
        raise ValueError(f"compare_systems takes 1 .. {MAX_SYSTEMS} systems per launch, got {len(names)}")
    rows = [_system_rows(*systems[k], normalise) for k in names]
    for k, r in zip(names, rows):
        if len(r) != len(rows[0]):
            raise ValueError(f"system {k!r} has {len(r)} examples, {names[0]!r} has {len(rows[0])}: the systems must be "
                             "scored on the same examples")
    stacked = np.concatenate(rows, axis=1)
    point = stacked.sum(0)
    if clusters is not None:
        stacked = cluster_sums(stacked, clusters)
    s = bootstrap_sums(stacked, None, n_resamples, seed, device)[0]
    rates, points, out = {}, {}, dict(systems={}, pairs={}, n_resamples=int(n_resamples), seed=int(seed), confidence=float(confidence))
    for i, k in enumerate(names):
        for name, col in (("cer", 4 * i), ("wer", 4 * i + 2)):
            rates[k, name] = _replicate_rates(s[:, col], s[:, col + 1])
            points[k, name] = int(point[col]) / max(1, int(point[col + 1]))
        out["systems"][k] = {name: _interval(rates[k, name], points[k, name], confidence) for name in ("cer", "wer")}
    for a in names:
        for b in names:
            if a == b:
                continue
            pair = {}
            for name in ("cer", "wer"):
                d = rates[a, name] - rates[b, name]
                pair[name] = _interval(d, points[a, name] - points[b, name], confidence)
                pair[name]["p_better"] = float(((d < 0).sum() + 0.5 * (d == 0).sum()) / len(d))
            out["pairs"][a, b] = pair
    return out
