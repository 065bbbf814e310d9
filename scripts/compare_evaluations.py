#!/usr/bin/env python3
"""Compare two or more evaluated systems on the same test set: bootstrapped CER / WER per system and the paired decision
the model cards' bold and italic marks rest on (the project's counterpart of the reference's comparison script, without
the plot).  Takes the per-example result files that `evaluate` writes with store_results (`prediction,label`), checks
that their label columns are identical row for row, aligns every system's predictions on the GPU (`error_counts`) and
resamples all systems on the same draws in one launch (`compare_systems`).  Prints, and writes to --out, one row per
system and rate: mean ± half_width, whether it is the best system (the lowest bootstrap mean), and whether its paired
difference interval against the best contains 0 (then the two are not told apart by this test set).
    python scripts/compare_evaluations.py a.csv b.csv [c.csv ...] [--n-resamples 1000] [--seed 0] [--confidence 0.95]
        [--no-normalise] [--out comparison.csv] [--device cuda]
A system is named by its file's stem.  At most 8 systems per call."""
import argparse
import csv
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from coral_amd.error_rates import compare_systems, error_counts  # noqa: E402

COLUMNS = ["system", "rate", "point", "mean", "half_width", "low", "high", "best", "difference_to_best_low",
           "difference_to_best_high", "p_better_than_best", "tied_with_best"]


def read_results(path):
    """-> (predictions, labels) of one result file."""
    with open(path, newline="") as f:
        reader = csv.DictReader(f)
        if not {"prediction", "label"} <= set(reader.fieldnames or []):
            raise ValueError(f"{path}: no prediction,label header (got {reader.fieldnames})")
        rows = list(reader)
    return [r["prediction"] for r in rows], [r["label"] for r in rows]


def compare(paths, n_resamples=1000, seed=0, confidence=0.95, normalise=True, device="cuda"):
    """-> (rows of COLUMNS, the result of compare_systems)"""
    if len(paths) < 2:
        raise ValueError("compare_evaluations needs at least two result files")
    names = [Path(p).stem for p in paths]
    if len(set(names)) != len(names):
        raise ValueError(f"the result files must have distinct stems (the systems' names), got {names}")
    systems, labels = {}, None
    for name, path in zip(names, paths):
        preds, labs = read_results(path)
        if labels is None:
            labels, first = labs, path
        elif len(labs) != len(labels):
            raise ValueError(f"{path} has {len(labs)} rows, {first} has {len(labels)}: not the same test set")
        elif labs != labels:
            at = next(i for i, (a, b) in enumerate(zip(labs, labels)) if a != b)
            raise ValueError(f"{path}: the label of row {at} differs from the one in {first}: not the same test set")
        systems[name] = (error_counts(preds, labs, "char", device), error_counts(preds, labs, "word", device))
    res = compare_systems(systems, normalise, n_resamples, seed, confidence, None, device)
    rows = []
    for rate in ("cer", "wer"):
        best = min(names, key=lambda k: res["systems"][k][rate]["mean"])
        for name in names:
            iv = res["systems"][name][rate]
            row = dict(system=name, rate=rate, best=name == best, **{k: iv[k] for k in ("point", "mean", "half_width", "low", "high")})
            if name != best:
                d = res["pairs"][name, best][rate]  # rate(name) - rate(best) on the same resamples
                row.update(difference_to_best_low=d["low"], difference_to_best_high=d["high"], p_better_than_best=d["p_better"],
                           tied_with_best=d["low"] <= 0.0 <= d["high"])
            rows.append(row)
    return rows, res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("results", nargs="+", help="per-example result files (prediction,label) over the same examples")
    ap.add_argument("--n-resamples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--confidence", type=float, default=0.95)
    ap.add_argument("--no-normalise", action="store_true", help="divide by the reference length alone (normalise=False)")
    ap.add_argument("--out", default="comparison.csv")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    try:
        rows, res = compare(args.results, args.n_resamples, args.seed, args.confidence, not args.no_normalise, args.device)
    except ValueError as e:
        raise SystemExit(str(e))
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=COLUMNS, restval="")
        w.writeheader()
        w.writerows(rows)
    for rate in ("cer", "wer"):
        print(f"{rate.upper()}  ({args.n_resamples} resamples, {100 * args.confidence:g} % intervals, seed {args.seed})")
        for row in (r for r in rows if r["rate"] == rate):
            mark = "best" if row["best"] else ("not told apart from the best" if row["tied_with_best"] else
                                               f"worse than the best (p_better {row['p_better_than_best']:.3f})")
            print(f"  {row['system']:30s} {100 * row['mean']:6.2f} % ± {100 * row['half_width']:.2f} %   {mark}")
    print(f"written to {args.out}")
    return rows


if __name__ == "__main__":
    main()
