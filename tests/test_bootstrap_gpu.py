"""ca_bootstrap_sums on the GPU (coral_amd/csrc/bootstrap.hip) against tests/bootstrap_ref.py, exact integer equality
throughout: every group size at which the lanes' stride, the draws in flight or the tail change, every row width class,
overlapping groups, sums beyond 2^31, determinism and paired draws, the C entry behind the host checks, and the host
side around it (`compare_systems`, `score_table(bootstrap=...)`, `evaluate` on the fixture checkpoint)."""
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bootstrap_ref as bref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
UNWRITTEN = -7  # the kernel writes sums >= 0, or -1 for a group it cannot serve
GROUP_SIZES = (1, 2, 63, 64, 65, 257, 5000)  # around one wave's stride (64), U strides in flight (256 at C = 4, 8), many trips


def _groups(rng, n, G, N):
    """G groups of n members each out of N examples.  G = 1: every example once, in order (n = N).  Otherwise drawn
    with replacement and unsorted: the groups overlap and members repeat."""
    if G == 1:
        return np.arange(n), np.array([0, n])
    return rng.randint(0, N, G * n), np.arange(G + 1) * n


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("C", [4, 8, 32])
def test_sums_equal_the_restatement(C, G):
    from coral_amd import ops

    rng = np.random.RandomState(100 * C + G)
    for n in GROUP_SIZES:
        N = n if G == 1 else max(4, (2 * n) // 3)  # fewer examples than draws: repeats inside a group
        vals = rng.randint(0, 1000, (N, C))
        members, goff = _groups(rng, n, G, N)
        assert G == 1 or len(np.unique(members)) < len(members)
        for R in (1, 3, 64) + ((1000,) if n == 65 else ()):
            seed = int(rng.randint(0, 1 << 62))
            got = ops.bootstrap_sums(vals, members, goff, R, seed)
            assert got.dtype == np.int64 and got.shape == (G, R, C)
            want = bref.sums(vals, members, goff, R, seed)
            assert np.array_equal(got, want), (n, C, R, G, np.argwhere(got != want)[:4].tolist())


def test_sums_beyond_int32():
    from coral_amd import ops

    rng = np.random.RandomState(21)
    n = 5000
    vals = rng.randint((1 << 21) - 1000, 1 << 21, (n, 4))
    vals[:, 3] = (1 << 31) - 1  # the largest value the contract allows
    got = ops.bootstrap_sums(vals, np.arange(n), [0, n], 3, 17)
    assert np.array_equal(got, bref.sums(vals, np.arange(n), [0, n], 3, 17))
    assert (got[:, :, :3] > 1 << 31).all() and (got[:, :, 3] == n * ((1 << 31) - 1)).all()


def test_determinism_seed_group_index_and_paired_columns():
    from coral_amd import ops

    rng = np.random.RandomState(22)
    n, R = 300, 16
    vals8 = rng.randint(0, 5000, (n, 8))
    members = rng.permutation(n)
    first = ops.bootstrap_sums(vals8, members, [0, n], R, 5)
    assert np.array_equal(ops.bootstrap_sums(vals8, members, [0, n], R, 5), first)  # bit-identical from run to run
    assert not np.array_equal(ops.bootstrap_sums(vals8, members, [0, n], R, 6)[0], first[0])  # another seed, other sums
    # the same group under another group index draws differently (the index is part of the hash input)
    twice = ops.bootstrap_sums(vals8, np.concatenate([members, members]), [0, n, 2 * n], R, 5)
    assert np.array_equal(twice[0], first[0]) and not np.array_equal(twice[1], first[0])
    assert np.array_equal(twice, bref.sums(vals8, np.concatenate([members, members]), [0, n, 2 * n], R, 5))
    # paired draws: every column sees the same draws, whatever stands beside it
    assert np.array_equal(ops.bootstrap_sums(vals8[:, :4], members, [0, n], R, 5), first[:, :, :4])
    assert np.array_equal(ops.bootstrap_sums(vals8[:, 4:], members, [0, n], R, 5), first[:, :, 4:])


def run_raw(vals, members, goff, R, seed, n_table=None, override=None):
    """The C entry point on device buffers built here: sums pre-filled, the table followed by rows that must not be read.
    -> (return code, int64 [G, R, C])"""
    from coral_amd import _lib

    vals = np.ascontiguousarray(vals, dtype=np.int32)
    N, C = vals.shape
    G = len(goff) - 1
    table = torch.from_numpy(np.concatenate([vals, np.full((8, C), 1 << 30, dtype=np.int32)])).cuda()
    mem = torch.from_numpy(np.concatenate([np.asarray(members, dtype=np.int32), np.zeros(64, dtype=np.int32)])).cuda()
    off = torch.from_numpy(np.asarray(goff, dtype=np.int64)).cuda()
    sums = torch.full((G, max(1, min(R, 4096)), C), UNWRITTEN, dtype=torch.int64, device="cuda")
    args = dict(vals=table.data_ptr(), N=N if n_table is None else n_table, C=C, members=mem.data_ptr(), n_members=len(members),
                goff=off.data_ptr(), G=G, R=R, seed=seed, sums=sums.data_ptr())
    args.update(override or {})
    rc = _lib.load().ca_bootstrap_sums(args["vals"], args["N"], args["C"], args["members"], args["n_members"], args["goff"],
                                       args["G"], args["R"], args["seed"], args["sums"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy()


def test_c_entry_behind_the_host_checks():
    from coral_amd import _lib

    rng = np.random.RandomState(23)
    vals = rng.randint(0, 100, (10, 4))
    members, goff = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 2, 7], [0, 10, 13]
    rc, got = run_raw(vals, members, goff, 5, 3)
    assert rc == 0 and np.array_equal(got, bref.sums(vals, members, goff, 5, 3))
    # refused before any launch: the output keeps its fill
    for bad in (dict(vals=None), dict(members=None), dict(goff=None), dict(sums=None), dict(C=6), dict(C=0), dict(C=36),
                dict(R=0), dict(G=0), dict(G=2, R=1 << 31), dict(G=1, R=1 << 32), dict(N=0)):
        rc, got = run_raw(vals, members, goff, 5, 3, override=bad)
        assert rc == -1 and b"ca_bootstrap_sums" in _lib.load().ca_last_error(), bad
        assert (got == UNWRITTEN).all(), bad
    # offsets the contract does not allow (an empty group, a group that ends behind the members): the group is marked,
    # nothing is read through them, and the other group is served
    want = bref.sums(vals, members, goff, 5, 3)
    rc, got = run_raw(vals, members, [0, 10, 10], 5, 3)
    assert rc == 0 and np.array_equal(got[0], want[0]) and (got[1] == -1).all()
    rc, got = run_raw(vals, members, [0, 10, 14], 5, 3)
    assert rc == 0 and np.array_equal(got[0], want[0]) and (got[1] == -1).all()
    rc, got = run_raw(vals, members, [-1, 10, 13], 5, 3)
    assert rc == 0 and (got[0] == -1).all() and np.array_equal(got[1], want[1])
    # a member outside the table (here: a table declared 7 rows long) adds nothing
    rc, got = run_raw(vals, members, goff, 5, 3, n_table=7)
    trimmed = vals.copy()
    trimmed[7:] = 0
    assert rc == 0 and np.array_equal(got, bref.sums(trimmed, members, goff, 5, 3))


def _synthetic_counts(rng, n, rate=0.1):
    """int64 [n, 4] hits, substitutions, deletions, insertions of n examples of about 150 characters."""
    length = rng.randint(120, 181, n)
    s, d, i = (rng.binomial(length, rate / 3) for _ in range(3))
    return np.stack([length - s - d, s, d, i], axis=1).astype(np.int64)


def test_compare_systems():
    from coral_amd import error_rates as er

    rng = np.random.RandomState(24)
    cc, wc = _synthetic_counts(rng, 150), _synthetic_counts(rng, 150, 0.3)
    worse_c, worse_w = cc.copy(), wc.copy()
    worse_c[:, 0] -= 1  # one hit of every example becomes a substitution: one more error, the same denominator
    worse_c[:, 1] += 1
    worse_w[:, 0] -= 1
    worse_w[:, 1] += 1
    res = er.compare_systems(dict(a=(cc, wc), same=(cc, wc), worse=(worse_c, worse_w)), n_resamples=100, seed=9)
    assert set(res) == {"systems", "pairs", "n_resamples", "seed", "confidence"} and len(res["pairs"]) == 6
    assert res["systems"]["a"] == res["systems"]["same"]
    for rate in ("cer", "wer"):
        d = res["pairs"]["a", "same"][rate]  # a system against itself: every replicate difference is exactly 0
        assert d["p_better"] == 0.5 and d["mean"] == d["std"] == d["low"] == d["high"] == d["point"] == 0.0
        better = res["pairs"]["a", "worse"][rate]
        assert better["p_better"] == 1.0 and better["high"] < 0 and res["pairs"]["worse", "a"][rate]["p_better"] == 0.0
        iv = res["systems"]["a"][rate]
        assert iv["low"] <= iv["mean"] <= iv["high"] and iv["half_width"] > 0
    # the stacked launch is the single launch of each system's own columns (paired draws), and the restatement's
    rows = er._system_rows(cc, wc, True)
    s = bref.sums(rows, np.arange(150), [0, 150], 100, 9)[0]
    assert res["systems"]["a"]["cer"] == er.intervals_from_sums(s[:, 0], s[:, 1], er._rate(cc, True))
    assert er.bootstrap_rates(cc, wc, n_resamples=100, seed=9) == res["systems"]["a"]
    # clusters: the same kernel on the summed rows
    keys = rng.randint(0, 20, 150).tolist()
    by = er.cluster_sums(rows, keys)
    s = bref.sums(by, np.arange(len(by)), [0, len(by)], 100, 9)[0]
    got = er.bootstrap_rates(cc, wc, n_resamples=100, seed=9, clusters=keys)
    assert got["wer"] == er.intervals_from_sums(s[:, 2], s[:, 3], er._rate(wc, True)) and got["cer"]["point"] == er._rate(cc, True)


def test_score_table_with_bootstrap():
    from coral_amd import error_rates as er

    rng = np.random.RandomState(25)
    n = 200
    rows = [dict(age=str(rng.choice(["young", "old", "middle"])), gender=str(rng.choice(["f", "m"])),
                 dialect=str(rng.choice(["x", "y", "z", "w"]))) for _ in range(n)]
    cc, wc = _synthetic_counts(rng, n), _synthetic_counts(rng, n, 0.3)
    cats = ["age", "gender", "dialect"]
    plain = er.score_table(rows, cats, cc, wc, normalise=True)
    boot = er.score_table(rows, cats, cc, wc, normalise=True, bootstrap=dict(n_resamples=50, seed=4, confidence=0.9))
    assert len(boot) == len(plain) == 4 * 3 * 5 and all(set(b) == set(p) | set(er.BOOTSTRAP_FIELDS) for b, p in zip(boot, plain))
    assert [{k: b[k] for k in p} for b, p in zip(boot, plain)] == plain  # the records and the plug-in rates as without it
    # the interval fields: the restatement's integers through the same float64 code, to the last bit
    sysrows = er._system_rows(cc, wc, True)
    groups = [np.flatnonzero([all(rec[c] is None or row[c] == rec[c] for c in cats) for row in rows]) for rec in plain]
    goff = np.concatenate(([0], np.cumsum([len(g) for g in groups])))
    want = bref.sums(sysrows, np.concatenate(groups), goff, 50, 4)
    for rec, g, s in zip(boot, groups, want):
        assert rec["n"] == len(g)
        for rate, col in (("cer", 0), ("wer", 2)):
            iv = er.intervals_from_sums(s[:, col], s[:, col + 1], rec[rate], 0.9)
            assert {k: rec[f"{rate}_{k}"] for k in er.INTERVAL_FIELDS} == {k: iv[k] for k in er.INTERVAL_FIELDS}
    assert boot[-1]["n"] == n and boot[-1]["cer_low"] <= boot[-1]["cer_mean"] <= boot[-1]["cer_high"]
    # with clusters every cell resamples the sums of its clusters inside the cell
    keys = rng.randint(0, 30, n).tolist()
    clustered = er.score_table(rows, cats, cc, wc, bootstrap=dict(n_resamples=50, seed=4, clusters=keys))
    vals, cgroups = er._resampling_units(sysrows, [np.isin(np.arange(n), g) for g in groups], keys)
    cwant = bref.sums(vals, np.concatenate(cgroups), np.concatenate(([0], np.cumsum([len(g) for g in cgroups]))), 50, 4)
    for rec, s in zip(clustered, cwant):
        assert rec["wer_std"] == er.intervals_from_sums(s[:, 2], s[:, 3], rec["wer"])["std"]


def test_evaluate_with_bootstrap(tmp_path, monkeypatch):
    import csv

    from coral_amd import error_rates as er
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.processor import dump_vocabulary

    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "ckpt"
    shutil.copytree(GOLDEN / "engine_ckpt_w2v2", mdir)
    dump_vocabulary(load_config("evaluation").characters_to_keep, mdir)
    rng = np.random.RandomState(15)
    texts = ["hej med dig", "det er en god dag", "å", "jeg hedder anna", "to tre fire", "ø æ å", "hvad sker der her", "nej"]
    examples = [dict(audio=(0.1 * rng.randn(int(16_000 * s))).astype(np.float32), text=t, age_group=a, gender=g, id_speaker=k)
                for s, t, a, g, k in zip((1.0, 1.5, 0.8, 2.0, 1.2, 0.9, 1.7, 1.1), texts, "yoyyooyo", "ffmmfmff", "abcabcab")]
    cats = ["age_group", "gender"]

    def run(*overrides):
        return evaluate(load_config("evaluation", [f"model_id={mdir}", "batch_size=4", "dataset=synthetic", "error_rates=device",
                                                   "score_categories=[age_group,gender]", *overrides]), examples)

    plain = run()
    assert "bootstrap" not in plain and all(set(t) == set(cats) | {"cer", "wer"} for t in plain["score_table"])
    assert next(csv.reader(open(plain["scores_csv"]))) == cats + ["cer", "wer"]
    boot = run("bootstrap_samples=200", "bootstrap_seed=3")
    assert set(boot) == set(plain) | {"bootstrap"}
    b = boot["bootstrap"]
    assert set(b) == {"cer", "wer", "n_resamples", "seed", "confidence"} and (b["n_resamples"], b["seed"], b["confidence"]) == (200, 3, 0.95)
    for rate in ("cer", "wer"):
        assert b[rate]["low"] <= b[rate]["mean"] <= b[rate]["high"] and b[rate]["point"] == boot[rate] == plain[rate]
    assert [{k: t[k] for k in p} for t, p in zip(boot["score_table"], plain["score_table"])] == plain["score_table"]
    assert all(set(t) == set(cats) | {"cer", "wer"} | set(er.BOOTSTRAP_FIELDS) for t in boot["score_table"])
    assert next(csv.reader(open(boot["scores_csv"]))) == cats + ["cer", "wer"] + list(er.BOOTSTRAP_FIELDS)
    rows = list(csv.DictReader(open(boot["scores_csv"])))
    assert [float(r["cer_half_width"]) for r in rows] == [t["cer_half_width"] for t in boot["score_table"]]
    clustered = run("bootstrap_samples=200", "bootstrap_seed=3", "bootstrap_cluster=id_speaker")
    assert clustered["bootstrap"]["cer"]["point"] == plain["cer"] and clustered["score_table"][-1]["n"] == 8


def test_compare_evaluations_script(tmp_path, capsys):
    import csv
    import importlib.util

    spec = importlib.util.spec_from_file_location("compare_evaluations", Path(__file__).resolve().parents[1] / "scripts" / "compare_evaluations.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.RandomState(26)
    words = ["hej", "med", "dig", "det", "er", "en", "god", "dag", "jeg", "hedder", "anna", "to", "tre", "fire"]
    labels = [" ".join(rng.choice(words, rng.randint(3, 9))) for _ in range(60)]
    bad = [lab.replace("e", "a", 1) + " øh" for lab in labels]  # one substituted letter (where there is an e) and a word more

    def write(name, preds, labs=labels):
        with open(tmp_path / name, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["prediction", "label"])
            w.writerows(zip(preds, labs))
        return str(tmp_path / name)

    good, copy, worse = write("good.csv", labels), write("copy.csv", labels), write("worse.csv", bad)
    rows = tool.main([good, copy, worse, "--n-resamples", "100", "--out", str(tmp_path / "cmp.csv")])
    by = {(r["system"], r["rate"]): r for r in rows}
    for rate in ("cer", "wer"):
        assert by["good", rate]["best"] and by["good", rate]["mean"] == 0.0  # (the first of equal means)
        assert by["copy", rate]["tied_with_best"] and by["copy", rate]["p_better_than_best"] == 0.5
        assert not by["worse", rate]["tied_with_best"] and by["worse", rate]["p_better_than_best"] == 0.0
        assert by["worse", rate]["difference_to_best_low"] > 0
    out = capsys.readouterr().out
    assert "not told apart from the best" in out and "worse than the best" in out
    written = list(csv.DictReader(open(tmp_path / "cmp.csv")))
    assert len(written) == 6 and list(written[0]) == tool.COLUMNS
    with pytest.raises(SystemExit, match="label of row 0 differs"):
        tool.main([good, write("other.csv", labels, ["x"] + labels[1:])])
    with pytest.raises(SystemExit, match="at least two"):
        tool.main([good])
