"""The draw rule of ca_bootstrap_sums and the host side of the bootstrapped rates in coral_amd/error_rates.py, without
a GPU: the rule of tests/bootstrap_ref.py as a generator (uniformity, distinct share, correlations), the bootstrap
standard deviation against the delta method, `intervals_from_sums` on hand values, cluster aggregation, the refusals
and the C ABI's declaration."""
import math
import re
import sys
from pathlib import Path
from statistics import NormalDist

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bootstrap_ref as bref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def test_vectorised_hash_is_the_scalar_hash():
    rng = np.random.RandomState(1)
    idx = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1] + [int(x) for x in rng.randint(0, 1 << 62, 50)]
    for seed in (0, 1, 12345, (1 << 64) - 1):
        got = bref.hash32(seed, np.array(idx, dtype=np.uint64)).tolist()
        assert got == [bref.hash32_scalar(seed, i) for i in idx] and max(got) < 1 << 32
    # k = (u * n) >> 32 at the edges of u
    assert bref.draws(0, 0, 1, 1).tolist() == [[0]]
    n, seed, g, R = 7, 3, 2, 5
    k = bref.draws(seed, g, R, n)
    want = [[(bref.hash32_scalar(seed, ((g * R + r) << 32) | j) * n) >> 32 for j in range(n)] for r in range(R)]
    assert k.tolist() == want
    # the vectorised sums against the definition, on overlapping groups with unordered, repeated members
    rng = np.random.RandomState(2)
    vals = rng.randint(0, 1 << 21, (9, 8))
    members, goff = [3, 1, 1, 8, 0, 5, 8, 2, 2, 7, 4], [0, 4, 5, 11]
    assert np.array_equal(bref.sums(vals, members, goff, 6, 99, chunk=8), bref.sums_one_by_one(vals, members, goff, 6, 99))


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("g", [0, 7])
def test_draw_rule_as_a_generator(seed, g):
    n = R = 1000
    k = bref.draws(seed, g, R, n)
    assert k.min() >= 0 and k.max() < n
    # chi-squared of the index histogram over n cells: expectation n - 1 = 999, sigma sqrt(2 * 999) = 44.7
    hist = np.bincount(k.reshape(-1), minlength=n)
    expect = n * R / n
    chi2 = float(((hist - expect) ** 2 / expect).sum())
    print(f"seed {seed} group {g}: chi2 {chi2:.1f}")
    assert abs(chi2 - 999) <= 6 * 44.7, chi2
    # the share of distinct examples in a replicate: 1 - (1 - 1/n)^n -> 1 - 1/e
    distinct = np.mean([len(np.unique(row)) for row in k]) / n
    print(f"  distinct share {distinct:.4f}")
    assert abs(distinct - (1 - 1 / math.e)) <= 0.01, distinct
    # lag-1 correlation along j inside the replicates, and correlation between neighbouring replicates at equal j
    x = k.astype(np.float64)
    lag1 = np.corrcoef(x[:, :-1].reshape(-1), x[:, 1:].reshape(-1))[0, 1]
    cross = np.corrcoef(x[:-1].reshape(-1), x[1:].reshape(-1))[0, 1]
    print(f"  lag-1 rho {lag1:+.5f}, cross-replicate rho {cross:+.5f}")
    assert abs(lag1) <= 0.01 and abs(cross) <= 0.01, (lag1, cross)


def test_bootstrap_std_against_the_delta_method():
    """The bootstrap standard deviation of the pooled rate sum(e) / sum(d) against its delta-method standard error
    sqrt(sum (e_i - r d_i)^2) / sum(d), r the pooled rate, on N = 4000 synthetic examples with R = 4000 replicates.
    The bound: the sample standard deviation s of R independent, near-normal replicates has relative standard error
    1 / sqrt(2 (R - 1)) (s^2 (R - 1) / sigma^2 is chi-squared with R - 1 degrees of freedom: variance 2 (R - 1), and
    the square root halves the relative error), so the ratio lies within 1 ± 5 / sqrt(2 (R - 1)) = 1 ± 0.056 at five
    sigma.  The delta method's own error is O(1 / N) = 2.5e-4 relative here, below a hundredth of that bound: not added."""
    N = R = 4000
    rng = np.random.RandomState(7)
    den = rng.randint(100, 201, N)  # about 150 characters an example
    err = rng.binomial(den, rng.beta(2, 18, N))  # per-example error rates around 10 %, over-dispersed
    vals = np.stack([err, den, np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)], axis=1)
    s = bref.sums(vals, np.arange(N), [0, N], R, seed=5)[0]
    from coral_amd import error_rates as er

    iv = er.intervals_from_sums(s[:, 0], s[:, 1], err.sum() / den.sum())
    r = err.sum() / den.sum()
    delta = math.sqrt(float(((err - r * den) ** 2).sum())) / den.sum()
    ratio = iv["std"] / delta
    print(f"bootstrap std {iv['std']:.6e}, delta-method se {delta:.6e}, ratio {ratio:.4f}")
    assert abs(ratio - 1) <= 5 / math.sqrt(2 * (R - 1)), ratio


def test_intervals_from_sums_by_hand():
    from coral_amd import error_rates as er

    # three replicates: rates 0.1, 0.2, 0.4
    iv = er.intervals_from_sums([1, 2, 4], [10, 10, 10], point=0.25, confidence=0.95)
    assert set(iv) == {"point", "mean", "std", "half_width", "low", "high"}
    mean = (0.1 + 0.2 + 0.4) / 3
    std = math.sqrt(((0.1 - mean) ** 2 + (0.2 - mean) ** 2 + (0.4 - mean) ** 2) / 2)  # ddof = 1
    assert iv["point"] == 0.25 and iv["mean"] == pytest.approx(mean, rel=1e-15)
    assert iv["std"] == pytest.approx(std, rel=1e-14) and iv["std"] == pytest.approx(0.15275252316519466, rel=1e-14)
    z = NormalDist().inv_cdf(0.975)
    assert z == pytest.approx(1.959963984540054, rel=1e-12) and iv["half_width"] == z * iv["std"]
    # linear quantiles of three sorted values at positions 0.025 * 2 and 0.975 * 2
    assert iv["low"] == pytest.approx(0.1 + 0.05 * (0.2 - 0.1), rel=1e-14)
    assert iv["high"] == pytest.approx(0.2 + 0.95 * (0.4 - 0.2), rel=1e-14)
    # another level: z of 0.9, quantiles at 0.05 and 0.95
    iv90 = er.intervals_from_sums([1, 2, 4], [10, 10, 10], point=0.25, confidence=0.9)
    assert iv90["half_width"] == pytest.approx(1.6448536269514722 * std, rel=1e-12)
    assert iv90["low"] == pytest.approx(0.11, rel=1e-14) and iv90["high"] == pytest.approx(0.38, rel=1e-14)
    # a zero denominator divides by 1, as `_rate` does
    iv0 = er.intervals_from_sums([0, 3, 1], [0, 0, 2], point=0.0)
    assert iv0["mean"] == pytest.approx((0.0 + 3.0 + 0.5) / 3, rel=1e-15)
    assert er._replicate_rates([0, 3, 1], [0, 0, 2]).tolist() == [0.0, 3.0, 0.5]
    # the division is the one of `_rate` on the same integers
    counts = np.array([[7, 2, 1, 3]])
    assert er._replicate_rates([6], [13])[0] == er._rate(counts, True) and er._replicate_rates([6], [10])[0] == er._rate(counts, False)


def test_system_rows_and_cluster_aggregation():
    from coral_amd import error_rates as er

    cc = np.array([[8, 1, 1, 0], [5, 0, 0, 5], [9, 1, 0, 0], [10, 0, 0, 0], [3, 2, 1, 1]])
    wc = np.array([[2, 1, 0, 0], [1, 0, 0, 1], [3, 0, 0, 0], [2, 0, 1, 0], [1, 1, 0, 0]])
    rows = er._system_rows(cc, wc, True)
    assert rows.tolist() == [[2, 10, 1, 3], [5, 10, 1, 2], [1, 10, 0, 3], [0, 10, 1, 3], [4, 7, 1, 2]]
    assert er._system_rows(cc, wc, False).tolist() == [[2, 10, 1, 3], [5, 5, 1, 1], [1, 10, 0, 3], [0, 10, 1, 3], [4, 6, 1, 2]]
    # two clusterings of the same five examples: other rows, the same total
    by_speaker = er.cluster_sums(rows, ["anna", "bo", "anna", "bo", "cleo"])
    assert by_speaker.tolist() == [[3, 20, 1, 6], [5, 20, 2, 5], [4, 7, 1, 2]]  # anna, bo, cleo: first appearance
    by_pair = er.cluster_sums(rows, [1, 1, 0, 0, 0])
    assert by_pair.tolist() == [[7, 20, 2, 5], [5, 27, 2, 8]]
    assert by_speaker.sum(0).tolist() == by_pair.sum(0).tolist() == rows.sum(0).tolist()
    assert er.cluster_sums(rows, list("abcde")).tolist() == rows.tolist()  # every example its own cluster
    with pytest.raises(ValueError, match="4 cluster keys for 5 examples"):
        er.cluster_sums(rows, [1, 2, 3, 4])
    # the units of a score table under clusters: every subset gets the sums of its clusters inside the subset
    masks = [np.array([1, 1, 1, 0, 0], dtype=bool), np.ones(5, dtype=bool)]
    vals, groups = er._resampling_units(rows, masks, ["anna", "bo", "anna", "bo", "cleo"])
    assert vals.tolist() == [[3, 20, 1, 6], [5, 10, 1, 2]] + by_speaker.tolist()
    assert [g.tolist() for g in groups] == [[0, 1], [2, 3, 4]]
    vals, groups = er._resampling_units(rows, masks, None)
    assert vals is rows and [g.tolist() for g in groups] == [[0, 1, 2], [0, 1, 2, 3, 4]]


def test_refusals_need_no_gpu():
    from coral_amd import error_rates as er, ops
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate

    with pytest.raises(ValueError, match="bootstrap_samples needs error_rates: device"):
        er.check_options("host", False, None, 1000)
    with pytest.raises(ValueError, match="n_resamples must be at least 2"):
        er.check_options("device", False, None, 1)
    with pytest.raises(ValueError, match="confidence must lie inside"):
        er.check_options("device", False, None, 100, 1.0)
    with pytest.raises(ValueError, match="bootstrap_cluster needs bootstrap_samples"):
        er.check_options("device", False, None, None, None, "id_speaker")
    assert er.check_options("device", True, ["age"], 1000, 0.9, "id_speaker") is True
    assert er.check_options("host", False) is False and er.check_options("host", False, None, None, 0.95) is False
    cc = np.array([[8, 1, 1, 0], [5, 0, 0, 5]])
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="n_resamples must be at least 2"):
            er.bootstrap_rates(cc, cc, n_resamples=bad)
        with pytest.raises(ValueError, match="n_resamples must be at least 2"):
            er.compare_systems(dict(a=(cc, cc)), n_resamples=bad)
        with pytest.raises(ValueError, match="n_resamples must be at least 2"):
            er.score_table([dict(a=1), dict(a=2)], ["a"], cc, cc, bootstrap=dict(n_resamples=bad))
    with pytest.raises(ValueError, match="n_resamples must be at least 2"):
        er.intervals_from_sums([1], [2], 0.5)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="confidence must lie inside"):
            er.intervals_from_sums([1, 2], [2, 2], 0.5, confidence=bad)
        with pytest.raises(ValueError, match="confidence must lie inside"):
            er.bootstrap_rates(cc, cc, confidence=bad)
    with pytest.raises(ValueError, match="1 .. 8 systems"):
        er.compare_systems({f"s{i}": (cc, cc) for i in range(9)})
    with pytest.raises(ValueError, match="system 'b' has 1 examples, 'a' has 2"):
        er.compare_systems(dict(a=(cc, cc), b=(cc[:1], cc[:1])))
    with pytest.raises(ValueError, match="2 character counts for 1 word counts"):
        er.compare_systems(dict(a=(cc, cc[:1])))
    # the wrapper's host checks come before any device work
    vals = np.arange(12).reshape(3, 4)
    with pytest.raises(ValueError, match="group 1 is empty"):
        er.bootstrap_sums(vals, [[0, 1], [], [2]])
    with pytest.raises(ValueError, match="group 0 is empty"):
        ops.bootstrap_sums(vals, [], [0, 0], 2)
    with pytest.raises(ValueError, match=r"member 2 is 3, outside \[0, 3\)"):
        er.bootstrap_sums(vals, [[0, 1], [3]])
    with pytest.raises(ValueError, match=r"member 0 is -1, outside \[0, 3\)"):
        ops.bootstrap_sums(vals, [-1], [0, 1], 2)
    with pytest.raises(ValueError, match="goff must start at 0, not decrease and end at the 3 members"):
        ops.bootstrap_sums(vals, [0, 1, 2], [0, 2, 1, 3], 2)
    with pytest.raises(ValueError, match="goff must start at 0"):
        ops.bootstrap_sums(vals, [0, 1, 2], [1, 3], 2)
    with pytest.raises(ValueError, match=r"values must lie in \[0, 2\^31\)"):
        ops.bootstrap_sums(vals - 1, [0], [0, 1], 2)
    with pytest.raises(ValueError, match=r"values must lie in \[0, 2\^31\)"):
        ops.bootstrap_sums(vals.astype(np.int64) + (1 << 31), [0], [0, 1], 2)
    with pytest.raises(ValueError, match="C a multiple of 4"):
        ops.bootstrap_sums(np.zeros((3, 6), dtype=np.int32), [0], [0, 1], 2)
    with pytest.raises(ValueError, match="C a multiple of 4"):
        ops.bootstrap_sums(np.zeros((3, 36), dtype=np.int32), [0], [0, 1], 2)
    with pytest.raises(ValueError, match="below 2\\^32"):
        ops.bootstrap_sums(vals, [0, 1], [0, 1, 2], 1 << 31)
    with pytest.raises(ValueError, match="R = 0 must be at least 1"):
        ops.bootstrap_sums(vals, [0], [0, 1], 0)
    # evaluate refuses by name before it loads anything
    ex = [dict(audio=np.zeros(16000, dtype=np.float32), text="a", id_speaker=1), dict(audio=np.zeros(16000, dtype=np.float32), text="b")]
    with pytest.raises(ValueError, match="bootstrap_samples needs error_rates: device"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "bootstrap_samples=200"]), ex)
    with pytest.raises(ValueError, match="n_resamples must be at least 2"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "error_rates=device", "bootstrap_samples=1"]), ex)
    with pytest.raises(ValueError, match="example 1 has no 'id_speaker'"):
        evaluate(load_config("evaluation", ["model_id=nowhere", "error_rates=device", "bootstrap_samples=200",
                                            "bootstrap_cluster=id_speaker"]), ex)


def test_config_keys_default_to_no_bootstrap():
    from coral_amd.config import load_config

    ev = load_config("evaluation")
    assert ev.bootstrap_samples is None and ev.bootstrap_seed == 0 and ev.bootstrap_confidence == 0.95
    assert ev.bootstrap_cluster is None


def test_c_abi():
    from coral_amd import _lib, error_rates as er

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    assert re.search(r"\bca_bootstrap_sums\s*\(", hdr) and "ca_bootstrap_sums" in _lib.SIGNATURES
    assert getattr(lib, "ca_bootstrap_sums") is not None
    assert int(re.search(r"#define CA_BOOTSTRAP_MAX_COLUMNS (\d+)", hdr).group(1)) == _lib.BOOTSTRAP_MAX_COLUMNS == 32
    assert "#define CA_BOOTSTRAP_MAX_GROUP (1 << 24)" in hdr and _lib.BOOTSTRAP_MAX_GROUP == 1 << 24
    assert er.MAX_SYSTEMS == 8
    # the argument check comes before any device work
    assert lib.ca_bootstrap_sums(None, 1, 4, None, 1, None, 1, 1, 0, None, None) == -1
    assert b"ca_bootstrap_sums" in lib.ca_last_error()
