"""Restatement of the alignment counts of ca_edit_counts (coral_amd/csrc/edit.hip) for the tests: hits, substitutions,
deletions and insertions of the minimum-edit-distance alignment with the fewest insertions.

    C[0][j] = (j, j),  C[i][0] = (i, 0),
    C[i][j] = lexmin(C[i-1][j-1] + (r != h, 0),  C[i-1][j] + (1, 0),  C[i][j-1] + (1, 1)),
    (d, I) = C[n][m],  D = I - (m - n),  S = d - I - D,  H = n - S - D.

A key (distance, insertions) is the integer distance * ONE + insertions, so the integer minimum is the lexicographic
one: `lexmin` is the only place that holds the tie rule.  `counts` walks the table row by row in plain Python;
`counts_numpy` walks it by anti-diagonals, one NumPy expression each, for the larger cases; `optimal_alignments`
enumerates the (S, D, I) of every optimal alignment of tiny strings, with no rule at all."""

from __future__ import annotations

import functools

import numpy as np

ONE = 1 << 32
_INF = 1 << 60


def lexmin(*keys):
    """THE TIE RULE: the smallest distance, and among equal distances the fewest insertions."""
    return functools.reduce(np.minimum, keys)


def _from_key(key: int, n: int, m: int) -> tuple:
    d, ins = divmod(int(key), ONE)
    dele = ins - (m - n)
    sub = d - ins - dele
    return n - sub - dele, sub, dele, ins


def counts(ref, hyp) -> tuple:
    """-> (hits, substitutions, deletions, insertions); plain Python, row by row."""
    n, m = len(ref), len(hyp)
    prev = [j * ONE + j for j in range(m + 1)]
    for i in range(1, n + 1):
        cur = [i * ONE] + [0] * m
        for j in range(1, m + 1):
            cur[j] = int(lexmin(prev[j - 1] + (ONE if ref[i - 1] != hyp[j - 1] else 0), prev[j] + ONE, cur[j - 1] + ONE + 1))
        prev = cur
    return _from_key(prev[m], n, m)


def counts_numpy(ref, hyp) -> tuple:
    """The same counts by anti-diagonals k = i + j (every cell of one depends on the two before it only)."""
    r, h = np.asarray(ref, dtype=np.int64), np.asarray(hyp, dtype=np.int64)
    n, m = len(r), len(h)
    if n == 0 or m == 0:
        return 0, 0, n, m
    i = np.arange(n + 1)
    ri = r[np.clip(i, 1, n) - 1]  # the reference token of row i
    d2 = np.full(n + 1, _INF, dtype=np.int64)  # diagonal k - 2, indexed by the row
    d2[0] = 0
    d1 = np.full(n + 1, _INF, dtype=np.int64)  # diagonal k - 1
    d1[0], d1[1] = ONE + 1, ONE
    inf1 = np.array([_INF], dtype=np.int64)
    for k in range(2, n + m + 1):
        j = k - i
        inside = (i >= 1) & (j >= 1) & (j <= m)
        differ = ri != h[np.clip(j, 1, m) - 1]
        sub = np.concatenate((inf1, d2[:-1])) + differ * ONE  # C[i-1][j-1]
        dele = np.concatenate((inf1, d1[:-1])) + ONE  # C[i-1][j]
        ins = d1 + (ONE + 1)  # C[i][j-1]
        cur = np.where(inside, lexmin(sub, dele, ins), _INF)
        if k <= m:
            cur[0] = k * ONE + k
        if k <= n:
            cur[k] = k * ONE
        d2, d1 = d1, cur
    return _from_key(d1[n], n, m)


def optimal_alignments(ref, hyp) -> set:
    """-> the set of (S, D, I) over ALL minimum-distance alignments (a prefix of an optimal path is optimal, so the sets
    are pruned to the optimal ones cell by cell).  For tiny strings."""
    n, m = len(ref), len(hyp)
    table = [[None] * (m + 1) for _ in range(n + 1)]
    table[0][0] = {(0, 0, 0)}
    for i in range(n + 1):
        for j in range(m + 1):
            if i == j == 0:
                continue
            s = set()
            if i and j:
                e = int(ref[i - 1] != hyp[j - 1])
                s |= {(a + e, b, c) for a, b, c in table[i - 1][j - 1]}
            if i:
                s |= {(a, b + 1, c) for a, b, c in table[i - 1][j]}
            if j:
                s |= {(a, b, c + 1) for a, b, c in table[i][j - 1]}
            best = min(sum(x) for x in s)
            table[i][j] = {x for x in s if sum(x) == best}
    return table[n][m]


def batch_counts(refs, hyps) -> np.ndarray:
    """int64 [n, 4] for lists of token sequences (the NumPy form)."""
    return np.array([counts_numpy(r, h) for r, h in zip(refs, hyps)], dtype=np.int64).reshape(-1, 4)


def rate(c, normalise: bool) -> float:
    h, s, d, i = (int(v) for v in np.asarray(c, dtype=np.int64).reshape(-1, 4).sum(0))
    return (s + d + i) / max(1, s + d + h + (i if normalise else 0))
