"""Restatement of ca_bootstrap_sums (coral_amd/csrc/bootstrap.hip) for the tests, in NumPy: ca_hash32 of
coral_amd/csrc/common.h in uint64 wrap-around arithmetic, the draw rule of include/coral_amd.h and the column sums.

    idx = ((g * R + r) << 32) | j        j = 0 .. n_g - 1
    u   = ca_hash32(seed, idx)
    k   = (u * n_g) >> 32
    sums[g, r, :] = sum over j of vals[members[goff[g] + k], :]

Everything is integer arithmetic, so the result is bit-exact by construction.  The tests import this module by path."""
import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def hash32(seed: int, idx) -> np.ndarray:
    """ca_hash32(seed, idx) for an array of uint64 indices -> uint64 array holding 32-bit values."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = idx + np.uint64(((int(seed) & _M64) * _GOLDEN + _GOLDEN) & _M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def hash32_scalar(seed: int, idx: int) -> int:
    """The same hash in Python integers (the check of the vectorised form)."""
    z = (idx + (seed & _M64) * _GOLDEN + _GOLDEN) & _M64
    z = ((z ^ (z >> 30)) * _MUL1) & _M64
    z = ((z ^ (z >> 27)) * _MUL2) & _M64
    return (z ^ (z >> 31)) >> 32


def draws(seed: int, g: int, R: int, n: int, replicates=None) -> np.ndarray:
    """k(g, r, j) for the listed replicates (default all R) and j < n -> int64 [len(replicates), n].  u < 2^32 and
    n <= 2^24, so u * n stays below 2^56: no wrap-around in the product."""
    r = np.arange(R, dtype=np.uint64) if replicates is None else np.asarray(replicates, dtype=np.uint64)
    w = np.uint64(g) * np.uint64(R) + r
    idx = (w[:, None] << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    return ((hash32(seed, idx) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sums(vals, members, goff, R: int, seed: int, chunk: int = 1 << 21, only=None) -> np.ndarray:
    """-> int64 [G, R, C], the contract of ca_bootstrap_sums.  Replicates are taken `chunk` draws at a time; a
    replicate's sum is formed as (how often each position of the group was drawn) @ (the rows at those positions), in
    int64: the same integers as adding the drawn rows one by one.  only: the groups to compute (the others stay 0)."""
    vals = np.asarray(vals, dtype=np.int64)
    members, goff = np.asarray(members, dtype=np.int64), np.asarray(goff, dtype=np.int64)
    G = len(goff) - 1
    out = np.zeros((G, R, vals.shape[1]), dtype=np.int64)
    for g in (range(G) if only is None else only):
        rows = vals[members[goff[g]:goff[g + 1]]]
        n = len(rows)
        step = max(1, chunk // n)
        for r0 in range(0, R, step):
            k = draws(seed, g, R, n, np.arange(r0, min(R, r0 + step)))
            flat = (np.arange(k.shape[0], dtype=np.int64)[:, None] * n + k).reshape(-1)
            times = np.bincount(flat, minlength=k.shape[0] * n).reshape(k.shape[0], n)
            out[g, r0:r0 + k.shape[0]] = times @ rows
    return out


def sums_one_by_one(vals, members, goff, R: int, seed: int) -> np.ndarray:
    """The same contract written as its definition, in Python integers (small cases: the check of `sums`)."""
    G, C = len(goff) - 1, len(vals[0])
    out = np.zeros((G, R, C), dtype=np.int64)
    for g in range(G):
        n = int(goff[g + 1] - goff[g])
        for r in range(R):
            for j in range(n):
                k = (hash32_scalar(seed, ((g * R + r) << 32) | j) * n) >> 32
                out[g, r] += np.asarray(vals[int(members[int(goff[g]) + k])], dtype=np.int64)
    return out
