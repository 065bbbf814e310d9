"""Float64 restatement of the resampler ca_resample implements (include/coral_amd.h, coral_amd/resample.py), evaluated
directly from the formula.  It does not read coral_amd.resample.plan, so a wrong table is caught.

    g = gcd(src, dst), O = src / g, Nw = dst / g, s = rolloff * min(1, Nw / O), L = lowpass_filter_width
    y[n] = sum over the integers m with |(m - n O / Nw) s| < L of x[m] h(m - n O / Nw),   x = 0 outside [0, len)
    h(d) = s * sinc(d s) * cos^2(pi d s / (2 L)),   sinc(t) = sin(pi t) / (pi t),   n_out = ceil(Nw len / O)
"""

from __future__ import annotations

import math

import numpy as np


def ratio(src: int, dst: int):
    g = math.gcd(int(src), int(dst))
    return int(src) // g, int(dst) // g


def kernel(d, s: float, L: int):
    """h(d) for distances d = m - n O / Nw (float64 array); 0 outside the support |d s| < L."""
    t = np.asarray(d, np.float64) * s
    return np.where(np.abs(t) < L, s * np.sinc(t) * np.cos(np.pi * t / (2 * L)) ** 2, 0.0)


def out_length(n: int, src: int, dst: int) -> int:
    O, Nw = ratio(src, dst)
    return -((-Nw * int(n)) // O)


def phase_table(src: int, dst: int, L: int = 32, rolloff: float = 0.99):
    """(O, Nw, K, off int64 [Nw], taps float64 [Nw, K]) straight from the definition: phase i sits at p = i O / Nw,
    off[i] is the smallest integer m with |(m - p) s| < L, taps[i][k] = h(off[i] + k - p), rows zero-padded to K."""
    O, Nw = ratio(src, dst)
    s = rolloff * min(1.0, Nw / O)
    W = int(math.ceil(L / s)) + 2
    rows, offs = [], []
    for i in range(Nw):
        m = np.arange((i * O) // Nw - W, (i * O) // Nw + W + 1, dtype=np.int64)
        d = (m * Nw - i * O).astype(np.float64) / Nw  # the numerator is an exact integer
        inside = np.abs(d * s) < L
        ms = m[inside]
        assert len(ms) and np.all(np.diff(ms) == 1)
        offs.append(int(ms[0]))
        rows.append(kernel(d[inside], s, L))
    K = max(len(r) for r in rows)
    taps = np.zeros((Nw, K), np.float64)
    for i, r in enumerate(rows):
        taps[i, :len(r)] = r
    return O, Nw, K, np.asarray(offs, np.int64), taps


def resample(x, src: int, dst: int, L: int = 32, rolloff: float = 0.99, round_taps: bool = True, int16: bool = False):
    """-> (y float64 [n_out], A float64 [n_out], K): the definition applied to the 1-D signal x (int16 samples are scaled
    by 1/32768 when `int16`), and A[n] = sum_k |h_k x_k|, what the error bound of a K-term fp32 sum scales with.
    round_taps: the taps rounded once to float32, as the device table holds them."""
    x = np.asarray(x, np.float64) * ((1.0 / 32768.0) if int16 else 1.0)
    O, Nw, K, off, taps = phase_table(src, dst, L, rolloff)
    if round_taps:
        taps = taps.astype(np.float32).astype(np.float64)
    n_out = out_length(len(x), src, dst)
    n = np.arange(n_out, dtype=np.int64)
    m0 = (n // Nw) * O + off[n % Nw]
    idx = m0[:, None] + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    xs = np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    prod = taps[n % Nw] * xs
    return prod.sum(axis=1), np.abs(prod).sum(axis=1), K


def bound(A, K: int):
    """|y_gpu - y_ref| <= (K + 2) 2^-23 A[n]: gamma_{K+1} of the running-error bound of a K-term fp32 dot product of
    fp32-rounded taps, in any summation order, doubled."""
    return (K + 2) * 2.0 ** -23 * np.asarray(A, np.float64)
