"""float64 NumPy references for CTC forced alignment (ca_ctc_align, include/coral_amd.h): the Viterbi recursion over
the blank-interleaved states with the kernel's tie rule, and a brute force over every frame sequence."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax64(logits):
    """float64 log-softmax over the last axis of (fp32) logits."""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def viterbi(lp, labels, blank):
    """lp float64 [T, V] log-probabilities, labels a list of ids (none the blank) -> (score, start, end).
    v_0(0) = lp[0][blank], v_0(1) = lp[0][l_0]; v_t(s) = lp[t][l'_s] + max(stay, s-1, s-2 if s odd and l'_s != l'_{s-2});
    ties take the smaller move, and at the end a tie between states 2L and 2L-1 takes 2L.  No alignment (or T = 0):
    (-inf, [-1] * L, [-1] * L).  start / end: a token's first frame on the path and the first frame behind its last."""
    lp = np.asarray(lp, np.float64)
    T, L = lp.shape[0], len(labels)
    S = 2 * L + 1
    none = (NEG, [-1] * L, [-1] * L)
    if T == 0:
        return none
    ext = [blank if s % 2 == 0 else int(labels[s // 2]) for s in range(S)]
    v = np.full(S, NEG)
    v[0] = lp[0, blank]
    if S > 1:
        v[1] = lp[0, ext[1]]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        nv = np.full(S, NEG)
        for s in range(S):
            best, mv = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, mv = v[s - 1], 1
            if s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2] and v[s - 2] > best:
                best, mv = v[s - 2], 2
            nv[s] = best + lp[t, ext[s]]
            bp[t, s] = mv
        v = nv
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    score = v[s]
    if not score > NEG:
        return none
    start, end = [-1] * L, [-1] * L
    above = -1
    for t in range(T - 1, -1, -1):
        if s % 2 == 1 and s != above:
            end[s // 2] = t + 1
        mv = int(bp[t, s]) if t > 0 else 0
        if s % 2 == 1 and (t == 0 or mv != 0):
            start[s // 2] = t
        above = s
        s -= mv
    return float(score), start, end


def collapse(frames, blank):
    out, prev = [], None
    for c in frames:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def brute_force(lp, labels, blank):
    """The best score over every frame sequence in {0..V-1}^T that collapses to `labels` (-inf if there is none)."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    labels = [int(c) for c in labels]
    best = NEG
    if T == 0:
        return best
    for frames in itertools.product(range(V), repeat=T):
        if collapse(frames, blank) == labels:
            best = max(best, float(sum(lp[t, c] for t, c in enumerate(frames))))
    return best


def path_of(start, end, labels, T, blank):
    """The frame sequence that start / end define: token i on [start_i, end_i), blank elsewhere."""
    frames = [blank] * T
    for i, c in enumerate(labels):
        for t in range(start[i], end[i]):
            frames[t] = int(c)
    return frames


def check_valid_alignment(start, end, labels, T):
    """Runs in order, non-empty, disjoint, inside [0, T], and a gap between equal neighbours."""
    prev_end = 0
    for i, c in enumerate(labels):
        assert 0 <= start[i] < end[i] <= T, (i, start[i], end[i], T)
        assert start[i] >= prev_end, (i, start[i], prev_end)
        if i > 0 and int(labels[i - 1]) == int(c):
            assert start[i] > prev_end, (i, "equal neighbours need a blank between them")
        prev_end = end[i]


def path_score(lp, frames):
    return float(sum(lp[t, c] for t, c in enumerate(frames)))
