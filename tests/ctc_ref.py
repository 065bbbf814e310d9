"""Test-side reference of the CTC loss and its gradient with respect to the logits, independent of `coral_amd`, and the
seeded inputs that tests/test_ctc_ref_cpu.py (no GPU) and tests/test_ctc_gpu.py build identically.

  ctc_ref      torch.log_softmax + torch.nn.functional.ctc_loss on the CPU, float64 (the reference) or float32 (the
               yardstick: what a correctly-rounded fp32 implementation of the same recursion loses on these inputs)
  single_path  closed form for an utterance with exactly one feasible alignment
  brute_force  sum over all V^T alignments (tiny T only)

A case is a `Case`: logits [B, T, V] float32, one list of targets per utterance, in_len [B], blank.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import torch

SLACKS = (0, 1, 2, -1)   # rows of a single-path family: in_len = shortest feasible length + slack (-1: infeasible)


@dataclass(frozen=True, eq=False)
class Case:
    logits: torch.Tensor   # [B, T, V] float32
    targets: tuple         # B tuples of ints
    in_len: tuple          # B ints
    blank: int
    paths: tuple = ()      # per utterance: the only feasible alignment (tuple of T class ids) or None

    @property
    def shape(self):
        return tuple(self.logits.shape)


def ctc_ref(logits, targets, in_len, blank, dtype=torch.float64):
    """(nll [B], grad [B, T, V]) in `dtype`.  zero_infinity: an infeasible utterance has nll 0 and a zero gradient;
    frames at and after in_len have a zero gradient."""
    B, T, V = logits.shape
    lg = logits.detach().to("cpu", dtype).clone().requires_grad_(True)
    lp = torch.log_softmax(lg, -1).transpose(0, 1)
    flat = torch.tensor([c for tg in targets for c in tg], dtype=torch.long)
    tl = torch.tensor([len(tg) for tg in targets], dtype=torch.long)
    il = torch.tensor([min(int(n), T) for n in in_len], dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(lp, flat, il, tl, blank=blank, reduction="none", zero_infinity=True)
    nll.sum().backward()
    return nll.detach(), lg.grad


def single_path(logits, path, in_len):
    """(nll, grad [T, V]) in float64 of one utterance whose only feasible alignment is `path` (class id per frame)."""
    lg = logits.detach().to("cpu", torch.float64)
    T, V = lg.shape
    lp = torch.log_softmax(lg, -1)
    idx = torch.tensor(list(path[:in_len]), dtype=torch.long)
    t = torch.arange(in_len)
    nll = -lp[t, idx].sum()
    grad = torch.zeros(T, V, dtype=torch.float64)
    grad[:in_len] = torch.softmax(lg[:in_len], -1)
    grad[t, idx] -= 1.0
    return nll, grad


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def brute_force(logits, target, in_len, blank):
    """(nll, grad [T, V]) in float64 by enumerating all V^in_len alignments; (0, 0) when none is feasible."""
    lg = logits.detach().to("cpu", torch.float64)
    T, V = lg.shape
    p = torch.softmax(lg, -1)
    total = 0.0
    occ = torch.zeros(T, V, dtype=torch.float64)   # occ[t, v] = sum of P(path) over feasible paths with path_t = v
    for path in itertools.product(range(V), repeat=in_len):
        if collapse(path, blank) != list(target):
            continue
        w = 1.0
        for t, c in enumerate(path):
            w *= float(p[t, c])
        total += w
        for t, c in enumerate(path):
            occ[t, c] += w
    grad = torch.zeros(T, V, dtype=torch.float64)
    if total == 0.0:
        return torch.tensor(0.0, dtype=torch.float64), grad
    grad[:in_len] = p[:in_len] - occ[:in_len] / total
    return -torch.log(torch.tensor(total, dtype=torch.float64)), grad


def min_frames(target):
    """Shortest input that can emit `target`: one frame per label plus a blank between equal neighbours."""
    return len(target) + sum(1 for a, b in zip(target, target[1:]) if a == b)


def feasible(case):
    return [min(n, case.shape[1]) >= min_frames(tg) and (n > 0) for tg, n in zip(case.targets, case.in_len)]


def _randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _labels(seed, L, symbols, no_repeat=False):
    g = torch.Generator().manual_seed(seed)
    out = [symbols[int(i)] for i in torch.randint(0, len(symbols), (L,), generator=g)]
    if no_repeat:
        for i in range(1, L):
            if out[i] == out[i - 1]:
                out[i] = symbols[(symbols.index(out[i]) + 1) % len(symbols)]
    return tuple(out)


# ---- (a) single-path and few-path families: V = 46, blank = 45, one batch of the four SLACKS per L -------------------
SHARP_L = (1, 2, 63, 64, 127, 128, 129, 256, 512)
PATH_BOOST = 10.0


def _sharp_logits(seed, T, V, blank, shortest):
    """randn logits for the four SLACKS rows.  The rows with slack are peaked on one alignment that spends the spare
    frames on the outermost blanks (slack 1: shortest + blank; slack 2: blank + shortest + blank): states 0 and
    S-1 = 2L, which the single-path row never visits, carry nearly all of those rows' probability."""
    lg = _randn(seed, len(SLACKS), T, V)
    for b, path in ((1, shortest + (blank,)), (2, (blank,) + shortest + (blank,))):
        lg[b, torch.arange(len(path)), torch.tensor(path)] += PATH_BOOST
    return lg


@functools.lru_cache(maxsize=None)
def alternating_case(L):
    """Labels a b a b ...: in_len = L has the single alignment a b a b ... (a skip transition at every step)."""
    V, blank = 46, 45
    a, b = 3 + L % 17, 24 + L % 19
    tg = tuple(a if i % 2 == 0 else b for i in range(L))
    in_len = tuple(L + s for s in SLACKS)
    T = max(in_len) + 3
    path = tg + (blank,) * (T - L)
    return Case(_sharp_logits(1000 + L, T, V, blank, tg), (tg,) * len(SLACKS), in_len, blank, (path, None, None, None))


@functools.lru_cache(maxsize=None)
def repeated_case(L):
    """One label L times: in_len = 2L-1 has the single alignment a _ a _ ... a (no skips, compulsory blanks)."""
    V, blank = 46, 45
    a = 1 + L % 41
    tg = (a,) * L
    in_len = tuple(2 * L - 1 + s for s in SLACKS)
    T = max(in_len) + 3
    path = tuple(a if t % 2 == 0 else blank for t in range(T))
    return Case(_sharp_logits(2000 + L, T, V, blank, path[:2 * L - 1]), (tg,) * len(SLACKS), in_len, blank, (path, None, None, None))


# ---- (b) both recursion paths in one launch ----------------------------------------------------------------------------
MIXED_L = (0, 1, 2, 127, 128, 129, 190, 190, 64, 40)
MIXED_IN_LEN = (400, 400, 3, 400, 400, 399, 400, 381, 64, 0)


@functools.lru_cache(maxsize=None)
def mixed_case(blank):
    """T = 400, V = 46; blank 45 with symbols 0..44, or blank 0 with symbols 1..45.  The row with in_len == L gets labels
    without equal neighbours (otherwise it would be infeasible); the last row (in_len = 0) is infeasible."""
    T, V = 400, 46
    symbols = [v for v in range(V) if v != blank]
    tg = tuple(_labels(3000 + i, L, symbols, no_repeat=(n == L)) for i, (L, n) in enumerate(zip(MIXED_L, MIXED_IN_LEN)))
    return Case(_randn(31, len(MIXED_L), T, V), tg, MIXED_IN_LEN, blank)


# ---- (c), (d) long utterances: the slow path at S = 1025 and the two ways of fetching log-probs ------------------------
@functools.lru_cache(maxsize=None)
def long_case(T, V, blank, Ls, in_len, seed):
    symbols = [v for v in range(V) if v != blank]
    tg = tuple(_labels(seed + 10 * i, L, symbols) for i, L in enumerate(Ls))
    return Case(_randn(seed, len(Ls), T, V), tg, tuple(in_len), blank)


def largest_case():
    return long_case(1040, 46, 45, (512, 512, 300), (1040, 1030, 1040), 41)


def largest_case_short_labels():
    """Same launch geometry as largest_case (shares its workspace), shorter labels and utterances."""
    return long_case(1040, 46, 45, (5, 130, 60), (700, 333, 90), 43)


LDS_BOUNDARY = ((640, 48, 47, (100, 130), (640, 633)),    # T*V*4 = 120 KiB exactly: log-probs in LDS
                (641, 48, 47, (100, 130), (641, 634)),    # one frame more: gathered from global memory
                (700, 46, 45, (120, 200), (700, 650)))


def lds_boundary_case(i):
    return long_case(*LDS_BOUNDARY[i], 50 + i)


# ---- (e) vocabulary width ----------------------------------------------------------------------------------------------
WIDE_V = (2, 64, 65, 128, 129, 200, 256)


@functools.lru_cache(maxsize=None)
def wide_case(V):
    """T = 96, blank = V // 2, L = [40, 7, 0].  V = 2 has one symbol, so its labels repeat it (2L-1 <= in_len holds)."""
    T, blank = 96, V // 2
    symbols = [v for v in range(V) if v != blank]
    tg = tuple(_labels(6000 + V + i, L, symbols) for i, L in enumerate((40, 7, 0)))
    return Case(_randn(60 + V, 3, T, V, scale=2.0), tg, (96, 50, 96), blank)


# ---- references, computed once per case ----------------------------------------------------------------------------------
_REF = {}


def reference(case):
    """(nll64 [B], grad64 [B, T, V], e32 [B]): the float64 reference - the closed form on single-path rows - and
    e32[b] = max |grad32 - grad64| over utterance b, the error of torch's own float32 CPU gradient on the same inputs."""
    key = id(case)
    if key not in _REF:
        nll, grad = ctc_ref(case.logits, case.targets, case.in_len, case.blank)
        _, g32 = ctc_ref(case.logits, case.targets, case.in_len, case.blank, dtype=torch.float32)
        e32 = (g32.double() - grad).abs().amax(dim=(1, 2))
        for b, path in enumerate(case.paths):
            if path is not None:
                nll[b], grad[b] = single_path(case.logits[b], path, case.in_len[b])
        _REF[key] = (case, nll, grad, e32)   # keeps `case` alive, so its id stays unique
    return _REF[key][1:]
