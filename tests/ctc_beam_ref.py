"""Test-side reference of the LM-fused CTC decoder, independent of `coral_amd`: a tiny ARPA reader, the
objective S(y) by brute force over every alignment, and a plain prefix beam search in float64 (or float32) that follows
the search rules word for word.

  S(y) = ln P_ctc(y) + alpha ln10 (sum_i log10 P_lm(w_i | ctx) [+ log10 P_lm(</s> | ctx)]) + beta n
         + unk_score_offset #{w_i not a unigram}          (without an LM: ln P_ctc(y) + beta n)
"""
from __future__ import annotations

import itertools
import math

import numpy as np

MASK64 = (1 << 64) - 1
PREFIX_SEED = 0x243F6A8885A308D3
LN10 = math.log(10.0)
DEFAULTS = dict(beam_width=100, alpha=0.5, beta=1.5, unk_score_offset=-10.0, token_min_logp=-5.0,
                beam_prune_logp=-10.0, score_boundary=True)


def mix64(h, x):
    z = ((h ^ ((x + 1) & MASK64)) * 0x9E3779B97F4A7C15) & MASK64
    z ^= z >> 32
    z = (z * 0xD6E8FEB86659FD93) & MASK64
    return z ^ (z >> 32)


def prefix_hash(ids):
    h = PREFIX_SEED
    for i in ids:
        h = mix64(h, int(i))
    return h


class RefLM:
    """ARPA back-off LM over word strings."""

    def __init__(self, path):
        self.grams = {}   # tuple of words -> (log10 p, back-off)
        self.order = 0
        n = 0
        for line in open(path, encoding="utf-8"):
            line = line.strip()
            if line.endswith("-grams:"):
                n = int(line[1:line.index("-")])
                self.order = max(self.order, n)
            elif line.startswith("\\") or not line or n == 0:
                continue
            else:
                tok = line.split()
                self.grams.setdefault(tuple(tok[1:n + 1]), (float(tok[0]), float(tok[n + 1]) if len(tok) > n + 1 else 0.0))
        self.unigrams = {g[0] for g in self.grams if len(g) == 1}
        self.prefixes = {w[:i] for w in self.unigrams for i in range(1, len(w) + 1)}
        self.has_unk = "<unk>" in self.unigrams

    def logp(self, ctx, w):
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(ctx), -1, -1):
            c = ctx[len(ctx) - k:]
            if c + (w,) in self.grams:
                return bo + self.grams[c + (w,)][0]
            if k > 0:
                bo += self.grams.get(c, (0.0, 0.0))[1]
        raise KeyError(w)

    def start(self):
        return ("<s>",) if "<s>" in self.unigrams and self.order > 1 else ()

    def close(self, ctx, word, p):
        """score added by closing `word` in context `ctx` -> (addend, next context)"""
        s = p["beta"]
        known = word in self.unigrams
        w = word if known else ("<unk>" if self.has_unk else None)
        if not known:
            s += p["unk_score_offset"]
        if w is None:
            return s, ()
        s += p["alpha"] * LN10 * self.logp(ctx, w)
        return s, ((tuple(ctx) + (w,))[-(self.order - 1):] if self.order > 1 else ())


def lm_bonus(y, delimiter, id2char, lm, p):
    """the LM + bonus part of S(y)"""
    words, cur = [], ""
    for c in list(y) + [delimiter]:
        if c == delimiter:
            if cur:
                words.append(cur)
            cur = ""
        else:
            cur += id2char[c]
    if lm is None:
        return p["beta"] * len(words)
    ctx, s = lm.start(), 0.0
    for w in words:
        a, ctx = lm.close(ctx, w, p)
        s += a
    if p["score_boundary"] and "</s>" in lm.unigrams:
        s += p["alpha"] * LN10 * lm.logp(ctx, "</s>")
    return s


def log_softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def brute_force(logits, blank, delimiter, id2char, lm, forbidden=(), **params):
    """{label string (tuple of ids): S(y)} over every string some alignment of the T frames collapses to."""
    p = dict(DEFAULTS, **params)
    lp = log_softmax64(logits)
    T, V = lp.shape
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        y = tuple(k for k, _ in itertools.groupby(path) if k != blank)
        if any(c in forbidden for c in path):
            continue
        mass.setdefault(y, []).append(sum(lp[t, c] for t, c in enumerate(path)))
    out = {}
    for y, terms in mass.items():
        m = max(terms)
        out[y] = m + math.log(sum(math.exp(v - m) for v in terms)) + lm_bonus(y, delimiter, id2char, lm, p)
    return out


def prefix_beam_search(logits, blank, delimiter, id2char, lm=None, forbidden=(), in_len=None, dtype=np.float64, **params):
    """-> (best ids, S of it, {ids: S} of every final beam).  Rules: DESIGN.md §8 / coral_amd/csrc/ctc_beam.hip."""
    p = dict(DEFAULTS, **params)
    F = dtype
    NEG = F(-np.inf)
    lp_all = log_softmax64(logits).astype(F)
    T, V = lp_all.shape
    T = T if in_len is None else min(T, int(in_len))
    unk = F(p["unk_score_offset"])
    add = lambda a, b: F(np.logaddexp(a, b))  # noqa: E731
    # beam: prefix -> [pb, pnb, lm score, provisional unk, context, open word, prefix hash (ranking ties)]
    beams = {(): [F(0.0), NEG, F(0.0), False, lm.start() if lm else (), "", PREFIX_SEED]}
    for t in range(T):
        lp = lp_all[t]
        syms = [c for c in range(V) if c != blank and c not in forbidden and lp[c] >= p["token_min_logp"]]
        new, merged = {}, {}
        for y, (pb, pnb, sc, pen, ctx, ow, h) in beams.items():
            tot = add(pb, pnb)
            last = y[-1] if y else -1
            for c in syms:
                v = lp[c] + (pb if c == last else tot)
                if not v > NEG:
                    continue
                y2 = y + (c,)
                if y2 in beams:
                    merged[y2] = v
                    continue
                if c == delimiter:
                    sc2, ctx2 = sc, ctx
                    if ow:
                        if lm is None:
                            sc2 = F(sc + F(p["beta"]))
                        else:
                            a, ctx2 = lm.close(ctx, ow, p)
                            sc2 = F(sc + F(a))
                    new[y2] = [NEG, v, sc2, False, ctx2, "", mix64(h, c)]
                else:
                    ow2 = ow + id2char[c]
                    pen2 = pen or (lm is not None and ow2 not in lm.prefixes)
                    new[y2] = [NEG, v, sc, pen2, ctx, ow2, mix64(h, c)]
        for y, (pb, pnb, sc, pen, ctx, ow, h) in beams.items():
            npb = add(pb, pnb) + lp[blank]
            npnb = add(pnb + lp[y[-1]] if y else NEG, merged.get(y, NEG))
            new[y] = [npb, npnb, sc, pen, ctx, ow, h]
        rank = {y: F(add(b[0], b[1]) + b[2] + (unk if b[3] else F(0.0))) for y, b in new.items()}
        rank = {y: r for y, r in rank.items() if r > NEG}
        if not rank:
            beams = {}
            break
        thr = max(rank.values()) + F(p["beam_prune_logp"])
        keep = sorted((y for y, r in rank.items() if r >= thr), key=lambda y: (-rank[y], new[y][6]))
        beams = {y: new[y] for y in keep[:p["beam_width"]]}
    finals = {}
    for y, (pb, pnb, sc, pen, ctx, ow, _) in beams.items():
        s = sc
        if lm is None:
            if ow:
                s = F(s + F(p["beta"]))
        else:
            if ow:
                a, ctx = lm.close(ctx, ow, p)
                s = F(s + F(a))
            if p["score_boundary"] and "</s>" in lm.unigrams:
                s = F(s + F(p["alpha"] * LN10 * lm.logp(ctx, "</s>")))
        finals[y] = F(add(pb, pnb) + s)
    finals = {y: s for y, s in finals.items() if s > NEG}
    if not finals:
        return (), float("-inf"), {}
    best = min(finals, key=lambda y: (-finals[y], prefix_hash(y)))
    return best, float(finals[best]), {y: float(s) for y, s in finals.items()}


def regime_logits(kind, seed, B, T, V, blank, lexicon_ids, delimiter):
    """Seeded logits fp32 [B, T, V]: label strings drawn from `lexicon_ids` (lists of symbol ids, one per word), laid
    on a random monotone alignment among blanks.  kind: "confident" (+12, N(0,1)), "noisy" (+8, N(0,2)),
    "flat" (N(0,1) alone)."""
    rng = np.random.RandomState(seed)
    boost, sigma = dict(confident=(12.0, 1.0), noisy=(8.0, 2.0), flat=(0.0, 1.0))[kind]
    x = (sigma * rng.randn(B, T, V)).astype(np.float32)
    if boost:
        for b in range(B):
            labels = []
            while len(labels) < T // 5:
                labels += list(lexicon_ids[rng.randint(len(lexicon_ids))]) + [delimiter]
            labels = labels[:T // 5]
            # a frame per label, one more between equal neighbours, the rest blanks at random places
            seq = []
            for i, c in enumerate(labels):
                if i and labels[i - 1] == c:
                    seq.append(blank)
                seq.append(c)
            frames = [blank] * T
            pos = np.sort(rng.choice(T, size=len(seq), replace=False))
            for q, c in zip(pos, seq):
                frames[q] = c
            x[b, np.arange(T), frames] += np.float32(boost)
    return x
