"""Test-side restatement of the extended CTC decoder (n-best and hotwords), independent of `coral_amd` and
built beside `ctc_beam_ref` (same structure as its `prefix_beam_search`, word for word where the rules are the same):

  S_h(y) = S(y) + hotword_weight #{ w_i in H }

H: every whitespace-separated word of every hotword entry, lower-cased, de-duplicated.  Ranking only: while the open last
word is a prefix of a hotword it adds hotword_weight * len(open) / len_min (len_min: the shortest hotword with that
prefix); the term is replaced by the exact one when the word closes.  `prefix_beam_search_nbest` returns every final
ranked by (S descending, prefix hash ascending) with S split into logit_score = ln(p_b + p_nb) and lm_score = the rest.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref as ref  # noqa: E402


def hot_set(hotwords):
    out = []
    for entry in hotwords or ():
        for w in entry.lower().split():
            if w not in out:
                out.append(w)
    return out


def hot_prefixes(words):
    """{prefix: length of the shortest hotword with that prefix}"""
    out = {}
    for w in words:
        for n in range(1, len(w) + 1):
            out[w[:n]] = min(out.get(w[:n], len(w)), len(w))
    return out


def words_of(y, delimiter, id2char):
    words, cur = [], ""
    for c in list(y) + [delimiter]:
        if c == delimiter:
            if cur:
                words.append(cur)
            cur = ""
        else:
            cur += id2char[c]
    return words


def brute_force(logits, blank, delimiter, id2char, lm, forbidden=(), hotwords=None, hotword_weight=10.0, **params):
    """{label string: S_h(y)}: `ctc_beam_ref.brute_force` plus the hotword term."""
    H = set(hot_set(hotwords))
    exact = ref.brute_force(logits, blank, delimiter, id2char, lm, forbidden, **params)
    return {y: s + hotword_weight * sum(w in H for w in words_of(y, delimiter, id2char)) for y, s in exact.items()}


def ranked(exact):
    """label strings of a {string: score} by (score descending, prefix hash ascending)"""
    return sorted(exact, key=lambda y: (-exact[y], ref.prefix_hash(y)))


def prefix_beam_search_nbest(logits, blank, delimiter, id2char, lm=None, forbidden=(), in_len=None, dtype=np.float64,
                             hotwords=None, hotword_weight=10.0, **params):
    """-> ranked list of (ids, S, logit_score, lm_score) over every final beam with S > -inf."""
    p = dict(ref.DEFAULTS, **params)
    F = dtype
    NEG = F(-np.inf)
    lp_all = ref.log_softmax64(logits).astype(F)
    T, V = lp_all.shape
    T = T if in_len is None else min(T, int(in_len))
    unk = F(p["unk_score_offset"])
    H = set(hot_set(hotwords)) if hotword_weight != 0 else set()
    hpfx = hot_prefixes(H)
    wh = F(hotword_weight)
    add = lambda a, b: F(np.logaddexp(a, b))  # noqa: E731

    def hot(ow):  # provisional bonus of the open word
        n = hpfx.get(ow)
        return F(0.0) if n is None else F(wh * (F(len(ow)) / F(n)))

    def close(ctx, ow):  # -> (addend, next context)
        if lm is None:
            a, ctx2 = p["beta"], ctx
        else:
            a, ctx2 = lm.close(ctx, ow, p)
        return a + (hotword_weight if ow in H else 0.0), ctx2

    # beam: prefix -> [pb, pnb, lm score, provisional unk, context, open word, prefix hash (ranking ties)]
    beams = {(): [F(0.0), NEG, F(0.0), False, lm.start() if lm else (), "", ref.PREFIX_SEED]}
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
                        a, ctx2 = close(ctx, ow)
                        sc2 = F(sc + F(a))
                    new[y2] = [NEG, v, sc2, False, ctx2, "", ref.mix64(h, c)]
                else:
                    ow2 = ow + id2char[c]
                    pen2 = pen or (lm is not None and ow2 not in lm.prefixes)
                    new[y2] = [NEG, v, sc, pen2, ctx, ow2, ref.mix64(h, c)]
        for y, (pb, pnb, sc, pen, ctx, ow, h) in beams.items():
            npb = add(pb, pnb) + lp[blank]
            npnb = add(pnb + lp[y[-1]] if y else NEG, merged.get(y, NEG))
            new[y] = [npb, npnb, sc, pen, ctx, ow, h]
        rank = {y: F(F(add(b[0], b[1]) + b[2] + (unk if b[3] else F(0.0))) + hot(b[5])) for y, b in new.items()}
        rank = {y: r for y, r in rank.items() if r > NEG}
        if not rank:
            beams = {}
            break
        thr = max(rank.values()) + F(p["beam_prune_logp"])
        keep = sorted((y for y, r in rank.items() if r >= thr), key=lambda y: (-rank[y], new[y][6]))
        beams = {y: new[y] for y in keep[:p["beam_width"]]}
    finals = []
    for y, (pb, pnb, sc, pen, ctx, ow, h) in beams.items():
        s = sc
        if ow:
            a, ctx = close(ctx, ow)
            s = F(s + F(a))
        if lm is not None and p["score_boundary"] and "</s>" in lm.unigrams:
            s = F(s + F(p["alpha"] * ref.LN10 * lm.logp(ctx, "</s>")))
        logit = add(pb, pnb)
        total = F(logit + s)
        if total > NEG:
            finals.append((y, float(total), float(logit), float(s), h))
    finals.sort(key=lambda f: (-f[1], f[4]))
    return [f[:4] for f in finals]
