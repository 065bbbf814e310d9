"""float64, dict-based restatement of the n-gram estimator of DESIGN.md §8 (interpolated modified Kneser-Ney with
raw-count pruning).  Independent of coral_amd/ngram_train.py and of the device code: it shares no function with them."""
import math
import re

import numpy as np

UNK, BOS, EOS = 0, 1, 2
RESERVED = ("<unk>", "<s>", "</s>")
FALLBACK = (0.5, 1.0, 1.5)
_WS = re.compile(r"[ \t\r\n]+")


def split_line(line: str) -> list:
    """Words of one line: maximal runs of characters other than space, tab, CR and LF."""
    return [w for w in _WS.split(line) if w]


def sentences_of(lines) -> list:
    return [s for s in (split_line(x) for l in lines for x in l.split("\n")) if s]


def discounts(t):
    """(t_1..t_4) -> ((D(1), D(2), D(3)), fell back)"""
    t1, t2, t3, t4 = t
    if 0 in (t1, t2, t3, t4):
        return FALLBACK, True
    y = t1 / (t1 + 2 * t2)
    d = (1 - 2 * y * t2 / t1, 2 - 3 * y * t3 / t2, 3 - 4 * y * t4 / t3)
    for k, dk in enumerate(d, start=1):
        if not 0 < dk < k:
            return FALLBACK, True
    return d, False


def zipf_corpus(n_tokens: int, n_types: int, seed: int, exponent: float = 1.1, mean_len: int = 8) -> list:
    """Seeded lines of about n_tokens words over at most n_types types with Zipf frequencies; some words hold multibyte
    characters, sentence lengths are geometric-like in 1 .. 4 mean_len."""
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, n_types + 1) ** exponent
    p /= p.sum()
    names = [("ø%d" if i % 7 == 3 else "w%d") % i for i in range(n_types)]
    draws = rng.choice(n_types, size=n_tokens, p=p)
    lens = 1 + rng.randint(0, 2 * mean_len - 1, size=n_tokens)
    lines, at, k = [], 0, 0
    while at < n_tokens:
        m = int(lens[k])
        k += 1
        lines.append(" ".join(names[i] for i in draws[at:at + m]))
        at += m
    return lines


class KNRef:
    """Every quantity of the definition for a corpus (list of lines) at order N:
      words / word_id   ids in order of first occurrence behind <unk>, <s>, </s>
      c[n], a[n]        raw and adjusted counts of the n-grams (tuples of ids), n = 1..N (index 0 unused)
      t[n]              [t_1..t_4];  D[n] = (0, D(1), D(2), D(3));  fallback[n]
      Z[n][h], Nk[n][h] sums over the n-grams h.x in G_n for the context h (a tuple of n - 1 ids);  gamma[n][h]
      p[n][g]           p_n(w | h) for g = h.w"""

    def __init__(self, lines, order: int):
        sents = sentences_of(lines)
        if not sents:
            raise ValueError("empty corpus")
        self.order = N = order
        self.words = list(RESERVED)
        self.word_id = {w: i for i, w in enumerate(self.words)}
        ids = []
        for s in sents:
            row = [BOS]
            for w in s:
                if w in RESERVED:
                    raise ValueError(f"reserved word {w}")
                if w not in self.word_id:
                    self.word_id[w] = len(self.words)
                    self.words.append(w)
                row.append(self.word_id[w])
            ids.append(row + [EOS])
        self.sentences = ids
        self.tokens = sum(len(s) for s in sents)
        c = [None] + [dict() for _ in range(N)]
        for s in ids:
            for j in range(len(s)):
                for n in range(1, min(N, j + 1) + 1):
                    g = tuple(s[j - n + 1:j + 1])
                    c[n][g] = c[n].get(g, 0) + 1
        self.c = c
        a = [None] + [dict() for _ in range(N)]
        a[N] = dict(c[N])
        for n in range(1, N):
            left = {}
            for g in c[n + 1]:
                left[g[1:]] = left.get(g[1:], 0) + 1
            for g in c[n]:
                a[n][g] = c[n][g] if g[0] == BOS else left.get(g, 0)
        a[1][(BOS,)] = 0
        a[1][(UNK,)] = 0
        self.c[1].setdefault((UNK,), 0)
        self.a = a
        for n in range(2, N + 1):
            assert all(v > 0 for v in a[n].values())
        self.t, self.D, self.fallback = [None], [None], [None]
        for n in range(1, N + 1):
            t = [sum(1 for v in a[n].values() if v == k) for k in (1, 2, 3, 4)]
            d, fb = discounts(t)
            self.t.append(t)
            self.D.append((0.0,) + tuple(d))
            self.fallback.append(fb)
        self.Z, self.Nk, self.gamma, self.p = [None], [None], [None], [None]
        V = len(self.words)
        for n in range(1, N + 1):
            Z, Nk = {}, {}
            for g, v in a[n].items():
                if v > 0:
                    h = g[:-1]
                    Z[h] = Z.get(h, 0) + v
                    Nk.setdefault(h, [0, 0, 0])[min(v, 3) - 1] += 1
            D = self.D[n]
            gamma = {h: (D[1] * Nk[h][0] + D[2] * Nk[h][1] + D[3] * Nk[h][2]) / Z[h] for h in Z}
            p = {}
            for g, v in a[n].items():
                if n == 1:
                    if g == (BOS,):
                        continue
                    p[g] = (v - D[min(v, 3)]) / Z[()] + gamma[()] / (V - 1)
                else:
                    h = g[:-1]
                    p[g] = (v - D[min(v, 3)]) / Z[h] + gamma[h] * self.p[n - 1][g[1:]]
            self.Z.append(Z)
            self.Nk.append(Nk)
            self.gamma.append(gamma)
            self.p.append(p)

    def default_prune(self):
        return [0] + [1] * (self.order - 1)

    def kept(self, prune):
        """per order (index 0 unused): the set of written n-grams"""
        N = self.order
        keep = [None] + [set() for _ in range(N)]
        ext = set()   # prefixes of the written grams of the order above
        for n in range(N, 0, -1):
            for g, cnt in self.c[n].items():
                if n == 1 or cnt > prune[n - 1] or g in ext:
                    keep[n].add(g)
            ext = {g[:-1] for g in keep[n]}
        return keep

    def rows(self, prune=None):
        """per order: [(ids, log10 p, log10 back-off)] in written order"""
        prune = self.default_prune() if prune is None else list(prune)
        assert len(prune) == self.order and prune[0] == 0
        keep = self.kept(prune)
        out = []
        for n in range(1, self.order + 1):
            rows = []
            for g in sorted(keep[n]):
                lp = 0.0 if g == (BOS,) else math.log10(self.p[n][g])
                bo = math.log10(self.gamma[n + 1][g]) if n < self.order and g in self.gamma[n + 1] else 0.0
                rows.append((g, lp, bo))
            out.append(rows)
        return out

    def to_lm(self, prune=None):
        from coral_amd.ngram import NGramLM

        return NGramLM(self.words, [{g: (lp, bo) for g, lp, bo in rows} for rows in self.rows(prune)])
