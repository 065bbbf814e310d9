"""Host side of the n-gram language model that `ca_ctc_beam_decode` fuses into the CTC beam search.

The reference trains a KenLM 3-gram after a finetune and stores it in `model_dir/language_model/`
(R/src/coral/ngram.py:322-358) for pyctcdecode.  Here the ARPA text file is read in plain Python (KenLM's binary
format needs KenLM and is refused with a message), scored on the host in float64 for tests, and flattened into sorted
hash tables the kernel binary-searches.  The n-gram itself is trained on the GPU by coral_amd/ngram_train.py (modified
Kneser-Ney).

Device tables, per million entries: 16 MB per million n-grams (8-byte hash + fp32 log10 p + fp32 back-off) and 12 MB
per million unigram prefixes (8-byte hash + int32 word id; a word of n characters has n prefixes).
"""

from __future__ import annotations

import json
import logging
import math
from pathlib import Path

import numpy as np

logger = logging.getLogger(__package__)

MAX_ORDER = 5
MASK64 = (1 << 64) - 1
PREFIX_SEED = 0x243F6A8885A308D3   # label-string prefixes (kernel side only; here for the tests)
WORD_SEED = 0x13198A2E03707344     # open word, over symbol ids
NGRAM_SEED = 0xA4093822299F31D0    # n-grams, over word ids
TOKEN_SEED = 0x082EFA98EC4E6C89    # corpus words, over their UTF-8 bytes (the tokeniser of coral_amd/csrc/ngram_train.hip)

# Decoder parameters and their defaults (recalled pyctcdecode defaults; nothing rests on them being that).
DEFAULT_PARAMS = dict(alpha=0.5, beta=1.5, unk_score_offset=-10.0, score_boundary=True, token_min_logp=-5.0,
                      beam_prune_logp=-10.0)
ATTR_KEYS = ("alpha", "beta", "unk_score_offset", "score_boundary")

BIN_MESSAGE = ("{path}: KenLM binary language models cannot be read without KenLM; export the model as ARPA text "
               "(the `.arpa` file lmplz writes) and put it in language_model/ instead")


def mix64(h: int, x: int) -> int:
    """One step of the 64-bit rolling hash (`beam_mix` in coral_amd/csrc/ctc_beam.hip)."""
    z = ((h ^ ((x + 1) & MASK64)) * 0x9E3779B97F4A7C15) & MASK64
    z ^= z >> 32
    z = (z * 0xD6E8FEB86659FD93) & MASK64
    z ^= z >> 32
    return z


def hash_ids(ids, seed: int) -> int:
    h = seed
    for i in ids:
        h = mix64(h, int(i))
    return h


def _mix64_np(h: np.ndarray, x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = (h ^ (x.astype(np.int64) + 1).astype(np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(32)
        z = z * np.uint64(0xD6E8FEB86659FD93)
        z ^= z >> np.uint64(32)
    return z


def load_attrs(lm_dir: str | Path) -> dict:
    """`language_model/attrs.json` overrides alpha / beta / unk_score_offset / score_boundary; a missing, unreadable or
    differently shaped file means the defaults (the layout is recalled from pyctcdecode, not verified)."""
    out = {k: DEFAULT_PARAMS[k] for k in ATTR_KEYS}
    path = Path(lm_dir) / "attrs.json"
    try:
        raw = json.loads(path.read_text())
    except (OSError, ValueError):
        return out
    if isinstance(raw, dict):
        for k in ATTR_KEYS:
            if isinstance(raw.get(k), (int, float, bool)):
                out[k] = bool(raw[k]) if k == "score_boundary" else float(raw[k])
    return out


class NGramLM:
    """Back-off n-gram LM read from an ARPA file.  `words[i]` is the unigram with word id i (file order);
    `grams[k]` maps a tuple of k + 1 word ids to (log10 p, log10 back-off)."""

    def __init__(self, words: list[str], grams: list[dict], counts: list[int] | None = None):
        self.words = list(words)
        self.word_id = {}
        for i, w in enumerate(self.words):
            self.word_id.setdefault(w, i)
        self.grams = grams
        self.order = len(grams)
        self.counts = counts or [len(g) for g in grams]   # lines read per order (= the \data\ header)
        self.bos_id = self.word_id.get("<s>", -1)
        self.eos_id = self.word_id.get("</s>", -1)
        self.unk_id = self.word_id.get("<unk>", -1)

    # ---- reading / writing -------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path: str | Path) -> "NGramLM":
        path = Path(path)
        if path.suffix in (".bin", ".binary"):
            raise ValueError(BIN_MESSAGE.format(path=path))
        header: dict[int, int] = {}
        words: list[str] = []
        word_id: dict[str, int] = {}
        grams: list[dict] = []
        counts: list[int] = []
        n = 0  # current section (0: before / inside \data\)
        with path.open("r", encoding="utf-8") as f:
            for raw in f:
                line = raw.strip()
                if not line:
                    continue
                if line.startswith("\\"):
                    if line == "\\data\\":
                        n = 0
                    elif line == "\\end\\":
                        break
                    elif line.endswith("-grams:"):
                        n = int(line[1:line.index("-")])
                        if n != len(grams) + 1 or n > MAX_ORDER:
                            raise ValueError(f"{path}: unexpected section {line!r} (orders 1..{MAX_ORDER}, ascending)")
                        grams.append({})
                        counts.append(0)
                    else:
                        raise ValueError(f"{path}: unknown section {line!r}")
                    continue
                if n == 0:
                    if line.startswith("ngram ") and "=" in line:
                        k, c = line[6:].split("=")
                        header[int(k)] = int(c)
                    continue
                tok = line.split()
                if len(tok) not in (n + 1, n + 2):
                    raise ValueError(f"{path}: malformed {n}-gram line {line!r}")
                logp = float(tok[0])
                bo = float(tok[n + 1]) if len(tok) == n + 2 else 0.0
                counts[n - 1] += 1
                if n == 1:
                    w = tok[1]
                    if w in word_id:  # R/src/coral/ngram.py:160-165 can add a second </s> line: the first line wins
                        logger.warning("%s: unigram %r listed twice, keeping the first", path, w)
                        continue
                    word_id[w] = len(words)
                    words.append(w)
                    grams[0][(word_id[w],)] = (logp, bo)
                else:
                    try:
                        key = tuple(word_id[w] for w in tok[1:n + 1])
                    except KeyError as e:
                        raise ValueError(f"{path}: {n}-gram {line!r} uses the word {e.args[0]!r} that is no unigram")
                    grams[n - 1].setdefault(key, (logp, bo))
        if not grams or not words:
            raise ValueError(f"{path}: no \\1-grams: section (is this an ARPA text file?)")
        for k, c in header.items():
            got = counts[k - 1] if k <= len(counts) else 0
            if got != c:
                raise ValueError(f"{path}: \\data\\ announces {c} {k}-grams, the file holds {got}")
        return cls(words, grams, counts)

    def write_arpa(self, path: str | Path) -> None:
        with Path(path).open("w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for k, g in enumerate(self.grams):
                f.write(f"ngram {k + 1}={len(g)}\n")
            for k, g in enumerate(self.grams):
                f.write(f"\n\\{k + 1}-grams:\n")
                for ids, (logp, bo) in g.items():
                    line = f"{logp!r}\t" + " ".join(self.words[i] for i in ids)
                    if k + 1 < self.order or bo != 0.0:
                        line += f"\t{bo!r}"
                    f.write(line + "\n")
            f.write("\n\\end\\\n")

    # ---- host scoring (float64; tests only) ---------------------------------------------------------
    def logp(self, ctx: tuple, w: int) -> float:
        """log10 P(w | ctx) for word ids, ARPA back-off rule (longest stored n-gram wins)."""
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(ctx), -1, -1):
            c = ctx[len(ctx) - k:]
            hit = self.grams[k].get(c + (w,))
            if hit is not None:
                return bo + hit[0]
            if k > 0:
                bo += self.grams[k - 1].get(c, (0.0, 0.0))[1]
        raise KeyError(f"word id {w} is no unigram")

    def start_context(self) -> tuple:
        return (self.bos_id,) if self.bos_id >= 0 and self.order > 1 else ()

    def advance(self, ctx: tuple, word: str) -> tuple[float, tuple, bool]:
        """-> (log10 P(word | ctx), next context, word is a unigram).  An unknown word scores as <unk> when the LM has
        one, else as log10 P = 0 followed by an empty context."""
        w = self.word_id.get(word, -1)
        known = w >= 0
        if not known:
            w = self.unk_id
        if w < 0:
            return 0.0, (), False
        lp = self.logp(ctx, w)
        nxt = (tuple(ctx) + (w,))[-(self.order - 1):] if self.order > 1 else ()
        return lp, nxt, known

    def score(self, words: list[str], score_boundary: bool = True) -> float:
        """sum of log10 P over the words (+ </s> when `score_boundary`), starting in the context <s>."""
        ctx = self.start_context()
        total = 0.0
        for word in words:
            lp, ctx, _ = self.advance(ctx, word)
            total += lp
        if score_boundary and self.eos_id >= 0:
            total += self.logp(ctx, self.eos_id)
        return total

    # ---- tables for the kernel ----------------------------------------------------------------------
    def device_tables(self, tokenizer, device="cpu") -> dict:
        """Flat tensors for `ops.ctc_beam_decode`: no pointers inside, hashes stored as the int64 bit pattern of the
        unsigned value and sorted as unsigned.
          pfx_keys / pfx_wid: rolling hash (WORD_SEED, symbol ids) of every prefix of every unigram the tokenizer can
            spell -> word id, or -1 for a proper prefix;
          ng_keys / ng_logp / ng_backoff: per order, hash (NGRAM_SEED, word ids) -> log10 p, back-off; ng_count per order.
        Raises on a hash collision."""
        import torch

        vocab = tokenizer.get_vocab()
        special = {"<s>", "</s>", "<unk>", "<pad>", getattr(tokenizer, "word_delimiter_token", "|")}
        sym = {c: i for c, i in vocab.items() if len(c) == 1 and c not in special}
        pfx: dict[int, tuple] = {}   # hash -> (symbol ids, word id)
        for wid, word in enumerate(self.words):
            if wid in (self.bos_id, self.eos_id, self.unk_id) or not word or any(c not in sym for c in word):
                continue
            h, ids = WORD_SEED, ()
            for n, c in enumerate(word):
                h = mix64(h, sym[c])
                ids += (sym[c],)
                val = wid if n == len(word) - 1 else -1
                old = pfx.get(h)
                if old is None:
                    pfx[h] = (ids, val)
                elif old[0] != ids:
                    raise ValueError(f"prefix hash collision between {old[0]} and {ids}")
                elif val >= 0:
                    pfx[h] = (ids, val)
        pk = np.array(sorted(pfx), dtype=np.uint64)
        pw = np.array([pfx[int(h)][1] for h in pk], dtype=np.int32)
        keys, logp, bo, count = [], [], [], []
        for k, g in enumerate(self.grams):
            ids = np.array(list(g.keys()), dtype=np.int64).reshape(len(g), k + 1)
            vals = np.array(list(g.values()), dtype=np.float64).reshape(len(g), 2)
            h = np.full(len(g), NGRAM_SEED, dtype=np.uint64)
            for j in range(k + 1):
                h = _mix64_np(h, ids[:, j])
            o = np.argsort(h, kind="stable")
            h = h[o]
            if len(h) > 1 and bool((h[1:] == h[:-1]).any()):
                raise ValueError(f"hash collision among the {k + 1}-grams")
            keys.append(h)
            logp.append(vals[o, 0].astype(np.float32))
            bo.append(vals[o, 1].astype(np.float32))
            count.append(len(g))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return dict(pfx_keys=t(pk.view(np.int64)), pfx_wid=t(pw), ng_keys=t(np.concatenate(keys).view(np.int64)),
                    ng_logp=t(np.concatenate(logp)), ng_backoff=t(np.concatenate(bo)), ng_count=count, order=self.order,
                    bos_wid=self.bos_id if self.order > 1 else -1, eos_wid=self.eos_id, unk_wid=self.unk_id)


def hotword_set(hotwords) -> list[str]:
    """The set H of DESIGN.md §8: every whitespace-separated word of every entry, lower-cased as the evaluation
    lower-cases text, de-duplicated, in first-seen order.  None or an empty list: no hotwords."""
    if isinstance(hotwords, str):
        raise TypeError("hotwords is a list of strings, not one string")
    seen: dict[str, None] = {}
    for entry in hotwords or ():
        for word in str(entry).lower().split():
            seen.setdefault(word, None)
    return list(seen)


def hotword_tables(hotwords, tokenizer, device="cpu") -> dict:
    """Flat tensors for `ops.ctc_beam_decode_ex`, in the pattern of pfx_keys / pfx_wid:
      hot_keys: rolling hash (WORD_SEED, symbol ids) of every prefix of every hotword, sorted as unsigned (stored as the
        int64 bit pattern);
      hot_frac: fp32 len(prefix) / len(shortest hotword with that prefix);  hot_word: uint8 1 where the prefix is itself
        a hotword.
    A word with a character outside the tokenizer's alphabet raises ValueError naming the word and the character."""
    import torch

    vocab = tokenizer.get_vocab()
    special = {"<s>", "</s>", "<unk>", "<pad>", getattr(tokenizer, "word_delimiter_token", "|")}
    sym = {c: i for c, i in vocab.items() if len(c) == 1 and c not in special}
    pfx: dict[int, list] = {}   # hash -> [symbol ids, len_min, is a hotword]
    for word in hotword_set(hotwords):
        for c in word:
            if c not in sym:
                raise ValueError(f"hotword {word!r}: the character {c!r} is not in the tokenizer's alphabet")
        h, ids = WORD_SEED, ()
        for n, c in enumerate(word):
            h = mix64(h, sym[c])
            ids += (sym[c],)
            old = pfx.setdefault(h, [ids, len(word), False])
            if old[0] != ids:
                raise ValueError(f"hotword prefix hash collision between {old[0]} and {ids}")
            old[1] = min(old[1], len(word))
            old[2] = old[2] or n == len(word) - 1
    hk = np.array(sorted(pfx), dtype=np.uint64)
    frac = np.array([np.float32(len(pfx[int(h)][0])) / np.float32(pfx[int(h)][1]) for h in hk], dtype=np.float32)
    flag = np.array([pfx[int(h)][2] for h in hk], dtype=np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return dict(hot_keys=t(hk.view(np.int64)), hot_frac=t(frac), hot_word=t(flag))


def find_language_model(model_dir: str | Path):
    """-> (path of `language_model/*.arpa` or None, a `.bin` was seen)."""
    lm_dir = Path(model_dir) / "language_model"
    if not lm_dir.is_dir():
        return None, False
    arpas = sorted(lm_dir.glob("*.arpa"))
    bins = sorted(lm_dir.glob("*.bin")) + sorted(lm_dir.glob("*.binary"))
    return (arpas[0] if arpas else None), bool(bins)
