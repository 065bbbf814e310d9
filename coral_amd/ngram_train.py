"""Training the n-gram language model on the GPU: interpolated modified Kneser-Ney (the estimator is defined in
DESIGN.md §8), the step the reference takes after a wav2vec2 finetune with `lmplz -o 3 --prune 0 1 1`
(R/src/coral/finetune.py:86-87, R/src/coral/ngram.py:96-176, 322-358).  Parity with lmplz is NOT pinned (KenLM is not
available to this project); the estimator is pinned against the float64 restatement of its definition in tests/kn_ref.py.

The corpus goes to the device as raw bytes, in chunks cut at line ends; tokenising, the vocabulary, counting, adjusted
counts, the statistics and the probabilities are kernels of coral_amd/csrc/ngram_train.hip.  The host touches the list of
unique words (to give out ids in order of first occurrence), the 4 count-of-counts per order (to form the discounts in
Python float64) and the finished tables.

Out of scope: building the corpus from `decoder_datasets` (hub download, removal of the evaluation sentences) and the
`.bin` compression of the ARPA file (R/src/coral/ngram.py:179-319, 361-387).
"""

from __future__ import annotations

import contextlib
import logging
import os
import re
import shutil
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import CoralAmdError
from .ngram import MAX_ORDER, TOKEN_SEED, NGramLM, mix64

logger = logging.getLogger(__package__)

RESERVED = ("<unk>", "<s>", "</s>")   # word ids 0, 1, 2
MAX_WORD_BYTES = _lib.NGT_MAX_WORD_BYTES
FALLBACK_DISCOUNTS = (0.5, 1.0, 1.5)
DEFAULT_CHUNK_BYTES = 1 << 26
MAX_VOCAB_ROUNDS = 16
WHITESPACE = b" \t\r\n"
_RESERVED_RE = re.compile(rb"(?:^|[ \t\r\n])(<unk>|<s>|</s>)(?=$|[ \t\r\n])")


def word_hash(word: bytes) -> int:
    """The tokeniser's hash of a word: `mix64` over its bytes under TOKEN_SEED (never 0)."""
    h = TOKEN_SEED
    for b in word:
        h = mix64(h, b)
    return h or 1


def default_prune(order: int) -> list[int]:
    """The reference's `--prune 0 1 1` (R/src/coral/ngram.py:127)."""
    return [0] + [1] * (order - 1)


def check_order_and_prune(order: int, prune) -> list[int]:
    if not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"n-gram order {order} outside 1..{MAX_ORDER}")
    prune = default_prune(order) if prune is None else [int(x) for x in prune]
    if len(prune) != order:
        raise ValueError(f"prune needs one threshold per order ({order}), got {prune}")
    if prune[0] != 0:
        raise ValueError(f"unigrams are never pruned: prune[0] must be 0, got {prune[0]}")
    if min(prune) < 0:
        raise ValueError(f"prune thresholds must not be negative, got {prune}")
    return prune


def kn_discounts(t) -> tuple[tuple[float, float, float], bool]:
    """Count-of-counts (t_1..t_4) of one order -> ((D(1), D(2), D(3)), fell back).  Python float64 from integers.
    Y = t_1 / (t_1 + 2 t_2), D(k) = k - (k + 1) Y t_{k+1} / t_k; a zero t_k or a D(k) outside (0, k) gives the fallback
    (0.5, 1, 1.5) for the order (lmplz's --discount_fallback)."""
    t = [int(x) for x in t]
    if len(t) != 4:
        raise ValueError("kn_discounts needs t_1..t_4")
    if min(t) <= 0:
        return FALLBACK_DISCOUNTS, True
    y = t[0] / (t[0] + 2 * t[1])
    d = tuple(k - (k + 1) * y * t[k] / t[k - 1] for k in (1, 2, 3))
    if any(not 0.0 < d[k - 1] < k for k in (1, 2, 3)):
        return FALLBACK_DISCOUNTS, True
    return d, False


def table_capacity_rule(n_whitespace: int, n_lines: int) -> int:
    """Slots per table when `table_capacity` is not given: the smallest power of two >= 2 P, P = whitespace bytes + line
    feeds + 4 >= words + sentences + 2 >= the distinct n-grams of any order (load <= 1/2).  It is an upper bound: a
    corpus that repeats itself needs far less, and `table_capacity=` says so."""
    need = 2 * (n_whitespace + n_lines + 4)
    cap = 2
    while cap < need:
        cap *= 2
    return cap


def iter_chunks(corpus, chunk_bytes: int = DEFAULT_CHUNK_BYTES):
    """Chunks of the corpus as bytes, each ending at a line end (the last one may end without).  `corpus`: a path, or
    an iterable of lines (str or bytes); a line is used as given, a line feed inside it ends a sentence like any other."""
    if isinstance(corpus, (str, os.PathLike)):
        with open(corpus, "rb") as f:
            rest = b""
            while True:
                block = f.read(chunk_bytes)
                if not block:
                    break
                data = rest + block
                cut = data.rfind(b"\n") + 1
                if cut == 0:   # a line longer than the chunk: keep reading
                    rest = data
                    continue
                rest = data[cut:]
                yield data[:cut]
            if rest:
                yield rest
        return
    if isinstance(corpus, (bytes, bytearray)):
        raise TypeError("corpus is a path or an iterable of lines, not a bytes object")
    buf, size = [], 0
    for line in corpus:
        raw = line.encode("utf-8") if isinstance(line, str) else bytes(line)
        if not raw.endswith(b"\n"):
            raw += b"\n"
        buf.append(raw)
        size += len(raw)
        if size >= chunk_bytes:
            yield b"".join(buf)
            buf, size = [], 0
    if buf:
        yield b"".join(buf)


class NGramTrainer:
    """The device tables of one training run and the stages over them (`feed` per chunk, `finalize`, `export`).
    capacities: slots of the vocabulary table and of the table of every order (powers of two); arena_bytes: room for
    the bytes of the unique words.  hash_bits < 64 narrows the word hash: for tests of the compare-on-probe path only."""

    def __init__(self, order: int, vocab_capacity: int, table_capacities, arena_bytes: int, device="cuda", hash_bits: int = 64):
        import torch

        from . import ops

        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"n-gram order {order} outside 1..{MAX_ORDER}")
        caps = [int(c) for c in table_capacities]
        for c in [int(vocab_capacity)] + caps:
            if c < 2 or c & (c - 1) or c > 1 << 31:
                raise ValueError(f"table capacity {c} is no power of two in [2, 2^31]")
        if len(caps) != order:
            raise ValueError("one table capacity per order")
        self.torch, self.ops = torch, ops
        self.order, self.hash_bits = order, hash_bits
        dev = self.device = torch.device(device)
        if dev.type != "cuda":
            raise CoralAmdError("n-gram training runs on the GPU (there is no CPU path)")
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        i32, i64, u8, f64 = torch.int32, torch.int64, torch.uint8, torch.float64
        self.status = z(_lib.NGT_ST_WORDS_N, i64)
        self.status[_lib.NGT_ST_LONG_AT] = -1
        self.gstat = z(24, i64)
        self.vkey, self.vrep, self.varena_at = z(vocab_capacity, i64), torch.full((vocab_capacity,), -1, dtype=i64, device=dev), \
            torch.full((vocab_capacity,), -1, dtype=i64, device=dev)
        self.slot_id = torch.full((vocab_capacity,), -1, dtype=i32, device=dev)
        self.arena, self.arena_top = z(max(int(arena_bytes), 256), u8), z(1, i64)
        self.new_count = z(1, i64)
        self.arrays = dict(
            key=[z(c, i64) for c in caps], ids=[torch.full((3 * c,), -1, dtype=i64, device=dev) for c in caps],
            count=[z(c, i32) for c in caps], left=[z(c, i32) for c in caps], adj=[z(c, i32) for c in caps],
            ctx_slot=[torch.full((c,), -1, dtype=i32, device=dev) for c in caps],
            suf_slot=[torch.full((c,), -1, dtype=i32, device=dev) for c in caps],
            cstat=[z(4 * c, i32) for c in caps], prob=[z(c, f64) for c in caps], keep=[z(c, u8) for c in caps],
            ext=[z(c, u8) for c in caps])
        self.desc = ops.ngt_tables_desc(order, self.arrays, self.gstat, self.status)
        self.capacities = dict(vocabulary=int(vocab_capacity), orders=caps, arena=int(self.arena.numel()))
        self.id_slots = []          # slots of the vocabulary table in id order (ids 3..), one tensor per chunk
        self.next_id = len(RESERVED)
        self.base_off = 0
        self.tokens = 0
        self.sentences_fed = 0
        self.finalized = False
        self.disc = None
        self.timings = None         # {stage: [(start event, end event)]} once `time_stages()` was called

    # ---- stage times (tools/measure_ngram_train.py) ---------------------------------------------------------
    def time_stages(self) -> None:
        self.timings = {}

    @contextlib.contextmanager
    def _stage(self, name: str):
        """Device events around the launches of one stage; the span includes the device's idle time while the host
        reads a status word inside the stage (the vocabulary rounds)."""
        if self.timings is None:
            yield
            return
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.timings.setdefault(name, []).append((a, b))

    def stage_ms(self) -> dict:
        self.torch.cuda.synchronize(self.device)
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in (self.timings or {}).items()}

    # ---- status -------------------------------------------------------------------------------------------
    def _check(self, chunk: bytes | None = None) -> np.ndarray:
        """Read the status words (synchronises) and raise what they report."""
        st = self.status.cpu().numpy()
        over = int(st[_lib.NGT_ST_OVERFLOW])
        if over:
            c = self.capacities
            full = []
            if over & 1:
                full.append(f"the vocabulary table ({c['vocabulary']} slots)")
            full += [f"the {n}-gram table ({c['orders'][n - 1]} slots)" for n in range(1, self.order + 1) if over >> n & 1]
            if over >> 6 & 1:
                full.append(f"the word arena ({c['arena']} bytes)")
            if over >> 7 & 1 or over >> 8 & 1:
                full.append("an output buffer")
            raise CoralAmdError("n-gram training: " + " and ".join(full) + " overflowed; pass a larger table_capacity")
        if st[_lib.NGT_ST_LONG]:
            at = int(st[_lib.NGT_ST_LONG_AT])
            head = ""
            if chunk is not None and 0 <= at - self.base_off < len(chunk):
                head = chunk[at - self.base_off: at - self.base_off + 40].decode("utf-8", "replace")
            raise ValueError(f"n-gram training: {int(st[_lib.NGT_ST_LONG])} word(s) above {MAX_WORD_BYTES} bytes, the first "
                             f"at byte {at} of the corpus: {head!r}...")
        if st[_lib.NGT_ST_COLLISION]:
            raise CoralAmdError("n-gram training: two different n-grams share a 64-bit hash (NGRAM_SEED); the decoder's "
                                "tables are keyed by that hash and could not hold them either")
        if st[_lib.NGT_ST_MISS]:
            raise CoralAmdError(f"n-gram training: {int(st[_lib.NGT_ST_MISS])} internal table look-ups failed")
        return st

    # ---- per chunk ----------------------------------------------------------------------------------------
    def tokenize(self, chunk: bytes) -> dict:
        """One chunk -> dict(text, n, nw, start, length, line, hash) of device tensors (the tokeniser alone)."""
        torch, ops = self.torch, self.ops
        n = len(chunk)
        if not 0 < n < 1 << 31:
            raise ValueError(f"a chunk holds 1 .. 2^31 - 1 bytes, got {n}")
        text = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).to(self.device)
        maxw = n // 2 + 1
        e = lambda dt: torch.empty(maxw, dtype=dt, device=self.device)  # noqa: E731
        blk = torch.zeros(2 * ops.ngt_tokenize_blocks(n), dtype=torch.int32, device=self.device)
        tok = dict(text=text, n=n, start=e(torch.int32), length=e(torch.int32), line=e(torch.int32), hash=e(torch.int64))
        with self._stage("tokenise"):
            ops.ngt_tokenize(text, n, self.base_off, self.hash_bits, blk, tok["start"], tok["length"], tok["line"],
                             tok["hash"], self.status)
        st = self._check(chunk)
        tok["nw"], tok["lines"] = int(st[_lib.NGT_ST_WORDS]), int(st[_lib.NGT_ST_LINES])
        return tok

    def add_words(self, tok: dict) -> "torch.Tensor":
        """Vocabulary stage of a tokenised chunk -> slot of every word; new words get the next ids in order of their
        first byte offset."""
        with self._stage("vocabulary"):
            return self._add_words(tok)

    def _add_words(self, tok: dict):
        torch, ops = self.torch, self.ops
        nw, dev = tok["nw"], self.device
        w_slot = torch.full((nw,), -1, dtype=torch.int32, device=dev)
        w_skip = torch.zeros(nw, dtype=torch.int32, device=dev)
        w_cand = torch.empty(nw, dtype=torch.int32, device=dev)
        for _ in range(MAX_VOCAB_ROUNDS):
            self.status[_lib.NGT_ST_PENDING] = 0
            ops.ngt_vocab_round(self.vkey, self.vrep, self.varena_at, tok["text"], tok["n"], self.base_off, self.arena,
                                tok["start"], tok["length"], tok["hash"], w_skip, w_slot, w_cand, nw, self.status)
            if not self._check()[_lib.NGT_ST_PENDING]:
                break
        else:
            raise CoralAmdError(f"n-gram training: more than {MAX_VOCAB_ROUNDS} different words share one word hash")
        self.new_count.zero_()
        new_slot = torch.empty(nw, dtype=torch.int32, device=dev)
        ops.ngt_vocab_commit(self.vkey, self.vrep, self.varena_at, tok["text"], self.base_off, self.arena, self.arena_top,
                             tok["start"], tok["length"], w_slot, nw, new_slot, self.new_count, self.status)
        self._check()
        k = int(self.new_count.item())
        if k:
            slots = new_slot[:k].long()
            slots = slots[torch.argsort(self.vrep[slots])]   # order of first occurrence (offset << 8 | length)
            if self.next_id + k >= 1 << 31:
                raise CoralAmdError("n-gram training: more than 2^31 word types")
            self.slot_id[slots] = torch.arange(self.next_id, self.next_id + k, dtype=torch.int32, device=dev)
            self.id_slots.append(slots)
            self.next_id += k
        return w_slot

    def feed(self, chunk: bytes) -> None:
        """Tokenise one chunk (it ends at a line end), extend the vocabulary and count its n-grams."""
        if self.finalized:
            raise RuntimeError("feed() after finalize()")
        tok = self.tokenize(chunk)
        if tok["nw"]:
            w_slot = self.add_words(tok)
            if self.tokens + 2 * tok["nw"] >= 1 << 31:
                raise CoralAmdError("n-gram training: counts are 32-bit, the corpus holds too many words")
            with self._stage("count"):
                self.ops.ngt_count(self.desc, w_slot, self.slot_id, tok["line"], tok["nw"], self.tokens == 0)
            self.tokens += tok["nw"]
        self.base_off += len(chunk)

    # ---- after the last chunk ---------------------------------------------------------------------------------
    def words(self) -> list[str]:
        """The vocabulary in id order; the reserved words inside the corpus are a ValueError."""
        torch = self.torch
        out = list(RESERVED)
        if self.id_slots:
            slots = torch.cat(self.id_slots)
            at = self.varena_at[slots].cpu().numpy()
            ln = (self.vrep[slots] & 255).cpu().numpy()
            arena = self.arena[: int(self.arena_top.item())].cpu().numpy().tobytes()
            out += [arena[a:a + l].decode("utf-8") for a, l in zip(at.tolist(), ln.tolist())]
        bad = sorted(set(out[len(RESERVED):]) & set(RESERVED))
        if bad:
            raise ValueError(f"n-gram training: the corpus contains the reserved word(s) {', '.join(bad)}")
        return out

    def finalize(self) -> None:
        """Adjusted counts, statistics, discounts (host) and probabilities."""
        torch, ops = self.torch, self.ops
        if self.finalized:
            raise RuntimeError("finalize() twice")
        if self.tokens == 0:
            raise ValueError("n-gram training: the corpus holds no words")
        self._check()
        with self._stage("adjust"):
            ops.ngt_adjust(self.desc)
        with self._stage("statistics"):
            ops.ngt_stats(self.desc)
        self._check()
        g = self.gstat.cpu().numpy()
        self.count_of_counts = [[int(g[4 * n + k]) for k in range(4)] for n in range(self.order)]
        both = [kn_discounts(t) for t in self.count_of_counts]
        self.discounts = [tuple(float(x) for x in d) for d, _ in both]
        self.discount_fallback = [fb for _, fb in both]
        disc = np.zeros(20, dtype=np.float64)
        for n, d in enumerate(self.discounts):
            disc[4 * n + 1: 4 * n + 4] = d
        self.disc = torch.from_numpy(disc).to(self.device)
        with self._stage("probabilities"):
            ops.ngt_probs(self.desc, self.disc, self.next_id)
        self._check()
        self.finalized = True

    def export(self, prune) -> list[dict]:
        """Per order: dict(ids [k, n] int32, count, adj, Z, N1, N2, N3 int64, logp, backoff float64) of the grams that
        `prune` keeps, rows in lexicographic order of the id tuples."""
        torch, ops = self.torch, self.ops
        prune = check_order_and_prune(self.order, prune)
        if not self.finalized:
            raise RuntimeError("export() before finalize()")
        for o in range(self.order):
            self.arrays["ext"][o].zero_()
        with self._stage("prune"):
            ops.ngt_prune(self.desc, prune)
        out = []
        for n in range(1, self.order + 1):
            k = int(self.arrays["keep"][n - 1].sum(dtype=torch.int64).item())
            room = max(k, 1)
            ids = torch.empty(room, n, dtype=torch.int32, device=self.device)
            ints = torch.empty(room, 6, dtype=torch.int32, device=self.device)
            f = torch.empty(room, 2, dtype=torch.float64, device=self.device)
            self.new_count.zero_()
            with self._stage("export"):
                ops.ngt_export(self.desc, n, self.disc, ids, ints, f, self.new_count)
            self._check()
            if int(self.new_count.item()) != k:
                raise CoralAmdError(f"n-gram export: {int(self.new_count.item())} rows of order {n}, {k} were flagged")
            ids, ints, f = ids[:k].cpu().numpy(), ints[:k].cpu().numpy().astype(np.int64), f[:k].cpu().numpy()
            o = np.lexsort(ids[:, ::-1].T) if k else np.zeros(0, dtype=np.int64)
            ids, ints, f = ids[o], ints[o], f[o]
            out.append(dict(ids=ids, count=ints[:, 0], adj=ints[:, 1], Z=ints[:, 2], N1=ints[:, 3], N2=ints[:, 4],
                            N3=ints[:, 5], logp=f[:, 0], backoff=f[:, 1]))
        return out


class TrainedNGramLM(NGramLM):
    """The NGramLM `train_ngram` returns: also `discounts` (D(1), D(2), D(3) per order), `discount_fallback` (per order),
    `count_of_counts` (t_1..t_4 per order), `prune` and `tokens`."""


def lm_from_export(words: list[str], rows: list[dict]) -> TrainedNGramLM:
    grams = []
    for r in rows:
        keys = map(tuple, r["ids"].tolist())
        grams.append(dict(zip(keys, zip(r["logp"].tolist(), r["backoff"].tolist()))))
    return TrainedNGramLM(words, grams)


def corpus_size(chunks) -> tuple[int, int, int]:
    """-> (bytes, whitespace bytes, line feeds) of an iterable of chunks (bytes.count and one regular-expression search:
    no tokenising on the host).  A reserved word standing as a word of the corpus is a ValueError."""
    size = ws = lf = 0
    for c in chunks:
        hit = _RESERVED_RE.search(c)
        if hit:
            raise ValueError(f"n-gram training: the corpus contains the reserved word {hit.group(1).decode()}")
        size += len(c)
        lf += c.count(b"\n")
        ws += sum(c.count(bytes([b])) for b in WHITESPACE) + 1   # + 1: a last line without a line feed
    return size, ws, lf


def train_ngram(corpus, order: int = 3, prune=None, device="cuda", table_capacity=None,
                chunk_bytes: int = DEFAULT_CHUNK_BYTES) -> TrainedNGramLM:
    """Interpolated modified Kneser-Ney n-gram of `order` over `corpus` (a path to a text file with one sentence per
    line, or an iterable of lines), pruned by raw count: prune[n-1] = tau_n, default [0, 1, 1, ..].
    table_capacity: slots of every hash table (an int: a power of two; or a sequence: vocabulary, then one per order);
    None sizes them from the corpus by `table_capacity_rule` (a path is read twice for that; an iterable is held in
    host memory).  A table that overflows raises CoralAmdError naming its capacity."""
    prune = check_order_and_prune(order, prune)
    is_path = isinstance(corpus, (str, os.PathLike))
    chunks = iter_chunks(corpus, chunk_bytes) if is_path else list(iter_chunks(corpus, chunk_bytes))
    size, ws, lf = corpus_size(chunks)
    if size == 0:
        raise ValueError("n-gram training: the corpus is empty")
    if table_capacity is None:
        caps = [table_capacity_rule(ws, lf)] * (order + 1)
    elif isinstance(table_capacity, int):
        caps = [table_capacity] * (order + 1)
    else:
        caps = [int(c) for c in table_capacity]
        if len(caps) != order + 1:
            raise ValueError("table_capacity as a sequence: the vocabulary table, then one per order")
    trainer = NGramTrainer(order, caps[0], caps[1:], size, device)
    for chunk in (iter_chunks(corpus, chunk_bytes) if is_path else chunks):
        trainer.feed(chunk)
    if trainer.tokens == 0:
        raise ValueError("n-gram training: the corpus holds no words")
    words = trainer.words()
    trainer.finalize()
    lm = lm_from_export(words, trainer.export(prune))
    lm.discounts, lm.discount_fallback = trainer.discounts, trainer.discount_fallback
    lm.count_of_counts, lm.prune, lm.tokens = trainer.count_of_counts, prune, trainer.tokens
    if any(lm.discount_fallback):
        logger.info("n-gram training: fallback discounts %s for order(s) %s", FALLBACK_DISCOUNTS,
                    [n + 1 for n, fb in enumerate(lm.discount_fallback) if fb])
    return lm


def add_eos_line(src: str | Path, dst: str | Path) -> None:
    """The reference's post-processing of the ARPA file (R/src/coral/ngram.py:147-169), restated: the 1-gram count of
    the header grows by one and the <s> line is followed by a copy of itself that names </s>."""
    done_count = done_line = False
    with Path(src).open("r", encoding="utf-8") as f_in, Path(dst).open("w", encoding="utf-8") as f_out:
        for line in f_in:
            if not done_count and line.startswith("ngram 1="):
                f_out.write(f"ngram 1={int(line.strip().split('=')[-1]) + 1}\n")
                done_count = True
            elif not done_line and "<s>" in line:
                f_out.write(line)
                f_out.write(line.replace("<s>", "</s>"))
                done_line = True
            else:
                f_out.write(line)


def train_and_store_ngram_model(config, device="cuda") -> Path | None:
    """What R/src/coral/ngram.py:26-39 does, with what exists here: train the `decoder_num_ngrams`-gram on
    `config.decoder_corpus_path` (one sentence per line), add the </s> line, and store `language_model/{N}gram.arpa` +
    `attrs.json` in the model directory through `Wav2Vec2ProcessorWithLM.save_pretrained`, a stale `language_model/`
    removed first.  Main process only.  -> the stored ARPA file."""
    from .processor import CTCTokenizer, WaveformFeatureExtractor, Wav2Vec2ProcessorWithLM

    if os.getenv("RANK", "0") != "0":
        return None
    corpus = config.get("decoder_corpus_path")
    if not corpus:
        raise ValueError("train_and_store_ngram_model needs decoder_corpus_path (a text file, one sentence per line)")
    order = int(config.model.decoder_num_ngrams)
    model_dir = Path(config.model_dir)
    model_dir.mkdir(parents=True, exist_ok=True)
    logger.info("Training n-gram language model...")
    lm = train_ngram(corpus, order=order, device=device)
    raw, correct = model_dir / f"raw_{order}gram.arpa", model_dir / f"{order}gram.arpa"
    lm.write_arpa(raw)
    logger.info("Adding end-of-sentence marker to n-gram language model...")
    add_eos_line(raw, correct)
    raw.unlink()
    logger.info("Storing n-gram language model...")
    processor = Wav2Vec2ProcessorWithLM(WaveformFeatureExtractor(int(config.model.sampling_rate)),
                                        CTCTokenizer.from_pretrained(model_dir), NGramLM.from_arpa(correct))
    if (model_dir / "language_model").exists():
        shutil.rmtree(model_dir / "language_model")
    processor.save_pretrained(model_dir)
    stored = model_dir / "language_model" / f"{order}gram.arpa"
    shutil.move(str(correct), str(stored))   # the stored file is the post-processed one, both </s> lines included
    return stored
