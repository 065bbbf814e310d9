"""Write tests/golden/whisper_chunk.npz from the installed transformers (CPU only, no model).

Recorded (every entry a JSON document inside the archive):

  * `merge`: seeded groups of token sequences and what `_find_longest_common_sequence` makes of them - the merged ids
    and, through its `token_timestamp_sequences` argument, where every merged token comes from.  Each token's "timestamp"
    is the pair (sequence, position): a left token's pair is below every pair of the sequence to its right, so the extra
    condition transformers puts on a match with token timestamps (left time <= right time) always holds and the merge is
    the plain one, while the returned timestamps name each kept token's origin, which pins the cuts.
  * `asr`: recordings as lists of per-chunk id rows with their strides in seconds, and what `_decode_asr` returns for
    them with return_timestamps=True and False over a stand-in tokenizer (text id t is " w<t>"; the ids of
    tests/whisper_ts_ref.py).  The rows come from a seeded "true" transcript with segment times: every chunk emits the
    segments that touch it, times relative to its start, with substitutions, a cut-off last segment now and then, and
    a few hand-written corner cases (duplicate start, timestamps inside both strides, an empty chunk).
  * `strides`: what the pipeline's `chunk_iter` yields (in samples) for recordings around the chunk boundaries,
    among them several whose last chunk is short, one of a single short chunk and one of an hour.

Asserted before anything is written: tests/whisper_chunk_ref.py reproduces every recorded result exactly.

usage: python tools/gen_whisper_chunk_goldens.py"""
from __future__ import annotations

import json
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import whisper_chunk_ref as C  # noqa: E402


class StandInTokenizer:
    """What `_decode_asr` asks of a tokenizer."""
    all_special_ids = list(C.SPECIAL_IDS)

    def decode(self, tokens, **_):
        tokens = [int(t) for t in tokens]
        if len(tokens) == 1 and tokens[0] in C.SPECIAL_IDS:
            return "<|da|>" if tokens[0] == C.LANG else f"<|s{tokens[0]}|>"
        return C.stand_in_decode(tokens)

    def convert_tokens_to_ids(self, tok):
        return {"<|notimestamps|>": C.NO_TIMESTAMPS, "<|startofprev|>": 62, "<|startoftranscript|>": C.SOT}[tok]

    def _strip_prompt(self, token_ids, prompt_token_id, decoder_start_token_id):
        return token_ids


def merge_cases(rng):
    cases = [[[1, 2, 3, 4], [3, 4, 5]], [[1, 2, 3]], [[1, 2], [3, 4]], [[1, 2, 3], [3, 9]], [[], [1, 2], [], [2, 3], []],
             [[7] * 9, [7] * 5, [7] * 12], [[1, 2, 3, 4, 5, 6], [5, 6]], [[5, 6], [1, 2, 5, 6, 7, 8, 9]]]
    for _ in range(60):  # a small vocabulary: overlaps and near-ties are common
        cases.append([[rng.randrange(12) for _ in range(rng.choice((0, 1, 2, 5, 9, 17, 40)))] for _ in range(rng.randint(1, 5))])
    for _ in range(20):  # true overlaps: windows of one stream with substitutions
        stream = [rng.randrange(40) for _ in range(rng.randint(30, 120))]
        seqs, at = [], 0
        while at < len(stream):
            n = rng.randint(8, 30)
            seqs.append([t if rng.random() > 0.1 else rng.randrange(40) for t in stream[max(0, at - rng.randint(0, 6)):at + n]])
            at += n - rng.randint(0, 6)
        cases.append(seqs)
    return cases


def true_transcript(rng, seconds):
    """[(start_s, end_s, [text ids])] covering the recording, times on the 0.02 s grid."""
    segs, t = [], round(rng.uniform(0, 1) / 0.02) * 0.02
    while t < seconds - 1.0:
        end = min(seconds, t + rng.uniform(1.5, 7.0))
        end = round(end / 0.02) * 0.02
        segs.append((t, end, [rng.randrange(50) for _ in range(rng.randint(1, 9))]))
        t = end if rng.random() < 0.7 else round((end + rng.uniform(0, 1.5)) / 0.02) * 0.02
    return segs


def chunk_row(rng, segs, a, b, timestamps, cut_last):
    """The id row a model would give for the audio [a, b) s: prefix, the segments that touch it, EOS and padding."""
    row = [C.SOT, C.LANG, C.TRANSCRIBE] + ([] if timestamps else [C.NO_TIMESTAMPS])
    tok = lambda s: C.TIMESTAMP_BEGIN + int(round(min(max(s - a, 0.0), b - a) / 0.02))  # noqa: E731
    inside = [s for s in segs if s[1] > a and s[0] < b]
    for n, (s, e, ids) in enumerate(inside):
        ids = [t if rng.random() > 0.08 else rng.randrange(50) for t in ids]
        if s < a:  # cut at the chunk's start: the words that fall before it are not heard
            ids = ids[int(len(ids) * (a - s) / (e - s)):]
        if e > b:
            ids = ids[:max(1, int(len(ids) * (b - s) / (e - s)))]
        if not timestamps:
            row += ids
            continue
        row += [tok(s)] + ids
        if not (n == len(inside) - 1 and (e > b or cut_last)):
            row += [tok(e)]
    return row + [C.EOS] * rng.randint(1, 3)


def asr_cases(rng):
    cases = []
    sr = C.SAMPLING_RATE
    for seconds, chunk_s, stride_s in ((70.0, 30.0, 5.0), (95.0, 30.0, 5.0), (41.0, 20.0, (4.0, 2.0)), (12.0, 30.0, 5.0),
                                      (130.0, 30.0, 5.0), (61.0, 30.0, 5.0), (55.0, 10.0, 1.0), (90.0, 30.0, 0.0)):
        for timestamps in (True, False):
            for cut_last in (False, True):
                left, right = stride_s if isinstance(stride_s, tuple) else (stride_s, stride_s)
                plan = C.chunk_strides(int(seconds * sr), int(chunk_s * sr), int(left * sr), int(right * sr))
                segs = true_transcript(rng, seconds)
                outs = [dict(tokens=chunk_row(rng, segs, s / sr, (s + n) / sr, timestamps, cut_last and rng.random() < 0.5),
                             stride=[n / sr, l / sr, r / sr]) for s, n, l, r in plan]
                cases.append(dict(timestamps=timestamps, outputs=outs))
    tb, P = C.TIMESTAMP_BEGIN, [C.SOT, C.LANG, C.TRANSCRIBE]
    hand = [
        # a duplicate start, then the true end
        [dict(tokens=P + [tb, tb, 1, 2, tb + 100, C.EOS], stride=[30.0, 0.0, 0.0])],
        # timestamps inside the right stride are skipped with their partner and resolved in the next chunk
        [dict(tokens=P + [tb, 1, 2, tb + 600, tb + 600, 3, 4, 5, tb + 1400, tb + 1400, 6, 7, C.EOS], stride=[30.0, 0.0, 5.0]),
         dict(tokens=P + [tb, 3, 4, 5, tb + 400, tb + 400, 6, 7, 8, tb + 900, C.EOS], stride=[30.0, 5.0, 0.0])],
        # an empty chunk in the middle, and one at the start
        [dict(tokens=P + [tb, 1, 2, 3, tb + 1200, C.EOS], stride=[30.0, 0.0, 5.0]),
         dict(tokens=P + [C.EOS], stride=[30.0, 5.0, 5.0]),
         dict(tokens=P + [tb + 300, 4, 5, tb + 700, C.EOS], stride=[30.0, 5.0, 0.0])],
        [dict(tokens=P + [C.EOS], stride=[30.0, 0.0, 5.0]),
         dict(tokens=P + [tb + 300, 4, 5, tb + 700, tb + 700, 6, C.EOS], stride=[25.0, 5.0, 0.0])],
        # no closing timestamp at all
        [dict(tokens=P + [tb + 10, 1, 2, 3, 4, C.EOS], stride=[30.0, 0.0, 5.0]),
         dict(tokens=P + [tb, 3, 4, 5, 6, C.EOS], stride=[12.0, 5.0, 0.0])],
    ]
    cases += [dict(timestamps=True, outputs=o) for o in hand]
    return cases


def main():
    from transformers.models.whisper import tokenization_whisper as T
    from transformers.pipelines.automatic_speech_recognition import chunk_iter

    rng = random.Random(20261021)
    tok = StandInTokenizer()
    out = {}

    merge = []
    for seqs in merge_cases(rng):
        stamps = [[(j, k) for k in range(len(s))] for j, s in enumerate(seqs)]
        plain = T._find_longest_common_sequence([list(s) for s in seqs])
        if len(seqs) > 1 or seqs[0]:
            ids, where = T._find_longest_common_sequence([list(s) for s in seqs], stamps)
        else:
            ids, where = plain, []
        assert [int(t) for t in ids] == [int(t) for t in plain]
        mine, cuts, _ = C.merge_sequences(seqs)
        assert mine == [int(t) for t in ids], (seqs, mine, ids)
        assert C.origins(seqs, cuts) == [tuple(w) for w in where], (seqs, cuts, where)
        merge.append(dict(seqs=seqs, merged=[int(t) for t in ids], origins=[list(w) for w in where]))
    out["merge"] = merge
    print(f"merge: {len(merge)} groups, {sum(1 for m in merge if len(m['merged']) < sum(map(len, m['seqs'])))} with a cut")

    asr = []
    for case in asr_cases(rng):
        outs = [dict(tokens=np.array([o["tokens"]]), stride=tuple(o["stride"])) for o in case["outputs"]]
        text, opt = T._decode_asr(tok, outs, return_timestamps=case["timestamps"], return_language=False,
                                  time_precision=C.TIME_PRECISION)
        mine = C.transcript(case["outputs"], C.stand_in_decode)
        assert mine["text"] == text, (mine["text"], text)
        rec = dict(case, text=text)
        if case["timestamps"]:
            rec["chunks"] = [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in opt["chunks"]]
            assert [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in mine["chunks"]] == rec["chunks"], \
                (mine["chunks"], rec["chunks"])
        else:
            assert len(mine["chunks"]) <= 1
        asr.append(rec)
    out["asr"] = asr
    print(f"asr: {len(asr)} recordings, {sum(len(a.get('chunks', [])) for a in asr)} timed segments, "
          f"{sum(1 for a in asr if a.get('chunks') and a['chunks'][-1]['timestamp'][1] is None)} without a closing timestamp")

    class Extractor:
        sampling_rate = C.SAMPLING_RATE

        def __call__(self, chunk, **_):
            return {}

    strides = []
    sr = C.SAMPLING_RATE
    for n, chunk_s, left_s, right_s in ((70 * sr, 30, 5, 5), (60 * sr, 30, 5, 5), (30 * sr, 30, 5, 5), (30 * sr + 1, 30, 5, 5),
                                        (12 * sr, 30, 5, 5), (44 * sr, 30, 5, 5), (45 * sr, 30, 5, 5), (45 * sr + 7, 30, 5, 5),
                                        (100 * sr + 123, 20, 4, 2), (3600 * sr, 30, 5, 5)):
        got = [list(map(int, it["stride"])) for it in chunk_iter(np.zeros(n, dtype=np.float32), Extractor(), chunk_s * sr,
                                                                 left_s * sr, right_s * sr)]
        mine = C.chunk_strides(n, chunk_s * sr, left_s * sr, right_s * sr)
        assert [list(m[1:]) for m in mine] == got, (n, mine[-3:], got[-3:])
        strides.append(dict(n=n, chunk_length_s=chunk_s, stride_length_s=[left_s, right_s], strides=got))
    out["strides"] = strides
    print("strides:", [(s["n"], len(s["strides"]), s["strides"][-1]) for s in strides])

    np.savez_compressed(C.GOLDEN, **{k: np.array(json.dumps(v)) for k, v in out.items()})
    print(C.GOLDEN.name, C.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
