"""Plain-Python restatement of the pipeline's chunked Whisper decoding: the overlap merge and the stride / timestamp
state machine.  Ints, floats and lists only - neither transformers nor the library is imported here.

`merge_sequences` restates `_find_longest_common_sequence` ($TF/models/whisper/tokenization_whisper.py), `segments_of`
the state machine of `_decode_asr` for `return_timestamps` False / True, `chunk_strides` the pipeline's `chunk_iter`.
tools/gen_whisper_chunk_goldens.py records transformers' own output in tests/golden/whisper_chunk.npz;
tests/test_whisper_chunk_cpu.py holds this file against it, tests/test_whisper_chunk_gpu.py holds ca_overlap_merge and
`transcribe_chunked` against this file.

The merge rule.  left = s_0, total = [].  For each next sequence `right` (L = len(left), R = len(right)), for
i = 1 .. L + R - 1 compare left[max(0, L-i) : min(L, L+R-i)] with right[max(0, i-L) : min(R, i)] (equal lengths):
matches = equal positions, score = matches / i + i / 10000.0 in float64 - one division, one division, one addition.  A
diagonal is accepted when matches > 1 and its score is strictly greater than the best so far (which starts at 0.0), so
equal scores keep the earlier i.  None accepted: the indices are (L, L, 0, 0), plain concatenation.  With the winning
(ls, le, rs, re): total += left[:(ls + le) // 2], left = right[(rs + re) // 2:].  At the end total += left.  The left
side of boundary j is what boundary j-1 left of sequence j: the boundaries of a group are sequential."""
from __future__ import annotations

import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "whisper_chunk.npz"

# the stand-in vocabulary of the goldens' timestamp cases (the ids of tests/whisper_ts_ref.py)
EOS, SOT, LANG, TRANSCRIBE, NO_TIMESTAMPS, TIMESTAMP_BEGIN = 50, 51, 52, 53, 63, 64
SPECIAL_IDS = tuple(range(50, 64))
TIME_PRECISION = 0.02
SAMPLING_RATE = 16_000


def diagonal(left, right, i):
    """(matches, score, (ls, le, rs, re)) of diagonal i."""
    L, R = len(left), len(right)
    ls, le = max(0, L - i), min(L, L + R - i)
    rs, re = max(0, i - L), min(R, i)
    assert le - ls == re - rs
    matches = sum(1 for a, b in zip(left[ls:le], right[rs:re]) if a == b)
    ratio = float(matches) / float(i)
    eps = float(i) / 10000.0
    return matches, ratio + eps, (ls, le, rs, re)


def best_diagonal(left, right):
    """-> (winning i or None, its score or 0.0, the indices (ls, le, rs, re))."""
    L, R = len(left), len(right)
    best, best_i, indices = 0.0, None, (L, L, 0, 0)
    for i in range(1, L + R):
        matches, score, idx = diagonal(left, right, i)
        if matches > 1 and score > best:
            best, best_i, indices = score, i, idx
    return best_i, best, indices


def merge_sequences(seqs):
    """-> (merged ids, [(left_mid, right_mid) per boundary], [winning i or None per boundary])."""
    if not seqs:
        return [], [], []
    left, total, cuts, wins = [int(t) for t in seqs[0]], [], [], []
    for right in seqs[1:]:
        right = [int(t) for t in right]
        i, _, (ls, le, rs, re) = best_diagonal(left, right)
        left_mid, right_mid = (ls + le) // 2, (rs + re) // 2
        total += left[:left_mid]
        left = right[right_mid:]
        cuts.append((left_mid, right_mid))
        wins.append(i)
    return total + left, cuts, wins


def origins(seqs, cuts):
    """Where every merged token comes from: [(sequence, position)], from the cuts of `merge_sequences`."""
    out, lo = [], 0  # lo: the first position of the current left side inside its own sequence
    for j, (left_mid, right_mid) in enumerate(cuts):
        out += [(j, lo + k) for k in range(left_mid)]
        lo = right_mid
    if seqs:
        j = len(seqs) - 1
        out += [(j, k) for k in range(lo, len(seqs[j]))]
    return out


def equal_score_pair():
    """(left, right) whose diagonals 100 and 200 hold two matches each and every other diagonal at most one:
    2 / 100 + 100 / 10000 and 2 / 200 + 200 / 10000 are the same two float64 numbers (0.02 and 0.01) added in the other
    order, so the two scores are equal bit for bit, and the earlier diagonal must win."""
    left = list(range(1000, 1200))
    right = list(range(5000, 5040))
    right[0], right[1] = left[100], left[101]      # diagonal 100: left[100 + k] against right[k]
    right[10], right[11] = left[10], left[11]      # diagonal 200: left[k] against right[k]
    return left, right


def chunk_strides(n_samples, chunk_len, stride_left, stride_right):
    """The pipeline's `chunk_iter` in samples -> [(start, n, left, right)]: steps of chunk_len - left - right; the first
    chunk has no left stride, the first one that reaches the end no right stride and is the last; a chunk that is not
    longer than its left stride is dropped."""
    out, step = [], chunk_len - stride_left - stride_right
    for start in range(0, n_samples, step):
        end = start + chunk_len
        n = min(end, n_samples) - start
        last = end >= n_samples
        left, right = (0 if start == 0 else stride_left), (0 if last else stride_right)
        if n > left:
            out.append((start, n, left, right))
        if last:
            break
    return out


def segments_of(outputs, timestamp_begin=TIMESTAMP_BEGIN, special_ids=SPECIAL_IDS, time_precision=TIME_PRECISION):
    """`_decode_asr`'s state machine over the chunks of one recording.  outputs: [dict(tokens=[ids], stride=(chunk_len_s,
    stride_left_s, stride_right_s))] -> [dict(start, end, runs)]: the segments in order, each with the token runs whose
    merge is its text.  A recording decoded without timestamps has no timestamp tokens and comes out as one segment
    (None, None) whose runs are the chunks' non-empty text runs.

    The time offset goes back by the left stride at a chunk's start and forward by chunk length minus right stride at
    its end.  A timestamp at or above the first one of the right stride's last run is skipped together with its partner
    (`skip`); one below stride_left / time_precision is skipped in a chunk that has text carried into it; a start equal
    to the segment's start is ignored; text left over at a chunk's end is carried into the next chunk.  A timestamp that
    decreases inside one chunk raises (transformers reads it as the seam of a sequential long-form generation, which a
    chunk of at most 30 s never is)."""
    special = set(int(t) for t in special_ids)
    tb = int(timestamp_begin)
    segments, previous = [], []
    start, time_offset, skip = None, 0.0, False
    for out in outputs:
        ids = [int(t) for t in out["tokens"]]
        chunk_len, stride_left, stride_right = out["stride"]
        last_timestamp, first_timestamp = None, tb
        time_offset -= stride_left
        right_stride_start = chunk_len - stride_right
        if stride_left:
            first_timestamp = stride_left / time_precision + tb
        if stride_right:
            for t in reversed(ids):
                if t >= tb:
                    if last_timestamp is not None and (t - tb) * time_precision < right_stride_start:
                        break
                    last_timestamp = t
        current, cur_max = [], 0.0
        for t in ids:
            if t in special:
                continue
            if t < tb:
                current.append(t)
                continue
            stamp = float((t - tb) * time_precision)
            if stamp < cur_max:
                raise ValueError(f"timestamp {stamp} after {cur_max} inside one chunk")
            cur_max = stamp
            time = round((t - tb) * time_precision + time_offset, 2)
            if last_timestamp and t >= last_timestamp:
                skip = True
            elif skip or (previous and t < first_timestamp):
                skip = False
            elif start is None:
                start = time
            elif time == start:
                pass
            else:
                previous.append(current)
                segments.append(dict(start=start, end=time, runs=previous))
                previous, current, start = [], [], None
        time_offset += chunk_len - stride_right
        if current:
            previous.append(current)
        elif not any(p for p in previous):
            start, previous = None, []
    if previous:
        segments.append(dict(start=start, end=None, runs=previous))
    return segments


def transcript(outputs, decode, joiner="", **kw):
    """-> dict(text, chunks=[dict(text, timestamp=(start, end))], merged=[ids per segment]) as `_decode_asr` returns them
    with return_timestamps=True.  decode: ids -> str."""
    chunks, merged = [], []
    for seg in segments_of(outputs, **kw):
        ids = merge_sequences(seg["runs"])[0]
        merged.append(ids)
        chunks.append(dict(text=decode(ids), timestamp=(seg["start"], seg["end"])))
    return dict(text=joiner.join(c["text"] for c in chunks), chunks=chunks, merged=merged)


def stand_in_decode(ids):
    """The goldens' stand-in tokenizer: text id t is the word " w<t>"."""
    return "".join(f" w{int(t)}" for t in ids)


def load_golden():
    import numpy as np

    z = np.load(GOLDEN)
    return {k: json.loads(str(z[k])) for k in z.files}
