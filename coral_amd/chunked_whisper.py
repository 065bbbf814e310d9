"""Long recordings through Whisper in chunks: overlapping 30 s chunks decoded as batches, token merge on the GPU.

The reference transcribes through `transformers.pipeline("automatic-speech-recognition")`; for a Whisper model its
`chunk_length_s` cuts overlapping chunks (`chunk_iter`), decodes them as one batch each and merges the token
sequences where they overlap ($TF/models/whisper/tokenization_whisper.py `_decode_asr`,
`_find_longest_common_sequence`).  This module is that mode: `longform.chunk_plan(..., align_to=1)` plans the chunks,
the engine's `generate` decodes them `batch_size` at a time - the decoder streams its weights once per token whatever
the batch, so the windows of ONE recording share that cost, which the sequential loop of longform_whisper.py cannot
do -, and `ca_overlap_merge` (csrc/chunk_merge.hip) merges all recordings in one launch.

Without timestamps a recording is one group: its chunks' rows, with the forced prefix, the special ids, the
timestamp range and the padding dropped by the kernel's skip bitmap while a row is loaded.  With timestamps the
pipeline's stride handling (`plan_segments`, restated from `_decode_asr`) runs on the host over the id rows: it decides
the segments and which token runs belong to each without ever needing a merge result, so every segment of every
recording is one group of the same single launch.

Differences from the pipeline, by design: a chunk that decodes to no text stays in its group as an empty row, so its
neighbours are concatenated (they do not overlap in audio) where the pipeline would search an overlap between them;
every chunk is decoded as one padded 30 s window (the pipeline hands `generate` the extractor's attention mask).
Greedy or beam search (beams without timestamps); the fallback, prompt and word-timestamp arguments are refused."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .longform import chunk_plan

MAX_CHUNK_SECONDS = 30.0
LONG_FORMS = ("sequential", "chunked")
_REFUSED = dict(temperature="temperature fallback", logprob_threshold="temperature fallback",
                compression_ratio_threshold="temperature fallback", no_speech_threshold="temperature fallback",
                prompt_ids="prompts", prompt="prompts", condition_on_prev_tokens="conditioning on previous text",
                prompt_condition_type="conditioning on previous text")


def check_chunked_arguments(chunk_length_s, num_beams, return_timestamps, other: dict) -> None:
    """The argument checks of `transcribe_chunked`; they run before any device work."""
    if isinstance(return_timestamps, str):
        raise ValueError(f"return_timestamps={return_timestamps!r} is not implemented in chunked long-form decoding (word "
                         "timestamps take the sequential loop: whisper_long_form: sequential)")
    if not any(return_timestamps is v for v in (True, False, None)):
        raise ValueError(f"return_timestamps must be true or false in chunked long-form decoding, got {return_timestamps!r}")
    for key, value in other.items():
        if key not in _REFUSED:
            raise TypeError(f"transcribe_chunked() got an unexpected keyword argument {key!r}")
        neutral = value is None or value is False or (key == "temperature" and value in (0, 0.0, (0.0,), [0.0]))
        if not neutral:
            raise ValueError(f"{key}={value!r}: {_REFUSED[key]} is not implemented in chunked long-form decoding (it takes "
                             "the sequential loop: whisper_long_form: sequential)")
    if not chunk_length_s or chunk_length_s <= 0:
        raise ValueError(f"chunk_length_s must be positive, got {chunk_length_s}")
    if chunk_length_s > MAX_CHUNK_SECONDS:
        raise ValueError(f"chunk_length_s={chunk_length_s}: a Whisper chunk is one window of at most {MAX_CHUNK_SECONDS:g} s")
    if int(num_beams) < 1:
        raise ValueError(f"num_beams must be a positive integer, got {num_beams}")
    if int(num_beams) > 1 and return_timestamps:
        raise ValueError(f"num_beams={num_beams}: return_timestamps is decoded greedily only (beam search with timestamps is "
                         "not implemented)")


def special_ids(model, processor) -> list[int]:
    """The ids that are neither text nor timestamps: the forced prefix, the padding, and every id from eos_token_id
    upward that the tokenizer lists as special (without tokenizer files: every id from eos_token_id up to the first
    timestamp, Whisper's layout)."""
    s = model.shape
    tb = model.forced_prefix()[-1] + 1
    tok = getattr(processor, "tokenizer", None)
    listed = None
    if tok is not None and hasattr(tok, "all_special_ids"):
        listed = [int(t) for t in tok.all_special_ids]
    elif tok is not None and hasattr(tok, "get_added_tokens_decoder"):
        listed = [int(i) for i, t in tok.get_added_tokens_decoder().items() if getattr(t, "special", False)]
    if listed is None:
        listed = list(range(s.eos_token_id, tb))
    ids = set(t for t in listed if s.eos_token_id <= t < tb) | set(model.forced_prefix()) | {s.eos_token_id, s.pad_token_id}
    return sorted(ids)


def plan_segments(outputs: list, timestamp_begin: int, special, time_precision: float = 0.02) -> list:
    """The stride and timestamp handling of the pipeline (`_decode_asr`) over one recording's chunks.
    outputs: [dict(tokens=id row, stride=(chunk seconds, left stride seconds, right stride seconds))] in order.
    -> [dict(start, end, runs)]: the segments, each with the runs of text tokens whose overlap merge is its text; end is
    None where the last segment has no closing timestamp.  Rows without timestamp tokens give one segment (None, None).
      * the time offset goes back by the left stride when a chunk starts and forward by chunk length minus right stride
        when it ends; times are round(token time + offset, 2);
      * a timestamp inside the right stride - from the first of the row's trailing timestamps at or past
        chunk length minus right stride - is skipped together with its partner and resolved by the next chunk;
      * a timestamp before stride_left / time_precision is skipped in a chunk that text was carried into;
      * a start equal to the open segment's start is ignored; text left at a chunk's end is carried into the next chunk.
    A timestamp that decreases inside one chunk cannot come out of the timestamp rules of one window: it raises."""
    special = special if isinstance(special, (set, frozenset)) else set(int(t) for t in special)
    tb = int(timestamp_begin)
    segments, carried = [], []
    start, offset, skip = None, 0.0, False
    for out in outputs:
        row = [int(t) for t in out["tokens"]]
        chunk_len, left, right = out["stride"]
        offset -= left
        first_kept = left / time_precision + tb if left else tb
        stride_from = None  # the first timestamp token that belongs to the right stride
        if right:
            for t in reversed(row):
                if t >= tb:
                    if stride_from is not None and (t - tb) * time_precision < chunk_len - right:
                        break
                    stride_from = t
        run, latest = [], 0.0
        for t in row:
            if t in special:
                continue
            if t < tb:
                run.append(t)
                continue
            if float((t - tb) * time_precision) < latest:
                raise ValueError(f"timestamp token {t} ({(t - tb) * time_precision:.2f} s) follows {latest:.2f} s inside one "
                                 "chunk: not an output of Whisper's timestamp rules")
            latest = float((t - tb) * time_precision)
            time = round((t - tb) * time_precision + offset, 2)
            if stride_from and t >= stride_from:
                skip = True
            elif skip or (carried and t < first_kept):
                skip = False
            elif start is None:
                start = time
            elif time != start:
                carried.append(run)
                segments.append(dict(start=start, end=time, runs=carried))
                carried, run, start = [], [], None
        offset += chunk_len - right
        if run:
            carried.append(run)
        elif not any(carried):
            carried, start = [], None
    if carried:
        segments.append(dict(start=start, end=None, runs=carried))
    return segments


def merge_groups(groups: list, device, skip=None, want_cuts: bool = False):
    """groups: [[id rows]] -> the merged ids of every group, through one upload, one `ca_overlap_merge` launch and one
    copy back.  skip: an `ops.skip_bitmap`.  -> (merged id lists, cuts or None)."""
    rows = [r for g in groups for r in g]
    if not rows:
        return [[] for _ in groups], None
    ld = max(1, max(len(r) for r in rows))
    table = np.zeros((len(rows), ld), dtype=np.int32)
    for i, r in enumerate(rows):
        table[i, :len(r)] = r
    group_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    res = ops.overlap_merge(torch.from_numpy(table).to(device), [len(r) for r in rows], group_off, skip=skip,
                            want_cuts=want_cuts)
    merged, _, cuts = ops.overlap_merge_read(res)
    return merged, cuts


def transcribe_chunked(model, processor, arrays: list, chunk_length_s: float = 30.0, stride_length_s=None,
                       batch_size: int = 16, max_length: int | None = None, num_beams: int = 1,
                       return_timestamps: bool = False, sampling_rate=None, **other) -> list[dict]:
    """Chunked long-form transcription with the pipeline's `chunk_length_s` semantics.  -> per recording
    {"text", "ids": the merged text ids, "chunk_ids": the id row `generate` gave for every chunk} and, with
    return_timestamps=True, "chunks": [{"text", "timestamp": (start_s, end_s)}] (end_s None where the last segment has
    no closing timestamp).  The chunks of all recordings are pooled into batches of batch_size (at most 128 // num_beams
    with beams); a recording of one chunk is decoded exactly as `transcribe_whisper` decodes a clip.
    stride_length_s: None = chunk_length_s / 6 each side, a number, or (left, right).  sampling_rate: as in
    `transcribe_whisper`.  Refused by name: return_timestamps="word", the temperature fallback keys, the prompt and
    conditioning keys, num_beams > 1 with return_timestamps."""
    num_beams = int(num_beams or 1)
    check_chunked_arguments(chunk_length_s, num_beams, return_timestamps, other)
    fe = processor.feature_extractor
    sr = fe.sampling_rate
    chunk_plan(0, chunk_length_s, stride_length_s, sr, align_to=1)  # (the stride checks, before any device work)
    model.eval()
    if sampling_rate is not None:
        from .resample import to_rate

        arrays = to_rate(arrays, sampling_rate, sr, model.engine.device)
    # the pipeline's ratio for a seq2seq model is 1: chunks and strides are whole samples
    plans = [chunk_plan(len(a), chunk_length_s, stride_length_s, sr, align_to=1) for a in arrays]
    s = model.shape
    dev = model.engine.device
    max_length = int(max_length or s.max_target_positions)
    timed = bool(return_timestamps)
    tb = model.forced_prefix()[-1] + 1
    queue = [(r, i) for r, p in enumerate(plans) for i in range(len(p["chunks"]))]
    per_batch = max(1, min(int(batch_size), 128 // num_beams)) if num_beams > 1 else max(1, int(batch_size))
    gen_kw = dict(num_beams=num_beams) if num_beams > 1 else {}
    if timed:
        gen_kw["return_timestamps"] = True
    chunk_ids = [[] for _ in arrays]
    for c0 in range(0, len(queue), per_batch):
        batch = queue[c0:c0 + per_batch]
        clips = []
        for r, i in batch:
            start, n, _, _ = plans[r]["chunks"][i]
            clips.append(np.asarray(arrays[r][start:start + n], dtype=np.float32))
        ids = model.generate(fe(clips, sampling_rate=sr), language="danish", task="transcribe", max_length=max_length, **gen_kw)
        ids = ids.tolist() if hasattr(ids, "tolist") else [list(map(int, row)) for row in ids]
        for (r, _), row in zip(batch, ids):
            chunk_ids[r].append(row)
    special = special_ids(model, processor)
    decode = lambda ids: processor.batch_decode([ids], skip_special_tokens=True)[0]  # noqa: E731
    if not timed:
        bitmap = ops.skip_bitmap(special + list(range(tb, s.vocab_size)), s.vocab_size, dev)
        merged, _ = merge_groups(chunk_ids, dev, skip=bitmap)
        return [dict(text=decode(m), ids=m, chunk_ids=c) for m, c in zip(merged, chunk_ids)]
    time_precision = MAX_CHUNK_SECONDS / s.max_source_positions
    special = frozenset(special)
    segments = []
    for r, rows in enumerate(chunk_ids):
        outs = [dict(tokens=row, stride=(n / sr, left / sr, right / sr))
                for row, (_, n, left, right) in zip(rows, plans[r]["chunks"])]
        segments.append(plan_segments(outs, tb, special, time_precision))
    merged, _ = merge_groups([seg["runs"] for segs in segments for seg in segs], dev)
    joiner = "" if getattr(processor, "tokenizer", None) is not None else " "  # (offline words carry no leading space)
    results, at = [], 0
    for segs, rows in zip(segments, chunk_ids):
        mine = merged[at:at + len(segs)]
        at += len(segs)
        chunks = [dict(text=decode(m), timestamp=(seg["start"], seg["end"])) for m, seg in zip(mine, segs)]
        results.append(dict(text=joiner.join(c["text"] for c in chunks if c["text"] or joiner == ""), chunks=chunks,
                            ids=[t for m in mine for t in m], chunk_ids=rows))
    return results
