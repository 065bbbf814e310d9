"""Whisper timestamps on the host: segments of a decoded window and the sequential long-form loop.

Restated from the installed transformers ($TF/models/whisper/generation_whisper.py), not imported from it:

  * `segments_of`  - `_retrieve_segment`: a window's generated ids are cut at every closed timestamp pair; the window
    then advances to the last closed pair, or by all its frames when it ends in a single timestamp or holds no pair;
  * `run_longform` - the loop of `WhisperGenerationMixin.generate` for inputs above 3000 frames with the arguments the
    ASR pipeline passes (R/src/coral/evaluate.py runs `pipeline(...)` with no generate_kwargs): no
    `condition_on_prev_tokens`, no prompt.  Every clip keeps a `seek` (in frames of 10 ms); each round decodes the window
    [seek, seek + 3000) of every unfinished clip as one batch.  What decodes a batch of windows is a parameter, so the
    loop itself needs no GPU;
  * `FallbackPolicy` / `decode_with_fallback` - `generate_with_fallback`, `_need_fallback`, `_retrieve_compression_ratio`:
    a window is decoded at temperature 0, scored by average log-probability, compression ratio of its ids and no-speech
    probability, decoded again with sampling where it fails, and skipped where it is silence.

Times are float64 seconds computed as transformers computes them: offset = seek * time_precision / input_stride,
time = offset + timestamp_index * time_precision."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import numpy as np

TIME_PRECISION = 0.02           # seconds per timestamp step (= one encoder position)
TIME_PRECISION_FEATURES = 0.01  # seconds per log-mel frame
INPUT_STRIDE = 2                # log-mel frames per encoder position
WINDOW_FRAMES = 3000

# arguments of transformers' long-form generate that change what the loop does and that this build does not implement
_LONGFORM_REFUSED = {"temperature": (None, 0.0, 1.0), "condition_on_prev_tokens": (None, False),
                     "no_speech_threshold": (None,), "logprob_threshold": (None,), "compression_ratio_threshold": (None,),
                     "prompt_ids": (None,), "prompt_condition_type": (None,),
                     "num_beams": (None, 1)}


def check_longform_arguments(other: dict) -> None:
    for name, val in other.items():
        neutral = _LONGFORM_REFUSED.get(name)
        if neutral is None:
            raise ValueError(f"long-form decoding: argument {name}={val!r} is not known to this build")
        if not any(val is n or (n is not None and type(val) is type(n) and val == n) for n in neutral):
            hint = "; pass `fallback=FallbackPolicy(...)`" if name in _FALLBACK_NAMES else ""
            raise ValueError(f"long-form decoding: {name}={val!r} is not implemented as a loose argument (greedy windows, "
                             f"each decoded from the forced prefix alone){hint}")


_FALLBACK_NAMES = ("temperature", "no_speech_threshold", "logprob_threshold", "compression_ratio_threshold")


# ---- temperature fallback ----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FallbackPolicy:
    """The arguments of transformers' long-form generate that drive `generate_with_fallback`.  temperatures: tried in
    order, 0 = greedy, > 0 = sampled; a threshold of None is not checked.  no_speech_threshold needs logprob_threshold (the
    skip rule is "below the log-prob threshold and above the no-speech threshold") and no_speech_token, the id whose
    probability at the start-of-transcript position is the no-speech probability.  seed: of the one CPU generator the
    sampling uniforms are drawn from."""
    temperatures: tuple = (0.0,)
    logprob_threshold: float | None = None
    compression_ratio_threshold: float | None = None
    no_speech_threshold: float | None = None
    no_speech_token: int | None = None
    seed: int = 0

    def __post_init__(self):
        ts = self.temperatures
        ts = (ts,) if isinstance(ts, (int, float)) and not isinstance(ts, bool) else tuple(ts)
        if not ts or any(not isinstance(t, (int, float)) or isinstance(t, bool) or not math.isfinite(t) or t < 0 for t in ts):
            raise ValueError(f"FallbackPolicy: temperatures must be non-negative finite numbers, got {self.temperatures!r}")
        object.__setattr__(self, "temperatures", tuple(float(t) for t in ts))
        if self.no_speech_threshold is not None and (self.logprob_threshold is None or self.no_speech_token is None):
            raise ValueError("FallbackPolicy: no_speech_threshold needs logprob_threshold and no_speech_token")

    @property
    def needs_stats(self) -> bool:
        return self.logprob_threshold is not None


def compression_ratio(ids, vocab_size: int) -> float:
    """`_retrieve_compression_ratio`: raw bytes over zlib-compressed bytes of the ids, int(log2(V) / 8) + 1 little-endian
    bytes each.  No tokenizer is involved."""
    length = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(length, "little") for t in ids)
    return len(raw) / len(zlib.compress(raw))


def need_fallback(policy: FallbackPolicy, ids_with_eos, avg_logprob, no_speech_prob, vocab_size: int):
    """`_need_fallback` -> (needs_fallback, should_skip, compression ratio or None)."""
    needs, skip, ratio = False, False, None
    if policy.compression_ratio_threshold is not None:
        ratio = compression_ratio(ids_with_eos, vocab_size)
        if ratio > policy.compression_ratio_threshold:
            needs = True
    if policy.logprob_threshold is not None and avg_logprob < policy.logprob_threshold:
        needs = True
    if policy.no_speech_threshold is not None:
        if avg_logprob < policy.logprob_threshold and no_speech_prob > policy.no_speech_threshold:
            needs, skip = False, True
    return needs, skip, ratio


def strip_padding(row, prefix_len: int, pad_id: int, eos_id: int) -> list[int]:
    """A generated row -> the tokens after the prefix without the padding, the EOS kept ('remove all padding tokens, except
    for the eos token': the sequence the statistics of `_need_fallback` are taken over)."""
    gen = [int(t) for t in row[prefix_len:]]
    if gen and gen[-1] == pad_id:
        n = sum(1 for t in gen if t == pad_id) - (1 if pad_id == eos_id else 0)
        if n:
            gen = gen[:-n]
    return gen


def decode_with_fallback(window_generate, batch, policy: FallbackPolicy, generator, prefix_len: int, pad_id: int,
                         eos_id: int, vocab_size: int, max_length: int):
    """`generate_with_fallback` for one batch of windows.  window_generate(batch, temperature, uniforms) -> (rows, stats):
    id rows as `generate` returns them and dict(sum_logprob, n_scored, no_speech_prob) per row (no_speech_prob may be None
    without a no-speech threshold); uniforms: float32 [len(batch), max_length] for a sampled attempt, None at temperature
    0.  Only the rows that failed are decoded again; a row keeps the result of the last attempt it took part in.
    -> (kept, should_skip): per window of `batch` dict(row, temperature, avg_logprob, compression_ratio, no_speech_prob).

    Restated as the installed transformers runs it, two details included: the flags of an attempt are written at the
    row's index WITHIN the attempt, and the no-speech probability read for it is that of the window at that index of the
    whole batch (the detector keeps the inputs of the first attempt).  With one window per batch neither shows."""
    import torch

    n = len(batch)
    kept, skip = [None] * n, [False] * n
    index_map, cur, nsp = list(range(n)), list(batch), None
    for k, temperature in enumerate(policy.temperatures):
        uniforms = torch.rand(len(cur), max_length, generator=generator) if temperature > 0 else None
        rows, stats = window_generate(cur, temperature, uniforms)
        if len(rows) != len(cur):
            raise ValueError(f"window_generate returned {len(rows)} rows for {len(cur)} windows")
        if k == 0 and policy.no_speech_threshold is not None:
            nsp = [float(p) for p in stats["no_speech_prob"]]
        next_map, next_cur = [], []
        for i, row in enumerate(rows):
            seq = strip_padding(row, prefix_len, pad_id, eos_id)
            avg = None
            if policy.needs_stats:
                avg = float(stats["sum_logprob"][i]) / max(int(stats["n_scored"][i]), 1)
            needs, skip[i], ratio = need_fallback(policy, seq, avg, None if nsp is None else nsp[i], vocab_size)
            kept[index_map[i]] = dict(row=row, temperature=temperature, avg_logprob=avg, compression_ratio=ratio,
                                      no_speech_prob=None if nsp is None else nsp[i])
            if needs:
                next_map.append(index_map[i])
                next_cur.append(cur[i])
        index_map = next_map
        if not index_map or k == len(policy.temperatures) - 1:
            break
        cur = next_cur
    return kept, skip


def strip_generated(row, prefix_len: int, pad_id: int, eos_id: int) -> list[int]:
    """A generated row -> the tokens after the prefix without the padding and the EOS (`generate_with_fallback`:
    'remove all padding tokens, except for the eos token', then 'remove eos token')."""
    gen = [int(t) for t in row[prefix_len:]]
    if gen and gen[-1] == pad_id:
        n = sum(1 for t in gen if t == pad_id) - (1 if pad_id == eos_id else 0)
        if n:
            gen = gen[:-n]
    if gen and gen[-1] == eos_id:
        gen = gen[:-1]
    return gen


def segments_of(ids, timestamp_begin: int, time_precision: float = TIME_PRECISION, num_frames: int = WINDOW_FRAMES,
                time_offset: float = 0.0, return_advance: bool = False, token_times=None):
    """ids: the tokens one window generated (no prefix, no EOS).  -> [(start_s, end_s, token ids)] as `_retrieve_segment`
    cuts them (a segment's ids keep its timestamp tokens); return_advance=True: (segments, frames to advance by).
    token_times: the window's time per token of `ids` (float32, from 0 at the window's start): a segment is then
    (start_s, end_s, token ids, token times), the times cut like the ids and shifted by the offset in float32, as
    `_retrieve_segment` adds its float64 scalar to the float32 tensor."""
    ids = [int(t) for t in ids]
    if token_times is not None:
        token_times = np.asarray(token_times, dtype=np.float32)
        if token_times.shape != (len(ids),):
            raise ValueError(f"segments_of: {token_times.shape} token times for {len(ids)} tokens")
    timed = (lambda a, b: (token_times[a:b] + np.float32(time_offset),)) if token_times is not None else (lambda a, b: ())
    is_ts = [t >= timestamp_begin for t in ids]
    single_ending = is_ts[-2:] == [False, True]
    slices = [i + 1 for i in range(len(ids) - 1) if is_ts[i] and is_ts[i + 1]]
    segments = []
    if slices:
        if single_ending:
            slices.append(len(ids))
        else:
            slices[-1] += 1  # the last segment keeps its closing timestamp and the one that opens the unfinished rest
        last = 0
        for i, cur in enumerate(slices):
            tokens = ids[last:cur]
            is_last = i == len(slices) - 1
            start = tokens[0] - timestamp_begin
            end = tokens[-1 if (not is_last or single_ending) else -2] - timestamp_begin
            segments.append((time_offset + float(start) * time_precision, time_offset + float(end) * time_precision, tokens)
                            + timed(last, cur))
            last = cur
        if single_ending:
            advance = num_frames  # no speech after the last timestamp
        else:
            advance = (ids[last - 2] - timestamp_begin) * INPUT_STRIDE  # the unfinished rest is decoded again
    else:
        stamps = [t for t in ids if t >= timestamp_begin]
        # (transformers multiplies a 0-dim integer tensor by Python floats here: the arithmetic is float32)
        last_pos = int(np.float32(num_frames) * np.float32(TIME_PRECISION_FEATURES) / np.float32(time_precision))
        if stamps and stamps[-1] != timestamp_begin:
            last_pos = float(stamps[-1] - timestamp_begin)
        segments.append((time_offset, time_offset + last_pos * time_precision, ids) + timed(0, len(ids)))
        advance = num_frames
    return (segments, int(advance)) if return_advance else segments


def run_longform(window_generate, num_frames, timestamp_begin: int, prefix_len: int, pad_id: int, eos_id: int,
                 time_precision: float = TIME_PRECISION, batch_size: int | None = None,
                 return_token_timestamps: bool | None = False, fallback: FallbackPolicy | None = None,
                 vocab_size: int | None = None, max_length: int | None = None, **other):
    """window_generate([(clip, seek), ...]) -> one generated id row per entry (prefix included, padded as `generate`
    pads).  num_frames: log-mel frames per clip.  -> per clip dict(segments=[(start_s, end_s, ids)], windows=[(seek,
    generated ids)]).  batch_size: at most that many windows per call (None: all unfinished clips at once).
    return_token_timestamps=True: window_generate returns (id rows, float32 times [rows, row length]); segments are
    (start_s, end_s, ids, token times) and windows (seek, generated ids, their times).
    fallback: a FallbackPolicy; the protocol is then window_generate(batch, temperature, uniforms) -> (rows, stats)
    (`decode_with_fallback`), vocab_size and max_length are needed, and every clip also carries window_stats: per window
    dict(seek, temperature, avg_logprob, compression_ratio, no_speech_prob, skipped).  A skipped window advances seek by
    its frames and contributes no segment."""
    check_longform_arguments(other)
    generator = None
    if fallback is not None:
        import torch

        if return_token_timestamps:
            raise ValueError("long-form decoding: return_token_timestamps=True is not implemented with fallback=")
        if vocab_size is None or max_length is None:
            raise ValueError("long-form decoding: fallback= needs vocab_size and max_length")
        generator = torch.Generator().manual_seed(int(fallback.seed))
    num_frames = [int(n) for n in num_frames]
    seek = [0] * len(num_frames)
    out = [dict(segments=[], windows=[]) for _ in num_frames]
    if fallback is not None:
        for o in out:
            o["window_stats"] = []
    while True:
        todo = [i for i, n in enumerate(num_frames) if seek[i] < n]
        if not todo:
            return out
        step = batch_size or len(todo)
        for a in range(0, len(todo), step):
            batch = todo[a:a + step]
            skipped = [False] * len(batch)
            if fallback is None:
                rows = window_generate([(i, seek[i]) for i in batch])
            else:
                kept, skipped = decode_with_fallback(window_generate, [(i, seek[i]) for i in batch], fallback, generator,
                                                     prefix_len, pad_id, eos_id, vocab_size, max_length)
                rows = [k["row"] for k in kept]
                for i, k, sk in zip(batch, kept, skipped):
                    out[i]["window_stats"].append(dict(seek=seek[i], skipped=bool(sk),
                                                       **{n: v for n, v in k.items() if n != "row"}))
            times = [None] * len(batch)
            if return_token_timestamps:
                rows, times = rows
                if len(times) != len(rows):
                    raise ValueError(f"window_generate returned {len(times)} rows of token times for {len(rows)} id rows")
            if len(rows) != len(batch):
                raise ValueError(f"window_generate returned {len(rows)} rows for {len(batch)} windows")
            for i, row, tt, sk in zip(batch, rows, times, skipped):
                gen = strip_generated(row, prefix_len, pad_id, eos_id)
                frames = min(num_frames[i] - seek[i], WINDOW_FRAMES)
                offset = seek[i] * time_precision / INPUT_STRIDE
                if tt is not None:  # (the generated tokens' share of the row's times)
                    tt = np.asarray(tt, dtype=np.float32)[prefix_len:prefix_len + len(gen)]
                out[i]["windows"].append((seek[i], gen) if tt is None else (seek[i], gen, tt))
                if not gen or sk:  # (empty: cannot happen under the timestamp rules; skipped: silence, no segment)
                    seek[i] += frames
                    continue
                segs, adv = segments_of(gen, timestamp_begin, time_precision, frames, offset, return_advance=True,
                                        token_times=tt)
                out[i]["segments"] += segs
                seek[i] += adv


def stitched_ids(segments, timestamp_begin: int) -> list[int]:
    """The text tokens of a recording's segments in order (timestamps dropped)."""
    return [t for seg in segments for t in seg[2] if t < timestamp_begin]
