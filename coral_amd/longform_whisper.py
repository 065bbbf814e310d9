"""Whisper timestamps on the host: segments of a decoded window and the sequential long-form loop.

Restated from the installed transformers ($TF/models/whisper/generation_whisper.py), not imported from it:

  * `segments_of`  - `_retrieve_segment`: a window's generated ids are cut at every closed timestamp pair; the window
    then advances to the last closed pair, or by all its frames when it ends in a single timestamp or holds no pair;
  * `run_longform` - the loop of `WhisperGenerationMixin.generate` for inputs above 3000 frames with the arguments the
    ASR pipeline passes (R/src/coral/evaluate.py runs `pipeline(...)` with no generate_kwargs).  Every clip keeps a
    `seek` (in frames of 10 ms); each round decodes the window [seek, seek + 3000) of every unfinished clip as one batch.
    What decodes a batch of windows is a parameter, so the loop itself needs no GPU;
  * `PromptPolicy` / `prepare_decoder_inputs` - `condition_on_prev_tokens`, `prompt_ids`, `prompt_condition_type`:
    `_prepare_segments`, `_prepare_decoder_input_ids` with the part of `_pad_to_max_length` it uses, and
    `_set_max_new_tokens_and_length`: a window's decoder input is the clip's previous text (or a prompt) behind
    <|startofprev|>, then the forced prefix, left-padded to the longest row of the round;
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
            hint = "; pass `fallback=FallbackPolicy(...)`" if name in _FALLBACK_NAMES else \
                "; pass `conditioning=PromptPolicy(...)`" if name in _PROMPT_NAMES else ""
            raise ValueError(f"long-form decoding: {name}={val!r} is not implemented as a loose argument (greedy windows, "
                             f"each decoded from the forced prefix alone){hint}")


_FALLBACK_NAMES = ("temperature", "no_speech_threshold", "logprob_threshold", "compression_ratio_threshold")
_PROMPT_NAMES = ("condition_on_prev_tokens", "prompt_ids", "prompt_condition_type")


# ---- previous-text conditioning and prompts --------------------------------------------------------------------------
@dataclass(frozen=True)
class PromptPolicy:
    """The arguments of transformers' long-form generate that change what the decoder sees.  prompt_ids: the ids
    `WhisperProcessor.get_prompt_ids` returns (<|startofprev|> first) or None; prompt_condition_type: "first-segment"
    (the prompt stands in front of the first window's previous text only) or "all-segments" (in front of every
    window's; needs condition_on_prev_tokens, as in transformers); condition_on_prev_tokens: a window's decoder input
    starts with the clip's text so far, the last max_target_positions // 2 - 1 tokens at most; prev_sot_token_id:
    <|startofprev|>, None = suppress_tokens[-2] of the run (`_prepare_decoder_input_ids`)."""
    prompt_ids: tuple | None = None
    prompt_condition_type: str | None = None
    condition_on_prev_tokens: bool = False
    prev_sot_token_id: int | None = None

    def __post_init__(self):
        kind = self.prompt_condition_type or "first-segment"
        if kind not in ("first-segment", "all-segments"):
            raise ValueError(f"PromptPolicy: prompt_condition_type={self.prompt_condition_type!r} does not exist "
                             "(first-segment, all-segments)")
        if not isinstance(self.condition_on_prev_tokens, bool):
            raise ValueError(f"PromptPolicy: condition_on_prev_tokens must be True or False, got {self.condition_on_prev_tokens!r}")
        if kind == "all-segments" and not self.condition_on_prev_tokens:
            raise ValueError("PromptPolicy: prompt_condition_type='all-segments' needs condition_on_prev_tokens=True")
        object.__setattr__(self, "prompt_condition_type", kind)
        if self.prompt_ids is not None:
            ids = tuple(int(t) for t in self.prompt_ids)
            if not ids or any(t < 0 for t in ids):
                raise ValueError("PromptPolicy: prompt_ids must be a non-empty sequence of token ids")
            object.__setattr__(self, "prompt_ids", ids)
        if self.prev_sot_token_id is not None and (isinstance(self.prev_sot_token_id, bool)
                                                   or not isinstance(self.prev_sot_token_id, int)):
            raise ValueError(f"PromptPolicy: prev_sot_token_id must be an id or None, got {self.prev_sot_token_id!r}")

    @property
    def active(self) -> bool:
        return self.condition_on_prev_tokens or self.prompt_ids is not None

    def prev_sot(self, suppress_tokens=None):
        """<|startofprev|> as `_prepare_decoder_input_ids` finds it: the configured id, else suppress_tokens[-2], else None."""
        if self.prev_sot_token_id is not None:
            return self.prev_sot_token_id
        if suppress_tokens is not None and len(suppress_tokens) >= 2:
            return int(list(suppress_tokens)[-2])
        return None

    def first_segments(self, clips: int, suppress_tokens=None) -> list:
        """`_prepare_segments`: with a first-segment prompt every clip starts with the prompt (without its leading
        <|startofprev|>) as a segment of its own, which the loop drops from what it returns."""
        if self.prompt_ids is not None and self.prompt_condition_type == "first-segment":
            ids = list(self.prompt_ids)
            # (transformers compares with generation_config.prev_sot_token_id alone here, not with the suppress_tokens fallback)
            ids = ids[1:] if ids[0] == self.prev_sot_token_id else ids
            return [[ids] for _ in range(clips)]
        return [[] for _ in range(clips)]


def prepare_decoder_inputs(init_tokens, segments, batch, do_condition, policy: PromptPolicy, pad_id: int,
                           max_target_positions: int, timestamp_begin: int, suppress_tokens=None):
    """`_prepare_decoder_input_ids` for one round.  init_tokens: the forced prefix; segments[i]: clip i's segments so far
    (token lists); batch: the clips of the round (`batch_idx_map`); do_condition: the per-row flags as transformers keeps
    them.  -> (rows, start, masked): equally long id rows, the number of leading pad positions of each, and whether
    transformers passes a decoder_attention_mask (ids != pad) for them.

    Restated as the installed transformers runs it, three details included: the previous-text branch is taken when ANY
    flag is set and CLIP 0 has a segment, whoever is in the batch; the flags are read at the clips' own indices; the
    longest row is taken over the rows with previous text only, and a shorter target cuts a row from the left."""
    init = [int(t) for t in init_tokens]
    cut_off = max_target_positions // 2 - 1
    prev_sot = policy.prev_sot(suppress_tokens)
    if any(do_condition) and len(segments[0]) > 0:
        if policy.prompt_ids is not None and policy.prompt_condition_type == "all-segments":
            prev_ids = list(policy.prompt_ids)
        else:
            prev_ids = [prev_sot] if prev_sot is not None else None
        rows, longest = [], 0
        for i in batch:
            segs = segments[i] if do_condition[i] else None
            if segs is not None and len(segs) > 0:
                seq = []
                for tokens in segs:
                    # a segment that ends with two timestamps gives the text in front and the first of them
                    skip = len(tokens) > 2 and tokens[-2] >= timestamp_begin
                    seq += [int(t) for t in (tokens[:-1] if skip else tokens)]
                seq = seq[-cut_off:]
                if prev_ids is not None:
                    seq = prev_ids + seq
                rows.append(seq)
                longest = max(longest, len(seq))
            else:
                rows.append(list(prev_ids) if prev_ids is not None else [])
        out, start = [], []
        for seq in rows:
            n = longest - len(seq)
            seq = [pad_id] * n + seq if n >= 0 else seq[-n:]  # (F.pad with a negative amount cuts)
            out.append(seq + init)
            start.append(max(n, 0))
        return out, start, True
    if policy.prompt_ids is not None:
        return [list(policy.prompt_ids) + init for _ in batch], [0] * len(batch), False
    return [list(init) for _ in batch], [0] * len(batch), False


def grown_max_length(max_length: int, decoder_len: int, max_target_positions: int, max_new_tokens=None) -> int:
    """`_set_max_new_tokens_and_length` for one round: -> the generation config's max_length after it (the increase is kept
    from round to round, as transformers keeps it in the generation config)."""
    if (max_new_tokens or 0) + decoder_len > max_target_positions:
        raise ValueError(f"long-form decoding: the decoder input (start tokens, prompt and previous text) is {decoder_len} "
                         f"tokens and max_new_tokens is {max_new_tokens or 0}: together they exceed the "
                         f"{max_target_positions} target positions; shorten the prompt or reduce max_new_tokens")
    if max_new_tokens is None:
        return min(max_length + min(max_target_positions // 2 - 1, decoder_len), max_target_positions)
    return max_length


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
                         eos_id: int, vocab_size: int, max_length: int, inputs: dict | None = None):
    """`generate_with_fallback` for one batch of windows.  window_generate(batch, temperature, uniforms) -> (rows, stats):
    id rows as `generate` returns them and dict(sum_logprob, n_scored, no_speech_prob) per row (no_speech_prob may be None
    without a no-speech threshold); uniforms: float32 [len(batch), max_length] for a sampled attempt, None at temperature
    0.  Only the rows that failed are decoded again; a row keeps the result of the last attempt it took part in.
    -> (kept, should_skip): per window of `batch` dict(row, temperature, avg_logprob, compression_ratio, no_speech_prob).

    Restated as the installed transformers runs it, two details included: the flags of an attempt are written at the
    row's index WITHIN the attempt, and the no-speech probability read for it is that of the window at that index of the
    whole batch (the detector keeps the inputs of the first attempt).  With one window per batch neither shows.
    inputs: the round's decoder inputs (`prepare_decoder_inputs`: dict with rows and start per window); window_generate
    then takes them as a fourth argument, cut down to the windows of the attempt with their own rows."""
    import torch

    n = len(batch)
    kept, skip = [None] * n, [False] * n
    index_map, cur, nsp = list(range(n)), list(batch), None
    for k, temperature in enumerate(policy.temperatures):
        uniforms = torch.rand(len(cur), max_length, generator=generator) if temperature > 0 else None
        if inputs is None:
            rows, stats = window_generate(cur, temperature, uniforms)
        else:
            mine = dict(inputs, rows=[inputs["rows"][j] for j in index_map], start=[inputs["start"][j] for j in index_map])
            rows, stats = window_generate(cur, temperature, uniforms, mine)
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
                 vocab_size: int | None = None, max_length: int | None = None, conditioning: PromptPolicy | None = None,
                 init_tokens=None, max_target_positions: int | None = None, suppress_tokens=None,
                 max_new_tokens: int | None = None, **other):
    """window_generate([(clip, seek), ...]) -> one generated id row per entry (prefix included, padded as `generate`
    pads).  num_frames: log-mel frames per clip.  -> per clip dict(segments=[(start_s, end_s, ids)], windows=[(seek,
    generated ids)]).  batch_size: at most that many windows per call (None: all unfinished clips at once).
    return_token_timestamps=True: window_generate returns (id rows, float32 times [rows, row length]); segments are
    (start_s, end_s, ids, token times) and windows (seek, generated ids, their times).
    fallback: a FallbackPolicy; the protocol is then window_generate(batch, temperature, uniforms) -> (rows, stats)
    (`decode_with_fallback`), vocab_size and max_length are needed, and every clip also carries window_stats: per window
    dict(seek, temperature, avg_logprob, compression_ratio, no_speech_prob, skipped).  A skipped window advances seek by
    its frames and contributes no segment.
    conditioning: a PromptPolicy (previous text and / or a prompt in front of the forced prefix); init_tokens (the forced
    prefix), max_target_positions and max_length are then needed, prefix_len is not used, and window_generate takes one
    more argument, the round's decoder inputs: dict(rows, start, masked, max_length, no_speech_index) - equally long id
    rows for the windows of the call, the number of leading pad positions of each, whether transformers masks them, the
    round's max_length (`grown_max_length`; with max_new_tokens the row length plus that) and the position of
    <|startoftranscript|> in the rows.  Rows are padded to the longest of the whole ROUND, whatever batch_size is: the
    padding counts as positions, so what a window decodes must not depend on how the round is cut into calls.  With
    fallback=, a window accepted at a temperature of 0.5 or more switches the conditioning off for the next window - at
    the window's index within the round, where transformers writes the flag (clips' own indices are where it reads
    it: the two differ once a clip in front has finished)."""
    check_longform_arguments(other)
    if conditioning is not None and not conditioning.active:
        conditioning = None
    if conditioning is not None:
        if return_token_timestamps:
            raise ValueError("long-form decoding: return_token_timestamps=True is not implemented with conditioning=")
        if init_tokens is None or max_target_positions is None or max_length is None:
            raise ValueError("long-form decoding: conditioning= needs init_tokens, max_target_positions and max_length")
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
    if conditioning is not None:
        history = conditioning.first_segments(len(num_frames), suppress_tokens)  # per clip: token lists, prompt first
        do_condition = [conditioning.condition_on_prev_tokens] * len(num_frames)
    out = [dict(segments=[], windows=[]) for _ in num_frames]
    if fallback is not None:
        for o in out:
            o["window_stats"] = []
    while True:
        todo = [i for i, n in enumerate(num_frames) if seek[i] < n]
        if not todo:
            return out
        step = batch_size or len(todo)
        inputs = None
        if conditioning is not None:
            ids, start, masked = prepare_decoder_inputs(init_tokens, history, todo, do_condition, conditioning, pad_id,
                                                        max_target_positions, timestamp_begin, suppress_tokens)
            prefix_len = len(ids[0])
            max_length = grown_max_length(max_length, prefix_len, max_target_positions, max_new_tokens)
            inputs = dict(rows=ids, start=start, masked=masked, no_speech_index=prefix_len - len(init_tokens),
                          max_length=max_length if max_new_tokens is None else prefix_len + max_new_tokens)
        for a in range(0, len(todo), step):
            batch = todo[a:a + step]
            skipped = [False] * len(batch)
            mine = None if inputs is None else dict(inputs, rows=inputs["rows"][a:a + step], start=inputs["start"][a:a + step])
            if fallback is None:
                rows = window_generate([(i, seek[i]) for i in batch], *(() if mine is None else (mine,)))
            else:
                kept, skipped = decode_with_fallback(window_generate, [(i, seek[i]) for i in batch], fallback, generator,
                                                     prefix_len, pad_id, eos_id, vocab_size,
                                                     max_length if mine is None else mine["max_length"], mine)
                rows = [k["row"] for k in kept]
                if conditioning is not None:
                    for j, k in enumerate(kept):
                        do_condition[a + j] = conditioning.condition_on_prev_tokens and k["temperature"] < 0.5
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
                if conditioning is not None:
                    history[i] += [seg[2] for seg in segs]
                seek[i] += adv


def stitched_ids(segments, timestamp_begin: int) -> list[int]:
    """The text tokens of a recording's segments in order (timestamps dropped)."""
    return [t for seg in segments for t in seg[2] if t < timestamp_begin]
