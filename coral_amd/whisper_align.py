"""Whisper word timestamps on the host: limits and arguments of the alignment kernels (csrc/align.hip), token times from
the DTW's jump frames, and the grouping of timed tokens into words.

Restated from the installed transformers, not imported from it:

  * `frames_of`, `times_from_jumps`        - `WhisperGenerationMixin._extract_token_timestamps`
    ($TF/models/whisper/generation_whisper.py): F_b = num_frames_b // 2 columns of the cross-attention enter the DTW;
    a row's times are P zeros, the jump times, and the last jump time once more.  Stated deviation: F_b is at least 1
    (transformers fails on an empty matrix);
  * `split_tokens_on_unicode`, `split_tokens_on_spaces`, `merge_punctuations`, `combine_tokens_into_words`,
    `collate_word_timestamps`              - the functions of the same names in $TF/models/whisper/tokenization_whisper.py,
    over a `decode(token ids) -> str` callable instead of a tokenizer (space-separated languages only);
  * `word_chunks`                          - `_decode_asr(return_timestamps="word")` for one output without strides: text
    tokens collect until a timestamp pair closes the chunk, a token's interval is (the time of the token in front of it,
    its own time), both rounded to 2 decimals, a word's interval runs from its first token's start to its last token's end.

Nothing here needs a GPU."""
from __future__ import annotations

import numpy as np

from ._lib import (ALIGN_MAX_FILTER_WIDTH, ALIGN_MAX_FRAMES, ALIGN_MAX_HEAD_DIM, ALIGN_MAX_HEADS, ALIGN_MAX_TOKENS)

TIME_PRECISION = 0.02
MEDIAN_FILTER_WIDTH = 7  # WhisperConfig.median_filter_width

PREPEND_PUNCTUATIONS = "\"'“¡¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"


# ---- limits and arguments ----------------------------------------------------------------------------------------------
def check_align_limits(A: int, Lw: int, F: int, head_dim: int, Te: int | None = None, filter_width: int | None = None):
    """The limits of ca_whisper_align_cost / ca_dtw_token_times (CA_ALIGN_MAX_*), refused by name."""
    if A > ALIGN_MAX_HEADS:
        raise ValueError(f"alignment_heads: {A} heads exceed the {ALIGN_MAX_HEADS} the alignment kernel takes")
    if Lw > ALIGN_MAX_TOKENS:
        raise ValueError(f"token timestamps: {Lw} tokens after the prefix exceed the {ALIGN_MAX_TOKENS} the DTW kernel takes")
    if F > ALIGN_MAX_FRAMES or (Te is not None and Te > ALIGN_MAX_FRAMES):
        raise ValueError(f"token timestamps: {max(F, Te or 0)} encoder positions exceed the {ALIGN_MAX_FRAMES} the alignment "
                         "kernels take")
    if head_dim % 8 or not 8 <= head_dim <= ALIGN_MAX_HEAD_DIM:
        raise ValueError(f"token timestamps: head_dim {head_dim} must be a multiple of 8 up to {ALIGN_MAX_HEAD_DIM}")
    if filter_width is not None:
        if filter_width <= 0 or filter_width % 2 != 1:
            raise ValueError("`filter_width` should be an odd number")  # (transformers' message)
        if filter_width > ALIGN_MAX_FILTER_WIDTH:
            raise ValueError(f"median_filter_width {filter_width} exceeds the {ALIGN_MAX_FILTER_WIDTH} the alignment kernel takes")


def check_alignment_heads(alignment_heads, n_layers: int, n_heads: int) -> list[tuple[int, int]]:
    if alignment_heads is None:
        # transformers' message ($TF/models/whisper/generation_whisper.py, _set_return_outputs)
        raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available. "
                         "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this property to "
                         "the generation config.")
    heads = [(int(l), int(h)) for l, h in alignment_heads]
    if not heads:
        raise ValueError("alignment_heads is empty")
    for l, h in heads:
        if not (0 <= l < n_layers and 0 <= h < n_heads):
            raise ValueError(f"alignment_heads: ({l}, {h}) is outside {n_layers} decoder layers x {n_heads} heads")
    return heads


def frames_of(num_frames, B: int, Te: int = ALIGN_MAX_FRAMES) -> list[int]:
    """F_b per clip: min(Te, num_frames_b // 2), at least 1; None: all Te positions.  An int serves every clip."""
    if num_frames is None:
        return [Te] * B
    if isinstance(num_frames, (int, np.integer)):
        num_frames = [int(num_frames)] * B
    nf = [int(n) for n in num_frames]
    if len(nf) != B:
        raise ValueError(f"num_frames: {len(nf)} entries for {B} clips")
    return [max(1, min(Te, n // 2)) for n in nf]


def times_from_jumps(jump, prefix_len: int, total_len: int, time_precision: float = TIME_PRECISION) -> np.ndarray:
    """jump int [B, Lw] (Lw = total_len - 1 - prefix_len) -> float32 seconds [B, total_len]."""
    jump = np.asarray(jump)
    B = jump.shape[0]
    times = np.zeros((B, total_len), dtype=np.float32)
    Lw = total_len - 1 - prefix_len
    if Lw <= 0:
        return times
    assert jump.shape == (B, Lw), (jump.shape, B, Lw)
    jt = (jump.astype(np.int64) * time_precision).astype(np.float32)  # (float64 product, stored as float32)
    times[:, prefix_len:prefix_len + Lw] = jt
    times[:, prefix_len + Lw] = jt[:, -1]
    return times


# ---- words -------------------------------------------------------------------------------------------------------------------
def split_tokens_on_unicode(decode, tokens):
    decoded_full = decode(list(tokens))
    replacement_char = "�"
    words, word_tokens, token_indices = [], [], []
    current_tokens, current_indices = [], []
    unicode_offset = 0
    for token_idx, token in enumerate(tokens):
        current_tokens.append(token)
        current_indices.append(token_idx)
        decoded = decode(current_tokens)
        if (replacement_char not in decoded or unicode_offset + decoded.index(replacement_char) >= len(decoded_full)
                or decoded_full[unicode_offset + decoded.index(replacement_char)] == replacement_char):
            words.append(decoded)
            word_tokens.append(current_tokens)
            token_indices.append(current_indices)
            current_tokens, current_indices = [], []
            unicode_offset += len(decoded)
    return words, word_tokens, token_indices


def split_tokens_on_spaces(decode, tokens, eos_id: int):
    subwords, subword_tokens_list, subword_indices_list = split_tokens_on_unicode(decode, tokens)
    words, word_tokens, token_indices = [], [], []
    for subword, subword_tokens, subword_indices in zip(subwords, subword_tokens_list, subword_indices_list):
        special = subword_tokens[0] >= eos_id
        with_space = subword.startswith(" ")
        punctuation = subword.strip() in "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
        if special or with_space or punctuation or len(words) == 0:
            words.append(subword)
            word_tokens.append(subword_tokens)
            token_indices.append(subword_indices)
        else:
            words[-1] = words[-1] + subword
            word_tokens[-1].extend(subword_tokens)
            token_indices[-1].extend(subword_indices)
    return words, word_tokens, token_indices


def merge_punctuations(words, tokens, indices, prepended=PREPEND_PUNCTUATIONS, appended=APPEND_PUNCTUATIONS):
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i].startswith(" ") and words[i].strip() in prepended:
            words[j] = words[i] + words[j]
            tokens[j] = tokens[i] + tokens[j]
            indices[j] = indices[i] + indices[j]
            words[i], tokens[i], indices[i] = "", [], []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i].endswith(" ") and words[j] in appended:
            words[i] += words[j]
            tokens[i] += tokens[j]
            indices[i] += indices[j]
            words[j], tokens[j], indices[j] = "", [], []
        else:
            i = j
        j += 1
    words[:] = [w for w in words if w]
    tokens[:] = [t for t in tokens if t]
    indices[:] = [x for x in indices if x]


def combine_tokens_into_words(decode, tokens, eos_id: int):
    """-> (words, the tokens of every word, the positions in `tokens` of every word)."""
    words, word_tokens, token_indices = split_tokens_on_spaces(decode, [int(t) for t in tokens], eos_id)
    merge_punctuations(words, word_tokens, token_indices)
    return words, word_tokens, token_indices


def collate_word_timestamps(decode, tokens, token_intervals, eos_id: int):
    """tokens with one (start, end) each -> [{"text", "timestamp": (first token's start, last token's end)}] per word."""
    words, _, token_indices = combine_tokens_into_words(decode, tokens, eos_id)
    return [dict(text=word, timestamp=(token_intervals[idx[0]][0], token_intervals[idx[-1]][1]))
            for word, idx in zip(words, token_indices)]


def word_chunks(decode, token_ids, token_times, timestamp_begin: int, eos_id: int, special_ids=(),
                time_precision: float = TIME_PRECISION, segment_size: int = 1500):
    """One recording's ids (text and timestamp tokens in order) with a time per id -> one chunk per word."""
    token_ids = [int(t) for t in token_ids]
    tt = [float(t) for t in token_times]
    if len(tt) != len(token_ids):
        raise ValueError(f"word_chunks: {len(tt)} token times for {len(token_ids)} tokens")
    special = set(int(t) for t in special_ids)
    tb = int(timestamp_begin)
    out = []
    chunk_start = None
    current_tokens, current_intervals = [], []
    cur_max_timestamp = prev_segments_len = penultimate_timestamp = 0.0
    for i, token in enumerate(token_ids):
        if token in special:
            continue
        if token >= tb:
            timestamp = float((token - tb) * time_precision)
            if timestamp < cur_max_timestamp:  # the next window's segment has started
                last_was_single_ending = i >= 2 and not (token_ids[i - 1] >= tb and token_ids[i - 2] >= tb)
                if last_was_single_ending:
                    prev_segments_len += time_precision * segment_size
                else:
                    cur_max_timestamp = penultimate_timestamp
                    prev_segments_len += penultimate_timestamp
            penultimate_timestamp = cur_max_timestamp
            cur_max_timestamp = timestamp
            time = round((token - tb) * time_precision + 0.0 + prev_segments_len, 2)
            if chunk_start is None:
                chunk_start = time
            elif time == chunk_start:
                pass
            else:
                out += collate_word_timestamps(decode, current_tokens, current_intervals, eos_id)
                chunk_start, current_tokens, current_intervals = None, [], []
        else:
            current_tokens.append(token)
            start = round(0.0, 2) if i == 0 else round(tt[i - 1] + 0.0, 2)
            current_intervals.append((start, round(tt[i] + 0.0, 2)))
    if current_tokens:
        out += collate_word_timestamps(decode, current_tokens, current_intervals, eos_id)
    return out


def cap_token_times(times, end_s: float) -> list[float]:
    """Token times of one recording, none later than its end (seconds)."""
    return [min(float(t), float(end_s)) for t in times]


def offline_decode(token_ids) -> str:
    """The rendering used without tokenizer.json: every token is the word " t<id>"."""
    return "".join(f" t{int(t)}" for t in token_ids)
