"""CTC forced alignment of known transcripts to their recordings: when was each word (or character) spoken.

`align` tokenises every text with the processor's tokenizer, runs the recordings through the wav2vec2 engine - whole, or
in overlapping chunks stitched by `longform.stitch_long` - and takes the single most probable CTC alignment of the
tokens to the logits on the GPU (`ca_ctc_align`, coral_amd/csrc/ctc_align.hip: Viterbi over the blank-interleaved
states).  The same kernel gives `evaluate.transcribe(..., timestamp_source="alignment")` its times, there for the ids a
decoder returned; here the caller brings the string, e.g. to locate a transcript's words or to screen a dataset for
samples whose text does not fit the audio (score -inf, or a low score per word).
"""

from __future__ import annotations

import math

import torch

from . import _lib
from .longform import char_offsets, stitch_long, timestamp_chunks, word_offsets

LEVELS = ("word", "char")
MAX_LABELS = _lib.CTC_ALIGN_MAX_LABELS


def tokenize(tokenizer, texts: list) -> list:
    """Texts -> id rows as the tokenizer encodes them (a character each, ' ' as the word delimiter), never truncated."""
    rows = [tokenizer.encode(t, truncation=False) for t in texts]
    for t, r in zip(texts, rows):
        if len(r) > MAX_LABELS:
            raise ValueError(f"a text of {len(r)} tokens cannot be aligned: the limit is {MAX_LABELS} tokens per "
                             f"recording (CA_CTC_ALIGN_MAX_LABELS); cut the recording and its text into segments first "
                             f"({t[:40]!r}...)")
    return rows


def word_groups(offsets: list, word_delimiter_char: str = " ") -> list:
    """Indices of the characters that make up each word of `longform.word_offsets(offsets)`, in its order."""
    groups, cur = [], []
    for i, o in enumerate(offsets):
        if o["char"] == word_delimiter_char:
            if cur:
                groups.append(cur)
            cur = []
        else:
            cur.append(i)
    if cur:
        groups.append(cur)
    return groups


def chunks_of(ids, start, end, tok_score, tokenizer, level: str, align_to: int, sampling_rate: int) -> list:
    """One aligned row -> [{"text", "timestamp": (start_s, end_s), "score"}], seconds by `longform.timestamp_chunks`'
    rule; a word's score is the mean of its characters' scores."""
    offs = char_offsets(ids, start, end, tokenizer)
    if level == "char":
        chunks = timestamp_chunks(offs, "char", align_to, sampling_rate)
        scores = [float(s) for s in tok_score]
    else:
        chunks = timestamp_chunks(word_offsets(offs), "word", align_to, sampling_rate)
        scores = [sum(float(tok_score[i]) for i in g) / len(g) for g in word_groups(offs)]
    assert len(chunks) == len(scores)
    return [dict(c, score=s) for c, s in zip(chunks, scores)]


def align(model, processor, arrays: list, texts: list, batch_size: int = 16, chunk_length_s: float = 0,
          stride_length_s=None, level: str = "word", sampling_rate=None) -> list:
    """Forced alignment of texts[i] to arrays[i] -> per recording {"text", "score", "chunks": [{"text", "timestamp":
    (start_s, end_s), "score"}]}, one chunk per word (level="word") or per character ("char", the word delimiter as " ").
    "score" is the log-probability of the alignment, a chunk's the mean log-probability of its characters' frames.
    chunk_length_s > 0 runs the recordings in overlapping chunks as `transcribe` does and aligns to the stitched logits.
    A recording whose text cannot be aligned (more tokens, counting a gap between equal neighbours, than frames) gets
    score = -inf and chunks = None; a text of more than CA_CTC_ALIGN_MAX_LABELS tokens raises.
    sampling_rate: the rate of `arrays`, one int or one per recording (None: the extractor's); recordings at another rate
    are resampled on the GPU first (coral_amd/resample.py)."""
    from .resample import to_rate
    from .wav2vec2 import Wav2Vec2CTCEngine

    eng = getattr(model, "engine", None)
    if not isinstance(eng, Wav2Vec2CTCEngine):
        raise ValueError("align is built for wav2vec2 (CTC) models only")
    if level not in LEVELS:
        raise ValueError(f"level must be 'word' or 'char', got {level!r}")
    if len(arrays) != len(texts):
        raise ValueError(f"{len(arrays)} recordings for {len(texts)} texts")
    if chunk_length_s is not None and chunk_length_s < 0:
        raise ValueError(f"chunk_length_s must be 0 (whole clips) or positive, got {chunk_length_s}")
    tok = processor.tokenizer
    ids = tokenize(tok, texts)
    if not arrays:
        return []
    sr = processor.feature_extractor.sampling_rate
    if sampling_rate is not None:
        arrays = to_rate(arrays, sampling_rate, sr, eng.device)
    align_to = int(math.prod(eng.s.conv_stride))
    model.eval()
    rows, scores = [], []
    if chunk_length_s:
        st = stitch_long(model, arrays, chunk_length_s, stride_length_s, batch_size, sr, want_logits=True)
        rows, scores = eng.align(ids, in_len=st["in_len"], logits=st["logits"])
    else:
        for i in range(0, len(arrays), batch_size):
            feats = [processor(a, sampling_rate=sr) for a in arrays[i:i + batch_size]]
            batch = processor.feature_extractor.pad(feats, padding="longest")
            with torch.no_grad():
                model(torch.from_numpy(batch["input_values"]), torch.from_numpy(batch["attention_mask"]))
            r, s = eng.align(ids[i:i + batch_size])  # every frame of the padded batch, as `transcribe` decodes them
            rows += r
            scores += s
    out = []
    for text, row_ids, (start, end, tok_score), score in zip(texts, ids, rows, scores):
        feasible = score > -math.inf
        out.append({"text": text, "score": float(score),
                    "chunks": chunks_of(row_ids, start, end, tok_score, tok, level, align_to, sr) if feasible else None})
    return out
