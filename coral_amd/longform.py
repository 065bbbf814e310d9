"""Long recordings through wav2vec2: overlapping chunks, stitched frames, character / word timestamps.

The reference transcribes through `transformers.pipeline("automatic-speech-recognition")`, whose CTC branch offers
`chunk_length_s` / `stride_length_s` and `return_timestamps="char" | "word"`
($TF/pipelines/automatic_speech_recognition.py: preprocess + chunk_iter, rescale_stride, _forward, postprocess;
$TF/models/wav2vec2/tokenization_wav2vec2.py: _compute_offsets, _get_word_offsets).  This module restates that
arithmetic on the host (`chunk_plan`, `frame_segments`, `word_offsets`) and runs the data path on the GPU: per batch of
chunks `ca_pcm_prepare` (each chunk's own zero-mean / unit-variance, read in place from the recording with row
stride = step), the engine forward with the attention mask, `ca_ctc_stitch` (argmax of the kept frames into one row per
recording); then `ca_ctc_collapse_offsets` over the finished rows and one device-to-host copy.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

W2V2_CONV_KERNEL, W2V2_CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
TIMESTAMP_MODES = (None, "char", "word")
TIMESTAMP_SOURCES = ("emission", "alignment")


def conv_frames(n: int, kernels=W2V2_CONV_KERNEL, strides=W2V2_CONV_STRIDE) -> int:
    """Frames the conv stack yields for n samples (floor((n - k) / s) + 1 per layer; <= 0: too short for one frame)."""
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1
    return n


def chunk_plan(n_samples: int, chunk_length_s: float, stride_length_s=None, sampling_rate: int = 16_000,
               align_to: int = 320) -> dict:
    """The pipeline's chunking of a recording of n_samples samples (preprocess + chunk_iter).
    -> {"chunk_len", "stride_left", "stride_right", "step", "chunks": [(start, n, left, right), ...]} in samples.
    stride_length_s: None = chunk_length_s / 6, a number = both sides, a pair = (left, right).  The first chunk has no
    left stride, the last (the first one that reaches the end of the recording) no right stride; a chunk that is not
    longer than its left stride is dropped."""
    if not chunk_length_s or chunk_length_s <= 0:
        raise ValueError(f"chunk_length_s must be positive, got {chunk_length_s}")
    if stride_length_s is None:
        stride_length_s = chunk_length_s / 6
    if isinstance(stride_length_s, (int, float)):
        stride_length_s = [stride_length_s, stride_length_s]
    chunk_len = int(round(chunk_length_s * sampling_rate / align_to) * align_to)
    left = int(round(stride_length_s[0] * sampling_rate / align_to) * align_to)
    right = int(round(stride_length_s[1] * sampling_rate / align_to) * align_to)
    step = chunk_len - left - right
    if step <= 0:
        raise ValueError(f"chunk_length_s={chunk_length_s} ({chunk_len} samples) must be longer than stride_length_s "
                         f"(left {left} + right {right} samples)")
    chunks = []
    for start in range(0, int(n_samples), step):
        end = start + chunk_len
        n = min(end, n_samples) - start
        is_last = end >= n_samples
        lft = 0 if start == 0 else left
        rgt = 0 if is_last else right
        if n > lft:
            chunks.append((start, n, lft, rgt))
        if is_last:
            break
    return dict(chunk_len=chunk_len, stride_left=left, stride_right=right, step=step, chunks=chunks)


def rescale_stride(n: int, left: int, right: int, align_to: int = 320) -> tuple:
    """(samples, left, right) -> (token_n, l, r) in frames, as the pipeline's `rescale_stride` with ratio 1 / align_to.
    token_n is round(n / align_to), not the conv stack's frame count."""
    token_n = int(round(n * (1 / align_to)))
    return token_n, int(round(left / n * token_n)), int(round(right / n * token_n))


def frame_segments(plan: dict, T_chunk: int, align_to: int = 320, row: int = 0, frames_of=conv_frames):
    """The `seg` rows of ca_ctc_stitch for one recording's chunks -> ([(row, frame offset, first kept frame, kept frames),
    ...], stitched length).  Kept frames of a chunk: [l, min(T_b, token_n - r)) with (token_n, l, r) = rescale_stride and
    T_b = min(T_chunk, frames_of(n)), the chunk's own frame count inside a logits buffer of T_chunk frames - the clipping
    NumPy's `items[:, l:token_n - r]` does.  A chunk too short for one frame keeps nothing."""
    seg, off = [], 0
    for _, n, left, right in plan["chunks"]:
        token_n, l, r = rescale_stride(n, left, right, align_to)
        T_b = max(0, min(int(T_chunk), frames_of(n)))
        keep = max(0, min(T_b, token_n - r) - l)
        seg.append((row, off, l, keep))
        off += keep
    return seg, off


def char_offsets(ids, start, end, tokenizer) -> list[dict]:
    """Collapsed ids with their frame offsets -> [{"char", "start_offset", "end_offset"}], the word delimiter as " "
    (what `decode(output_char_offsets=True)` yields)."""
    delim = tokenizer.word_delimiter_token
    out = []
    for i, s, e in zip(ids, start, end):
        tok = tokenizer.inv.get(int(i), tokenizer.unk_token)
        out.append({"char": " " if tok == delim else tok, "start_offset": int(s), "end_offset": int(e)})
    return out


def word_offsets(offsets: list[dict], word_delimiter_char: str = " ") -> list[dict]:
    """`Wav2Vec2CTCTokenizer._get_word_offsets`: runs of non-delimiter characters -> {"word", "start_offset",
    "end_offset"} (first character's start, last character's end)."""
    words, last_state, word, start, end = [], "SPACE", "", 0, 0
    for o in offsets:
        state = "SPACE" if o["char"] == word_delimiter_char else "WORD"
        if state == last_state:
            end = o["end_offset"]
            word += o["char"]
        elif state == "SPACE":
            words.append({"word": word, "start_offset": start, "end_offset": end})
        else:
            start, end, word = o["start_offset"], o["end_offset"], o["char"]
        last_state = state
    if last_state == "WORD":
        words.append({"word": word, "start_offset": start, "end_offset": end})
    return words


def timestamp_chunks(offsets: list[dict], key: str, align_to: int, sampling_rate: int) -> list[dict]:
    """Frame offsets -> the pipeline's `chunks`: seconds = offset * align_to / sampling_rate."""
    return [{"text": o[key], "timestamp": (o["start_offset"] * align_to / sampling_rate,
                                           o["end_offset"] * align_to / sampling_rate)} for o in offsets]


def check_timestamp_mode(return_timestamps, with_lm: bool, timestamp_source: str = "emission") -> None:
    if return_timestamps not in TIMESTAMP_MODES:
        raise ValueError(f"return_timestamps must be None, 'char' or 'word', got {return_timestamps!r}")
    if timestamp_source not in TIMESTAMP_SOURCES:
        raise ValueError(f"timestamp_source must be 'emission' or 'alignment', got {timestamp_source!r}")
    if return_timestamps is not None and with_lm and timestamp_source == "emission":
        raise ValueError("return_timestamps is not available with LM decoding (the beam search records no emission "
                         "frames): load the processor with no_lm, drop return_timestamps, or pass "
                         "timestamp_source=\"alignment\" (the forced alignment of the returned string)")


def align_rows(eng, ids: list, logits=None, in_len=None) -> list:
    """Decoded id rows -> (ids, start, end) per row with the frames of their CTC forced alignment to the same logits
    (`Wav2Vec2CTCEngine.align`): what `decode_rows` takes, whichever decoder produced the ids."""
    rows, _ = eng.align(ids, in_len=in_len, logits=logits)
    return [(list(r), start, end) for r, (start, end, _) in zip(ids, rows)]


def collapse_rows(raw: torch.Tensor, in_len, blank: int):
    """ca_ctc_collapse_offsets over raw int32 [R, T] on the device -> per row (ids, start, end) as host lists, through one
    device-to-host copy."""
    R, T = raw.shape
    dev = raw.device
    out = torch.empty(3 * R * T + R, dtype=torch.int32, device=dev)
    ids, start, end = (out[k * R * T:(k + 1) * R * T].view(R, T) for k in range(3))
    olen = out[3 * R * T:]
    ws = torch.empty(max(1, ops.ctc_collapse_workspace_bytes(R, T)), dtype=torch.uint8, device=dev)
    ops.ctc_collapse_offsets(raw, in_len, ids, start, end, olen, ws, R, T, blank)
    host = out.cpu().numpy()
    n = host[3 * R * T:]
    h = host[:3 * R * T].reshape(3, R, T)
    return [tuple(h[k, r, :int(n[r])].tolist() for k in range(3)) for r in range(R)]


def decode_rows(rows, tokenizer, return_timestamps, align_to: int, sampling_rate: int) -> list[dict]:
    """(ids, start, end) per recording -> [{"text"} (+ "chunks")]."""
    out = []
    for ids, start, end in rows:
        item = {"text": tokenizer.decode(ids, group_tokens=False)}
        if return_timestamps is not None:
            offs = char_offsets(ids, start, end, tokenizer)
            if return_timestamps == "word":
                offs = word_offsets(offs)
            item["chunks"] = timestamp_chunks(offs, return_timestamps, align_to, sampling_rate)
        out.append(item)
    return out


def stitch_long(model, arrays: list, chunk_length_s: float, stride_length_s=None, batch_size: int = 16,
                sampling_rate: int = 16_000, want_logits: bool = False, on_batch=None) -> dict:
    """The GPU half of `transcribe_long`: every recording's chunks through the engine, kept frames stitched.
    -> {"raw": int32 [R, Tout] device, "logits": fp32 [R, Tout, Vp] device or None, "lengths": host list of stitched
    lengths, "in_len": int32 [R] device, "plans", "segs"}.  Chunks of all recordings form one queue cut into batches of
    batch_size.  on_batch(first chunk of the batch, chunk logits buffer [B, T, Vp], seg rows): a test hook called after
    each forward."""
    eng = model.engine
    s, dev = eng.s, eng.device
    align_to = int(math.prod(s.conv_stride))
    model.eval()
    plans = [chunk_plan(len(a), chunk_length_s, stride_length_s, sampling_rate, align_to) for a in arrays]
    R = len(arrays)
    frames_of = lambda n: conv_frames(n, s.conv_kernel, s.conv_stride)  # noqa: E731
    queue = [(r, i) for r, p in enumerate(plans) for i in range(len(p["chunks"]))]
    # every batch is padded to the longest chunk of the call: one workspace for all full batches
    N = max((c[1] for p in plans for c in p["chunks"]), default=0)
    T_chunk = frames_of(N) if N else 0
    segs, lengths = [], []
    for r, p in enumerate(plans):
        sg, total = frame_segments(p, T_chunk, align_to, row=r, frames_of=frames_of)
        segs.append(sg)
        lengths.append(total)
    Tout = max(lengths + [1])
    V, Vp = s.vocab_size, (s.vocab_size + 7) // 8 * 8
    raw = torch.full((R, Tout), s.pad_token_id, dtype=torch.int32, device=dev)
    logits = torch.zeros(R, Tout, Vp, dtype=torch.float32, device=dev) if want_logits else None
    in_len = torch.tensor(lengths, dtype=torch.int32).to(dev)
    res = dict(raw=raw, logits=logits, lengths=lengths, in_len=in_len, plans=plans, segs=segs, align_to=align_to)
    if not queue or T_chunk < 1:
        return res
    seg_dev = torch.tensor([segs[r][i] for r, i in queue], dtype=torch.int32).to(dev)
    len_dev = torch.tensor([plans[r]["chunks"][i][1] for r, i in queue], dtype=torch.int32).to(dev)
    pcm = {}
    for c0 in range(0, len(queue), batch_size):
        batch = queue[c0:c0 + batch_size]
        B = len(batch)
        y = torch.empty(B, N, dtype=torch.float32, device=dev)
        mask = torch.empty(B, N, dtype=torch.int32, device=dev)
        k = 0
        while k < B:  # one ca_pcm_prepare per (recording, batch) run of consecutive chunks
            r, i0 = batch[k]
            m = k
            while m < B and batch[m][0] == r:
                m += 1
            if r not in pcm:
                pcm = {r: torch.from_numpy(np.ascontiguousarray(arrays[r], dtype=np.float32)).to(dev)}
            step = plans[r]["step"]
            ops.pcm_prepare(pcm[r][i0 * step:], len_dev[c0 + k:c0 + m], y[k:m], mask[k:m], m - k, N, step)
            k = m
        with torch.no_grad():
            eng(y, mask)
        w = eng._saved["w"]
        assert w["T"] == T_chunk and w["Vp"] == Vp
        ops.ctc_stitch(w["logits"], seg_dev[c0:c0 + B], raw, logits, B, T_chunk, V, Vp, R, Tout)
        if on_batch is not None:
            on_batch(c0, w["logits"].view(B, T_chunk, Vp), [segs[r][i] for r, i in batch])
    return res


def transcribe_long(model, processor, arrays: list, chunk_length_s: float, stride_length_s=None, batch_size: int = 16,
                    return_timestamps=None, timestamp_source: str = "emission", n_best=None, hotwords=None,
                    hotword_weight: float = 10.0) -> list[dict]:
    """Chunked wav2vec2 transcription with the pipeline's semantics -> [{"text": str}] plus, with
    return_timestamps="char" | "word", "chunks": [{"text", "timestamp": (start_s, stop_s)}] per recording.
    With a `Wav2Vec2ProcessorWithLM` the stitched logits go to the LM-fused beam search (no emission frames there).
    timestamp_source="alignment": the times are those of the CTC forced alignment of the decoded ids (greedy or beam) to
    the stitched logits (`ca_ctc_align`), which serves both decoders.  n_best / hotwords / hotword_weight: as in
    `evaluate.transcribe` (LM decoding only); with n_best every result carries "n_best"."""
    from .nbest import check_nbest_arguments, lm_decode, nbest_records
    from .wav2vec2 import Wav2Vec2CTCEngine

    if not isinstance(getattr(model, "engine", None), Wav2Vec2CTCEngine):
        raise ValueError("chunk_length_s > 0 is built for wav2vec2 (CTC) models only: Whisper long-form decoding is not")
    with_lm = getattr(processor, "lm", None) is not None
    check_timestamp_mode(return_timestamps, with_lm, timestamp_source)
    check_nbest_arguments(processor, n_best, hotwords, hotword_weight)
    if not arrays:
        return []
    eng = model.engine
    sr = processor.feature_extractor.sampling_rate
    aligned = return_timestamps is not None and timestamp_source == "alignment"
    st = stitch_long(model, arrays, chunk_length_s, stride_length_s, batch_size, sr, want_logits=with_lm or aligned)
    if with_lm:
        ids, hyps = lm_decode(eng, processor, n_best, hotwords, hotword_weight, in_len=st["in_len"], logits=st["logits"])
        if not aligned:
            res = [{"text": processor.tokenizer.decode(r, group_tokens=False)} for r in ids]
        else:
            res = decode_rows(align_rows(eng, ids, st["logits"], st["in_len"]), processor.tokenizer, return_timestamps,
                              st["align_to"], sr)
        for item, h in zip(res, hyps or []):
            item["n_best"] = nbest_records(h, processor.tokenizer)
        return res
    else:
        rows = collapse_rows(st["raw"], st["in_len"], eng.s.pad_token_id)
        if aligned:
            rows = align_rows(eng, [r[0] for r in rows], st["logits"], st["in_len"])
    return decode_rows(rows, processor.tokenizer, return_timestamps, st["align_to"], sr)
