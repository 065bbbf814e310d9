"""Write tests/golden/whisper_word.npz from the installed transformers (CPU only).

The fixture model and audio are those of tests/whisper_ts_ref.py, the alignment heads and the clips' valid frames those
of tests/whisper_word_ref.py.  Recorded:

  * `short_ids`, `short_times`: `WhisperForConditionalGeneration.generate(..., attention_mask, return_timestamps=True,
    return_token_timestamps=True)` on the three short clips - the id rows `_extract_token_timestamps` was given and the
    token_timestamps it returned; `short_cost{b}` / `short_path{b}`: the fp32 matrix transformers fed
    `_dynamic_time_warping` for clip b and the path it returned;
  * `long_*`: one long recording through the sequential loop: per window (seek, id row, token_timestamps row), and the
    final segments' ids and token_timestamps;
  * `dtw_{name}`: the paths `_dynamic_time_warping` returns for the seeded matrices of whisper_word_ref.DTW_CASES;
  * `words`, `asr`: `_combine_tokens_into_words` and `_decode_asr(return_timestamps="word")` over the stand-in tokenizer.

Asserted before anything is written: the restatements (tests/whisper_word_ref.py, coral_amd/whisper_align.py,
coral_amd/longform_whisper.py) reproduce every recorded path, time, segment and word chunk exactly; the restated cost
from transformers' own cross-attention weights equals the matrix transformers fed its DTW bit for bit; the quantised
matrices take every branch of the DTW rule.

usage: python tools/gen_whisper_word_goldens.py"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import whisper_ts_ref as R  # noqa: E402
import whisper_word_ref as W  # noqa: E402
from coral_amd import whisper_align as A  # noqa: E402
from coral_amd.longform_whisper import run_longform  # noqa: E402
from gen_whisper_ts_goldens import hf_model  # noqa: E402


class StandInTokenizer:
    """What `_combine_tokens_into_words` and `_decode_asr` ask of a tokenizer, over whisper_word_ref.WORD_TABLE."""
    language = "danish"
    eos_token_id = W.WORD_EOS
    all_special_ids = [W.WORD_EOS, 41, 42]

    def decode(self, tokens, decode_with_timestamps=False, **_):
        return W.word_decode([int(t) for t in tokens])

    def convert_tokens_to_ids(self, tok):
        return {"<|notimestamps|>": W.WORD_TIMESTAMP_BEGIN - 1, "<|startofprev|>": 42, "<|startoftranscript|>": 41}[tok]

    def _strip_prompt(self, token_ids, prompt_token_id, decoder_start_token_id):
        return token_ids


def main():
    import transformers.models.whisper.generation_whisper as G
    from transformers.models.whisper import tokenization_whisper as T

    torch.manual_seed(0)
    model = hf_model()
    model.generation_config.alignment_heads = [list(h) for h in W.ALIGNMENT_HEADS]
    assert model.config.median_filter_width == W.FILTER_WIDTH
    P = len(R.PREFIX)
    out = dict(recipe=np.array(json.dumps(R.RECIPE)), alignment_heads=np.array(json.dumps([list(h) for h in W.ALIGNMENT_HEADS])))

    dtw_calls, ext_calls, seeks = [], [], []
    real_dtw, real_ext, real_fb = G._dynamic_time_warping, model._extract_token_timestamps, model.generate_with_fallback

    def spy_dtw(matrix):
        res = real_dtw(matrix)
        dtw_calls.append((np.array(matrix), np.array(res[0]), np.array(res[1])))
        return res

    def spy_ext(generate_outputs, alignment_heads, time_precision=0.02, num_frames=None, num_input_ids=None):
        res = real_ext(generate_outputs, alignment_heads, time_precision=time_precision, num_frames=num_frames,
                       num_input_ids=num_input_ids)
        ca = [torch.cat([x[i] for x in generate_outputs.cross_attentions], dim=2) for i in range(model.config.decoder_layers)]
        wts = torch.stack([ca[l][:, h] for l, h in alignment_heads]).permute(1, 0, 2, 3)[:, :, num_input_ids:]
        ext_calls.append(dict(ids=generate_outputs.sequences.clone(), times=res.clone(), weights=wts.clone(),
                              num_frames=None if num_frames is None else [int(n) for n in num_frames], P=num_input_ids))
        return res

    def spy_fb(*a, **kw):
        seeks.append([int(s) for s in kw["seek"]])
        return real_fb(*a, **kw)

    G._dynamic_time_warping = spy_dtw
    model._extract_token_timestamps = spy_ext
    model.generate_with_fallback = spy_fb

    # ---- the three short clips, each with its own number of valid frames ----
    feats = R.short_features()
    mask = torch.zeros(len(feats), 3000, dtype=torch.long)
    for b, n in enumerate(W.SHORT_NUM_FRAMES):
        mask[b, :n] = 1
    with torch.no_grad():
        model.generate(feats, attention_mask=mask, return_timestamps=True, return_token_timestamps=True, language="danish",
                       task="transcribe")
    # (with an attention mask transformers keeps seeking inside a clip until its valid frames are used up: the FIRST round
    # is the batch of three whole windows, what `WhisperEngine.generate` is held against; later rounds are not recorded)
    call = ext_calls[0]
    assert call["ids"].shape[0] == len(feats) and len(dtw_calls) >= len(feats), (call["ids"].shape, len(dtw_calls))
    del dtw_calls[len(feats):]
    ext_calls.clear()
    assert call["P"] == P and call["num_frames"] == W.SHORT_NUM_FRAMES, (call["P"], call["num_frames"])
    ids, times = call["ids"].numpy(), call["times"].numpy()
    assert times.dtype == np.float32
    prev = np.load(R.GOLDEN)["short_ids"]
    print("short ids equal to whisper_ts.npz's:", ids.shape == prev.shape and bool((ids == prev).all()))
    out["short_ids"], out["short_times"] = ids.astype(np.int64), times
    out["short_num_frames"] = np.array(W.SHORT_NUM_FRAMES, dtype=np.int64)
    Ltot = ids.shape[1]
    frames = W.frames_of(W.SHORT_NUM_FRAMES, len(feats))
    for b, (m, text, time) in enumerate(dtw_calls):
        assert m.shape == (Ltot - 1 - P, frames[b]) and m.dtype == np.float64
        m32 = m.astype(np.float32)
        assert (m32.astype(np.float64) == m).all()
        mine = W.cost_from_weights(call["weights"][b], frames[b])
        assert np.array_equal(mine.numpy(), m32), "the restated cost differs from the matrix transformers fed its DTW"
        t2, j2 = W.dtw(m32)
        assert np.array_equal(t2, text) and np.array_equal(j2, time), b
        row = W.token_times(W.jump_frames(text, time), P, Ltot)
        assert np.array_equal(row, times[b]), (b, row, times[b])
        assert np.array_equal(A.times_from_jumps(W.jump_frames(text, time)[None], P, Ltot)[0], times[b])
        out[f"short_cost{b}"] = m32
        out[f"short_path{b}"] = np.stack([text, time]).astype(np.int16)
        print(f"short {b}: Lw {m.shape[0]}, F {m.shape[1]}, times {times[b][P:P + 6]} ..")
    dtw_calls.clear()

    # ---- one long recording ----
    mel = R.long_features()[0]
    seeks.clear()
    with torch.no_grad():
        res = model.generate(mel[None], attention_mask=torch.ones(1, mel.shape[1], dtype=torch.long), return_timestamps=True,
                             return_token_timestamps=True, return_segments=True, language="danish", task="transcribe")
    assert len(seeks) == len(ext_calls) and all(len(s) == 1 for s in seeks)
    segs = res["segments"][0]
    table = {}
    for (seek,), c in zip(seeks, ext_calls):
        assert c["num_frames"] == [mel.shape[1] - seek], (c["num_frames"], mel.shape[1], seek)
        table[seek] = (c["ids"][0].tolist(), c["times"][0].numpy())
    mine = run_longform(lambda batch: ([table[s][0] for _, s in batch], [table[s][1] for _, s in batch]), [mel.shape[1]],
                        R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS, return_token_timestamps=True)[0]
    assert [w[0] for w in mine["windows"]] == [s for (s,) in seeks]
    assert len(mine["segments"]) == len(segs)
    for got, want in zip(mine["segments"], segs):
        assert got[2] == [int(t) for t in want["tokens"]]
        wt = want["token_timestamps"].numpy()
        assert wt.dtype == np.float32 and np.array_equal(got[3], wt), (got[3], wt)
        assert got[0] == float(want["start"]) and got[1] == float(want["end"])
    Lr = max(len(r) for r, _ in table.values())
    order = [s for (s,) in seeks]
    out["long_frames"] = np.array(mel.shape[1])
    out["long_seek"] = np.array(order, dtype=np.int64)
    out["long_len"] = np.array([len(table[s][0]) for s in order], dtype=np.int64)
    out["long_ids"] = np.array([table[s][0] + [-1] * (Lr - len(table[s][0])) for s in order], dtype=np.int64)
    out["long_times"] = np.array([np.pad(table[s][1], (0, Lr - len(table[s][1]))) for s in order], dtype=np.float32)
    Ls = max(len(s["tokens"]) for s in segs)
    out["long_seg_len"] = np.array([len(s["tokens"]) for s in segs], dtype=np.int64)
    out["long_seg_ids"] = np.array([[int(t) for t in s["tokens"]] + [-1] * (Ls - len(s["tokens"])) for s in segs], dtype=np.int64)
    out["long_seg_times"] = np.array([np.pad(s["token_timestamps"].numpy(), (0, Ls - len(s["tokens"]))) for s in segs],
                                     dtype=np.float32)
    print(f"long: {mel.shape[1]} frames, seeks {order}, {len(segs)} segments")
    G._dynamic_time_warping = real_dtw

    # ---- synthetic DTW cases ----
    branches = {}
    for name in W.DTW_CASES:
        m = W.dtw_case(name)
        text, time = real_dtw(m.astype(np.float64))
        t2, j2 = W.dtw(m)
        assert np.array_equal(t2, text) and np.array_equal(j2, time), name
        out[f"dtw_{name}"] = np.stack([text, time]).astype(np.int16)
        if W.DTW_CASES[name][3]:
            branches[name] = W.dtw_branches(m)
            assert name != "ties" or all(v > 0 for v in branches[name].values()), (name, branches[name])
    nan = np.full((1, 6), np.nan)
    text, time = real_dtw(nan)
    assert np.array_equal(W.dtw(nan)[0], text) and np.array_equal(W.dtw(nan)[1], time)
    assert (W.jump_frames(text, time) == 0).all()
    out["dtw_nan"] = np.stack([text, time]).astype(np.int16)
    out["dtw_branches"] = np.array(json.dumps(branches))
    print("tie branches:", branches)

    # ---- words ----
    tok = StandInTokenizer()
    words = []
    for case in W.WORD_CASES:
        w, wt, wi = T._combine_tokens_into_words(tok, list(case), "danish")
        assert (w, wt, wi) == tuple(A.combine_tokens_into_words(W.word_decode, case, W.WORD_EOS)), case
        words.append(dict(words=w, tokens=wt, indices=wi))
    asr = []
    for ids_, tt in W.ASR_CASES:
        text, opt = T._decode_asr(tok, [dict(tokens=np.array([ids_]), token_timestamps=np.array([tt]))],
                                  return_timestamps="word", return_language=False, time_precision=0.02)
        chunks = [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in opt["chunks"]]
        got = A.word_chunks(W.word_decode, ids_, tt, W.WORD_TIMESTAMP_BEGIN, W.WORD_EOS, special_ids=tok.all_special_ids)
        assert [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in got] == chunks, (got, chunks)
        asr.append(dict(text=text, chunks=chunks))
    out["words"], out["asr"] = np.array(json.dumps(words)), np.array(json.dumps(asr))
    np.savez_compressed(W.GOLDEN, **out)
    print(W.GOLDEN.name, W.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
