"""Write tests/golden/whisper_ts.npz from the installed transformers (CPU only).

The fixture model, its recipe and its audio are those of tests/whisper_ts_ref.py.  Recorded:

  * `short_ids`: greedy ids of the three short clips under [begin-suppress, WhisperTimeStampLogitsProcessor], forced
    prefix <|sot|><|da|><|transcribe|> (`GenerationMixin.generate` with the processors `_retrieve_logit_processors`
    builds, as tools/gen_goldens.py records the beam fixtures);
  * per long recording: `WhisperForConditionalGeneration.generate(whole-recording features, return_timestamps=True,
    return_segments=True)` - every window's (seek, ids) as `generate_with_fallback` returned them, and the final
    segments (start, end as float64, ids);
  * `proc_*`: random (history, scores) cases with the -inf pattern of the processor's output.

Asserted before anything is written: the restated rules (tests/whisper_ts_ref.py) reproduce every recorded id from
the model's teacher-forced logits; every branch of the rules is taken at least once; `run_longform` replaying the
recorded windows reproduces seeks and segments; the oracle's whole-recording log-mel equals WhisperFeatureExtractor's
with truncation=False.

usage: python tools/gen_whisper_ts_goldens.py"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import whisper_ts_ref as R  # noqa: E402
from coral_amd.longform_whisper import run_longform  # noqa: E402


def hf_model():
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    kw = dict(R.CONFIG)
    hc = WhisperConfig(**kw, max_source_positions=1500, bos_token_id=kw["pad_token_id"], dropout=0.0, attention_dropout=0.0,
                       activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0, apply_spec_augment=False,
                       attn_implementation="eager", suppress_tokens=None, begin_suppress_tokens=None)
    model = WhisperForConditionalGeneration(hc)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in R.fixture_params().items():
            sd[k].copy_(v)
    model.eval()
    gc = model.generation_config
    gc.forced_decoder_ids = None
    gc.suppress_tokens = None
    gc.begin_suppress_tokens = list(R.BEGIN_SUPPRESS)
    gc.no_timestamps_token_id = R.NO_TIMESTAMPS
    gc.max_initial_timestamp_index = R.MAX_INITIAL_TIMESTAMP_INDEX
    gc.is_multilingual = True
    gc.lang_to_id = {"<|da|>": R.LANG}
    gc.task_to_id = {"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE}
    gc.max_length = R.MAX_LENGTH
    gc.pad_token_id, gc.eos_token_id, gc.decoder_start_token_id = R.EOS, R.EOS, R.SOT
    gc.bos_token_id = R.EOS
    return model


def replay_rules(model, feats, rows, counts):
    """Teacher-forced logits of the recorded rows -> the restated rules must pick every recorded token; counts the
    branches (with the scores at hand: the log-prob rule really forced the timestamp, the monotonic mask really removed
    the best one, the cap really cut)."""
    tb, P = R.TIMESTAMP_BEGIN, len(R.PREFIX)
    for b, row in enumerate(rows):
        row = [int(t) for t in row]
        with torch.no_grad():
            lg = model(input_features=feats[b:b + 1], decoder_input_ids=torch.tensor([row[:-1]])).logits[0].numpy()
        for t in range(P, len(row)):
            hist = row[P:t]
            if hist and hist[-1] == R.EOS:
                break
            x = lg[t - 1].astype(np.float64)
            if t == P:
                x[R.BEGIN_SUPPRESS] = -np.inf
            y, info = R.timestamp_rules(x, hist, tb, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX, detail=True)
            got = R.pick(y)
            assert got == row[t], (b, t, got, row[t], info["lse"], info["text_max"])
            raw_ts = tb + int(np.argmax(x[tb:]))
            if not hist and raw_ts > tb + R.MAX_INITIAL_TIMESTAMP_INDEX:
                counts["initial_cap"] += 1
            if hist and got >= tb and hist[-1] < tb and info["forced"] and x[:tb - 1].max() > x[got]:
                counts["timestamp_by_logprob"] += 1
            if hist and got < tb and got != R.EOS and hist[-1] < tb:
                counts["text_while_open"] += 1
            if hist and got >= tb and hist[-1] >= tb:
                counts["pair_closed"] += 1
            if len(hist) >= 2 and hist[-1] >= tb and hist[-2] >= tb and got < tb:
                counts["text_after_pair"] += 1
            if hist and got >= tb and raw_ts != got and not np.isfinite(info["before"][raw_ts]):
                counts["monotonic_mask"] += 1
            if len(hist) >= 2 and hist[-1] >= tb and hist[-2] < tb and got == R.EOS:
                counts["eos_after_single"] += 1


def main():
    from transformers import WhisperFeatureExtractor
    from transformers.generation import GenerationMixin
    from transformers.generation.logits_process import (LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)

    torch.manual_seed(0)
    model = hf_model()
    gc = model.generation_config
    out = dict(recipe=np.array(json.dumps(R.RECIPE)))
    counts = {k: 0 for k in R.BRANCHES}
    P = len(R.PREFIX)

    # ---- short form ----
    feats = R.short_features()
    procs = LogitsProcessorList([SuppressTokensAtBeginLogitsProcessor(R.BEGIN_SUPPRESS, begin_index=P),
                                 WhisperTimeStampLogitsProcessor(gc, begin_index=P)])
    with torch.no_grad():
        ids = GenerationMixin.generate(model, input_features=feats, decoder_input_ids=torch.tensor([R.PREFIX] * len(feats)),
                                       do_sample=False, num_beams=1, max_length=R.MAX_LENGTH, logits_processor=procs,
                                       use_cache=True, begin_suppress_tokens=None, suppress_tokens=None)
    out["short_ids"] = ids.numpy()
    replay_rules(model, feats, ids.tolist(), counts)
    for r in ids.tolist():
        print("short", r)

    # ---- long form ----
    fe = WhisperFeatureExtractor(feature_size=80)
    for n, (wave, mel) in enumerate(zip(R.long_waves(), R.long_features())):
        hf_mel = fe(wave, sampling_rate=R.SAMPLING_RATE, truncation=False, padding="longest", return_tensors="pt").input_features[0]
        assert hf_mel.shape == mel.shape and float((hf_mel - mel).abs().max()) <= 1e-4, (hf_mel.shape, mel.shape)
        windows = []
        inner = model.generate_with_fallback

        def spy(*a, **kw):
            res = inner(*a, **kw)
            windows.append((int(kw["seek"][0]), [int(t) for t in res[0][0]]))
            return res

        model.generate_with_fallback = spy
        try:
            with torch.no_grad():
                res = model.generate(mel[None], return_timestamps=True, return_segments=True, language="danish",
                                     task="transcribe")
        finally:
            del model.generate_with_fallback
        segs = res["segments"][0]
        starts = np.array([float(s["start"]) for s in segs], dtype=np.float64)
        ends = np.array([float(s["end"]) for s in segs], dtype=np.float64)
        toks = [[int(t) for t in s["tokens"]] for s in segs]
        # the restated loop, replaying the recorded windows
        table = {seek: R.PREFIX + gen + [R.EOS] for seek, gen in windows}
        mine = run_longform(lambda batch: [table[seek] for _, seek in batch], [mel.shape[1]], R.TIMESTAMP_BEGIN, P, R.EOS,
                            R.EOS)[0]
        assert [w[0] for w in mine["windows"]] == [w[0] for w in windows], (mine["windows"], windows)
        assert [s[2] for s in mine["segments"]] == toks
        assert [s[0] for s in mine["segments"]] == starts.tolist() and [s[1] for s in mine["segments"]] == ends.tolist()
        for seek, gen in windows:
            replay_rules(model, R.window_features(mel, seek)[None], [R.PREFIX + gen], counts)
        L = max(len(g) for _, g in windows)
        out[f"long{n}_seek"] = np.array([s for s, _ in windows], dtype=np.int64)
        out[f"long{n}_len"] = np.array([len(g) for _, g in windows], dtype=np.int64)
        out[f"long{n}_ids"] = np.array([g + [-1] * (L - len(g)) for _, g in windows], dtype=np.int64)
        out[f"long{n}_seg_start"], out[f"long{n}_seg_end"] = starts, ends
        Ls = max(len(t) for t in toks)
        out[f"long{n}_seg_len"] = np.array([len(t) for t in toks], dtype=np.int64)
        out[f"long{n}_seg_ids"] = np.array([t + [-1] * (Ls - len(t)) for t in toks], dtype=np.int64)
        out[f"long{n}_frames"] = np.array(mel.shape[1])
        print(f"long{n}: {mel.shape[1]} frames, seeks {[s for s, _ in windows]}, {len(segs)} segments, "
              f"{starts[0]:.2f} .. {ends[-1]:.2f} s")

    print("branches:", counts)
    assert all(counts[k] > 0 for k in R.BRANCHES), counts
    out["branch_counts"] = np.array([counts[k] for k in R.BRANCHES], dtype=np.int64)

    # ---- the processor itself on random cases ----
    V, tb = R.CONFIG["vocab_size"], R.TIMESTAMP_BEGIN
    rng = np.random.RandomState(5)
    hists = [[], [tb + 3], [tb + 3, 7], [tb + 3, 7, 9], [tb + 3, 7, tb + 40], [tb + 3, 7, tb + 40, tb + 40],
             [tb + 3, 7, tb + 40, tb + 40, 12], [tb, 5, tb + 1499], [tb, 5, tb + 1500], [tb, 5, tb + 1500, tb + 1500],
             [tb + 2, 7, tb + 1400, tb + 1400, 9, tb + 1500], [5, 6], [7], [tb + 10, tb + 10]]
    for _ in range(26):
        n = int(rng.randint(1, 30))
        h, t = [], 0
        for _ in range(n):
            if rng.rand() < 0.4:
                t = min(1500, t + int(rng.randint(0, 200)))
                h.append(tb + t)
            else:
                h.append(int(rng.randint(0, R.NO_TIMESTAMPS)))
        hists.append(h)
    n = len(hists)
    Lh = max(len(h) for h in hists)
    out["proc_V"] = np.array(V)
    out["proc_seed"] = np.arange(1000, 1000 + n)
    # the step of the score grid decides the side the log-prob rule falls on: wide = the best text token wins
    out["proc_step"] = np.array([(2e-4, 3e-3, 2e-2)[i % 3] for i in range(n)], dtype=np.float32)
    out["proc_cap"] = np.array([(-1, 50)[i % 2] for i in range(n)], dtype=np.int64)
    out["proc_hist_len"] = np.array([len(h) for h in hists], dtype=np.int64)
    out["proc_hist"] = np.array([h + [-1] * (Lh - len(h)) for h in hists], dtype=np.int64)
    masks = []
    for i, h in enumerate(hists):
        probe = dict(proc_V=out["proc_V"], proc_seed=out["proc_seed"], proc_step=out["proc_step"], proc_cap=out["proc_cap"],
                     proc_hist_len=out["proc_hist_len"], proc_hist=out["proc_hist"],
                     proc_mask=np.zeros((n, (V + 7) // 8), dtype=np.uint8))
        scores, hist, cap, _ = R.processor_case(probe, i)
        gc.max_initial_timestamp_index = cap
        proc = WhisperTimeStampLogitsProcessor(gc, begin_index=P)
        res = proc(torch.tensor([R.PREFIX + hist]), torch.from_numpy(scores)[None])[0].numpy()
        masks.append(np.packbits(np.isneginf(res)))
    gc.max_initial_timestamp_index = R.MAX_INITIAL_TIMESTAMP_INDEX
    out["proc_mask"] = np.stack(masks)
    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
