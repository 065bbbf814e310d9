"""`evaluate(config)` — mirror of R/src/coral/evaluate.py:29-85: load the saved model + processor (wav2vec2 or
Whisper, by the saved architecture), transcribe the evaluation examples in batches (greedy CTC - or the LM-fused CTC
beam search when the model directory holds `language_model/*.arpa` and `no_lm` is false -, or log-mel +
greedy `generate(language="danish", task="transcribe")`, on the GPU), normalise both sides like the reference
(lower / strip) and report CER / WER.  `error_rates: device` takes the rates from alignment counts computed on the
GPU (coral_amd/error_rates.py) and opens the reference's normalised rates (`normalise_error_rates`) and its demographic
slicing (`get_score_df`, :161-216, restated without pandas: `score_categories`); the default, `host`, is
coral_amd/metrics.py as before."""

from __future__ import annotations

import csv
import logging
import math
from pathlib import Path

import torch

from . import ops
from .data import synthetic_examples
from .metrics import cer, wer
from .model_setup import load_model_setup

logger = logging.getLogger(__package__)

WHISPER_CHUNK_LENGTH_REFUSAL = (
    "chunk_length_s > 0 is built for wav2vec2 models and for Whisper's chunked long-form mode only: with "
    "whisper_long_form: sequential a Whisper model transcribes recordings longer than 30 s without it (transformers' "
    "sequential long-form decoding): set chunk_length_s to 0, or set whisper_long_form: chunked (the pipeline's "
    "overlapping chunks, decoded as batches and merged on the GPU)")


def transcribe(model, processor, arrays: list, batch_size: int = 16, chunk_length_s: float = 0, stride_length_s=None,
               return_timestamps=None, timestamp_source: str = "emission", sampling_rate=None, n_best=None, hotwords=None,
               hotword_weight: float = 10.0):
    """ASR-pipeline equivalent ($TF/pipelines/automatic_speech_recognition.py:345,569-575,679):
    feature-extract, forward, argmax over all frames, CTC collapse, decode.  -> list of texts.
    chunk_length_s > 0: overlapping chunks with the pipeline's `chunk_length_s` / `stride_length_s` semantics
    (coral_amd/longform.py); 0: every clip whole.  return_timestamps="char" | "word": a list of {"text", "chunks":
    [{"text", "timestamp": (start_s, stop_s)}]} instead (greedy decoding only, unless timestamp_source="alignment").
    A whole clip of more than 4096 frames (81.9 s), or one decoded with timestamps, is collapsed by
    `ca_ctc_collapse_offsets`.  timestamp_source="alignment": the times come from the CTC forced alignment of the decoded
    ids to the same logits (`ca_ctc_align`) - with the greedy decoder and with the LM-fused beam search alike.
    sampling_rate: the rate of `arrays`, one int or one per recording (None: the extractor's).  Recordings at another
    rate are resampled on the GPU first (coral_amd/resample.py), so chunking and times see audio at the model's rate.
    n_best, hotwords, hotword_weight: the arguments of those names of `Wav2Vec2ProcessorWithLM.batch_decode` (LM decoding
    only).  hotwords: words or phrases whose words each add hotword_weight to a hypothesis.  n_best: the
    result per recording is {"text", "n_best": [{"text", "score", "logit_score", "lm_score", "posterior"}]} (+ "chunks"
    with timestamps, which are the first hypothesis'); "text" is the first hypothesis, what the call returns without
    n_best.  Refused by name: either argument with a processor without an LM, and n_best > beam_width."""
    from .longform import align_rows, check_timestamp_mode, collapse_rows, decode_rows, transcribe_long
    from .nbest import check_nbest_arguments, lm_decode, nbest_records
    from .resample import to_rate

    with_lm = getattr(processor, "lm", None) is not None
    check_timestamp_mode(return_timestamps, with_lm, timestamp_source)
    check_nbest_arguments(processor, n_best, hotwords, hotword_weight)
    if chunk_length_s is not None and chunk_length_s < 0:
        raise ValueError(f"chunk_length_s must be 0 (whole clips) or positive, got {chunk_length_s}")
    if sampling_rate is not None:
        arrays = to_rate(arrays, sampling_rate, processor.feature_extractor.sampling_rate, model.engine.device)
    if chunk_length_s:
        res = transcribe_long(model, processor, arrays, chunk_length_s, stride_length_s, batch_size, return_timestamps,
                              timestamp_source, n_best=n_best, hotwords=hotwords, hotword_weight=hotword_weight)
        return res if return_timestamps is not None or n_best is not None else [r["text"] for r in res]
    model.eval()
    out = []
    for i in range(0, len(arrays), batch_size):
        feats = [processor(a, sampling_rate=processor.feature_extractor.sampling_rate) for a in arrays[i:i + batch_size]]
        batch = processor.feature_extractor.pad(feats, padding="longest")
        with torch.no_grad():
            model(torch.from_numpy(batch["input_values"]), torch.from_numpy(batch["attention_mask"]))
        eng = model.engine
        T = eng._saved["w"]["T"]
        if with_lm:  # Wav2Vec2ProcessorWithLM: LM-fused beam search on the GPU
            ids, hyps = lm_decode(eng, processor, n_best, hotwords, hotword_weight)
            if return_timestamps is not None:  # (timestamp_source="alignment": the check above refuses the other)
                res = decode_rows(align_rows(eng, ids), processor.tokenizer, return_timestamps,
                                  math.prod(eng.s.conv_stride), processor.feature_extractor.sampling_rate)
            elif hyps is not None:
                res = [{"text": processor.tokenizer.decode(r, group_tokens=False)} for r in ids]
            if hyps is not None:
                for item, h in zip(res, hyps):
                    item["n_best"] = nbest_records(h, processor.tokenizer)
            if return_timestamps is not None or hyps is not None:
                out += res
                continue
        elif T > 4096 or return_timestamps is not None:
            # every frame of the padded batch, as the greedy kernel below decodes them: identity segments
            w, B, s = eng._saved["w"], eng._saved["B"], eng.s
            seg = torch.tensor([(b, 0, 0, T) for b in range(B)], dtype=torch.int32).to(eng.device)
            raw = torch.empty(B, T, dtype=torch.int32, device=eng.device)
            ops.ctc_stitch(w["logits"], seg, raw, None, B, T, s.vocab_size, w["Vp"], B, T)
            sr = processor.feature_extractor.sampling_rate
            rows = collapse_rows(raw, None, s.pad_token_id)
            if return_timestamps is not None and timestamp_source == "alignment":
                rows = align_rows(eng, [r[0] for r in rows])
            res = decode_rows(rows, processor.tokenizer, return_timestamps, math.prod(s.conv_stride), sr)
            out += res if return_timestamps is not None else [r["text"] for r in res]
            continue
        else:
            ids, _ = eng.greedy_decode()
        out += [processor.tokenizer.decode(r, group_tokens=False) for r in ids]
    return out


def transcribe_whisper(model, processor, arrays: list, batch_size: int = 16, max_length: int | None = None,
                       num_beams: int = 1, return_timestamps: bool = False, temperature=None, logprob_threshold=None,
                       compression_ratio_threshold=None, no_speech_threshold=None, sample_seed: int = 0, prompt_ids=None,
                       condition_on_prev_tokens=None, prompt_condition_type=None, prompt: str | None = None,
                       sampling_rate=None, long_form: str = "sequential", chunk_length_s=None, stride_length_s=None):
    """The Whisper branch of the ASR pipeline ($TF/pipelines/automatic_speech_recognition.py:345,529,600): pad / trim
    every clip to 30 s, log-mel on the GPU, `model.generate(input_features, language="danish", task="transcribe")`
    (R/src/coral/evaluate.py:56-60), decode the generated ids without special tokens.
    -> (texts, id rows).  Without the byte-level BPE files (offline) the texts are the ids rendered as words.
    num_beams >= 2: beam search (`generate_kwargs={"num_beams": k}` of the pipeline); a batch is then decoded at most
    128 // num_beams clips at a time (the decoder's row limit).
    A clip longer than 30 s is not cut: it goes through the sequential long-form loop of transformers' `generate`
    (coral_amd/longform_whisper.py: windows of 30 s decoded with timestamps, each starting where the last closed
    segment of the one before ended) and its segments are stitched to one text; its id row is the segments' ids in
    order, timestamps included.  return_timestamps=True: every clip takes that loop and the first result is a list of
    {"text", "chunks": [{"text", "timestamp": (start_s, end_s)}]}.  return_timestamps="word": the same loop with token
    timestamps (cross-attention alignment + dynamic time warping, each window with num_frames = min(3000, frames left));
    one chunk per word (coral_amd/whisper_align.py).  All of these are greedy only.
    temperature (a number or a list tried in order), logprob_threshold, compression_ratio_threshold, no_speech_threshold:
    transformers' temperature fallback (coral_amd/longform_whisper.py `FallbackPolicy`): every clip then takes the window
    loop; a window that fails a threshold is decoded again with sampling at the next temperature (uniforms from a CPU
    generator seeded with sample_seed), one that is silence is skipped; with return_timestamps every chunk's window
    carries avg_logprob, temperature and no_speech_prob under "windows".  Not with beams, not with "word".
    prompt_ids, condition_on_prev_tokens, prompt_condition_type: transformers' arguments of those names
    (coral_amd/longform_whisper.py `PromptPolicy`): every clip then takes the window loop, and a window's decoder input
    starts with the clip's text so far and / or the prompt, left-padded over the round's windows.  prompt: a string in
    place of prompt_ids, through the processor's (or its tokenizer's) `get_prompt_ids`.  With the fallback arguments a
    window accepted at a temperature of 0.5 or more leaves the next one unconditioned.  Not with beams, not with "word".
    sampling_rate: the rate of `arrays`, one int or one per recording (None: the extractor's).  Recordings at another
    rate are resampled on the GPU first (coral_amd/resample.py); the 30 s rule then applies to the resampled audio.
    long_form="chunked": the pipeline's `chunk_length_s` mode instead of the sequential loop (coral_amd/chunked_whisper.py):
    every recording is cut into overlapping chunks of chunk_length_s seconds (0 / None: 30; stride_length_s as in
    `transcribe`), the chunks of all recordings are decoded as batches of batch_size and merged on the GPU
    (`ca_overlap_merge`); the id rows are then the merged text ids.  Greedy or beams (beams without timestamps); "word",
    the fallback and the prompt arguments are refused by name.  long_form="sequential" (the default) is everything
    above, unchanged, and still refuses chunk_length_s > 0."""
    from .resample import to_rate

    if long_form not in ("sequential", "chunked"):
        raise ValueError(f"long_form must be \"sequential\" or \"chunked\", got {long_form!r}")
    if long_form == "chunked":
        from .chunked_whisper import transcribe_chunked

        res = transcribe_chunked(model, processor, arrays, chunk_length_s or 30.0, stride_length_s, batch_size, max_length,
                                 num_beams or 1, return_timestamps, sampling_rate, temperature=temperature,
                                 logprob_threshold=logprob_threshold, compression_ratio_threshold=compression_ratio_threshold,
                                 no_speech_threshold=no_speech_threshold, prompt_ids=prompt_ids, prompt=prompt,
                                 condition_on_prev_tokens=condition_on_prev_tokens, prompt_condition_type=prompt_condition_type)
        if return_timestamps:
            return [dict(text=r["text"], chunks=r["chunks"]) for r in res], [r["ids"] for r in res]
        return [r["text"] for r in res], [r["ids"] for r in res]
    if chunk_length_s:
        raise ValueError(WHISPER_CHUNK_LENGTH_REFUSAL)
    model.eval()
    if prompt is not None:
        getter = getattr(processor, "get_prompt_ids", None) or getattr(getattr(processor, "tokenizer", None), "get_prompt_ids", None)
        if prompt_ids is not None:
            raise ValueError("prompt= and prompt_ids= name the same thing: pass one of them")
        if getter is None:
            raise ValueError("prompt=: this processor's tokenizer has no get_prompt_ids (the byte-level BPE files are not "
                             "loaded); pass prompt_ids=, the ids transformers' get_prompt_ids returns for the string")
        prompt_ids = [int(t) for t in getter(prompt)]
    prompting = model.prompt_policy(prompt_ids, condition_on_prev_tokens, prompt_condition_type)
    policy = model.fallback_policy(temperature, logprob_threshold, compression_ratio_threshold, no_speech_threshold,
                                   sample_seed)
    texts, rows = [], []
    max_length = int(max_length or model.shape.max_target_positions)
    num_beams = int(num_beams or 1)
    if num_beams < 1:
        raise ValueError(f"num_beams must be a positive integer, got {num_beams}")
    from .whisper import N_SAMPLES

    word = isinstance(return_timestamps, str) and return_timestamps == "word"
    if not word and not any(return_timestamps is v for v in (True, False, None)):
        raise ValueError(f"return_timestamps must be true, false or \"word\" for a Whisper model, got {return_timestamps!r}")
    if policy is not None:
        if num_beams > 1:
            raise ValueError(f"num_beams={num_beams}: temperature / logprob_threshold / compression_ratio_threshold / "
                             "no_speech_threshold are not implemented with beam search")
        if word:
            raise ValueError("return_timestamps=\"word\" is not implemented with temperature fallback")
    if prompting is not None:
        if num_beams > 1:
            raise ValueError(f"num_beams={num_beams}: prompt_ids / condition_on_prev_tokens / prompt_condition_type are not "
                             "implemented with beam search")
        if word:
            raise ValueError("return_timestamps=\"word\" is not implemented with prompt_ids / condition_on_prev_tokens")
    if sampling_rate is not None:
        arrays = to_rate(arrays, sampling_rate, processor.feature_extractor.sampling_rate, model.engine.device)
    looped = [i for i, a in enumerate(arrays)
              if return_timestamps or policy is not None or prompting is not None or len(a) > N_SAMPLES]
    if looped and num_beams > 1:
        raise ValueError(f"num_beams={num_beams}: return_timestamps / recordings longer than 30 s are decoded greedily "
                         "only (beam search with timestamps is not implemented)")
    taken = set(looped)
    plain = [i for i in range(len(arrays)) if i not in taken]
    gen_kw = dict(num_beams=num_beams) if num_beams > 1 else {}
    if num_beams > 1:
        batch_size = max(1, min(batch_size, 128 // num_beams))
    for i in range(0, len(plain), batch_size):
        feats = processor.feature_extractor([arrays[j] for j in plain[i:i + batch_size]],
                                            sampling_rate=processor.feature_extractor.sampling_rate)
        ids = model.generate(feats, language="danish", task="transcribe", max_length=max_length, **gen_kw)
        ids = ids.tolist() if hasattr(ids, "tolist") else [list(map(int, r)) for r in ids]
        rows += ids
        texts += processor.batch_decode(ids, skip_special_tokens=True)
    if not looped:
        return texts, rows
    # back into the order of `arrays`
    results, all_rows = [None] * len(arrays), [None] * len(arrays)
    for i, t, r in zip(plain, texts, rows):
        results[i], all_rows[i] = t, r
    timed, timed_rows = _transcribe_whisper_windows(model, processor, [arrays[i] for i in looped], batch_size, max_length,
                                                    "word" if word else bool(return_timestamps), policy, prompting)
    for i, t, r in zip(looped, timed, timed_rows):
        results[i], all_rows[i] = t, r
    return results, all_rows


def _transcribe_whisper_windows(model, processor, arrays, batch_size, max_length, return_timestamps, policy=None,
                                prompting=None):
    """The long-form loop over `arrays` (clips above 30 s, or every clip when timestamps are asked for), all of them
    sharing its rounds.  -> (texts, or {"text", "chunks"} per clip with return_timestamps; id rows).
    return_timestamps="word": one chunk per word from the windows' token times.  prompting: a PromptPolicy; the loop then
    hands every call the decoder inputs of its windows."""
    from .longform_whisper import run_longform, stitched_ids
    from .whisper import N_SAMPLES
    from .whisper_align import cap_token_times, offline_decode, word_chunks

    word = return_timestamps == "word"

    fe = processor.feature_extractor
    prefix_len, tb = len(model.forced_prefix(return_timestamps=True)), model.forced_prefix()[-1] + 1
    # a clip of at most 30 s is padded to 30 s before the log-mel, as the pipeline's extractor pads it; a longer one
    # keeps its length (truncation=False) and its own maximum
    mels = [fe(a, sampling_rate=fe.sampling_rate)[0] if len(a) <= N_SAMPLES else fe.whole(a) for a in arrays]
    # the frames that hold audio: what the extractor's attention mask counts.  The seek loop runs over the padded 30 s, as
    # transformers' does for a clip of one window; the DTW of a window sees only what is left of the true frames
    true_frames = [min(m.shape[1], max(1, len(a) // 160)) for m, a in zip(mels, arrays)]

    def window_generate(batch, inputs=None):
        feats = torch.stack([torch.nn.functional.pad(mels[c][:, seek:seek + 3000], (0, max(0, 3000 - (mels[c].shape[1] - seek))))
                             for c, seek in batch])
        if inputs is not None:
            return model.prompted_window(feats, inputs, True)
        if word:  # (num_frames = min(3000, true frames left): the padding behind them never enters the DTW)
            return model.generate(feats, language="danish", task="transcribe", max_length=max_length, return_timestamps=True,
                                  return_token_timestamps=True,
                                  num_frames=[min(3000, true_frames[c] - seek) for c, seek in batch])
        return model.generate(feats, language="danish", task="transcribe", max_length=max_length, return_timestamps=True)

    s = model.shape
    if policy is not None:
        attempt = model.fallback_attempts(policy, max_length, True)

        def window_generate(batch, temperature, uniforms, inputs=None):  # noqa: F811  (the protocol under a policy)
            feats = {(c, seek): torch.nn.functional.pad(mels[c][:, seek:seek + 3000],
                                                        (0, max(0, 3000 - (mels[c].shape[1] - seek)))) for c, seek in batch}
            return attempt(batch, temperature, uniforms, feats, inputs)

    extra = {}
    if prompting is not None:
        extra = dict(conditioning=prompting, init_tokens=model.forced_prefix(return_timestamps=True),
                     max_target_positions=s.max_target_positions)
    done = run_longform(window_generate, [m.shape[1] for m in mels], tb, prefix_len, s.pad_token_id, s.eos_token_id,
                        batch_size=batch_size, return_token_timestamps=word, fallback=policy,
                        vocab_size=s.vocab_size if policy is not None else None,
                        max_length=max_length if policy is not None or prompting is not None else None, **extra)
    tok = getattr(processor, "tokenizer", None)
    decode = offline_decode if tok is None else (lambda ids: tok.decode([int(t) for t in ids], skip_special_tokens=False))
    results, rows = [], []
    for n, res in enumerate(done):
        rows.append([t for seg in res["segments"] for t in seg[2]])
        text = processor.batch_decode([stitched_ids(res["segments"], tb)], skip_special_tokens=True)[0]
        if word:
            # (a window the seek loop opens in the padding behind a short clip's end has no true frame left: F_b = 1,
            # all its times are its offset; they are capped at the clip's end)
            times = cap_token_times([t for seg in res["segments"] for t in seg[3]], true_frames[n] * 0.01)
            chunks = word_chunks(decode, rows[-1], times, tb, s.eos_token_id)
            results.append(dict(text=text, chunks=chunks))
        elif return_timestamps:
            chunks = [dict(text=processor.batch_decode([[t for t in ids if t < tb]], skip_special_tokens=True)[0],
                           timestamp=(start, end)) for start, end, ids, *_ in res["segments"]]
            results.append(dict(text=text, chunks=chunks))
            if policy is not None:
                results[-1]["windows"] = res["window_stats"]
        else:
            results.append(text)
    return results, rows


def _whisper_timestamp_mode(value):
    """`return_timestamps` of evaluation.yaml for a Whisper model: "word" stays, anything else as before (its truth value)."""
    return "word" if isinstance(value, str) and value == "word" else bool(value or False)


def _plain(value):
    """A temperature from the configuration: a number, None, or a list of numbers as a tuple."""
    return value if value is None or isinstance(value, (int, float)) else tuple(float(t) for t in value)


def _ids(value):
    """prompt_ids from the configuration: None or a list of ids."""
    return None if value is None else [int(t) for t in value]


def saved_model_type(model_dir) -> str:
    """"wav2vec2" or "whisper", from the `architectures` / `model_type` of the saved config.json (the ASR pipeline
    dispatches on the loaded model's class the same way, $TF/pipelines/automatic_speech_recognition.py:195-215)."""
    import json

    cfg = json.loads((Path(model_dir) / "config.json").read_text())
    arch = " ".join(cfg.get("architectures") or []) + " " + str(cfg.get("model_type", ""))
    if "whisper" in arch.lower():
        return "whisper"
    if "wav2vec2" in arch.lower():
        return "wav2vec2"
    raise ValueError(f"{model_dir}: unsupported architecture {arch.strip()!r}")


def evaluate(config, examples: list | None = None) -> dict:
    """config: evaluation.yaml keys (+ `model_dir`).  examples: list of {"audio": array, "text": str} and optionally
    "sampling_rate" (an example without one is at `config.sampling_rate`, the target; another rate is resampled on the
    GPU); defaults to a seeded synthetic set (no hub access here).  Serves both model types, like the reference's
    pipeline-based `evaluate` (R/src/coral/evaluate.py:29-85, :123-158)."""
    from .config import DictConfig

    from .error_rates import BOOTSTRAP_FIELDS, batch_scores, bootstrap_rates, check_options, score_table

    categories = list(config.get("score_categories", None) or [])
    normalise = bool(config.get("normalise_error_rates", False) or False)
    boot_cluster = config.get("bootstrap_cluster", None)
    boot = None  # bootstrap_samples: null leaves every output below as it is without the key
    if config.get("bootstrap_samples", None) is not None:
        confidence = config.get("bootstrap_confidence", None)
        boot = dict(n_resamples=int(config.bootstrap_samples), seed=int(config.get("bootstrap_seed", 0) or 0),
                    confidence=0.95 if confidence is None else float(confidence))
    on_device = check_options(config.get("error_rates", "host"), normalise, categories,
                              None if boot is None else boot["n_resamples"], None if boot is None else boot["confidence"],
                              boot_cluster)
    for i, e in enumerate(examples or []):  # before anything is transcribed
        for c in categories:
            if c not in e:
                raise ValueError(f"score_categories: example {i} has no {c!r}")
        if boot_cluster is not None and boot_cluster not in e:
            raise ValueError(f"bootstrap_cluster: example {i} has no {boot_cluster!r}")
    model_dir = config.get("model_dir", config.model_id)
    mtype = saved_model_type(model_dir)
    chunk_length_s = config.get("chunk_length_s", 0) or 0
    long_form = config.get("whisper_long_form", None) or "sequential"
    if mtype == "whisper" and long_form not in ("sequential", "chunked"):
        raise ValueError(f"whisper_long_form must be sequential or chunked, got {long_form!r}")
    if mtype == "whisper" and chunk_length_s > 0 and long_form != "chunked":
        raise ValueError(WHISPER_CHUNK_LENGTH_REFUSAL)
    if mtype == "whisper" and (config.get("n_best", None) is not None or config.get("hotwords", None) is not None):
        raise ValueError("n_best / hotwords belong to the LM-fused CTC beam search of wav2vec2 models; a Whisper model has "
                         "neither (num_beams is its beam search)")
    if mtype == "whisper" and long_form == "chunked":  # what the mode refuses, before the model is loaded
        from .chunked_whisper import check_chunked_arguments

        check_chunked_arguments(chunk_length_s or 30.0, config.get("num_beams", 1) or 1,
                                _whisper_timestamp_mode(config.get("return_timestamps", False)),
                                dict(temperature=_plain(config.get("temperature", None)),
                                     logprob_threshold=config.get("logprob_threshold", None),
                                     compression_ratio_threshold=config.get("compression_ratio_threshold", None),
                                     no_speech_threshold=config.get("no_speech_threshold", None),
                                     prompt_ids=_ids(config.get("prompt_ids", None)),
                                     condition_on_prev_tokens=bool(config.get("condition_on_prev_tokens", False) or False),
                                     prompt_condition_type=config.get("prompt_condition_type", None)))
    mcfg = DictConfig(model=DictConfig(type=mtype, sampling_rate=config.sampling_rate, decoder=None),
                      model_dir=model_dir, padding="longest",
                      max_seconds_per_example=config.max_seconds_per_example)
    setup = load_model_setup(mcfg)
    # `no_lm` (R/src/coral/evaluate.py:123-158): false decodes with model_dir/language_model/ when there is one
    saved = setup.load_saved() if mtype == "whisper" else setup.load_saved(no_lm=bool(config.get("no_lm", False)))
    model, processor = saved.model, saved.processor
    id_rows = timed = nbest = None
    rates = None  # one per example when any of them names a rate
    if examples is not None and any(e.get("sampling_rate") is not None for e in examples):
        rates = [e.get("sampling_rate") for e in examples]
    if mtype == "whisper":
        if examples is None:
            import numpy as np

            rng = np.random.RandomState(99)
            examples = []
            for _ in range(2 * config.batch_size):
                n = int(rng.uniform(config.min_seconds_per_example, min(3.0, config.max_seconds_per_example)) * config.sampling_rate)
                w = np.clip(0.1 * rng.randn(n), -1, 1).astype(np.float32)
                examples.append(dict(audio=w / np.abs(w).max(), text=""))
        preds, id_rows = transcribe_whisper(model, processor, [e["audio"] for e in examples], config.batch_size,
                                            config.get("generation_max_length", None), config.get("num_beams", 1) or 1,
                                            return_timestamps=_whisper_timestamp_mode(config.get("return_timestamps", False)),
                                            temperature=_plain(config.get("temperature", None)),
                                            logprob_threshold=config.get("logprob_threshold", None),
                                            compression_ratio_threshold=config.get("compression_ratio_threshold", None),
                                            no_speech_threshold=config.get("no_speech_threshold", None),
                                            sample_seed=int(config.get("sample_seed", 0) or 0),
                                            prompt_ids=_ids(config.get("prompt_ids", None)),
                                            condition_on_prev_tokens=bool(config.get("condition_on_prev_tokens", False) or False),
                                            prompt_condition_type=config.get("prompt_condition_type", None),
                                            sampling_rate=rates, long_form=long_form, chunk_length_s=chunk_length_s,
                                            stride_length_s=config.get("stride_length_s", None))
        if preds and isinstance(preds[0], dict):
            timed, preds = preds, [p["text"] for p in preds]
    else:
        if examples is None:
            examples = [dict(audio=ex["input_values"], text=ex["text"])
                        for ex in synthetic_examples(processor, 2 * config.batch_size, 99, config.min_seconds_per_example,
                                                     min(3.0, config.max_seconds_per_example), config.sampling_rate)]
        n_best = config.get("n_best", None)
        hotwords = config.get("hotwords", None)
        extra = {}  # n_best: null and hotwords: null leave the call, and every output below, as they are without the keys
        if n_best is not None or hotwords is not None:
            weight = config.get("hotword_weight", None)
            extra = dict(n_best=None if n_best is None else int(n_best), hotwords=None if hotwords is None else list(hotwords),
                         hotword_weight=10.0 if weight is None else float(weight))
        preds = transcribe(model, processor, [e["audio"] for e in examples], config.batch_size,
                           chunk_length_s=chunk_length_s, stride_length_s=config.get("stride_length_s", None),
                           timestamp_source=config.get("timestamp_source", "emission"), sampling_rate=rates, **extra)
        if n_best is not None:
            nbest, preds = [p["n_best"] for p in preds], [p["text"] for p in preds]
    preds = [p.lower().strip() for p in preds]
    labels = [e["text"].lower().strip() if config.lower_case else e["text"].strip() for e in examples]
    scores = dict(model_type=mtype, n=len(examples))
    table = None
    if any(labels) and on_device:  # the same two rates from alignment counts (ca_edit_counts), and what only counts give
        device = model.engine.device if hasattr(model, "engine") else "cuda"
        res = batch_scores(preds, labels, normalise, device)
        scores.update(cer=res["cer"], wer=res["wer"],
                      error_counts=dict(char=res["char_counts"].sum(0).tolist(), word=res["word_counts"].sum(0).tolist()))
        if nbest is not None:  # how good the best hypothesis in each list is; the hypotheses normalised like the predictions
            from .error_rates import _rate, oracle_counts

            texts = [[h["text"].lower().strip() for h in hyps] for hyps in nbest]
            oc, ow = oracle_counts(texts, labels, "char", device), oracle_counts(texts, labels, "word", device)
            scores.update(oracle_cer=_rate(oc["counts"], normalise), oracle_wer=_rate(ow["counts"], normalise),
                          oracle_index=dict(char=oc["index"].tolist(), word=ow["index"].tolist()))
        if boot is not None:  # the published form: mean ± half_width of the resampled rates (ca_bootstrap_sums)
            if boot_cluster is not None:
                missing = [i for i, e in enumerate(examples) if boot_cluster not in e]
                if missing:
                    raise ValueError(f"bootstrap_cluster: example {missing[0]} has no {boot_cluster!r}")
                boot["clusters"] = [e[boot_cluster] for e in examples]
            scores["bootstrap"] = dict(bootstrap_rates(res["char_counts"], res["word_counts"], normalise, device=device, **boot),
                                       n_resamples=boot["n_resamples"], seed=boot["seed"], confidence=boot["confidence"])
        if categories:
            table = scores["score_table"] = score_table(examples, categories, res["char_counts"], res["word_counts"], normalise,
                                                        bootstrap=None if boot is None else dict(boot, device=device))
    elif any(labels):  # CER / WER need reference texts (a synthetic Whisper set has none: ids-only output)
        scores.update(cer=cer(preds, labels), wer=wer(preds, labels))
    name = str(config.model_id).replace("/", "--") + "." + str(config.dataset).split("::")[0].replace("/", "--")
    if config.store_results and table is not None:
        with Path(f"{name}.scores.csv").open("w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=categories + ["cer", "wer"] + (list(BOOTSTRAP_FIELDS) if boot is not None else []))
            w.writeheader()
            w.writerows(table)
        scores["scores_csv"] = f"{name}.scores.csv"
    if config.store_results:
        path = Path(f"{name}.csv")
        with path.open("w", newline="") as f:
            w = csv.writer(f)
            if id_rows is not None and getattr(processor, "tokenizer", None) is None:
                w.writerow(["prediction", "label", "token_ids"])
                w.writerows((p, l, " ".join(map(str, r))) for p, l, r in zip(preds, labels, id_rows))
            else:
                w.writerow(["prediction", "label"])
                w.writerows(zip(preds, labels))
        scores["csv"] = str(path)
    if config.store_results and nbest is not None:
        import json

        with Path(f"{name}.nbest.jsonl").open("w", encoding="utf-8") as f:
            for label, hyps in zip(labels, nbest):
                f.write(json.dumps(dict(label=label, n_best=hyps), ensure_ascii=False) + "\n")
        scores["nbest_jsonl"] = f"{name}.nbest.jsonl"
    if nbest is not None:
        scores["n_best"] = nbest
    if id_rows is not None:
        scores["token_ids"] = id_rows
    if timed is not None:
        scores["chunks"] = [p["chunks"] for p in timed]
    return scores
