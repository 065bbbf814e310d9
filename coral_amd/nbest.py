"""N-best lists and hotwords in the transcription paths: the host glue between `evaluate.transcribe` /
`longform.transcribe_long` and `Wav2Vec2CTCEngine.beam_decode(n_best=, hotwords=, hotword_weight=)` - the arguments of
those names of transformers' `Wav2Vec2ProcessorWithLM.batch_decode` (the objective is this project's own,
parity with pyctcdecode is unpinned)."""

from __future__ import annotations

import math

DEFAULT_BEAM_WIDTH = 100


def check_nbest_arguments(processor, n_best, hotwords, hotword_weight) -> bool:
    """Refuses by name what the LM-fused beam search cannot serve.  -> True when the extended decode is asked for."""
    if n_best is None and hotwords is None:
        return False
    if getattr(processor, "lm", None) is None:
        what = "n_best" if n_best is not None else "hotwords"
        raise ValueError(f"{what} needs the LM-fused beam search: this processor has no LM decoder (greedy CTC decoding "
                         "returns one string and has no word scores); load a model directory with language_model/ and "
                         "no_lm: false")
    if n_best is not None:
        beam_width = int(processor.decoder_params.get("beam_width", DEFAULT_BEAM_WIDTH))
        if isinstance(n_best, bool) or not isinstance(n_best, int) or n_best < 1:
            raise ValueError(f"n_best must be a positive integer or None, got {n_best!r}")
        if n_best > beam_width:
            raise ValueError(f"n_best={n_best} is larger than beam_width={beam_width}: the search keeps no more prefixes "
                             "than that")
    if isinstance(hotwords, str):
        raise ValueError("hotwords is a list of words or phrases, not one string")
    if isinstance(hotword_weight, bool) or not isinstance(hotword_weight, (int, float)) or not math.isfinite(hotword_weight):
        raise ValueError(f"hotword_weight must be a finite number, got {hotword_weight!r}")
    return True


def lm_decode(eng, processor, n_best=None, hotwords=None, hotword_weight=10.0, **kw):
    """The LM-fused decode of the last forward (or of kw["logits"]) -> (best ids per row, n-best hypotheses per row or
    None).  Without n_best and hotwords this is the call the transcription paths have always issued."""
    tables = processor.device_tables(eng.device)
    if n_best is None and hotwords is None:
        ids, _ = eng.beam_decode(tables, tokenizer=processor.tokenizer, **kw, **processor.decoder_params)
        return ids, None
    hyps = eng.beam_decode(tables, tokenizer=processor.tokenizer, n_best=n_best or 1,
                           hotwords=processor.hotword_tables(hotwords, eng.device) or [],
                           hotword_weight=hotword_weight, **kw, **processor.decoder_params)
    return [h[0]["ids"] if h else [] for h in hyps], (hyps if n_best is not None else None)


def nbest_records(hyps: list, tokenizer) -> list[dict]:
    """One row's hypotheses -> [{"text", "score", "logit_score", "lm_score", "posterior"}], best first; `posterior` is
    the softmax of the returned scores (float64 on the host)."""
    if not hyps:
        return []
    top = max(h["score"] for h in hyps)
    w = [math.exp(h["score"] - top) for h in hyps]
    z = sum(w)
    return [dict(text=tokenizer.decode(h["ids"], group_tokens=False), score=h["score"], logit_score=h["logit_score"],
                 lm_score=h["lm_score"], posterior=v / z) for h, v in zip(hyps, w)]
