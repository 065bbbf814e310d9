"""Float64 restatement of the scored pick (ca_pick_scored_advance) and of the statistics of Whisper's temperature
fallback ($TF/models/whisper/generation_whisper.py: generate_with_fallback, _need_fallback, _retrieve_avg_logprobs,
_retrieve_compression_ratio), and the fixture of tests/golden/whisper_fallback.npz.

The sampler is this project's definition, not torch.multinomial: over the allowed set of a row, with m its maximum,
p_i = exp((x_i - m) / T), S = sum p_i, target = u S; the token is the smallest allowed i with p_i > 0 whose inclusive
prefix sum exceeds the target, and the last allowed i with p_i > 0 where none does.  tools/gen_whisper_fallback_goldens.py
runs transformers' own loop with torch.multinomial replaced by `sample_pick` on recorded uniforms."""
from __future__ import annotations

import json
import math
import zlib
from pathlib import Path

import numpy as np

import whisper_ts_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "whisper_fallback.npz"
NO_SPEECH_TOKEN = R.NO_TIMESTAMPS - 1  # the text id declared <|nospeech|>: the one in front of <|notimestamps|>, as transformers takes it
# The fixture model is random-init: its greedy windows loop and score the best average log-probabilities (-3.68 .. -3.62),
# a window sampled at 0.2 or above always scores lower (-3.96 .. -3.80 at 0.2), so "failed the log-prob threshold at 0, passed
# at a later temperature" cannot occur with Whisper's own list.  0.05 stands in front of it: nearly greedy, it re-rolls the
# near-ties of the text logits and lands on either side of a threshold cut inside the greedy range.
TEMPERATURES = (0.0, 0.05, 0.2, 0.4)
SEED = 1234
DELTA = 2.0 ** -16              # acceptance half-width relative to S: twice the bound of 128 fp32 additions (128 * 2^-24)


def allowed_row(scores, suppress=None, history=None, timestamp_begin=None, eos_id=None, cap=None):
    """-> float64 row, -inf outside the allowed set.  history None: the suppress mask alone."""
    x = np.array(scores, dtype=np.float64)
    if suppress is not None:
        x[np.asarray(suppress).astype(bool)] = -np.inf
    if history is None:
        return x
    return R.timestamp_rules(x, history, timestamp_begin, eos_id, cap)


def weights(row, inv_t):
    row = np.asarray(row, dtype=np.float64)
    ok = np.isfinite(row)
    p = np.zeros_like(row)
    if ok.any():
        p[ok] = np.exp((row[ok] - row[ok].max()) * float(inv_t))
    return p


def sample_pick(row, inv_t, u) -> int:
    """The inverse-CDF rule in float64.  u is taken at the precision it is given (the kernel reads it as fp32)."""
    p = weights(row, inv_t)
    mass = np.nonzero(p > 0)[0]
    if mass.size == 0:
        return 0
    cdf = np.cumsum(p)
    target = float(u) * cdf[-1]
    hit = mass[cdf[mass] > target]
    return int(hit[0]) if hit.size else int(mass[-1])


def acceptable(row, inv_t, u, delta=DELTA):
    """The tokens whose float64 interval [prefix before, prefix after] meets [target - delta S, target + delta S]."""
    p = weights(row, inv_t)
    cdf = np.cumsum(p)
    S = cdf[-1]
    target = float(u) * S
    lo, hi = target - delta * S, target + delta * S
    before = cdf - p
    return set(np.nonzero((p > 0) & (cdf >= lo) & (before <= hi))[0].tolist())


def logprob(row, tok) -> float:
    """x_tok - logsumexp(allowed set) at temperature 1."""
    row = np.asarray(row, dtype=np.float64)
    ok = np.isfinite(row)
    m = row[ok].max()
    return float(row[tok] - (m + math.log(np.exp(row[ok] - m).sum())))


# ---- the statistics of generate_with_fallback ----------------------------------------------------------------------------
def compression_ratio(ids, vocab_size: int) -> float:
    """_retrieve_compression_ratio: zlib over the ids' little-endian bytes, int(log2(V) / 8) + 1 bytes each."""
    length = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(length, "little") for t in ids)
    return len(raw) / len(zlib.compress(raw))


def need_fallback(avg_logprob, ratio, no_speech_prob, temperature, logprob_threshold, compression_ratio_threshold,
                  no_speech_threshold):
    """_need_fallback -> (needs_fallback, should_skip)."""
    needs, skip = False, False
    if compression_ratio_threshold is not None and ratio > compression_ratio_threshold:
        needs = True
    if logprob_threshold is not None and avg_logprob < logprob_threshold:
        needs = True
    if no_speech_threshold is not None and no_speech_prob is not None:
        if logprob_threshold is not None and avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold:
            needs, skip = False, True
    return needs, skip


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    assert json.loads(str(z["recipe"])) == R.RECIPE, "tests/golden/whisper_fallback.npz was written with another recipe"
    return z
