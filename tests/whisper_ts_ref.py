"""NumPy restatement of Whisper's timestamp rules and the fixture of tests/golden/whisper_ts.npz.

`timestamp_rules` restates `WhisperTimeStampLogitsProcessor.__call__` ($TF/generation/logits_process.py) for one row:
the same masks in the same order, the log-prob rule in float64 (the processor's fp32 log_softmax decides the same way
wherever |logsumexp(timestamps) - max(text)| is above fp32 resolution; the tests assert that gap).  `pick` is the greedy
token that follows.  tools/gen_whisper_ts_goldens.py records the processor's own output for random cases and
transformers' own generations on the fixture below; tests/test_whisper_ts_cpu.py holds this file against them.

The fixture is a seeded random-init model (oracle.whisper_ref.synth_params): d_model 64, 4 heads, 2 + 2 layers, 80
mels, 64 text / special ids followed by 1501 timestamp ids.  With such weights every logit is ~N(0, 0.16^2), so
logsumexp over 1501 timestamps (~ log 1501 = 7.3) beats every text token at every step and no positive rescaling of
the timestamp rows changes that (it only widens their spread).  `fixture_params` therefore gives the decoder's final
LayerNorm bias a component gamma along a seeded unit direction g and moves the timestamp rows of the (tied) embedding
to scale * row - delta_v * g: timestamp logits sit delta_v * (gamma + noise) lower, per context now above and now
below the text maximum; the EOS row gets + eps * g.  The recipe is recorded in the fixture file and asserted."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "whisper_ts.npz"

N_TEXT, N_TS = 64, 1501
CONFIG = dict(d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4,
              encoder_ffn_dim=128, decoder_ffn_dim=128, num_mel_bins=80, vocab_size=N_TEXT + N_TS, max_target_positions=64,
              pad_token_id=50, decoder_start_token_id=51, eos_token_id=50)
EOS, SOT, LANG, TRANSCRIBE, TRANSLATE, NO_TIMESTAMPS = 50, 51, 52, 53, 54, 63
TIMESTAMP_BEGIN = NO_TIMESTAMPS + 1
PREFIX = [SOT, LANG, TRANSCRIBE]            # return_timestamps=True: no <|notimestamps|>
PREFIX_NO_TS = PREFIX + [NO_TIMESTAMPS]
BEGIN_SUPPRESS = [20, EOS]
MAX_INITIAL_TIMESTAMP_INDEX = 50
MAX_LENGTH = 64
SAMPLING_RATE, HOP = 16_000, 160
RECIPE = dict(seed=32, gamma=6.0, scale=1.0, delta0=0.96, delta1=0.12, eps=0.06)
SHORT_SECONDS = (4.0, 11.5, 27.0)
LONG_SECONDS = (70.0, 95.0)


# ---- the rules ----------------------------------------------------------------------------------------------------------
def timestamp_rules(scores, history, timestamp_begin, eos_id, max_initial_timestamp_index=None, detail=False):
    """scores float [V] (the suppress sets already at -inf), history = the tokens generated since begin_index.
    -> the processed row (a float64 copy with -inf where the processor masks).  detail=True: (row, info dict)."""
    x = np.array(scores, dtype=np.float64)
    V, tb = x.shape[0], int(timestamp_begin)
    seq = [int(t) for t in history]
    x[tb - 1] = -np.inf
    last = len(seq) >= 1 and seq[-1] >= tb
    penult = len(seq) < 2 or seq[-2] >= tb
    if last:
        if penult:
            x[tb:] = -np.inf
        else:
            x[:eos_id] = -np.inf
    stamps = [t for t in seq if t >= tb]
    if stamps:
        t_last = stamps[-1] if (last and not penult) else stamps[-1] + 1
        x[tb:t_last] = -np.inf
    if not seq:
        x[:tb] = -np.inf
        if max_initial_timestamp_index is not None:
            x[tb + max_initial_timestamp_index + 1:] = -np.inf
    before = x.copy()
    ts, text = x[tb:], x[:tb]
    m = ts.max() if ts.size else -np.inf
    lse = m + np.log(np.exp(ts - m).sum()) if np.isfinite(m) else -np.inf
    tmax = text.max() if text.size else -np.inf
    forced = bool(lse > tmax)
    if forced:
        x[:tb] = -np.inf
    if detail:
        return x, dict(lse=float(lse), text_max=float(tmax), forced=forced, before=before, last=last, penult=penult)
    return x


def pick(row) -> int:
    """First maximum; 0 when everything is masked (as ca_argmax_masked)."""
    return int(np.argmax(row)) if np.isfinite(row).any() else 0


def advance(ids, done, tok, pos, klen, picks, pad_id, eos_id):
    """The bookkeeping of ca_argmax_advance on NumPy state (in place)."""
    for r, p in enumerate(picks):
        step = pad_id if done[r] else int(p)
        ids[r, pos[r] + 1] = step
        if step == eos_id:
            done[r] = True
        tok[r] = step
        pos[r] += 1
        klen[r] += 1


def grammar_ok(gen, timestamp_begin, eos_id) -> bool:
    """gen = generated tokens up to and without EOS / padding: starts with a timestamp, timestamps never decrease, a new
    segment does not start before the last one ended, at most two timestamps in a row."""
    tb = timestamp_begin
    if not gen or gen[0] < tb:
        return False
    stamps = [t for t in gen if t >= tb]
    if any(b < a for a, b in zip(stamps, stamps[1:])):
        return False
    run = 0
    for t in gen:
        run = run + 1 if t >= tb else 0
        if run > 2 or t == eos_id:
            return False
    return True


def strip_row(row, prefix_len, pad_id, eos_id):
    """One generated row -> its tokens after the prefix, without the EOS and the padding behind it."""
    gen = [int(t) for t in row[prefix_len:]]
    while gen and gen[-1] == pad_id:
        gen.pop()
    if pad_id != eos_id and gen and gen[-1] == eos_id:
        gen.pop()
    return gen


BRANCHES = ("initial_cap", "text_while_open", "timestamp_by_logprob", "pair_closed", "text_after_pair", "monotonic_mask",
            "eos_after_single")


def branches_from_ids(rows, prefix_len, timestamp_begin, eos_id, cap):
    """What the ids alone show of the branches the rules took (rows with their EOS, padding stripped)."""
    tb, seen = timestamp_begin, set()
    for row in rows:
        gen = [int(t) for t in row[prefix_len:]]
        if gen and tb <= gen[0] <= tb + cap:
            seen.add("initial_cap")
        for i in range(1, len(gen)):
            a, b = gen[i - 1], gen[i]
            a2 = gen[i - 2] if i >= 2 else None
            if a == eos_id:
                break
            if a < tb and b < tb and b != eos_id:
                seen.add("text_while_open")
            if a < tb and b >= tb:
                seen.add("timestamp_after_text")
            if a >= tb and b >= tb:
                seen.add("pair_closed")
            if a >= tb and (a2 is None or a2 >= tb) and b < tb and b != eos_id and i >= 2:
                seen.add("text_after_pair")
            if a >= tb and a2 is not None and a2 < tb and b == eos_id:
                seen.add("eos_after_single")
    return seen


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def fixture_config():
    from oracle import whisper_ref as w

    return w.WhisperConfig(**CONFIG)


def fixture_params(recipe=None):
    from oracle import whisper_ref as w

    r = dict(RECIPE if recipe is None else recipe)
    c = fixture_config()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(int(r["seed"]))
    gdir = torch.randn(c.d_model, generator=g)
    gdir = gdir / gdir.norm()
    delta = r["delta0"] + r["delta1"] * torch.randn(N_TS, generator=g)
    P["model.decoder.layer_norm.bias"] = P["model.decoder.layer_norm.bias"] + r["gamma"] * gdir
    E = P["model.decoder.embed_tokens.weight"].clone()
    E[TIMESTAMP_BEGIN:] = r["scale"] * E[TIMESTAMP_BEGIN:] - delta[:, None] * gdir[None, :]
    E[EOS] = E[EOS] + r["eps"] * gdir
    P["model.decoder.embed_tokens.weight"] = E
    return P


def fixture_wave(seconds: float, seed: int) -> np.ndarray:
    """Seeded noise whose loudness changes every few seconds (so a window's log-mel maximum differs from the
    recording's), a whole number of hops long."""
    rng = np.random.RandomState(seed)
    n = int(round(seconds * SAMPLING_RATE / HOP)) * HOP
    w = rng.randn(n).astype(np.float32)
    edges = np.arange(0, n, 3 * SAMPLING_RATE)
    for a, amp in zip(edges, rng.uniform(0.005, 0.3, size=len(edges))):
        w[a:a + 3 * SAMPLING_RATE] *= np.float32(amp)
    return w


def short_waves():
    return [fixture_wave(s, 700 + i) for i, s in enumerate(SHORT_SECONDS)]


def long_waves():
    return [fixture_wave(s, 800 + i) for i, s in enumerate(LONG_SECONDS)]


def short_features() -> torch.Tensor:
    from oracle import whisper_ref as w

    return torch.from_numpy(np.stack([w.log_mel(w.pad_or_trim(a)) for a in short_waves()]))


def long_features() -> list:
    """Whole-recording log-mel [80, frames] per recording: the clamp uses the recording's maximum."""
    from oracle import whisper_ref as w

    return [torch.from_numpy(w.log_mel(a)) for a in long_waves()]


def window_features(mel: torch.Tensor, seek: int, n: int = 3000) -> torch.Tensor:
    """Frames [seek, seek + n) of a recording's log-mel, zero-padded to n ($TF generation_whisper._get_input_segment)."""
    cut = mel[:, seek:seek + n]
    return torch.nn.functional.pad(cut, (0, n - cut.shape[1]))


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    assert json.loads(str(z["recipe"])) == RECIPE, "tests/golden/whisper_ts.npz was written with another recipe"
    return z


def processor_case(z, i):
    """Case i of the recorded processor runs -> (scores float32 [V], history list, cap or None, -inf mask bool [V])."""
    V = int(z["proc_V"])
    rng = np.random.RandomState(int(z["proc_seed"][i]))
    scores = (rng.permutation(V).astype(np.float32) - V / 2) * np.float32(z["proc_step"][i])
    n = int(z["proc_hist_len"][i])
    hist = z["proc_hist"][i, :n].tolist()
    cap = int(z["proc_cap"][i])
    mask = np.unpackbits(z["proc_mask"][i])[:V].astype(bool)
    return scores, hist, (None if cap < 0 else cap), mask


def check_timestamp_rows(lg_rows, ids, want, prefix_len, accept, forced, begin_suppress=BEGIN_SUPPRESS,
                         cap=MAX_INITIAL_TIMESTAMP_INDEX, eos_id=EOS, label=""):
    """The policy of tests/greedy_check.py under the timestamp rules.  lg_rows(b, seq) -> raw fp32 oracle logits
    [len(seq) - 1, V] of row b's OWN sequence.  The rules are applied here; their log-prob rule is a comparison of two
    oracle numbers (logsumexp of the timestamps, text maximum), so it has near-ties of its own:
      1. every token is within `accept` of the maximum of the processed row - with the log-prob rule applied as the
         oracle decides it or, where |logsumexp - text max| <= accept, either way;
      2. where that gap exceeds `forced` the oracle's side of the rule holds, and where moreover the processed row's top-2
         margin exceeds `forced` the token is its argmax;
      3. the first position where `ids` leaves `want` is a near-tie: top-2 margin at most `forced`, or rule gap at most
         `accept`.
    -> [(first divergence or None, what was near there)]."""
    report = []
    for b, seq in enumerate(ids):
        seq = [int(t) for t in seq]
        lg = np.asarray(lg_rows(b, seq), dtype=np.float64)
        ref = [int(t) for t in want[b]]
        n = min(len(seq), len(ref))
        div = next((t for t in range(n) if seq[t] != ref[t]), None if len(seq) == len(ref) else n)
        near = None
        for t in range(prefix_len, len(seq)):
            hist = seq[prefix_len:t]
            if hist and hist[-1] == eos_id:  # the row had finished: padding from here on
                assert all(v == seq[t] for v in seq[t:]), (label, b, t)
                break
            x = lg[t - 1].copy()
            if t == prefix_len and begin_suppress:
                x[list(begin_suppress)] = -np.inf
            y, info = timestamp_rules(x, hist, TIMESTAMP_BEGIN, eos_id, cap, detail=True)
            gap = abs(info["lse"] - info["text_max"]) if np.isfinite(info["lse"]) and np.isfinite(info["text_max"]) else np.inf
            other = info["before"] if info["forced"] else np.where(np.arange(len(x)) < TIMESTAMP_BEGIN, -np.inf, info["before"])
            tok = seq[t]
            ok = y[tok] >= y.max() - accept or (gap <= accept and other[tok] >= other.max() - accept)
            assert ok, (label, b, t, tok, pick(y), gap)
            top2 = np.sort(y[np.isfinite(y)])[-2:]
            margin = float(top2[-1] - top2[0]) if len(top2) == 2 else np.inf
            if gap > forced:
                assert np.isfinite(y[tok]), (label, b, t, tok, "the other side of the log-prob rule", gap)
                if margin > forced:
                    assert tok == pick(y), (label, b, t, tok, pick(y), margin)
            if t == div:
                near = dict(margin=margin, rule_gap=float(gap))
                assert margin <= forced or gap <= accept, (label, b, f"sequences part at position {t}: top-2 margin {margin:.4f}, "
                                                               f"log-prob rule gap {gap:.4f}: neither is a near-tie ({forced}, {accept})")
        assert div is None or div >= prefix_len, (label, b, "the forced prefix differs")
        report.append((div, near))
        print(f"  {label} row {b}: " + ("identical to the reference ids" if div is None else
                                         f"first divergence at token {div} of {len(seq)}: {near}"))
    return report
