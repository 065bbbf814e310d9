"""Write tests/golden/whisper_fallback.npz from the installed transformers (CPU only).

transformers' own long-form `generate(..., temperature=(0.0, 0.05, 0.2, 0.4), logprob_threshold, compression_ratio_threshold,
no_speech_threshold)` runs on the timestamp fixture model (tests/whisper_ts_ref.py) over a batch of recordings.  Inside
this tool only, `torch.multinomial` is replaced by this project's sampler definition (tests/whisper_fallback_ref.py
`sample_pick`: inverse CDF in float64 over the processed row before the temperature warper) on uniforms drawn as
`run_longform` draws them: one CPU generator seeded once, torch.rand(rows of the attempt, max_length) per sampled attempt, the
uniform of position p in column p.  So transformers' loop runs under the sampler the kernel implements.

Recorded: every round's windows, every attempt (temperature, rows, ids, average log-probability and its token count,
compression ratio, no-speech probability, the two flags of `_need_fallback`), the final segments, and about 40 sampled
steps (processed row, history, u, pick).  The thresholds are chosen here from a first run that takes every window through
every temperature, so that each branch of the loop occurs; each is asserted before the file is written, and so is that
`run_longform(fallback=...)` replaying the record reproduces it.

usage: python tools/gen_whisper_fallback_goldens.py"""
from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import whisper_fallback_ref as F  # noqa: E402
import whisper_ts_ref as R  # noqa: E402
from coral_amd.longform_whisper import FallbackPolicy, run_longform  # noqa: E402
from gen_whisper_ts_goldens import hf_model  # noqa: E402

P = len(R.PREFIX)
V = R.CONFIG["vocab_size"]


class Recorder:
    """The hooks into transformers: the sampler, the per-attempt statistics, the rounds."""

    def __init__(self, model):
        self.model = model
        self.gen = torch.Generator().manual_seed(F.SEED)
        self.rounds = []      # dict(batch=[(clip, seek)], attempts=[dict(T, rows=[dict(...)])], skip=[...], final=[ids])
        self.cases = []       # sampled steps
        self.pre = None       # (processed scores before the temperature, input length, temperature)
        self.uniforms = None

    # -- the sampler --
    def warper_call(self, orig):
        rec = self

        def call(warper, input_ids, scores):
            if input_ids.shape[1] == P:  # a sampled attempt begins: its uniforms
                rec.uniforms = torch.rand(input_ids.shape[0], R.MAX_LENGTH, generator=rec.gen)
            rec.pre = (scores.detach().clone(), input_ids.detach().clone(), float(warper.temperature))
            return orig(warper, input_ids, scores)

        return call

    def multinomial(self, probs, num_samples=1, **kw):
        assert num_samples == 1 and self.pre is not None
        scores, input_ids, T = self.pre
        assert scores.shape == probs.shape
        inv_t = float(np.float32(1.0 / T))
        pos = input_ids.shape[1]
        out = []
        for r in range(scores.shape[0]):
            row = scores[r].double().numpy()
            heavy = np.isfinite(row) & ((row - row[np.isfinite(row)].max()) * inv_t > -60.0)
            assert (probs[r].numpy()[~np.isfinite(row)] == 0).all() and (probs[r].numpy()[heavy] > 0).all(), \
                "another warper (top-k, top-p) is active"
            u = float(self.uniforms[r, pos])
            tok = F.sample_pick(row, inv_t, u)
            out.append(tok)
            hist = input_ids[r, P:].tolist()
            if R.EOS not in hist:
                self.cases.append(dict(row=scores[r].numpy().copy(), hist=hist, u=np.float32(u), inv_t=np.float32(inv_t),
                                       pick=tok, single=len(F.acceptable(row, inv_t, u)) == 1))
        self.pre = None
        return torch.tensor(out, dtype=torch.int64)[:, None]

    # -- the statistics --
    def need_fallback(self, orig):
        rec = self

        def call(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
            needs, skip = orig(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
            rnd = rec.rounds[-1]
            if index == 0:
                rnd["attempts"].append(dict(T=float(temperature or 0.0), rows=[]))
            seq = [int(t) for t in seek_sequence.tolist()]
            scores = seek_outputs[index]["scores"]
            avg = float(rec.model._retrieve_avg_logprobs(scores, seek_sequence, temperature))
            n = min(len(scores), len(seq))
            nsp = float("nan")
            for p in logits_processor:
                if type(p).__name__ == "WhisperNoSpeechDetection":
                    nsp = float(p.no_speech_prob[index])
            rnd["attempts"][-1]["rows"].append(dict(ids=seq, avg=avg, n=n, ratio=float(F.compression_ratio(seq, vocab_size)),
                                                    nsp=nsp, needs=bool(needs), skip=bool(skip)))
            assert F.compression_ratio(seq, vocab_size) == rec.model._retrieve_compression_ratio(seek_sequence, vocab_size)
            return needs, skip

        return call

    def with_fallback(self, orig):
        rec = self

        def call(*a, **kw):
            seeks = [int(t) for t in kw["seek"]]
            rec.rounds.append(dict(batch=[(int(c), seeks[int(c)]) for c in kw["batch_idx_map"]], attempts=[]))
            res = orig(*a, **kw)
            rec.rounds[-1]["skip"] = [bool(x) for x in res[2]]
            rec.rounds[-1]["final"] = [[int(t) for t in s] for s in res[0]]
            return res

        return call


def recordings():
    waves = R.long_waves() + [R.fixture_wave(48.0, 802), R.fixture_wave(33.0, 803)]
    from oracle import whisper_ref as w

    return [torch.from_numpy(w.log_mel(a)) for a in waves]


def run_hf(mels, thresholds):
    """One long-form generate over the batch -> (Recorder, segments per clip)."""
    from transformers.generation import logits_process as lp

    model = hf_model()
    model.generation_config.top_k = 0      # (the defaults, 50 and 1.0, would cut the distribution the loop samples from)
    model.generation_config.top_p = 1.0
    rec = Recorder(model)
    frames = [m.shape[1] for m in mels]
    T = max(frames)
    feats = torch.stack([torch.nn.functional.pad(m, (0, T - m.shape[1])) for m in mels])
    mask = torch.zeros(len(mels), T, dtype=torch.long)
    for b, n in enumerate(frames):
        mask[b, :n] = 1
    orig_call, orig_multi = lp.TemperatureLogitsWarper.__call__, torch.multinomial
    lp.TemperatureLogitsWarper.__call__ = rec.warper_call(orig_call)
    torch.multinomial = rec.multinomial
    model._need_fallback = rec.need_fallback(model._need_fallback)
    model.generate_with_fallback = rec.with_fallback(model.generate_with_fallback)
    try:
        with torch.no_grad():
            res = model.generate(feats, attention_mask=mask, return_timestamps=True, return_segments=True, language="danish",
                                 task="transcribe", temperature=F.TEMPERATURES, condition_on_prev_tokens=False, **thresholds)
    finally:
        lp.TemperatureLogitsWarper.__call__, torch.multinomial = orig_call, orig_multi
    return rec, res["segments"], frames


def attempt_keys(rnd):
    """The (clip, seek) rows of every attempt of a round: all, then those that needed a fallback, in order."""
    keys, out = list(rnd["batch"]), []
    for att in rnd["attempts"]:
        assert len(att["rows"]) == len(keys), (len(att["rows"]), keys)
        out.append(list(keys))
        keys = [k for k, r in zip(keys, att["rows"]) if r["needs"]]
    return out


def branches(rec, thr):
    seen = set()
    last_t = F.TEMPERATURES[-1]
    for rnd in rec.rounds:
        keys = attempt_keys(rnd)
        if len(keys) > 1 and 0 < len(keys[1]) < len(keys[0]):
            seen.add("partial_batch")
        fate = {}
        for ks, att in zip(keys, rnd["attempts"]):
            for k, r in zip(ks, att["rows"]):
                fate.setdefault(k, []).append((att["T"], r))
        for k, steps in fate.items():
            t0, r0 = steps[0]
            if not r0["needs"] and not r0["skip"]:
                seen.add("accepted_at_0")
            by_lp = r0["avg"] < thr["logprob_threshold"] and r0["ratio"] <= thr["compression_ratio_threshold"]
            if r0["needs"] and by_lp and any(not r["needs"] and not r["skip"] for _, r in steps[1:]):
                seen.add("logprob_then_accepted")
            if any(r["needs"] and r["ratio"] > thr["compression_ratio_threshold"] for _, r in steps):
                seen.add("compression_ratio")
            if steps[-1][0] == last_t and steps[-1][1]["needs"]:
                seen.add("exhausted")
        if any(rnd["skip"]):
            seen.add("skipped")
    return seen


def clear_of_thresholds(rec, thr) -> bool:
    """No decision of the record sits on a threshold: the replay rebuilds an average from sum and count (a rounding), and
    a reader should not have to wonder."""
    rows = [r for rnd in rec.rounds for att in rnd["attempts"] for r in att["rows"]]
    return all(abs(r["avg"] - thr["logprob_threshold"]) > 1e-4 and abs(r["ratio"] - thr["compression_ratio_threshold"]) > 1e-4
               and abs(r["nsp"] - thr["no_speech_threshold"]) > 1e-4 * thr["no_speech_threshold"] for r in rows)


BRANCHES = ("accepted_at_0", "logprob_then_accepted", "compression_ratio", "exhausted", "skipped", "partial_batch")


def replay(rec, frames, policy):
    """run_longform(fallback=policy) fed with the recorded attempts."""
    flat = [(ks, att) for rnd in rec.rounds for ks, att in zip(attempt_keys(rnd), rnd["attempts"])]
    gen = torch.Generator().manual_seed(F.SEED)
    it = iter(flat)

    def window_generate(batch, temperature, uniforms):
        ks, att = next(it)
        assert list(batch) == ks and temperature == att["T"], (batch, ks, temperature, att["T"])
        if temperature > 0:
            assert torch.equal(uniforms, torch.rand(len(batch), R.MAX_LENGTH, generator=gen))
        else:
            assert uniforms is None
        rows = [R.PREFIX + r["ids"] for r in att["rows"]]
        return rows, dict(sum_logprob=[r["avg"] * r["n"] for r in att["rows"]], n_scored=[r["n"] for r in att["rows"]],
                          no_speech_prob=[r["nsp"] for r in att["rows"]])

    out = run_longform(window_generate, frames, R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS, fallback=policy, vocab_size=V,
                       max_length=R.MAX_LENGTH)
    assert next(it, None) is None, "the restated loop asked for fewer attempts than transformers ran"
    return out


def main():
    torch.manual_seed(0)
    mels = recordings()
    # a first run that takes every window through every temperature: what the statistics look like
    probe, _, frames = run_hf(mels, dict(logprob_threshold=1e9, compression_ratio_threshold=1e9, no_speech_threshold=None))
    rows = [(att["T"], r) for rnd in probe.rounds for att in rnd["attempts"] for r in att["rows"]]
    print(f"probe: {len(probe.rounds)} rounds, {len(rows)} decoded windows")
    for t in F.TEMPERATURES:
        a = [r["avg"] for tt, r in rows if tt == t]
        c = [r["ratio"] for tt, r in rows if tt == t]
        print(f"  T={t}: avg logprob {min(a):.3f} .. {max(a):.3f}, compression ratio {min(c):.3f} .. {max(c):.3f}")

    def cuts(vals, qs):
        v = np.unique(np.round(np.asarray(vals, dtype=np.float64), 6))
        mids = (v[1:] + v[:-1]) / 2
        return [float(mids[min(len(mids) - 1, int(q * len(mids)))]) for q in qs]

    # greedy windows of this model loop (high compression ratio, the best log-probabilities); sampled ones do not.  So
    # both thresholds are cut inside the greedy windows' range: some pass at temperature 0, the others fall back.
    lp_c = cuts([r["avg"] for t, r in rows if t == 0.0], (0.5, 0.65, 0.35, 0.8, 0.2, 0.9))
    cr_c = cuts([r["ratio"] for t, r in rows if t == 0.0], (0.5, 0.75))
    chosen = None
    for lp_t, cr_t in itertools.product(lp_c, cr_c):
        first = run_hf(mels, dict(logprob_threshold=lp_t, compression_ratio_threshold=cr_t, no_speech_threshold=1e9))[0]
        nsp = [r["nsp"] for rnd in first.rounds for att in rnd["attempts"][:1] for r in att["rows"] if r["avg"] < lp_t]
        for ns_t in (cuts(nsp, (0.7, 0.4)) if len(set(nsp)) > 1 else []):
            thr = dict(logprob_threshold=lp_t, compression_ratio_threshold=cr_t, no_speech_threshold=ns_t)
            rec, segments, frames = run_hf(mels, thr)
            seen = branches(rec, thr)
            print(f"  thresholds {thr}: {sorted(seen)}", flush=True)
            if seen >= set(BRANCHES) and clear_of_thresholds(rec, thr):
                chosen = (thr, rec, segments)
                break
        if chosen:
            break
    assert chosen is not None, "no threshold set takes every branch: change the recordings or the recipe"
    thr, rec, segments = chosen
    policy = FallbackPolicy(F.TEMPERATURES, thr["logprob_threshold"], thr["compression_ratio_threshold"],
                            thr["no_speech_threshold"], F.NO_SPEECH_TOKEN, F.SEED)
    mine = replay(rec, frames, policy)
    out = dict(recipe=np.array(json.dumps(R.RECIPE)), temperatures=np.array(F.TEMPERATURES), seed=np.array(F.SEED),
               thresholds=np.array([thr["logprob_threshold"], thr["compression_ratio_threshold"], thr["no_speech_threshold"]]),
               frames=np.array(frames, dtype=np.int64), branches=np.array(json.dumps(sorted(branches(rec, thr)))))
    for b, segs in enumerate(segments):
        toks = [[int(t) for t in s["tokens"]] for s in segs]
        starts = [float(s["start"]) for s in segs]
        ends = [float(s["end"]) for s in segs]
        assert [s[2] for s in mine[b]["segments"]] == toks, b
        assert [s[0] for s in mine[b]["segments"]] == starts and [s[1] for s in mine[b]["segments"]] == ends, b
        Ls = max([len(t) for t in toks] + [1])
        out[f"clip{b}_seg_start"], out[f"clip{b}_seg_end"] = np.array(starts, dtype=np.float64), np.array(ends, dtype=np.float64)
        out[f"clip{b}_seg_len"] = np.array([len(t) for t in toks], dtype=np.int64)
        out[f"clip{b}_seg_ids"] = np.array([t + [-1] * (Ls - len(t)) for t in toks], dtype=np.int64).reshape(len(toks), Ls)
        seeks = [k[1] for rnd in rec.rounds for k in rnd["batch"] if k[0] == b]
        assert [w["seek"] for w in mine[b]["window_stats"]] == seeks
        skips = [sk for rnd in rec.rounds for k, sk in zip(rnd["batch"], rnd["skip"]) if k[0] == b]
        assert [w["skipped"] for w in mine[b]["window_stats"]] == skips
        out[f"clip{b}_seek"], out[f"clip{b}_skip"] = np.array(seeks, dtype=np.int64), np.array(skips, dtype=bool)
    # the attempts, flat
    att = [(ri, ai, a["T"], k, r) for ri, rnd in enumerate(rec.rounds)
           for ai, (ks, a) in enumerate(zip(attempt_keys(rnd), rnd["attempts"])) for k, r in zip(ks, a["rows"])]
    L = max(len(r["ids"]) for *_, r in att)
    out["att_round"] = np.array([a[0] for a in att], dtype=np.int64)
    out["att_index"] = np.array([a[1] for a in att], dtype=np.int64)
    out["att_T"] = np.array([a[2] for a in att], dtype=np.float64)
    out["att_clip"] = np.array([a[3][0] for a in att], dtype=np.int64)
    out["att_seek"] = np.array([a[3][1] for a in att], dtype=np.int64)
    out["att_len"] = np.array([len(a[4]["ids"]) for a in att], dtype=np.int64)
    out["att_ids"] = np.array([a[4]["ids"] + [-1] * (L - len(a[4]["ids"])) for a in att], dtype=np.int64)
    for name, key, dt in (("att_avg_logprob", "avg", np.float64), ("att_n", "n", np.int64), ("att_ratio", "ratio", np.float64),
                          ("att_nsp", "nsp", np.float64), ("att_needs", "needs", bool), ("att_skip", "skip", bool)):
        out[name] = np.array([a[4][key] for a in att], dtype=dt)
    # the sampled steps: a spread over temperatures and history lengths
    cases = rec.cases
    step = max(1, len(cases) // 40)
    cases = cases[::step][:40]
    single = sum(c["single"] for c in cases)
    print(f"{len(rec.cases)} sampled steps, {len(cases)} recorded, {single} with a one-token acceptance set")
    assert len(cases) >= 30 and single >= 0.9 * len(cases)
    Lh = max(len(c["hist"]) for c in cases)
    out["case_row"] = np.stack([c["row"] for c in cases]).astype(np.float32)
    out["case_hist_len"] = np.array([len(c["hist"]) for c in cases], dtype=np.int64)
    out["case_hist"] = np.array([c["hist"] + [-1] * (Lh - len(c["hist"])) for c in cases], dtype=np.int64)
    out["case_u"] = np.array([c["u"] for c in cases], dtype=np.float32)
    out["case_inv_t"] = np.array([c["inv_t"] for c in cases], dtype=np.float32)
    out["case_pick"] = np.array([c["pick"] for c in cases], dtype=np.int64)
    np.savez_compressed(F.GOLDEN, **out)
    print(F.GOLDEN.name, F.GOLDEN.stat().st_size, "bytes; thresholds", thr)
    assert F.GOLDEN.stat().st_size < 1_000_000


if __name__ == "__main__":
    main()
