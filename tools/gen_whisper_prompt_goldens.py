"""Write tests/golden/whisper_prompt.npz from the installed transformers (CPU only).

The fixture is that of tests/whisper_prompt_ref.py (the timestamp fixture's model and recipe, three recordings decoded
as one long-form batch).  For every run of RUNS there - previous-text conditioning alone, with a first-segment and an
all-segments prompt, a prompt without conditioning, and conditioning under temperature fallback -
`WhisperForConditionalGeneration.generate(..., return_timestamps=True, return_segments=True)` is recorded attempt by
attempt: the windows (clip, seek), the decoder_input_ids and whether a decoder_attention_mask went with them, max_length,
the generated ids, the statistics of `_need_fallback`, and for the attempts of the first two rounds the logits of the
first free position as the model computed them inside generate; at the end the segments and the padded sequences.

Asserted before anything is written:
  * every branch of BRANCHES (tests/whisper_prompt_ref.py) occurs;
  * `run_longform(conditioning=...)` replaying the recorded windows hands out every recorded decoder input, mask and
    max_length (`prepare_decoder_inputs`, `grown_max_length`) and reproduces seeks and segments of every run;
  * the position-id reading: masked_decoder with positions counted over the PADDED row reproduces the recorded logits
    to 1e-5, and with positions counted from the first valid token it misses them by more than 1e-3 on padded rows.

usage: python tools/gen_whisper_prompt_goldens.py"""
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

import whisper_prompt_ref as PR  # noqa: E402
import whisper_ts_ref as R  # noqa: E402
import gen_whisper_ts_goldens as TS  # noqa: E402  (the timestamp fixture's recipe)

from coral_amd.longform_whisper import FallbackPolicy, run_longform  # noqa: E402

V = R.CONFIG["vocab_size"]
MTP = PR.MAX_TARGET_POSITIONS


def hf_model():
    """gen_whisper_ts_goldens.hf_model with the target positions of this fixture: the recipe is imported, the two things
    it reads from whisper_ts_ref are pointed at this fixture while it runs."""
    keep = R.CONFIG, R.fixture_params
    R.CONFIG, R.fixture_params = PR.CONFIG, PR.fixture_params
    try:
        return TS.hf_model()
    finally:
        R.CONFIG, R.fixture_params = keep


class Recorder:
    def __init__(self, model):
        self.model, self.attempts, self.round = model, [], -1
        self.prefill = []

    def with_fallback(self, orig):
        rec = self

        def call(*a, **kw):
            rec.round += 1
            seeks = [int(t) for t in kw["seek"]]
            batch = [(int(c), seeks[int(c)]) for c in kw["batch_idx_map"]]
            dec = kw["decoder_input_ids"].clone()
            mask = kw["kwargs"].get("decoder_attention_mask")
            if mask is not None:
                assert torch.equal(mask, dec != R.EOS)
            rec.cur = dict(batch=batch, dec=dec, masked=mask is not None, max_length=int(kw["generation_config"].max_length),
                           keys=list(range(len(batch))), attempt=0)
            res = orig(*a, **kw)
            rec.final = [[int(t) for t in s] for s in res[0]]
            return res

        return call

    def need_fallback(self, orig):
        rec = self

        def call(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
            needs, skip = orig(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
            assert not skip
            cur = rec.cur
            if index == 0:
                keys = cur["keys"]
                rec.attempts.append(dict(round=rec.round, attempt=cur["attempt"], T=float(temperature or 0.0),
                                         batch=[cur["batch"][j] for j in keys], dec=cur["dec"][keys], masked=cur["masked"],
                                         max_length=cur["max_length"], rows=[], logits=rec.prefill.pop(0)))
                rec.prefill.clear()
                cur["attempt"] += 1
                cur["next"] = []
            att = rec.attempts[-1]
            seq = [int(t) for t in seek_sequence.tolist()]
            avg, n = float("nan"), 0
            if isinstance(seek_outputs[index], dict) and "scores" in seek_outputs[index]:
                scores = seek_outputs[index]["scores"]
                avg = float(rec.model._retrieve_avg_logprobs(scores, seek_sequence, temperature))
                n = min(len(scores), len(seq))
            att["rows"].append(dict(ids=seq, avg=avg, n=n, needs=bool(needs)))
            if needs:
                cur["next"].append(cur["keys"][index])
            if index == len(cur["keys"]) - 1:
                cur["keys"] = cur["next"]
            return needs, skip

        return call

    def forward(self, orig):
        rec = self

        def call(*a, **kw):
            out = orig(*a, **kw)
            ids = kw.get("decoder_input_ids")
            if ids is not None and ids.shape[1] > 1:  # a pass over the whole decoder input: generate's first step
                rec.prefill.append(out.logits[:, -1].detach().clone())
            return out

        return call


def run_hf(mels, args):
    model = hf_model()
    gc = model.generation_config
    gc.top_k, gc.top_p = 0, 1.0
    gc.prev_sot_token_id = PR.PREV_SOT
    rec = Recorder(model)
    frames = [m.shape[1] for m in mels]
    T = max(frames)
    feats = torch.stack([torch.nn.functional.pad(m, (0, T - m.shape[1])) for m in mels])
    mask = torch.zeros(len(mels), T, dtype=torch.long)
    for b, n in enumerate(frames):
        mask[b, :n] = 1
    model._need_fallback = rec.need_fallback(model._need_fallback)
    model.generate_with_fallback = rec.with_fallback(model.generate_with_fallback)
    model.forward = rec.forward(model.forward)
    kw = dict(args)
    if kw.get("prompt_ids") is not None:
        kw["prompt_ids"] = torch.tensor(kw["prompt_ids"])
    torch.manual_seed(1234)
    with torch.no_grad():
        res = model.generate(feats, attention_mask=mask, return_timestamps=True, return_segments=True, language="danish",
                             task="transcribe", **kw)
    return rec, res, frames


def replay(rec, frames, run, fallback):
    """run_longform(conditioning=...) fed with the recorded attempts; every decoder input it prepares is checked."""
    it = iter(rec.attempts)

    def check(batch, inputs, att):
        assert list(batch) == att["batch"], (batch, att["batch"])
        assert inputs["rows"] == att["dec"].tolist(), (run, att["round"], inputs["rows"], att["dec"].tolist())
        assert inputs["masked"] == att["masked"]
        assert [r.count(R.EOS) for r in inputs["rows"]] == inputs["start"] or not att["masked"]
        assert inputs["max_length"] == att["max_length"], (inputs["max_length"], att["max_length"])
        return [inputs["rows"][i] + r["ids"] for i, r in enumerate(att["rows"])]

    def plain(batch, inputs):
        att = next(it)
        return check(batch, inputs, att)

    def scored(batch, temperature, uniforms, inputs):
        att = next(it)
        assert temperature == att["T"]
        rows = check(batch, inputs, att)
        return rows, dict(sum_logprob=[r["avg"] * r["n"] for r in att["rows"]], n_scored=[r["n"] for r in att["rows"]],
                          no_speech_prob=None)

    out = run_longform(scored if fallback else plain, frames, R.TIMESTAMP_BEGIN, len(R.PREFIX), R.EOS, R.EOS,
                       fallback=fallback, vocab_size=V, max_length=R.MAX_LENGTH, conditioning=PR.policy_of(run),
                       init_tokens=R.PREFIX, max_target_positions=MTP)
    assert next(it, None) is None, "the restated loop asked for fewer attempts than transformers ran"
    return out


def branches(recs):
    seen = set()
    for run, rec in recs.items():
        sizes = [len(a["batch"]) for a in rec.attempts if a["attempt"] == 0]
        if any(b < a for a, b in zip(sizes, sizes[1:])):
            seen.add("batch_shrinks")
        hot = {}  # index within the last round -> accepted there at a temperature >= 0.5
        for a in rec.attempts:
            pads = (a["dec"] == R.EOS).sum(1).tolist() if a["masked"] else [0] * len(a["batch"])
            plen = a["dec"].shape[1] - len(R.PREFIX)
            if a["round"] == 0 and a["attempt"] == 0 and not a["masked"] and plen == 0:
                seen.add("first_window_without_prev")
            if len({p for p in pads if p > 0}) >= 2:
                seen.add("different_padding_in_a_batch")
            lead = len(PR.PROMPT) if run == "all" else 1
            if a["masked"] and any(p == 0 and plen == PR.CUT_OFF + lead for p in pads):
                seen.add("cut_at_cut_off")
            if run == "first" and a["round"] == 0 and a["dec"][0, :plen].tolist() == [PR.PREV_SOT] + list(PR.PROMPT[1:]):
                seen.add("first_segment_prompt")
            if run == "all" and a["round"] > 0 and a["dec"][0, :len(PR.PROMPT)].tolist() == list(PR.PROMPT):
                seen.add("all_segments_prompt")
            if run != "fallback":
                continue
            if a["attempt"] == 0:
                # the flag is read at the clip's own index (and was written at the row's index within its round)
                for j, (clip, _) in enumerate(a["batch"]):
                    if hot.get(clip) and a["masked"] and pads[j] == plen - 1 and max(pads) > min(pads):
                        seen.add("unconditioned_after_hot_fallback")
                keys = list(range(len(a["batch"])))
            for j, r in zip(keys, a["rows"]):
                hot[j] = a["T"] >= 0.5
            keys = [j for j, r in zip(keys, a["rows"]) if r["needs"]]
    return seen


def main():
    mels = PR.features()
    params, cfg = PR.fixture_params(), PR.fixture_config()
    from oracle import whisper_ref as w

    recs, results = {}, {}
    out = dict(recipe=np.array(json.dumps(R.RECIPE)), frames=np.array([m.shape[1] for m in mels], dtype=np.int64),
               prompt=np.array(PR.PROMPT, dtype=np.int64))
    for run, args in PR.RUNS.items():
        args = dict(args)
        if run == "fallback":
            # a threshold inside the greedy windows' range of average log-probabilities (its lower third): most pass, the
            # others are sampled at 0.6 and accepted there (the last temperature)
            probe, _, _ = run_hf(mels, dict(args, logprob_threshold=-1e9))
            avgs = sorted(r["avg"] for a in probe.attempts for r in a["rows"])
            k = int(len(avgs) * 0.3)
            args["logprob_threshold"] = float((avgs[k - 1] + avgs[k]) / 2)
            out["fallback_logprob_threshold"] = np.array(args["logprob_threshold"])
        rec, res, frames = run_hf(mels, args)
        recs[run], results[run] = rec, res
        print(f"{run}: {rec.round + 1} rounds, {len(rec.attempts)} attempts, P per attempt "
              f"{[a['dec'].shape[1] for a in rec.attempts]}, max_length {[a['max_length'] for a in rec.attempts]}", flush=True)
    seen = branches(recs)
    tb = R.TIMESTAMP_BEGIN
    for run, res in results.items():
        if any(len(s["tokens"]) > 2 and int(s["tokens"][-2]) >= tb for segs in res["segments"] for s in segs):
            seen.add("double_timestamp_ending")
    print("branches:", sorted(seen))
    assert seen >= set(PR.BRANCHES), set(PR.BRANCHES) - seen

    worst_ok, worst_other = 0.0, np.inf
    for run, rec in recs.items():
        res = results[run]
        fb = None
        if run == "fallback":
            fb = FallbackPolicy(PR.FALLBACK_TEMPERATURES, float(out["fallback_logprob_threshold"]), None, None, None, 0)
        mine = replay(rec, frames, run, fb)
        for b, segs in enumerate(res["segments"]):
            toks = [[int(t) for t in s["tokens"]] for s in segs]
            assert [s[2] for s in mine[b]["segments"]] == toks, (run, b)
            assert [s[0] for s in mine[b]["segments"]] == [float(s["start"]) for s in segs], (run, b)
            assert [s[1] for s in mine[b]["segments"]] == [float(s["end"]) for s in segs], (run, b)
            seeks = [k[1] for a in rec.attempts if a["attempt"] == 0 for k in a["batch"] if k[0] == b]
            assert [wd[0] for wd in mine[b]["windows"]] == seeks, (run, b)
            Ls = max([len(t) for t in toks] + [1])
            out[f"{run}_clip{b}_seg_start"] = np.array([float(s["start"]) for s in segs], dtype=np.float64)
            out[f"{run}_clip{b}_seg_end"] = np.array([float(s["end"]) for s in segs], dtype=np.float64)
            out[f"{run}_clip{b}_seg_len"] = np.array([len(t) for t in toks], dtype=np.int64)
            out[f"{run}_clip{b}_seg_ids"] = np.array([t + [-1] * (Ls - len(t)) for t in toks], dtype=np.int64).reshape(len(toks), Ls)
        out[f"{run}_sequences"] = res["sequences"].numpy().astype(np.int64)
        # the attempts, flat over their rows
        meta, dec, gen, avg, n, needs, lrow, lg = [], [], [], [], [], [], [], []
        pmax = max(a["dec"].shape[1] for a in rec.attempts)
        r0 = 0
        for k, a in enumerate(rec.attempts):
            P = a["dec"].shape[1]
            meta.append(dict(round=a["round"], attempt=a["attempt"], T=a["T"], batch=a["batch"], P=P, masked=a["masked"],
                             max_length=a["max_length"]))
            pads = (a["dec"] == R.EOS).sum(1).tolist() if a["masked"] else [0]
            keep_logits = a["round"] < 2  # (the first window and the first padded round of every run)
            # the position-id reading, against the logits generate computed
            enc = w.encoder(PR.window_batch(mels, a["batch"]), params, cfg)
            m = a["dec"] != R.EOS if a["masked"] else torch.ones_like(a["dec"], dtype=torch.bool)
            with torch.no_grad():
                padded = PR.masked_decoder(a["dec"], m, enc, params, cfg)[:, -1]
                other = PR.masked_decoder(a["dec"], m, enc, params, cfg, positions="mask")[:, -1]
            err = float((padded - a["logits"]).abs().max())
            worst_ok = max(worst_ok, err)
            assert err <= 1e-5, (run, a["round"], err)
            for j, pd in enumerate(pads if a["masked"] else []):
                if pd > 0:
                    worst_other = min(worst_other, float((other[j] - a["logits"][j]).abs().max()))
            if keep_logits:
                lrow.append(r0)
                lg.append(a["logits"].numpy().astype(np.float32))
            for j, r in enumerate(a["rows"]):
                dec.append(a["dec"][j].tolist() + [-1] * (pmax - P))
                gen.append(r["ids"])
                avg.append(r["avg"])
                n.append(r["n"])
                needs.append(r["needs"])
            r0 += len(a["rows"])
        L = max(len(g) for g in gen)
        out[f"{run}_meta"] = np.array(json.dumps(meta))
        out[f"{run}_dec_ids"] = np.array(dec, dtype=np.int64)
        out[f"{run}_gen_len"] = np.array([len(g) for g in gen], dtype=np.int64)
        out[f"{run}_gen_ids"] = np.array([g + [-1] * (L - len(g)) for g in gen], dtype=np.int64)
        out[f"{run}_avg_logprob"] = np.array(avg, dtype=np.float64)
        out[f"{run}_n_scored"] = np.array(n, dtype=np.int64)
        out[f"{run}_needs"] = np.array(needs, dtype=bool)
        out[f"{run}_logits_row"] = np.array(lrow, dtype=np.int64)
        out[f"{run}_logits"] = np.concatenate(lg).astype(np.float32)
    print(f"position ids: padded-row positions reproduce generate's first-step logits to {worst_ok:.2e}; positions counted "
          f"from the first valid token miss them by at least {worst_other:.2e} on every padded row")
    assert worst_other > 1e-3
    out["position_check"] = np.array([worst_ok, worst_other])
    out["branches"] = np.array(json.dumps(sorted(seen)))
    np.savez_compressed(PR.GOLDEN, **out)
    print(PR.GOLDEN.name, PR.GOLDEN.stat().st_size, "bytes")
    assert PR.GOLDEN.stat().st_size < 500_000


if __name__ == "__main__":
    main()
