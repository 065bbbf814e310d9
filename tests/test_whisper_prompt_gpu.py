"""Whisper prompts and previous-text conditioning on a real MI355X: `generate(prefix_rows=, prefix_start=)` - left-padded
decoder inputs, the padding masked by CaAttnDesc.kstart in the causal prefill and in every token step - against the fp32
restated masked decoder of tests/whisper_prompt_ref.py, window by window on the decoder inputs transformers built
(tests/golden/whisper_prompt.npz), and the public surface on top of it."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_prompt_ref as PR  # noqa: E402
import whisper_ts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Tie margins.  The timestamp tests (tests/test_whisper_ts_gpu.py) use 1.5 x and 3 x a logit error of 0.0256 (accept 0.0384,
# forced 0.0768).  MEASURED_LOGIT_ERROR is the largest |engine - fp32 restated masked decoder| logit over the
# teacher-forced windows of test_logit_error_of_masked_windows..., measured on an MI355X: 0.0278 (these windows are up to
# 128 positions long, the timestamp fixture's 64).  It exceeds 0.0256, so the margins here are the policy's 1.5 x and 3 x
# of the NEW value: accept 0.0417, forced 0.0834.  The test measures it again and fails if it has grown.
TS_LOGIT_ERROR = 0.0256
MEASURED_LOGIT_ERROR = 0.0278
ACCEPT, FORCED = 1.5 * max(TS_LOGIT_ERROR, MEASURED_LOGIT_ERROR), 3 * max(TS_LOGIT_ERROR, MEASURED_LOGIT_ERROR)
_STATE = {}
TS_KW = dict(begin_suppress_tokens=R.BEGIN_SUPPRESS, return_timestamps=True, timestamp_begin=R.TIMESTAMP_BEGIN,
             max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)


def _engine():
    from coral_amd.whisper import WhisperEngine, WhisperShape

    if "eng" not in _STATE:
        eng = WhisperEngine(WhisperShape(**PR.CONFIG), DEV)
        _STATE["P"] = PR.fixture_params()
        eng.load_state_dict(_STATE["P"])
        _STATE.update(eng=eng, mels=PR.features(), z=PR.load_golden(), enc={})
    return _STATE["eng"], _STATE["P"], PR.fixture_config()


def _oracle_enc(batch):
    """The fp32 encoder states of a batch of windows, computed once per window."""
    from oracle import whisper_ref as w

    eng, P, c = _engine()
    for key in batch:
        if key not in _STATE["enc"]:
            with torch.no_grad():
                _STATE["enc"][key] = w.encoder(PR.window_batch(_STATE["mels"], [key]), P, c)[0]
    return torch.stack([_STATE["enc"][k] for k in batch])


def _oracle_rows(att):
    """lg_rows(b, seq) of check_timestamp_rows for the windows of a recorded attempt: the masked decoder on row b's own
    sequence, the row's padding masked."""
    eng, P, c = _engine()
    enc = _oracle_enc(att["batch"])
    start = [int(s) for s in att["start"]] if att["masked"] else [0] * len(att["batch"])

    def rows(b, seq):
        ids = torch.tensor([seq[:-1]])
        mask = torch.arange(ids.shape[1])[None, :] >= start[b]
        with torch.no_grad():
            return PR.masked_decoder(ids, mask, enc[b:b + 1], P, c)[0].numpy()

    return rows, start


def _generate(eng, att, start, **kw):
    feats = PR.window_batch(_STATE["mels"], att["batch"])
    return eng.generate(feats, None, att["max_length"], prefix_rows=torch.from_numpy(att["rows"]).long(),
                        prefix_start=torch.tensor(start, dtype=torch.int32), **TS_KW, **kw)


def _greedy_attempts(run):
    _engine()
    return [a for a in PR.rounds_of(_STATE["z"], run) if a["T"] == 0.0]


@pytest.mark.parametrize("run", ["prev", "all", "fallback"])
def test_windows_decoded_from_the_recorded_decoder_inputs(run):
    """Window by window from the decoder inputs and features transformers had, so a near-tie cannot cascade into later
    prompts: the engine's ids are a greedy path of the fp32 masked decoder under the timestamp rules within the tie
    policy (tests/greedy_check.py, as whisper_ts_ref.check_timestamp_rows applies it under those rules) and leave
    transformers' recorded ids only at a near-tie.  Rows whose log-prob rule is nowhere near a tie also pass
    greedy_check.check_greedy_rows itself on the processed oracle rows."""
    from greedy_check import check_greedy_rows

    eng, P, c = _engine()
    two_pads = cut = False
    plain_rows = 0
    for att in _greedy_attempts(run)[:4]:
        rows, start = _oracle_rows(att)
        Pn = att["rows"].shape[1]
        got = _generate(eng, att, start)
        want = [att["rows"][b].tolist() + att["ids"][b] for b in range(len(att["batch"]))]
        assert [r[:Pn] for r in got] == att["rows"].tolist(), "the rows returned keep the prefix columns given"
        R.check_timestamp_rows(rows, got, want, Pn, ACCEPT, FORCED, label=f"{run} round {att['round']}")
        for b, r in enumerate(got):
            gen = R.strip_row(r, Pn, R.EOS, R.EOS)
            assert R.grammar_ok(gen, R.TIMESTAMP_BEGIN, R.EOS), r
            # check_greedy_rows on the processed rows, where the log-prob rule is clear of a tie all along the row
            seq = r[:Pn + len(gen)]
            lg = np.asarray(rows(b, seq), dtype=np.float64)
            proc, clear = [], True
            for t in range(1, len(seq)):
                x = lg[t - 1].copy()
                if t < Pn:
                    proc.append(x)
                    continue
                if t == Pn:
                    x[list(R.BEGIN_SUPPRESS)] = -np.inf
                y, info = R.timestamp_rules(x, seq[Pn:t], R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX, detail=True)
                if np.isfinite(info["lse"]) and np.isfinite(info["text_max"]) and abs(info["lse"] - info["text_max"]) <= FORCED:
                    clear = False
                proc.append(np.where(np.isfinite(y), y, -1e30))
            if clear:
                check_greedy_rows(lambda _b, _s: torch.from_numpy(np.stack(proc)), [seq], [want[b][:len(seq)]], Pn, ACCEPT, FORCED,
                                  label=f"{run} round {att['round']} row {b}")
                plain_rows += 1
        if att["masked"]:
            two_pads |= len({s for s in start if s > 0}) >= 2
            cut |= any(s == 0 and Pn - len(R.PREFIX) >= PR.CUT_OFF + 1 for s in start)
    print(f"{run}: {plain_rows} rows also through check_greedy_rows")
    assert cut, "no compared window was cut at the cut-off"
    if run == "fallback":
        assert two_pads, "no compared batch had two different non-zero amounts of left padding"


def _teacher_forced(eng, att, start, rows_sel=None):
    """Engine logits of every free position of the recorded windows, teacher-forced on transformers' ids through
    decode_step (prefill with the padding masked, then one token at a time): -> fp32 [B, n, V], and the id rows."""
    sel = list(range(len(att["batch"]))) if rows_sel is None else rows_sel
    batch = [att["batch"][b] for b in sel]
    n = min(len(att["ids"][b]) for b in sel) - 1
    ids = torch.tensor([att["rows"][b].tolist() + att["ids"][b][:n] for b in sel])
    Pn = att["rows"].shape[1]
    kv = eng.cross_kv(eng.encode(PR.window_batch(_STATE["mels"], batch)))
    cache = eng.new_decode_cache(len(sel), Pn + n + 1)
    ks = torch.tensor([start[b] for b in sel], dtype=torch.int32, device=DEV)
    out = [eng.decode_step(ids[:, :Pn], kv, cache, kstart=ks).float().cpu()]
    for t in range(n):
        out.append(eng.decode_step(ids[:, Pn + t:Pn + t + 1], kv, cache, kstart=ks).float().cpu())
    return torch.stack(out, 1), ids


def test_logit_error_of_masked_windows_and_independence_of_the_padding():
    """The figure behind the margins: engine against the fp32 masked decoder, teacher-forced on the recorded ids of the
    first padded round of the `prev` and `fallback` runs (rows with 63, 60 and 0 positions of padding in one batch).  And
    a row decoded alone sees the logits it sees inside the batch that pads it (both padded to one P, so the positions are
    the same) within that figure."""
    eng, P, c = _engine()
    worst = 0.0
    for run in ("prev", "fallback"):
        att = [a for a in _greedy_attempts(run) if a["masked"]][0]
        rows, start = _oracle_rows(att)
        got, ids = _teacher_forced(eng, att, start)
        Pn = att["rows"].shape[1]
        for b in range(len(att["batch"])):
            ref = torch.from_numpy(rows(b, ids[b].tolist() + [0]))[Pn - 1:]
            worst = max(worst, float((got[b] - ref).abs().max()))
    print(f"largest |engine - fp32 masked decoder| teacher-forced logit on the recorded windows: {worst:.4f}")
    assert worst <= MEASURED_LOGIT_ERROR * 1.25 + 1e-3, "the margins were derived from a smaller logit error: measure again"
    assert set(start) >= {0} and len({s for s in start if s > 0}) >= 2
    alone_worst = 0.0
    for b in range(len(att["batch"])):
        alone, _ = _teacher_forced(eng, att, start, [b])
        alone_worst = max(alone_worst, float((alone[0] - got[b, :alone.shape[1]]).abs().max()))
    print(f"a row alone against the row inside its padded batch: {alone_worst:.4f}")
    assert alone_worst <= MEASURED_LOGIT_ERROR


def test_without_the_new_arguments_no_kstart_reaches_the_attention_and_the_launches_stay(monkeypatch):
    """The default path passes kstart=None wherever no prompt is in play; the same rows as unpadded prefix_rows issue the
    same attention launches with a first key of zero, and decode the same ids bit for bit."""
    from coral_amd import ops

    eng, P, c = _engine()
    seen = []
    real = ops._attn_desc

    def spy(*a, **kw):
        d = real(*a, **kw)
        seen.append((d.Tq, d.Tk, d.causal, bool(d.klen), d.kstart is not None))
        return d

    monkeypatch.setattr(ops, "_attn_desc", spy)
    feats = R.short_features()[:2]
    for kw in (dict(), dict(use_graph=False)):
        seen.clear()
        plain = eng.generate(feats, R.PREFIX, R.MAX_LENGTH, **TS_KW, **kw)
        base = list(seen)
        assert base and not any(s[-1] for s in base), "a kstart pointer reached ca_attn_fwd without a prompt"
        seen.clear()
        rows = torch.tensor([R.PREFIX] * 2)
        same = eng.generate(feats, None, R.MAX_LENGTH, prefix_rows=rows, prefix_start=torch.zeros(2, dtype=torch.int32), **TS_KW, **kw)
        assert same == plain
        te = PR.CONFIG.get("max_source_positions", 1500)
        self_attn = [s for s in seen if s[1] != te]
        assert self_attn and all(s[-1] for s in self_attn) and not any(s[-1] for s in seen if s[1] == te)
        if kw:  # launch by launch (under capture the warm-up and the captured steps show, which is the same for both)
            assert [s[:3] for s in seen] == [s[:3] for s in base]
    # the refusals of the new arguments, by name
    rows, st = torch.tensor([R.PREFIX] * 2), torch.zeros(2, dtype=torch.int32)
    for bad, match in ((dict(num_beams=2), "beam"), (dict(use_cache=False), "use_cache"),
                       (dict(prefix_start=torch.tensor([0, 3], dtype=torch.int32)), r"\[0, P"),
                       (dict(prefix_rows=torch.tensor([[R.SOT, R.EOS, R.LANG]] * 2)), "pad id"),
                       (dict(prefix_rows=torch.zeros(2, R.MAX_LENGTH, dtype=torch.int64)), "max_length")):
        args = dict(dict(prefix_rows=rows, prefix_start=st), **bad)
        ts = {} if "num_beams" in bad else TS_KW
        with pytest.raises(ValueError, match=match):
            eng.generate(feats, None, R.MAX_LENGTH, **args, **ts)
    with pytest.raises(ValueError, match="replaces prefix"):
        eng.generate(feats, R.PREFIX, R.MAX_LENGTH, prefix_rows=rows, prefix_start=st, **TS_KW)


def test_public_surface_conditioning_and_prompts(tmp_path):
    """`transcribe_whisper(condition_on_prev_tokens=True)`, with a prompt, with the fallback keys, and
    `generate(prompt_ids=)`: text and chunks on a fixture recording; the loop's windows are those the engine decodes from
    the loop's own decoder inputs."""
    from coral_amd.evaluate import transcribe_whisper
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

    model = WhisperForConditionalGeneration(WhisperShape(**PR.CONFIG), device=DEV).eval()
    model.engine.load_state_dict(PR.fixture_params())
    model.engine.refresh_derived()
    model.generation_config = dict(no_timestamps_token_id=R.NO_TIMESTAMPS, lang_to_id={"<|da|>": R.LANG},
                                   task_to_id={"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE},
                                   max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX, prev_sot_token_id=PR.PREV_SOT)
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    waves = PR.waves()
    long_, short = waves[2], R.short_waves()[0]
    base, base_rows = transcribe_whisper(model, proc, [long_, short], batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True)
    cond, cond_rows = transcribe_whisper(model, proc, [long_, short], batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True,
                                         condition_on_prev_tokens=True)
    for item in cond:
        assert set(item) == {"text", "chunks"} and item["chunks"] and isinstance(item["text"], str)
        for ch in item["chunks"]:
            assert ch["timestamp"][0] <= ch["timestamp"][1]
    assert cond[0]["chunks"][-1]["timestamp"][1] > 30.0
    # the first window has no previous text: it starts as it does without conditioning
    assert cond_rows[0][:4] == base_rows[0][:4]
    assert cond_rows[0] != base_rows[0], "later windows start from the previous text"
    both, _ = transcribe_whisper(model, proc, [long_], batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True,
                                 condition_on_prev_tokens=True, prompt_ids=list(PR.PROMPT), prompt_condition_type="all-segments",
                                 temperature=PR.FALLBACK_TEMPERATURES,
                                 logprob_threshold=float(PR.load_golden()["fallback_logprob_threshold"]))
    assert both[0]["chunks"] and {"avg_logprob", "temperature"} <= set(both[0]["windows"][0])
    feats = proc.feature_extractor([short, R.short_waves()[1]])
    rows = model.generate(feats, max_length=R.MAX_LENGTH, return_timestamps=True, prompt_ids=list(PR.PROMPT))
    assert all(r[:len(R.PREFIX)] == R.PREFIX for r in rows)
    dec = torch.tensor([list(PR.PROMPT) + R.PREFIX] * 2)
    want = model.engine.generate(feats, None, R.MAX_LENGTH + len(PR.PROMPT) + len(R.PREFIX), prefix_rows=dec,
                                 prefix_start=torch.zeros(2, dtype=torch.int32), begin_suppress_tokens=[220, R.EOS],
                                 return_timestamps=True, timestamp_begin=R.TIMESTAMP_BEGIN,
                                 max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)
    assert rows == [R.PREFIX + r[dec.shape[1]:] for r in want]
    assert rows != model.generate(feats, max_length=R.MAX_LENGTH, return_timestamps=True), "the prompt changes what is decoded"
    with pytest.raises(ValueError, match="beam"):
        transcribe_whisper(model, proc, [long_], num_beams=2, condition_on_prev_tokens=True)
    with pytest.raises(ValueError, match="word"):
        transcribe_whisper(model, proc, [long_], return_timestamps="word", prompt_ids=list(PR.PROMPT))
    with pytest.raises(ValueError, match="get_prompt_ids"):
        transcribe_whisper(model, proc, [long_], prompt="Aarhus")
    with pytest.raises(ValueError, match="all-segments"):
        model.generate(feats, prompt_ids=list(PR.PROMPT), prompt_condition_type="all-segments")
