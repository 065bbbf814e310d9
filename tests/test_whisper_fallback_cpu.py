"""Whisper temperature fallback without a GPU: `run_longform(fallback=...)` against transformers' own recorded run
(tests/golden/whisper_fallback.npz, tools/gen_whisper_fallback_goldens.py: every round, attempt, flag, skip, seek and
segment), the restated statistics, the C ABI of the two new launches, and what stays refused."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_fallback_ref as F  # noqa: E402
import whisper_ts_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
P = len(R.PREFIX)
V = R.CONFIG["vocab_size"]


def _policy(z):
    from coral_amd.longform_whisper import FallbackPolicy

    lp, cr, ns = z["thresholds"].tolist()
    assert tuple(z["temperatures"].tolist()) == F.TEMPERATURES and int(z["seed"]) == F.SEED
    return FallbackPolicy(F.TEMPERATURES, lp, cr, ns, F.NO_SPEECH_TOKEN, F.SEED)


def _attempts(z):
    """[(keys, temperature, rows)] in the order transformers ran them; rows: dict per decoded window."""
    out = []
    for i in range(len(z["att_round"])):
        key = (int(z["att_round"][i]), int(z["att_index"][i]))
        if not out or out[-1][0] != key:
            out.append((key, float(z["att_T"][i]), []))
        out[-1][2].append(dict(key=(int(z["att_clip"][i]), int(z["att_seek"][i])), ids=z["att_ids"][i, :int(z["att_len"][i])].tolist(),
                               avg=float(z["att_avg_logprob"][i]), n=int(z["att_n"][i]), ratio=float(z["att_ratio"][i]),
                               nsp=float(z["att_nsp"][i]), needs=bool(z["att_needs"][i]), skip=bool(z["att_skip"][i])))
    return out


def _replay(z, policy, seen=None):
    from coral_amd.longform_whisper import run_longform

    it = iter(_attempts(z))
    gen = torch.Generator().manual_seed(F.SEED)

    def window_generate(batch, temperature, uniforms):
        key, T, rows = next(it)
        assert list(batch) == [r["key"] for r in rows], (key, batch)
        assert temperature == T
        if T > 0:  # the uniforms of the attempt: drawn in order from the one seeded generator
            assert uniforms.dtype == torch.float32 and torch.equal(uniforms, torch.rand(len(batch), R.MAX_LENGTH, generator=gen))
        else:
            assert uniforms is None
        if seen is not None:
            seen.append((key, T, [r["key"] for r in rows]))
        return [R.PREFIX + r["ids"] for r in rows], dict(sum_logprob=[r["avg"] * r["n"] for r in rows],
                                                         n_scored=[r["n"] for r in rows], no_speech_prob=[r["nsp"] for r in rows])

    out = run_longform(window_generate, z["frames"].tolist(), R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS, fallback=policy, vocab_size=V,
                       max_length=R.MAX_LENGTH)
    assert next(it, None) is None, "transformers ran attempts the restated loop did not ask for"
    return out


def test_loop_replays_transformers_attempts_skips_seeks_and_segments():
    z = F.load_golden()
    policy = _policy(z)
    seen = []
    out = _replay(z, policy, seen)
    assert len(seen) == len(_attempts(z)) > len(set(k[0] for k, _, _ in seen))  # some round took more than one attempt
    for b in range(len(z["frames"])):
        stats = out[b]["window_stats"]
        assert [w["seek"] for w in stats] == z[f"clip{b}_seek"].tolist()
        assert [w["skipped"] for w in stats] == z[f"clip{b}_skip"].tolist()
        want = [ids[:k].tolist() for ids, k in zip(z[f"clip{b}_seg_ids"], z[f"clip{b}_seg_len"])]
        assert [s[2] for s in out[b]["segments"]] == want
        assert [s[0] for s in out[b]["segments"]] == z[f"clip{b}_seg_start"].tolist()  # equal as floats
        assert [s[1] for s in out[b]["segments"]] == z[f"clip{b}_seg_end"].tolist()
    # the kept row of a window is the one of the last attempt it took part in, at that attempt's temperature
    last = {}
    for _, T, rows in _attempts(z):
        for r in rows:
            last[r["key"]] = (T, r)
    for b in range(len(z["frames"])):
        for (seek, gen), w in zip(out[b]["windows"], out[b]["window_stats"]):
            T, r = last[(b, seek)]
            assert w["temperature"] == T and gen == [t for t in r["ids"] if t != R.EOS]
            assert w["compression_ratio"] == r["ratio"]  # equal as floats
            assert abs(w["avg_logprob"] - r["avg"]) <= 1e-12 * abs(r["avg"])


def test_statistics_and_flags_of_every_recorded_attempt():
    from coral_amd.longform_whisper import compression_ratio, need_fallback

    z = F.load_golden()
    policy = _policy(z)
    for _, T, rows in _attempts(z):
        for r in rows:
            assert compression_ratio(r["ids"], V) == r["ratio"] == F.compression_ratio(r["ids"], V)  # equal as floats
            needs, skip, ratio = need_fallback(policy, r["ids"], r["avg"], r["nsp"], V)
            assert (needs, skip, ratio) == (r["needs"], r["skip"], r["ratio"])
            assert (needs, skip) == F.need_fallback(r["avg"], r["ratio"], r["nsp"], T, policy.logprob_threshold,
                                                    policy.compression_ratio_threshold, policy.no_speech_threshold)
            assert 1 <= r["n"] <= R.MAX_LENGTH - P and r["avg"] < 0 and 0 < r["nsp"] < 1


def test_every_branch_of_the_loop_is_in_the_record():
    z = F.load_golden()
    lp, cr, ns = z["thresholds"].tolist()
    assert set(json.loads(str(z["branches"]))) >= {"accepted_at_0", "logprob_then_accepted", "compression_ratio", "exhausted",
                                                    "skipped", "partial_batch"}
    fate, sizes = {}, {}
    for (rnd, k), T, rows in _attempts(z):
        sizes.setdefault(rnd, []).append(len(rows))
        for r in rows:
            fate.setdefault((rnd,) + r["key"], []).append((T, r))
    seen = set()
    for steps in fate.values():
        (T0, r0), (Tn, rn) = steps[0], steps[-1]
        assert T0 == 0.0 and [T for T, _ in steps] == list(F.TEMPERATURES[:len(steps)])
        if not r0["needs"] and not r0["skip"]:
            seen.add("accepted_at_0")
        if r0["needs"] and r0["avg"] < lp and r0["ratio"] <= cr and any(not r["needs"] and not r["skip"] for _, r in steps[1:]):
            seen.add("logprob_then_accepted")
        if any(r["needs"] and r["ratio"] > cr for _, r in steps):
            seen.add("compression_ratio")
        if Tn == F.TEMPERATURES[-1] and rn["needs"]:
            seen.add("exhausted")
        if any(r["skip"] and r["avg"] < lp and r["nsp"] > ns for _, r in steps):
            seen.add("skipped")
    if any(len(s) > 1 and 0 < s[1] < s[0] for s in sizes.values()):
        seen.add("partial_batch")
    assert seen == {"accepted_at_0", "logprob_then_accepted", "compression_ratio", "exhausted", "skipped", "partial_batch"}
    assert any(z[f"clip{b}_skip"].any() for b in range(len(z["frames"])))


def test_recorded_sampled_steps_follow_the_restated_sampler():
    """The processed rows transformers sampled from: the restated float64 rule gives the recorded pick, the timestamp rules
    leave an already processed row as it is, and at least 90 % of the cases have a one-token acceptance interval (a
    condition the GPU test relies on, asserted by the tool as well)."""
    z = F.load_golden()
    n = len(z["case_pick"])
    assert n >= 30
    single = 0
    for i in range(n):
        row = z["case_row"][i].astype(np.float64)
        hist = z["case_hist"][i, :int(z["case_hist_len"][i])].tolist()
        inv_t, u = float(z["case_inv_t"][i]), float(z["case_u"][i])
        assert F.sample_pick(row, inv_t, u) == int(z["case_pick"][i])
        again = R.timestamp_rules(row, hist, R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX)
        assert np.array_equal(np.isfinite(again), np.isfinite(row)), (i, hist)
        ok = F.acceptable(row, inv_t, u)
        assert int(z["case_pick"][i]) in ok
        single += len(ok) == 1
    assert single >= 0.9 * n
    assert len(set(z["case_inv_t"].tolist())) >= 2


def test_policy_and_loop_argument_checks():
    from coral_amd.longform_whisper import FallbackPolicy, run_longform

    assert FallbackPolicy(0.4).temperatures == (0.4,) and FallbackPolicy([0, 0.2]).temperatures == (0.0, 0.2)
    with pytest.raises(ValueError, match="temperatures"):
        FallbackPolicy(())
    with pytest.raises(ValueError, match="temperatures"):
        FallbackPolicy((0.0, -0.2))
    with pytest.raises(ValueError, match="no_speech_threshold"):
        FallbackPolicy((0.0,), no_speech_threshold=0.6)
    with pytest.raises(ValueError, match="vocab_size"):
        run_longform(lambda *a: None, [100], 64, 3, 50, 50, fallback=FallbackPolicy((0.0, 0.2)))
    with pytest.raises(ValueError, match="return_token_timestamps"):
        run_longform(lambda *a: None, [100], 64, 3, 50, 50, fallback=FallbackPolicy((0.0, 0.2)), vocab_size=V, max_length=64,
                     return_token_timestamps=True)
    # the loose keyword route still refuses the four by name, and now says where they go
    for kw in (dict(temperature=(0.0, 0.2)), dict(logprob_threshold=-1.0), dict(compression_ratio_threshold=1.35),
               dict(no_speech_threshold=0.6)):
        with pytest.raises(ValueError, match=next(iter(kw)) + r".*FallbackPolicy"):
            run_longform(lambda batch: [], [4000], 100, 3, 0, 0, **kw)
    with pytest.raises(ValueError, match="condition_on_prev_tokens"):
        run_longform(lambda batch: [], [4000], 100, 3, 0, 0, condition_on_prev_tokens=True)
    # one temperature, no threshold: one greedy attempt per round, no statistics needed
    calls = []

    def one(batch, temperature, uniforms):
        calls.append((temperature, uniforms))
        return [[1, 2, 3, 100, 5, 140, 0]] * len(batch), dict(sum_logprob=None, n_scored=None, no_speech_prob=None)

    out = run_longform(one, [2500], 100, 3, 0, 0, fallback=FallbackPolicy((0.0,)), vocab_size=200, max_length=16)
    assert calls == [(0.0, None)] and out[0]["window_stats"][0]["skipped"] is False and len(out[0]["segments"]) == 1


def test_engine_wrapper_and_evaluation_refuse_by_name():
    """Argument checks run before any device work (the engine is never built)."""
    from coral_amd.evaluate import transcribe_whisper
    from coral_amd.whisper import WhisperEngine
    from coral_amd.whisper_setup import WhisperForConditionalGeneration

    class Shape:
        vocab_size, eos_token_id, max_target_positions = 1565, 50, 64

    eng = WhisperEngine.__new__(WhisperEngine)
    eng.s, eng.device = Shape(), "cpu"
    with pytest.raises(ValueError, match="temperature=0.4.*beam"):
        eng.generate(None, [51, 52, 53], 20, num_beams=2, temperature=0.4, sample_uniforms=torch.zeros(1, 20))
    with pytest.raises(ValueError, match="return_stats.*beam"):
        eng.generate(None, [51, 52, 53], 20, num_beams=2, return_stats=True)
    with pytest.raises(ValueError, match="sample_uniforms"):
        eng.generate(None, [51, 52, 53], 20, temperature=0.4)
    with pytest.raises(ValueError, match="sample_uniforms"):
        eng.generate(None, [51, 52, 53], 20, temperature=0.4, sample_uniforms=torch.zeros(1, 19))
    with pytest.raises(ValueError, match="temperature"):
        eng.generate(None, [51, 52, 53], 20, temperature=-1.0)
    with pytest.raises(ValueError, match="no_speech_token"):
        eng.generate(None, [51, 52, 53], 20, return_stats=True, no_speech_token=1565)
    model = WhisperForConditionalGeneration.__new__(WhisperForConditionalGeneration)
    model.generation_config = dict(lang_to_id={"<|da|>": 52}, task_to_id={"transcribe": 53}, no_timestamps_token_id=63)
    model.shape = type("S", (), dict(vocab_size=1565, decoder_start_token_id=51, max_target_positions=64))()
    assert model.fallback_policy() is None and model.fallback_policy(0.0) is None and model.fallback_policy((0.0,)) is None
    pol = model.fallback_policy((0.0, 0.2), -1.0, 1.35, 0.6, 5)
    assert pol.no_speech_token == F.NO_SPEECH_TOKEN and pol.seed == 5 and pol.temperatures == (0.0, 0.2)
    with pytest.raises(ValueError, match="temperature.*beam"):
        model.generate(torch.zeros(2, 80, 3000), num_beams=2, temperature=(0.0, 0.2))
    with pytest.raises(ValueError, match="return_token_timestamps"):
        model.generate(torch.zeros(2, 80, 3000), temperature=(0.0, 0.2), return_timestamps=True, return_token_timestamps=True)
    model.eval = lambda: None
    with pytest.raises(ValueError, match="num_beams=2.*temperature"):
        transcribe_whisper(model, None, [np.zeros(16000, dtype=np.float32)], num_beams=2, temperature=(0.0, 0.2))
    with pytest.raises(ValueError, match="word"):
        transcribe_whisper(model, None, [np.zeros(16000, dtype=np.float32)], return_timestamps="word", logprob_threshold=-1.0)


def test_configuration_defaults_leave_decoding_as_it_is():
    from coral_amd.config import load_config

    cfg = load_config("evaluation", ["model_id=x"])
    for key in ("temperature", "logprob_threshold", "compression_ratio_threshold", "no_speech_threshold"):
        assert cfg.get(key, "missing") is None, key
    assert cfg.get("sample_seed", None) == 0


def test_new_symbols_are_declared_on_both_sides():
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym, nargs in (("ca_pick_scored_advance", 24), ("ca_row_token_prob", 7)):
        m = re.search(rf"\b{sym}\s*\(([^;]*)\);", hdr)
        assert m and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[sym][1]), sym
    assert callable(ops.pick_scored_advance) and callable(ops.row_token_prob)
    # argument validation needs no GPU
    null = [None] * 24
    args = list(null)
    args[3:6], args[6], args[8] = [1, 8, 8], 0.0, 0
    args[13], args[17:19], args[20:23] = 1, [0, 1], [0, 4, -1]
    assert lib.ca_pick_scored_advance(*args) == -1 and b"ca_pick_scored_advance" in lib.ca_last_error()
    assert lib.ca_row_token_prob(None, None, 1, 8, 8, 9, None) == -1 and b"ca_row_token_prob" in lib.ca_last_error()
