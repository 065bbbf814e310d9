"""Whisper temperature fallback on a real MI355X: ca_pick_scored_advance and ca_row_token_prob against the float64
restatement (tests/whisper_fallback_ref.py), generate(temperature, return_stats) and the fallback loop on the fixture model
against the fp32 oracle, and the transformers fixtures of tests/golden/whisper_fallback.npz.

The sampled pick is judged by an interval, not by equality: the kernel's prefix sums are fp32, at most 128 additions behind
any of them, so a prefix is within 128 * 2^-24 * S = 2^-17 S of its float64 value; the pick must be a token whose float64
interval meets [target - d, target + d] with d = 2^-16 S (F.DELTA), twice that bound."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_fallback_ref as F  # noqa: E402
import whisper_ts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGPROB_TOL = 2e-5  # per scored step: the terms stay below 32 in magnitude (2^-24 * 32 * 2 roundings = 4e-6), the log of
#                     a sum behind at most 128 additions adds 128 * 2^-24 = 8e-6, logf and expf their few ulp

# (rows, V, ldv): the fixture vocabulary, aligned and not; whisper-large's; an odd V on an unaligned stride
SHAPES = [(1, 1565, 1565), (5, 1565, 1568), (16, 1565, 1568), (3, 51866, 51872), (2, 51865, 51867)]


def _vocab(V):
    return (V - R.N_TS, 50257) if V > 50000 else (R.TIMESTAMP_BEGIN, R.EOS)


def _histories(tb, start, n):
    """n histories from a list that holds every branch of the rules (and a few generate() cannot produce)."""
    fixed = [[], [tb + 3], [tb + 3, 7], [tb + 3, 7, 9, 11], [tb + 3, 7, tb + 40], [tb + 3, 7, tb + 40, tb + 40],
             [tb + 3, 7, tb + 40, tb + 40, 12], [tb + 3, 7, tb + 900, tb + 900, 12, 13], [tb, 5, tb + 1499],
             [tb, 5, tb + 1500, tb + 1500, 6], [5, 6], [tb + 10, tb + 10],
             [tb + 1] + [3 + (i % 40) for i in range(70)] + [tb + 1200]]
    return [fixed[(start + i) % len(fixed)] for i in range(n)]


def _state(hists, begin, L, tb, done=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = len(hists)
    ids = torch.randint(0, 40, (n, L), generator=g)
    ids[:, begin:] = tb + 1400
    pos = torch.zeros(n, dtype=torch.int32)
    for r, h in enumerate(hists):
        ids[r, begin:begin + len(h)] = torch.tensor(h, dtype=torch.int64)
        pos[r] = begin + len(h) - 1
    done = torch.zeros(n, dtype=torch.bool) if done is None else torch.tensor(done)
    st = dict(ids=ids, pos=pos, klen=(pos + 1).clone(), tok=torch.zeros(n, dtype=torch.int32), done=done,
              out=torch.full((n,), -7, dtype=torch.int32), slp=torch.zeros(n), ns=torch.zeros(n, dtype=torch.int32))
    return {k: v.to(DEV) for k, v in st.items()}


def _pick(lg, sup, st, V, ldv, inv_t, u, pad, eos, ts):
    from coral_amd import ops

    rows = st["out"].shape[0]
    ops.pick_scored_advance(lg, sup, st["out"], rows, V, ldv, inv_t, u, st["slp"], st["ns"], st["done"], st["ids"], st["tok"],
                            st["pos"], st["klen"], pad, eos, timestamps=ts)
    torch.cuda.synchronize()


def _logits(g, rows, V, ldv, scale):
    lg = torch.zeros(rows, ldv)
    lg[:, :V] = torch.randn(rows, V, generator=g) * scale
    lg[:, V:] = 1e30  # pad columns are never read
    return lg


def _copy(st):
    return {k: v.clone() for k, v in st.items()}


@pytest.mark.parametrize("rows,V,ldv", SHAPES)
def test_greedy_mode_is_the_argmax_launches_bit_for_bit(rows, V, ldv):
    """inv_temperature = 0 against ca_argmax_timestamps_advance (with a history) and ca_argmax_advance (without): the
    token and every piece of state.  Random logits: near-ties of the log-prob rule are not avoided, the two launches
    must fall the same way on them."""
    from coral_amd import ops

    tb, eos = _vocab(V)
    rng = np.random.RandomState(V + rows)
    g = torch.Generator().manual_seed(V * 3 + rows)
    begin, L = 4, 96
    for trial, scale in enumerate((0.05, 1.0, 4.0)):
        hists = _histories(tb, trial * rows, rows)
        lg = _logits(g, rows, V, ldv, scale).to(DEV)
        sup = (torch.rand(V, generator=g) < 0.05).to(torch.uint8).to(DEV)
        done = [bool(rng.rand() < 0.25) for _ in range(rows)]
        for ts in ((begin, tb, 50), None):
            a = _state(hists, begin, L, tb, done, seed=trial)
            b = _copy(a)
            _pick(lg, sup, a, V, ldv, 0.0, None, eos, eos, ts)
            if ts is None:
                ops.argmax_advance(lg, sup, b["out"], rows, V, ldv, b["done"], b["ids"], b["tok"], b["pos"], b["klen"], eos, eos)
            else:
                ops.argmax_timestamps_advance(lg, sup, b["out"], rows, V, ldv, b["done"], b["ids"], b["tok"], b["pos"],
                                              b["klen"], eos, eos, *ts)
            torch.cuda.synchronize()
            for k in ("out", "ids", "tok", "pos", "klen", "done"):
                assert torch.equal(a[k], b[k]), (k, trial, ts)


@pytest.mark.parametrize("rows,V,ldv", SHAPES)
def test_sampled_pick_lies_in_the_float64_interval_and_logprob_is_scored(rows, V, ldv):
    tb, eos = _vocab(V)
    rng = np.random.RandomState(7 * V + rows)
    g = torch.Generator().manual_seed(V + 11 * rows)
    begin, L = 4, 96
    for trial, (scale, T) in enumerate(((1.0, 0.2), (0.3, 0.4), (2.0, 1.0), (1.0, 0.6))):
        inv_t = float(np.float32(1.0 / T))
        hists = _histories(tb, trial * rows + 1, rows)
        lg = _logits(g, rows, V, ldv, scale)
        lg[0, 5:9] = -float("inf")  # -inf inside a window
        sup = (torch.rand(V, generator=g) < 0.05).to(torch.uint8)
        done = [bool(r == rows - 1 and rows > 1) for r in range(rows)]
        for ts in ((begin, tb, 50), None):
            st = _state(hists, begin, L, tb, done, seed=trial)
            u = torch.rand(rows, L, generator=g)
            before = _copy(st)
            _pick(lg.to(DEV), sup.to(DEV), st, V, ldv, inv_t, u.to(DEV), eos, eos, ts)
            again = _copy(before)
            _pick(lg.to(DEV), sup.to(DEV), again, V, ldv, inv_t, u.to(DEV), eos, eos, ts)
            for k in st:
                assert torch.equal(st[k], again[k]), ("two runs differ", k)
            out, slp, ns = st["out"].cpu().tolist(), st["slp"].cpu().tolist(), st["ns"].cpu().tolist()
            for r in range(rows):
                row = F.allowed_row(lg[r, :V].numpy(), sup.numpy(), None if ts is None else hists[r], tb, eos, 50)
                if not np.isfinite(row).any():
                    continue
                p = int(before["pos"][r])
                ok = F.acceptable(row, inv_t, float(u[r, p + 1]))
                assert out[r] in ok, (trial, ts, r, out[r], sorted(ok), F.sample_pick(row, inv_t, float(u[r, p + 1])))
                assert np.isfinite(row[out[r]]) and not sup[out[r]]
                if done[r]:
                    assert slp[r] == 0.0 and ns[r] == 0 and int(st["tok"][r]) == eos
                else:
                    assert ns[r] == 1 and abs(slp[r] - F.logprob(row, out[r])) <= LOGPROB_TOL, (slp[r], F.logprob(row, out[r]))
                    assert int(st["ids"][r, p + 1]) == out[r] and int(st["pos"][r]) == p + 1


def test_sampling_edge_cases():
    V, ldv = 1565, 1568
    tb, eos = R.TIMESTAMP_BEGIN, R.EOS
    begin, L = 3, 16
    lg = torch.full((6, ldv), -float("inf"))
    lg[0, [10, 11, 12, 30]] = torch.tensor([0.0, 1.0, 0.5, -200.0])   # u = 0: the first token with mass (30 has none at T 0.2)
    lg[1, [10, 11, 12, 30]] = torch.tensor([0.0, 1.0, 0.5, -200.0])   # u = 1 - 2^-24: the last token with mass
    lg[2, 33] = 0.7                                                      # a one-token allowed set
    lg[3, :V] = torch.randn(V, generator=torch.Generator().manual_seed(1))
    lg[3, 21] = 40.0                                                     # a dominant logit at T = 0.2: every u picks it
    lg[4, :V] = lg[3, :V]
    lg[5, :V] = lg[3, :V]
    u = torch.zeros(6, L)
    u[1], u[2], u[3], u[4], u[5] = 1 - 2.0 ** -24, 0.37, 0.0, 1 - 2.0 ** -24, 0.5
    hists = [[tb + 1, 4]] * 6
    st = _state(hists, begin, L, tb)
    _pick(lg.to(DEV), None, st, V, ldv, 5.0, u.to(DEV), eos, eos, (begin, tb, 50))
    assert st["out"].cpu().tolist() == [10, 12, 33, 21, 21, 21]
    # the same rows without a history, u = 1 - 2^-24 on a row whose last tokens have mass
    lg2 = torch.zeros(1, ldv)
    st = _state([[]], begin, L, tb)
    _pick(lg2.to(DEV), None, st, V, ldv, 1.0, u[1:2].to(DEV), eos, eos, None)
    assert st["out"].cpu().tolist() == [V - 1]


def test_a_launch_of_4096_rows_follows_the_distribution_and_the_masks():
    """4096 rows share one logit row (ldv = 0) and one history; u runs over the grid (i + 1/2) / N.  Eight tokens carry the
    mass: a count differs from N p_k by at most 1 (the grid) + 2 d N / S (both ends of the interval move by at most d)."""
    V = 1565
    tb, eos = R.TIMESTAMP_BEGIN, R.EOS
    begin, L, N = 3, 12, 4096
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(1, V, generator=g)
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[[9, 10]] = 1
    hist = [tb + 5, 3]  # an open segment: text from eos up, timestamps above tb + 5
    mass = [9, 12, 17, 33, 51, tb + 2, tb + 6, tb + 7, tb + 400, tb + 1500]  # 9 suppressed, tb + 2 below the last timestamp
    lg[0, mass] = torch.tensor([30.0, 20.0, 23.0, 20.5, 19.0, 30.0, 20.2, 21.5, 18.0, 20.0])
    row = F.allowed_row(lg[0].numpy(), sup.numpy(), hist, tb, eos, 50)
    p = F.weights(row, 1.0)
    heavy = np.nonzero(p / p.sum() > 1e-3)[0].tolist()
    assert len(heavy) == 8 and 9 not in heavy and tb + 2 not in heavy
    st = _state([hist] * N, begin, L, tb)
    u = torch.zeros(N, L)
    u[:, begin + len(hist)] = (torch.arange(N, dtype=torch.float64) + 0.5).div(N).float()
    _pick(lg.to(DEV), sup.to(DEV), st, V, 0, 1.0, u.to(DEV), eos, eos, (begin, tb, 50))
    out = st["out"].cpu().numpy()
    assert np.isfinite(row[out]).all(), "a suppressed token or one outside the windows was picked"
    counts = np.bincount(out, minlength=V)
    slack = 1 + 2 * F.DELTA * N
    for k in heavy:
        assert abs(counts[k] - N * p[k] / p.sum()) <= slack, (k, counts[k], N * p[k] / p.sum())
    want = [F.logprob(row, int(t)) for t in out[:64]]
    assert np.abs(st["slp"].cpu().numpy()[:64] - np.array(want)).max() <= LOGPROB_TOL
    assert st["ns"].cpu().tolist() == [1] * N


@pytest.mark.parametrize("rows,V,ldv", [(3, 1565, 1568), (2, 51866, 51872), (2, 51865, 51867)])
def test_row_token_prob_is_the_softmax_of_the_raw_row(rows, V, ldv):
    from coral_amd import ops

    g = torch.Generator().manual_seed(V)
    lg = _logits(g, rows, V, ldv, 2.0)
    tok = 40
    lg[0, tok] = 9.0
    out = torch.zeros(rows, dtype=torch.float32, device=DEV)
    ops.row_token_prob(lg.to(DEV), out, rows, V, ldv, tok)
    want = torch.softmax(lg[:, :V].double(), 1)[:, tok].numpy()
    got = out.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) / want).max() <= 1e-5, (got, want)


# ---- transformers' recorded sampled steps ------------------------------------------------------------------------------------
def test_recorded_steps_with_a_one_token_interval_give_transformers_pick():
    """The processed rows transformers' loop sampled from (tests/golden/whisper_fallback.npz), with their histories and
    uniforms: the pick lies in the float64 interval set, and where that set is one token it is the recorded pick.  The rows
    are already processed, and the rules leave a processed row as it is: with the history and without it the launch must
    pick the same token."""
    z = F.load_golden()
    n, V = len(z["case_pick"]), R.CONFIG["vocab_size"]
    tb, eos, begin, L = R.TIMESTAMP_BEGIN, R.EOS, len(R.PREFIX), R.MAX_LENGTH
    hists = [z["case_hist"][i, :int(z["case_hist_len"][i])].tolist() for i in range(n)]
    ldv = 1568
    lg = torch.zeros(n, ldv)
    lg[:, :V] = torch.from_numpy(z["case_row"])
    singles = 0
    for inv_t in sorted(set(z["case_inv_t"].tolist())):
        sel = [i for i in range(n) if float(z["case_inv_t"][i]) == inv_t]
        for ts in ((begin, tb, R.MAX_INITIAL_TIMESTAMP_INDEX), None):
            st = _state([hists[i] for i in sel], begin, L, tb)
            u = torch.zeros(len(sel), L)
            for r, i in enumerate(sel):
                u[r, begin + len(hists[i])] = float(z["case_u"][i])
            _pick(lg[sel].contiguous().to(DEV), None, st, V, ldv, float(inv_t), u.to(DEV), eos, eos, ts)
            out = st["out"].cpu().tolist()
            for r, i in enumerate(sel):
                ok = F.acceptable(z["case_row"][i].astype(np.float64), float(inv_t), float(z["case_u"][i]))
                assert out[r] in ok, (i, ts, out[r], sorted(ok))
                if len(ok) == 1:
                    assert out[r] == int(z["case_pick"][i]), (i, ts)
                    singles += ts is None
    assert singles >= 0.9 * n  # (the tool's condition)


# ---- the engine --------------------------------------------------------------------------------------------------------------
ACCEPT = 0.0384          # the fixture's logit margin (tests/test_whisper_ts_gpu.py: 1.5 x the measured bf16 logit error)
LOGPROB_MARGIN = 2 * ACCEPT  # a log-probability is a difference of two such quantities
_STATE = {}
KW = dict(begin_suppress_tokens=R.BEGIN_SUPPRESS, return_timestamps=True, timestamp_begin=R.TIMESTAMP_BEGIN,
          max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)


def _engine():
    from coral_amd.whisper import WhisperEngine, WhisperShape

    if "eng" not in _STATE:
        eng = WhisperEngine(WhisperShape(**R.CONFIG), DEV)
        _STATE["P"] = R.fixture_params()
        eng.load_state_dict(_STATE["P"])
        _STATE["eng"] = eng
    return _STATE["eng"], _STATE["P"], R.fixture_config()


def _oracle_avg_logprobs(P, c, feats, rows, nsp_token=None):
    """Teacher-forced fp32 oracle on the engine's own ids: the average log-probability of the generated tokens (EOS
    included) under the restated rules.  Where the oracle's log-prob rule is a near-tie (|logsumexp(timestamps) - text
    maximum| <= ACCEPT) and masks the engine's token, the other side of the rule is taken, as the greedy policy does."""
    from oracle import whisper_ref as w

    Pn = len(R.PREFIX)
    avgs, nsps = [], []
    with torch.no_grad():
        enc = w.encoder(feats, P, c)
        for b, seq in enumerate(rows):
            seq = [int(t) for t in seq]
            lg = w.decoder(torch.tensor([seq[:-1]]), enc[b:b + 1], P, c)[0].double().numpy()
            nsps.append(float(torch.softmax(torch.from_numpy(lg[0]), 0)[nsp_token]) if nsp_token is not None else None)
            total, n = 0.0, 0
            for t in range(Pn, len(seq)):
                hist = seq[Pn:t]
                if hist and hist[-1] == R.EOS:
                    break
                x = lg[t - 1].copy()
                if t == Pn:
                    x[list(R.BEGIN_SUPPRESS)] = -np.inf
                y, info = R.timestamp_rules(x, hist, R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX, detail=True)
                if not np.isfinite(y[seq[t]]):
                    assert abs(info["lse"] - info["text_max"]) <= ACCEPT, (b, t, seq[t], info["lse"], info["text_max"])
                    y = info["before"] if info["forced"] else np.where(np.arange(len(x)) < R.TIMESTAMP_BEGIN, -np.inf, info["before"])
                total += F.logprob(y, seq[t])
                n += 1
            avgs.append((total / n, n))
    return avgs, nsps


def test_scored_greedy_is_todays_timestamp_path_and_its_logprobs_match_the_oracle(monkeypatch):
    from coral_amd import ops

    eng, P, c = _engine()
    feats = R.short_features()
    calls = []
    real = ops.pick_scored_advance
    monkeypatch.setattr(ops, "pick_scored_advance", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    today = eng.generate(feats, R.PREFIX, R.MAX_LENGTH, **KW)
    assert not calls, "with the defaults generate issues the launches it issued before"
    ids, stats = eng.generate(feats, R.PREFIX, R.MAX_LENGTH, return_stats=True, no_speech_token=F.NO_SPEECH_TOKEN, **KW)
    assert calls and ids == today  # byte-identical ids
    eager, stats2 = eng.generate(feats, R.PREFIX, R.MAX_LENGTH, return_stats=True, no_speech_token=F.NO_SPEECH_TOKEN,
                                 use_graph=False, **KW)
    assert eager == ids and stats2 == stats
    want, nsp = _oracle_avg_logprobs(P, c, feats, ids, F.NO_SPEECH_TOKEN)
    for b, (avg, n) in enumerate(want):
        got = stats["sum_logprob"][b] / stats["n_scored"][b]
        print(f"  clip {b}: avg logprob engine {got:.4f}, oracle {avg:.4f} over {n} tokens; no-speech {stats['no_speech_prob'][b]:.5f} "
              f"/ {nsp[b]:.5f}")
        assert stats["n_scored"][b] == n and abs(got - avg) <= LOGPROB_MARGIN
        assert abs(np.log(stats["no_speech_prob"][b] / nsp[b])) <= LOGPROB_MARGIN
    # a subset of the clips against a gather of the batch's cross K|V: the rows of the batch, without the encoder
    kv = eng.cross_kv(eng.encode(feats))
    monkeypatch.setattr(eng, "encode", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the encoder ran again")))
    sub, st = eng.generate(None, R.PREFIX, R.MAX_LENGTH, return_stats=True, cross_kv=eng.gather_cross_kv(kv, [2, 0]), **KW)
    strip = lambda r: R.strip_row(r, len(R.PREFIX), R.EOS, R.EOS)  # noqa: E731
    assert [strip(r) for r in sub] == [strip(ids[2]), strip(ids[0])]
    assert st["n_scored"] == [stats["n_scored"][2], stats["n_scored"][0]] and st["no_speech_prob"] is None


def test_sampled_generate_is_deterministic_obeys_the_grammar_and_scores_its_own_ids():
    eng, P, c = _engine()
    feats = R.short_features()
    u = torch.rand(3, R.MAX_LENGTH, generator=torch.Generator().manual_seed(F.SEED))
    runs = [eng.generate(feats, R.PREFIX, R.MAX_LENGTH, temperature=0.4, sample_uniforms=u, return_stats=True, **KW)
            for _ in range(2)]
    assert runs[0] == runs[1]
    ids, stats = runs[0]
    greedy = eng.generate(feats, R.PREFIX, R.MAX_LENGTH, **KW)
    assert ids != greedy, "sampling at T = 0.4 left every token at the argmax"
    Pn = len(R.PREFIX)
    for r in ids:
        assert r[:Pn] == R.PREFIX and R.grammar_ok(R.strip_row(r, Pn, R.EOS, R.EOS), R.TIMESTAMP_BEGIN, R.EOS), r
    want, _ = _oracle_avg_logprobs(P, c, feats, ids)
    for b, (avg, n) in enumerate(want):
        got = stats["sum_logprob"][b] / stats["n_scored"][b]
        print(f"  clip {b} at T = 0.4: avg logprob engine {got:.4f}, oracle {avg:.4f} over {n} tokens")
        assert stats["n_scored"][b] == n and abs(got - avg) <= LOGPROB_MARGIN


def _window_generate(eng, mels, calls):
    """The protocol of run_longform under a policy on the engine: the encoder once per batch of windows, later attempts
    against a gather of its cross K|V."""
    held = {}

    def attempt(batch, temperature, uniforms):
        if any(k not in held.get("keys", {}) for k in batch):
            feats = torch.stack([R.window_features(mels[c], seek) for c, seek in batch])
            held["kv"], held["keys"] = eng.cross_kv(eng.encode(feats)), {k: i for i, k in enumerate(batch)}
            calls.append(("encode", len(batch)))
        calls.append((temperature, len(batch)))
        kv = eng.gather_cross_kv(held["kv"], [held["keys"][k] for k in batch])
        return eng.generate(None, R.PREFIX, R.MAX_LENGTH, temperature=float(temperature), sample_uniforms=uniforms,
                            return_stats=True, no_speech_token=F.NO_SPEECH_TOKEN, cross_kv=kv, **KW)

    return attempt


def test_fallback_loop_on_the_engine():
    """One greedy temperature and no threshold: the windows, seeks and segments of today's long-form path, byte for byte.
    The recorded thresholds and temperatures: a run is deterministic given the seed, no window is encoded twice, and the
    reported average log-probabilities are those of the fp32 oracle on the engine's own ids."""
    from coral_amd.longform_whisper import FallbackPolicy, run_longform

    eng, P, c = _engine()
    mels = R.long_features()
    frames = [m.shape[1] for m in mels]
    Pn, V = len(R.PREFIX), R.CONFIG["vocab_size"]

    def plain(batch):
        feats = torch.stack([R.window_features(mels[c_], seek) for c_, seek in batch])
        return eng.generate(feats, R.PREFIX, R.MAX_LENGTH, **KW)

    today = run_longform(plain, frames, R.TIMESTAMP_BEGIN, Pn, R.EOS, R.EOS)
    calls = []
    one = run_longform(_window_generate(eng, mels, calls), frames, R.TIMESTAMP_BEGIN, Pn, R.EOS, R.EOS,
                       fallback=FallbackPolicy((0.0,)), vocab_size=V, max_length=R.MAX_LENGTH)
    for a, b in zip(today, one):
        assert a["windows"] == b["windows"] and a["segments"] == b["segments"]
    assert all(t == 0.0 or t == "encode" for t, _ in calls)
    z = F.load_golden()
    lp, cr, ns = z["thresholds"].tolist()
    policy = FallbackPolicy(F.TEMPERATURES, lp, cr, ns, F.NO_SPEECH_TOKEN, F.SEED)
    runs, logs = [], []
    for _ in range(2):
        calls = []
        runs.append(run_longform(_window_generate(eng, mels, calls), frames, R.TIMESTAMP_BEGIN, Pn, R.EOS, R.EOS, fallback=policy,
                                 vocab_size=V, max_length=R.MAX_LENGTH))
        logs.append(calls)
    assert logs[0] == logs[1] and all(a["windows"] == b["windows"] and a["segments"] == b["segments"] and
                                      a["window_stats"] == b["window_stats"] for a, b in zip(*runs))
    attempts = [t for t, _ in logs[0] if t != "encode"]
    assert any(t > 0 for t in attempts), "no window fell back: the thresholds of the record do not bite on the engine"
    # an encoder pass per round of windows, however many attempts the round took
    rounds = sum(1 for t, _ in logs[0] if t == "encode")
    assert rounds < len(attempts) and rounds == max(len(r["windows"]) for r in runs[0])
    # the kept windows' statistics against the oracle
    for b, res in enumerate(runs[0]):
        rows = [R.PREFIX + gen + [R.EOS] for _, gen in res["windows"]]
        feats = torch.stack([R.window_features(mels[b], seek) for seek, _ in res["windows"]])
        want, _ = _oracle_avg_logprobs(P, c, feats, rows)
        for (avg, n), w in zip(want, res["window_stats"]):
            print(f"  clip {b} seek {w['seek']}: T {w['temperature']}, avg logprob engine {w['avg_logprob']:.4f}, oracle {avg:.4f}")
            if n < R.MAX_LENGTH - Pn:  # (a window cut at max_length has no EOS: its last step is not in `rows`)
                assert abs(w["avg_logprob"] - avg) <= LOGPROB_MARGIN


def test_public_surface_transcribe_and_generate_with_fallback():
    """`transcribe_whisper` and the wrapper's `generate` with the recorded thresholds: neutral arguments leave today's
    results as they are; with a policy every clip takes the window loop, a prediction carries its windows' statistics, a
    seeded run repeats itself and another seed draws other uniforms."""
    from coral_amd.evaluate import transcribe_whisper
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

    model = WhisperForConditionalGeneration(WhisperShape(**R.CONFIG), device=DEV).eval()
    model.engine.load_state_dict(R.fixture_params())
    model.engine.refresh_derived()
    model.generation_config = dict(no_timestamps_token_id=R.NO_TIMESTAMPS, lang_to_id={"<|da|>": R.LANG},
                                   task_to_id={"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE},
                                   max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    short, long_ = R.short_waves()[1], R.long_waves()[0]
    lp, cr, ns = F.load_golden()["thresholds"].tolist()
    kw = dict(batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True)
    today, today_rows = transcribe_whisper(model, proc, [short, long_], **kw)
    same, same_rows = transcribe_whisper(model, proc, [short, long_], temperature=0.0, **kw)
    assert same_rows == today_rows and same == today and "windows" not in today[0]
    th = dict(temperature=F.TEMPERATURES, logprob_threshold=lp, compression_ratio_threshold=cr, no_speech_threshold=ns)
    a, a_rows = transcribe_whisper(model, proc, [short, long_], sample_seed=F.SEED, **th, **kw)
    b, b_rows = transcribe_whisper(model, proc, [short, long_], sample_seed=F.SEED, **th, **kw)
    assert a_rows == b_rows and a == b
    temps = [w["temperature"] for item in a for w in item["windows"]]
    assert any(t > 0 for t in temps) and set(temps) <= set(F.TEMPERATURES)
    for item in a:
        assert set(item) == {"text", "chunks", "windows"}
        for w in item["windows"]:
            assert set(w) == {"seek", "skipped", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
            assert w["avg_logprob"] < 0 and 0 < w["no_speech_prob"] < 1
    c_rows = transcribe_whisper(model, proc, [short, long_], sample_seed=F.SEED + 1, **th, **kw)[1]
    assert c_rows != a_rows
    # the wrapper's generate on clips of one window
    feats = proc.feature_extractor([short, R.short_waves()[0]])
    plain = model.generate(feats, max_length=R.MAX_LENGTH, return_timestamps=True)
    one = model.generate(feats, max_length=R.MAX_LENGTH, return_timestamps=True, temperature=(0.0,), logprob_threshold=-1e9)
    strip = lambda r: R.strip_row(r, len(R.PREFIX), R.EOS, R.EOS)  # noqa: E731
    assert [strip(r) for r in one] == [strip(r) for r in plain]
    rows, stats = model.generate(feats, max_length=R.MAX_LENGTH, return_timestamps=True, return_fallback_stats=True,
                                 sample_seed=F.SEED, **th)
    assert len(rows) == 2 and len(rows[0]) == len(rows[1]) and all(r[:3] == R.PREFIX for r in rows)
    assert [set(s) for s in stats] == [{"skipped", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}] * 2
