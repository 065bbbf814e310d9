"""Whisper timestamps on a real MI355X: ca_argmax_timestamps / ca_argmax_timestamps_advance against the NumPy
restatement (tests/whisper_ts_ref.py), generate(return_timestamps=True) and the long-form loop against the fp32 oracle
under the tie policy of the greedy tests, and the transformers fixtures of tests/golden/whisper_ts.npz."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_ts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Tie margins.  The greedy tests of the 200-token tiny fixture use (2e-2, 5e-2) (tests/test_whisper_beam_gpu.py MARGINS).
# This is a new model: its final LayerNorm carries a bias of norm 6 (tests/whisper_ts_ref.py), its logits reach 10.6 where
# the tiny fixture's stay below 1, so bf16 moves them further.  MEASURED_LOGIT_ERROR is the largest |engine - fp32 oracle|
# teacher-forced logit over the recorded ids of the three clips, measured on an MI355X (0.02556, all of it in the
# timestamp block; the text block stays within 0.0061) - test_generate_with_timestamps... measures it again
# and fails if it has grown.  The margins are the policy's 1.5 x and 3 x that error (NOTEBOOK.md R6.4: "within 1.5 x the
# error of the maximum, equal to the argmax beyond 3 x the error"), never below the tiny pair.
MEASURED_LOGIT_ERROR = 0.0256
ACCEPT, FORCED = max(2e-2, 1.5 * MEASURED_LOGIT_ERROR), max(5e-2, 3 * MEASURED_LOGIT_ERROR)

SHAPES = [(3, 51865, 51872), (2, 51866, 51872), (2, 1565, 1568), (1, 1565, 1565)]


def _vocab(V):
    """(timestamp_begin, eos) of a vocabulary whose last 1501 ids are the timestamps."""
    return (V - R.N_TS, 50257) if V > 50000 else (R.TIMESTAMP_BEGIN, R.EOS)


def _histories(tb, eos):
    """(history, cap) covering every branch of the rules; text ids are small numbers below eos."""
    return [([], None), ([], 50), ([], 0),                        # the first token: a timestamp, capped or not
            ([tb + 3], 50),                                         # one timestamp (penultimate counts as one): text next
            ([tb + 3, 7], 50), ([tb + 3, 7, 9, 11], None),          # open segment: text or a timestamp above the last
            ([tb + 3, 7, tb + 40], 50),                             # a segment's end: its pair (>= the same time) or EOS
            ([tb + 3, 7, tb + 40, tb + 40], None),                  # closed pair: text, timestamps masked
            ([tb + 3, 7, tb + 40, tb + 40, 12], 50),                # after the pair: timestamps above tb + 40 only
            ([tb + 3, 7, tb + 900, tb + 900, 12, 13], None),        # the monotonic mask removes most timestamps
            ([tb, 5, tb + 1499], 50), ([tb, 5, tb + 1500], None),   # one or two timestamps left
            ([tb, 5, tb + 1500, tb + 1500, 6], 50),                 # none left: text
            ([tb, 5, tb + 1500, tb + 1500], None),
            ([5, 6], 50), ([7], None), ([tb + 10, tb + 10], 50),    # histories generate() cannot produce
            ([tb + 1] + [3 + (i % 40) for i in range(70)] + [tb + 1200], None)]  # longer than one wave's stride


def _grid_logits(g, rows, V, ldv, step):
    lg = torch.zeros(rows, ldv)
    for r in range(rows):
        lg[r, :V] = (torch.randperm(V, generator=g).float() - V / 2) * step
    lg[:, V:] = 1e30  # pad columns are never read
    return lg


def _reference(lg, sup, V, hist, tb, eos, cap):
    x = lg[:V].double().numpy().copy()
    if sup is not None:
        x[sup.numpy().astype(bool)] = -np.inf
    return R.timestamp_rules(x, hist, tb, eos, cap, detail=True)


def _ids_table(g, hists, begin, ld_ids, tb):
    """A history table: a random prefix, the row's history, then timestamps that must not be read."""
    ids = torch.randint(0, 40, (len(hists), ld_ids), generator=g)
    ids[:, begin:] = tb + 1400
    pos = torch.zeros(len(hists), dtype=torch.int32)
    for r, h in enumerate(hists):
        ids[r, begin:begin + len(h)] = torch.tensor(h, dtype=torch.int64)
        pos[r] = begin + len(h) - 1
    return ids, pos


@pytest.mark.parametrize("rows,V,ldv", SHAPES)
def test_timestamp_pick_equals_the_restated_rules(rows, V, ldv):
    """Tie-free logits (a permuted grid per row); the test asserts in float64 that no case is a near-tie of the log-prob
    rule (gap >= 1e-3, three orders above the fp32 error of a 1501-term sum), so the picks are exact.  Grid steps from
    2e-4 to 4e-2 put cases on both sides of the rule.  A launch has one cap, so the cases are launched cap by cap: every
    shape sees an empty history with cap 50, with cap 0 and without one.  The suppress mask removes, besides 5 % of the
    vocabulary, the token the rules would pick for the launch's first row without it."""
    from coral_amd import ops

    tb, eos = _vocab(V)
    cases = _histories(tb, eos)
    g = torch.Generator().manual_seed(V + rows)
    begin, ld_ids = 4, 96
    sides, n_launch = set(), 0
    launches = []
    for cap in (None, 50, 0):
        group = [h for h, c_ in cases if c_ == cap]
        assert [] in group
        launches += [(cap, (group[a:a + rows] + group[:rows])[:rows]) for a in range(0, len(group), rows)]
    capped_empty = 0
    for step in (2e-4, 3e-3, 4e-2):
        for cap, hists in launches:
            lg = _grid_logits(g, rows, V, ldv, step)
            sup = (torch.rand(V, generator=g) < 0.05).to(torch.uint8)
            use_sup = (n_launch % 3) != 2
            if use_sup:  # the pick the first row would otherwise make
                first = R.pick(_reference(lg[0], sup, V, hists[0], tb, eos, cap)[0])
                sup[first] = 1
            capped_empty += sum(1 for h in hists if not h and cap == 50)
            ids, pos = _ids_table(g, hists, begin, ld_ids, tb)
            out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
            ops.argmax_timestamps(lg.to(DEV), sup.to(DEV) if use_sup else None, out, rows, V, ldv, ids.to(DEV), pos.to(DEV),
                                  begin, tb, eos, cap)
            torch.cuda.synchronize()
            n_launch += 1
            for r, h in enumerate(hists):
                y, info = _reference(lg[r], sup if use_sup else None, V, h, tb, eos, cap)
                if np.isfinite(info["lse"]) and np.isfinite(info["text_max"]):
                    assert abs(info["lse"] - info["text_max"]) >= 1e-3, ("near-tie in the fixture", step, h)
                    sides.add(info["forced"])
                assert int(out[r]) == R.pick(y), (step, h, cap, int(out[r]), R.pick(y), info["lse"], info["text_max"])
                if use_sup and np.isfinite(y).any():  # (everything masked: index 0, as ca_argmax_masked)
                    assert not sup[int(out[r])] and (r > 0 or int(out[r]) != first)
    assert sides == {True, False} and capped_empty >= 3


@pytest.mark.parametrize("V,ldv", [(51865, 51872), (1565, 1565)])
def test_log_prob_rule_sums_the_timestamps(V, ldv):
    """Hand-made rows, one per side: every timestamp logit lies below the best text token; 1501 of them add up to
    logsumexp = log(1501) + about -0.7 = 6.6.  Text maximum 5 -> the rule forces the best timestamp (a kernel that compared
    the timestamp MAXIMUM would pick the text token); text maximum 8 -> the text token stays."""
    from coral_amd import ops

    tb, eos = _vocab(V)
    lg = torch.full((2, ldv), -3.0)
    k = torch.arange(R.N_TS, dtype=torch.float32)
    ts = -0.001 * ((k * 7) % R.N_TS)  # distinct values in (-1.501, 0]
    lg[:, tb:V] = ts
    lg[0, 17], lg[1, 17] = 5.0, 8.0
    lg[:, V:] = 1e30
    hist = [tb, 3]
    for r in range(2):
        y, info = R.timestamp_rules(lg[r, :V].double().numpy(), hist, tb, eos, None, detail=True)
        assert info["before"][tb:].max() < info["text_max"] - 4 and abs(info["lse"] - info["text_max"]) > 1.0
        assert info["forced"] == (r == 0)
    ids, pos = _ids_table(torch.Generator().manual_seed(1), [hist, hist], 3, 16, tb)
    out = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.argmax_timestamps(lg.to(DEV), None, out, 2, V, ldv, ids.to(DEV), pos.to(DEV), 3, tb, eos, None)
    best_ts = R.pick(R.timestamp_rules(lg[0, :V].double().numpy(), hist, tb, eos, None))
    assert best_ts > tb and out.tolist() == [best_ts, 17]  # (tb itself is masked: the history opened at tb)


def test_advance_variant_keeps_the_books_of_argmax_advance():
    from coral_amd import ops

    V, ldv = 1565, 1568
    tb, eos, pad = R.TIMESTAMP_BEGIN, R.EOS, R.EOS
    g = torch.Generator().manual_seed(77)
    hists = [[], [tb + 3, 7], [tb + 3, 7, tb + 40], [tb + 3, 7, tb + 40, tb + 40], [tb + 2, 9, 9]]
    rows, begin, L = len(hists), 3, 24
    ids, pos = _ids_table(g, hists, begin, L, tb)
    lg = _grid_logits(g, rows, V, ldv, 3e-3)
    lg[2, eos] = 50.0  # row 2 closes with EOS: the only text-side token above the timestamps' total
    done = torch.tensor([False, False, False, False, True])  # row 4 had finished: it records pad
    klen = (pos + 1).clone()
    tok = torch.zeros(rows, dtype=torch.int32)
    want_ids, want_done, want_tok, want_pos, want_klen = (ids.numpy().copy(), done.numpy().copy(), tok.numpy().copy(),
                                                          pos.numpy().copy(), klen.numpy().copy())
    picks = []
    for r, h in enumerate(hists):
        y, info = R.timestamp_rules(lg[r, :V].double().numpy(), h, tb, eos, 50, detail=True)
        if np.isfinite(info["lse"]) and np.isfinite(info["text_max"]):
            assert abs(info["lse"] - info["text_max"]) >= 1e-3
        picks.append(R.pick(y))
    assert picks[2] == eos and picks[0] <= tb + 50 and picks[3] < tb
    R.advance(want_ids, want_done, want_tok, want_pos, want_klen, picks, pad, eos)
    d = dict(ids=ids.to(DEV), done=done.to(DEV), tok=tok.to(DEV), pos=pos.to(DEV), klen=klen.to(DEV))
    out = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ops.argmax_timestamps_advance(lg.to(DEV), None, out, rows, V, ldv, d["done"], d["ids"], d["tok"], d["pos"], d["klen"],
                                  pad, eos, begin, tb, 50)
    torch.cuda.synchronize()
    assert out.tolist() == picks
    assert np.array_equal(d["ids"].cpu().numpy(), want_ids) and d["done"].cpu().tolist() == want_done.tolist()
    assert d["tok"].cpu().tolist() == want_tok.tolist() and d["pos"].cpu().tolist() == want_pos.tolist()
    assert d["klen"].cpu().tolist() == want_klen.tolist()
    assert want_tok[4] == pad and want_done.tolist() == [False, False, True, False, True]


@pytest.mark.parametrize("entry", ["argmax_advance", "argmax_timestamps_advance", "pick_scored_advance"])
def test_a_full_row_stores_no_id_and_still_keeps_its_books(entry):
    """Rows 0 and 2 stand at the last column of `ids`: their token has no cell (pos + 1 == ld_ids) and must not be stored
    - an unchecked store lands in the next row's first cell and, for the last row, behind the table, both of which lie
    inside the flat buffer here -, while out, tok, pos, klen and done move as for row 1, which has one cell left."""
    from coral_amd import ops

    rows, V, ldv, L, begin = 3, 1565, 1568, 16, 4
    tb, eos, pad, cap = R.TIMESTAMP_BEGIN, R.EOS, R.EOS, 50
    g = torch.Generator().manual_seed(16)
    hists = [[tb + 3] + [5 + i for i in range(L - begin - 1)],           # open segments, text last
             [tb + 3, 7, tb + 40, tb + 40] + [9 + i for i in range(L - begin - 5)],
             [tb + 1] + [3 + i for i in range(L - begin - 1)]]
    assert [begin + len(h) - 1 for h in hists] == [L - 1, L - 2, L - 1]
    flat = torch.full((rows * L + 8,), -5, dtype=torch.int64)
    table, pos = _ids_table(g, hists, begin, L, tb)
    flat[:rows * L] = table.flatten()
    lg = _grid_logits(g, rows, V, ldv, 3e-3)
    done = torch.tensor([False, False, True])  # row 2 had finished: it takes pad
    klen, tok = (pos + 1).clone(), torch.zeros(rows, dtype=torch.int32)
    picks = []
    for r, h in enumerate(hists):
        x = lg[r, :V].double().numpy()
        if entry != "argmax_advance":
            x, info = R.timestamp_rules(x, h, tb, eos, cap, detail=True)
            assert abs(info["lse"] - info["text_max"]) >= 1e-3, "near-tie in the fixture"
        picks.append(R.pick(x))
    # the reference bookkeeping on a table one column wider: the column the full rows have not got takes their token
    wide = np.concatenate([table.numpy(), np.full((rows, 1), -5, dtype=np.int64)], axis=1)
    want_done, want_tok, want_pos, want_klen = done.numpy().copy(), tok.numpy().copy(), pos.numpy().copy(), klen.numpy().copy()
    R.advance(wide, want_done, want_tok, want_pos, want_klen, picks, pad, eos)
    want_flat = flat.numpy().copy()
    want_flat[1 * L + L - 1] = picks[1]
    assert np.array_equal(want_flat[:rows * L].reshape(rows, L), wide[:, :L])

    flat_d = flat.to(DEV)
    ids = flat_d[:rows * L].view(rows, L)
    d = dict(done=done.to(DEV), tok=tok.to(DEV), pos=pos.to(DEV), klen=klen.to(DEV))
    out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    head = (lg.to(DEV), None, out, rows, V, ldv)
    books = (d["done"], ids, d["tok"], d["pos"], d["klen"], pad, eos)
    if entry == "argmax_advance":
        ops.argmax_advance(*head, *books)
    elif entry == "argmax_timestamps_advance":
        ops.argmax_timestamps_advance(*head, *books, begin, tb, cap)
    else:
        slp, ns = torch.zeros(rows, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV)
        ops.pick_scored_advance(*head, 0.0, None, slp, ns, *books, timestamps=(begin, tb, cap))
    torch.cuda.synchronize()
    assert out.tolist() == picks
    assert np.array_equal(flat_d.cpu().numpy(), want_flat)
    assert d["tok"].cpu().tolist() == want_tok.tolist() and d["pos"].cpu().tolist() == want_pos.tolist() == [L, L - 1, L]
    assert d["klen"].cpu().tolist() == want_klen.tolist() and d["done"].cpu().tolist() == want_done.tolist()
    assert want_tok[2] == pad and picks[1] != -5


# ---- the engine ------------------------------------------------------------------------------------------------------------
_STATE = {}


def _engine():
    from coral_amd.whisper import WhisperEngine, WhisperShape

    if "eng" not in _STATE:
        eng = WhisperEngine(WhisperShape(**R.CONFIG), DEV)
        _STATE["P"] = R.fixture_params()
        eng.load_state_dict(_STATE["P"])
        _STATE["eng"] = eng
    return _STATE["eng"], _STATE["P"], R.fixture_config()


def _generate(eng, feats, **kw):
    return eng.generate(feats, R.PREFIX, R.MAX_LENGTH, begin_suppress_tokens=R.BEGIN_SUPPRESS, return_timestamps=True,
                        timestamp_begin=R.TIMESTAMP_BEGIN, max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX, **kw)


def _oracle_rows(P, c, feats):
    from oracle import whisper_ref as w

    with torch.no_grad():
        enc = w.encoder(feats, P, c)

    def rows(b, seq):
        with torch.no_grad():
            return w.decoder(torch.tensor([seq[:-1]]), enc[b:b + 1], P, c)[0].numpy()

    return rows, enc


def test_generate_with_timestamps_on_the_fixture_clips():
    """Eager loop and captured graph give the same ids; they are a greedy path of the fp32 oracle under the timestamp
    rules within the tie policy, part from the recorded transformers ids only at a near-tie, and obey the grammar."""
    from oracle import whisper_ref as w

    eng, P, c = _engine()
    z = R.load_golden()
    feats = R.short_features()
    graph = _generate(eng, feats)
    eager = _generate(eng, feats, use_graph=False)
    assert graph == eager
    nocache = _generate(eng, feats, use_cache=False)
    rows, enc = _oracle_rows(P, c, feats)
    want = z["short_ids"].tolist()
    # the figure behind the margins: engine vs oracle, teacher-forced on the recorded ids
    with torch.no_grad():
        ref = w.decoder(torch.tensor(want), enc, P, c)
    got = eng.decode(torch.tensor(want), eng.encode(feats)).float().cpu()
    err = float((got - ref).abs().max())
    print(f"largest |engine - oracle| teacher-forced logit on the recorded ids: {err:.4f} "
          f"(logits up to {float(ref.abs().max()):.2f}); accept {ACCEPT}, forced {FORCED}")
    assert err <= MEASURED_LOGIT_ERROR * 1.25 + 1e-3, "the margins were derived from a smaller logit error: measure again"
    P_len = len(R.PREFIX)
    for label, ids in (("graph", graph), ("no-cache", nocache)):
        R.check_timestamp_rows(rows, ids, want, P_len, ACCEPT, FORCED, label=label)
        for r in ids:
            assert r[:P_len] == R.PREFIX and len(r) <= R.MAX_LENGTH
            assert R.grammar_ok(R.strip_row(r, P_len, c.pad_token_id, c.eos_token_id), R.TIMESTAMP_BEGIN, c.eos_token_id), r


def test_timestamps_bypass_the_one_launch_kernel_and_beams_are_refused(monkeypatch):
    """On a shape the one-launch-per-token kernel takes (head size 64, d_model 384: the smallest of the Whisper family;
    the fixture model's head size is 16, which that kernel never takes).  Without timestamps generate goes through
    ca_whisper_decode_token - the spy is live -, with them it does not: that kernel picks with the plain masked argmax
    and would ignore the rules.  The graph path's ids equal the eager loop's and obey the grammar."""
    from coral_amd import ops
    from coral_amd.whisper import WhisperEngine, WhisperShape
    from oracle import whisper_ref as w

    kw = dict(R.CONFIG, d_model=384, encoder_layers=1, decoder_layers=2, encoder_attention_heads=6, decoder_attention_heads=6,
              encoder_ffn_dim=1536, decoder_ffn_dim=1536)
    eng = WhisperEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(w.synth_params(w.WhisperConfig(**kw), seed=77))
    feats = torch.randn(2, 80, 3000, generator=torch.Generator().manual_seed(5)) * 0.5
    assert ops.whisper_decode_token_supported(2, 384, 1536, 6, kw["vocab_size"])
    calls = []
    real = ops.whisper_decode_token
    monkeypatch.setattr(ops, "whisper_decode_token", lambda d: (calls.append(1), real(d))[1])
    plain = eng.generate(feats, R.PREFIX_NO_TS, 20, begin_suppress_tokens=R.BEGIN_SUPPRESS)
    assert calls, "without timestamps this shape decodes with one launch per token"
    assert len(plain) == 2 and all(r[:4] == R.PREFIX_NO_TS for r in plain)
    calls.clear()
    graph = _generate(eng, feats)
    assert not calls, "with timestamps the one-launch kernel must be bypassed"
    P_len, L, B, V = len(R.PREFIX), R.MAX_LENGTH, 2, kw["vocab_size"]
    for r in graph:
        assert r[:P_len] == R.PREFIX and len(r) > P_len + 2
        assert R.grammar_ok(R.strip_row(r, P_len, R.EOS, R.EOS), R.TIMESTAMP_BEGIN, R.EOS), r
    # The graph path's launch sequence, run here launch by launch without capture: every pick must be what the restated
    # rules give on the very logits the launch read (exact: the same fp32 numbers; a step where the log-prob rule is
    # nearer than 1e-4 to a tie could fall either way in fp32 and is not judged), and the ids must be the graph path's.
    kv = eng.cross_kv(eng.encode(feats))
    cache = eng.new_decode_cache(B, L)
    g = eng._graph_state(cache, kv, R.EOS, R.EOS)
    g["ts"] = (P_len, R.TIMESTAMP_BEGIN, R.MAX_INITIAL_TIMESTAMP_INDEX)
    sup = torch.zeros(V, dtype=torch.uint8, device=DEV)
    sup_begin = sup.clone()
    sup_begin[torch.tensor(R.BEGIN_SUPPRESS, device=DEV)] = 1
    ids0 = torch.tensor([R.PREFIX] * B, dtype=torch.int64, device=DEV)
    base = eng.decode_step(ids0, kv, cache).contiguous()
    ops.argmax_timestamps(base, sup_begin, g["nxt"], B, V, V, ids0, torch.full((B,), P_len - 1, dtype=torch.int32, device=DEV),
                          P_len, R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX)
    g["out"][:, :P_len] = ids0
    g["out"][:, P_len] = g["nxt"].long()
    g["tok"].copy_(g["nxt"])
    g["pos"].fill_(P_len)
    g["klen"].fill_(P_len + 1)
    judged = 0
    for n in range(P_len + 1, L):
        hist = g["out"][:, P_len:n].cpu().tolist()
        eng._token_step_launches(cache, g, sup)
        torch.cuda.synchronize()
        lg = g["logits"][:, :V].double().cpu().numpy()
        for b_ in range(B):
            y, info = R.timestamp_rules(lg[b_], hist[b_], R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX, detail=True)
            if R.EOS in hist[b_] or (np.isfinite(info["lse"]) and abs(info["lse"] - info["text_max"]) < 1e-4):
                continue
            judged += 1
            assert int(g["nxt"][b_]) == R.pick(y), (n, b_, int(g["nxt"][b_]), R.pick(y), hist[b_])
    assert judged > B * (L - P_len - 1) // 2
    assert [r[:len(q)] for r, q in zip(g["out"].cpu().tolist(), graph)] == graph
    assert not calls
    with pytest.raises(ValueError, match="return_timestamps"):
        _generate(eng, feats, num_beams=2)


def test_without_timestamps_generate_is_the_parent_commits_path(monkeypatch):
    """return_timestamps=False (the default): not one call of the new launches, and the ids of the old fixtures are
    those of the parent commit's eager loop (decode_step + ca_argmax_masked), restated here launch for launch."""
    from coral_amd import ops
    from whisper_beam_ref import MAX_LENGTH, fixture

    from coral_amd.whisper import WhisperEngine, WhisperShape

    def boom(*a, **k):
        raise AssertionError("a timestamp launch on the path without timestamps")

    monkeypatch.setattr(ops, "argmax_timestamps", boom)
    monkeypatch.setattr(ops, "argmax_timestamps_advance", boom)
    for name in ("tiny", "tiny_eos18"):
        kw, c, P, feats, prefix, sup, sup_begin = fixture(name)
        eng = WhisperEngine(WhisperShape(**kw), DEV)
        eng.load_state_dict(P)
        got = eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin)
        assert got == eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin,
                                   return_timestamps=False)
        assert got == eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin,
                                   use_graph=False)
        # the parent's loop
        B, V = feats.shape[0], c.vocab_size
        kv = eng.cross_kv(eng.encode(feats))
        m = torch.zeros(V, dtype=torch.uint8, device=DEV)
        m[torch.tensor(sup, device=DEV)] = 1
        mb = m.clone()
        mb[torch.tensor(sup_begin, device=DEV)] = 1
        ids = torch.tensor([prefix] * B, dtype=torch.int64, device=DEV)
        done = torch.zeros(B, dtype=torch.bool, device=DEV)
        nxt = torch.empty(B, dtype=torch.int32, device=DEV)
        cache, feed = eng.new_decode_cache(B, MAX_LENGTH), ids
        while ids.shape[1] < MAX_LENGTH and not bool(done.all()):
            base = eng.decode_step(feed, kv, cache).contiguous()
            ops.argmax_masked(base, mb if ids.shape[1] == len(prefix) else m, nxt, B, V, V)
            step = torch.where(done, torch.full_like(nxt, c.pad_token_id), nxt).to(torch.int64)
            ids = torch.cat([ids, step[:, None]], 1)
            feed = step[:, None]
            done |= step == c.eos_token_id
        assert got == ids.tolist()


# ---- long recordings ---------------------------------------------------------------------------------------------------------
def test_whole_recording_log_mel_matches_the_oracle():
    """ca_logmel at N != 480000: frames = N / 160, the clamp from the recording's own maximum (tolerance of the 30 s
    log-mel test, tests/test_whisper_gpu.py)."""
    eng, P, c = _engine()
    for wave, ref in zip(R.long_waves(), R.long_features()):
        got = eng.log_mel(torch.from_numpy(wave[None]))[0].cpu()
        assert got.shape == ref.shape and got.shape[1] == len(wave) // 160 > 3000
        assert float((got - ref).abs().max()) <= 1e-4
        # a window's own maximum would clamp differently somewhere: the fixture does tell the two apart
        from oracle import whisper_ref as w

        alone = torch.from_numpy(w.log_mel(wave[:480_000]))
        assert float((alone - ref[:, :3000]).abs().max()) > 1e-2


def test_longform_on_the_two_recordings():
    """Both recordings through run_longform in shared rounds, windows cut from the engine's own whole-recording log-mel.
    Every window's ids pass the tie policy against the oracle on that window's features; segments follow one another in
    time from the first second to the recording's last window (a random-init model's timestamps are not the audio's, and
    a padded last window may place them up to its 30 s: "cover [0, duration]" is asserted in that form); where no window parts from the recorded ids, seeks and segments are the
    recorded ones."""
    from coral_amd.longform_whisper import run_longform, segments_of

    eng, P, c = _engine()
    z = R.load_golden()
    waves = R.long_waves()
    mels = [eng.log_mel(torch.from_numpy(a[None]))[0] for a in waves]
    oracle_mels = R.long_features()
    P_len = len(R.PREFIX)

    def window_generate(batch):
        feats = torch.stack([torch.nn.functional.pad(mels[i][:, s:s + 3000], (0, max(0, 3000 - (mels[i].shape[1] - s))))
                             for i, s in batch])
        return _generate(eng, feats)

    res = run_longform(window_generate, [m.shape[1] for m in mels], R.TIMESTAMP_BEGIN, P_len, c.pad_token_id, c.eos_token_id)
    for n, r in enumerate(res):
        frames = mels[n].shape[1]
        recorded = {int(s): ids[:k].tolist() for s, ids, k in zip(z[f"long{n}_seek"], z[f"long{n}_ids"], z[f"long{n}_len"])}
        seeks = [s for s, _ in r["windows"]]
        assert seeks[0] == 0 and all(a < b for a, b in zip(seeks, seeks[1:])) and seeks[-1] < frames
        starts, ends = [s[0] for s in r["segments"]], [s[1] for s in r["segments"]]
        assert starts[0] <= R.MAX_INITIAL_TIMESTAMP_INDEX * 0.02 and all(a <= b for a, b in zip(starts, starts[1:]))
        assert all(s <= e for s, e in zip(starts, ends)) and all(a <= b for a, b in zip(ends, ends[1:]))
        assert all(nxt >= end for end, nxt in zip(ends, starts[1:])), "a segment starts before the one in front of it ended"
        # the last window reaches the end of the recording, and its last step takes the loop past it
        last_frames = frames - seeks[-1]
        assert 0 < last_frames <= 3000
        assert seeks[-1] + segments_of(r["windows"][-1][1], R.TIMESTAMP_BEGIN, num_frames=last_frames,
                                       return_advance=True)[1] >= frames
        # every segment lies inside the window that produced it (a padded window may place timestamps up to its 30 s)
        assert ends[-1] <= seeks[-1] * 0.01 + 30.0 and ends[-1] >= seeks[-1] * 0.01
        parted = False
        for seek, gen in r["windows"]:
            assert R.grammar_ok(gen, R.TIMESTAMP_BEGIN, c.eos_token_id), (n, seek, gen)
            if seek not in recorded:
                assert parted, (n, seek, "a seek transformers did not visit, with no divergence before it")
                continue
            rows, _ = _oracle_rows(P, c, R.window_features(oracle_mels[n], seek)[None])
            rep = R.check_timestamp_rows(rows, [R.PREFIX + gen], [R.PREFIX + recorded[seek]], P_len, ACCEPT, FORCED,
                                         label=f"recording {n} seek {seek}")
            parted = parted or rep[0][0] is not None
        if not parted:
            assert seeks == z[f"long{n}_seek"].tolist()
            assert [s[2] for s in r["segments"]] == [ids[:k].tolist() for ids, k in zip(z[f"long{n}_seg_ids"], z[f"long{n}_seg_len"])]
            assert starts == z[f"long{n}_seg_start"].tolist() and ends == z[f"long{n}_seg_end"].tolist()
        print(f"recording {n}: seeks {seeks}, {len(starts)} segments, " + ("parted from" if parted else "equal to") +
              " the recorded run")


def test_transcribe_whisper_long_and_timed(tmp_path):
    """The public surface: a saved checkpoint with its generation config, `transcribe_whisper` on a short and a long
    clip.  Without timestamps the short clip keeps the one-window call and the long one is no longer cut at 30 s; with
    them every clip carries its segments."""
    from coral_amd.evaluate import transcribe_whisper
    from coral_amd.longform_whisper import stitched_ids
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

    model = WhisperForConditionalGeneration(WhisperShape(**R.CONFIG), device=DEV).eval()
    model.engine.load_state_dict(R.fixture_params())
    model.engine.refresh_derived()
    model.generation_config = dict(no_timestamps_token_id=R.NO_TIMESTAMPS, lang_to_id={"<|da|>": R.LANG},
                                   task_to_id={"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE},
                                   max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)
    model.save_pretrained(tmp_path / "m")
    model = WhisperForConditionalGeneration.from_pretrained(str(tmp_path / "m"), device=DEV).eval()
    assert model.generation_config["max_initial_timestamp_index"] == R.MAX_INITIAL_TIMESTAMP_INDEX
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    short, long_ = R.short_waves()[1], R.long_waves()[0]
    texts, rows = transcribe_whisper(model, proc, [short, long_], batch_size=2, max_length=R.MAX_LENGTH)
    plain = model.generate(proc.feature_extractor([short]), max_length=R.MAX_LENGTH)
    assert rows[0] == [int(v) for v in plain[0]] and rows[0][:4] == R.PREFIX_NO_TS
    assert isinstance(texts[1], str) and rows[1][0] >= R.TIMESTAMP_BEGIN
    timed, trows = transcribe_whisper(model, proc, [short, long_], batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True)
    assert trows[1] == rows[1]  # the long clip takes the same loop either way
    for item in timed:
        assert set(item) == {"text", "chunks"} and item["chunks"]
        for ch in item["chunks"]:
            assert set(ch) == {"text", "timestamp"} and ch["timestamp"][0] <= ch["timestamp"][1]
    assert timed[1]["text"] == texts[1]
    assert timed[1]["chunks"][-1]["timestamp"][1] > 30.0  # past the first window: the clip was not cut
    with pytest.raises(ValueError, match="num_beams"):
        transcribe_whisper(model, proc, [long_], num_beams=2)
    assert stitched_ids([(0.0, 1.0, [R.TIMESTAMP_BEGIN, 5, 6, R.TIMESTAMP_BEGIN + 50])], R.TIMESTAMP_BEGIN) == [5, 6]
