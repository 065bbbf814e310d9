"""Whisper beam search on a real MI355X: the two kernels of csrc/beam.hip and the key_slot self-attention exactly, the
engine's search against the fp32 oracle under the tie policy of the greedy tests (tests/greedy_check.py), the
transformers fixtures (tests/golden/whisper_beam.npz) and the public surface."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_beam_ref as bref  # noqa: E402
from whisper_beam_ref import CASES, FIXTURES, MAX_LENGTH, fixture  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
# the tie margins of the greedy tests of the same fixtures at the same depth (24 tokens):
# tests/test_whisper_gpu.py (whisper_tiny) and tests/test_depth_gpu.py (whisper_mid)
MARGINS = {"tiny": (2e-2, 5e-2), "tiny_eos18": (2e-2, 5e-2), "mid": (3e-2, 6e-2), "mid_eos795": (3e-2, 6e-2)}


# ---- ca_beam_select ------------------------------------------------------------------------------------------------------
def _select(logits, sup, run, B, k, V):
    from coral_amd import ops

    lg = logits.to(DEV).contiguous()
    cs = torch.zeros(B, 2 * k, dtype=torch.float32, device=DEV)
    cp = torch.zeros(B, 2 * k, dtype=torch.int32, device=DEV)
    ct = torch.zeros(B, 2 * k, dtype=torch.int32, device=DEV)
    ws = torch.zeros(ops.beam_select_workspace_bytes(B, k, V), dtype=torch.uint8, device=DEV)
    ops.beam_select(lg, None if sup is None else sup.to(DEV), run.to(DEV), B, k, V, lg.stride(0), cs, cp, ct, ws)
    torch.cuda.synchronize()
    return cs.cpu().numpy(), cp.cpu().numpy(), ct.cpu().numpy()


def _reference_ranking(logits, sup, run, B, k, V):
    """float64 log-softmax, suppress as -inf after it, + running score; (score desc, flat index asc)."""
    x = logits[:, :V].double()
    lp = x - x.max(-1, keepdim=True)[0]
    lp = lp - lp.exp().sum(-1, keepdim=True).log()
    if sup is not None:
        lp[:, sup.bool()] = float("-inf")
    acc = (lp + run.double()[:, None]).reshape(B, k * V).numpy()
    order = np.argsort(-acc, axis=1, kind="stable")
    return acc, order


@pytest.mark.parametrize("B,k,V,ldv", [(2, 5, 51865, 51872), (3, 2, 51866, 51872), (1, 16, 51865, 51872), (2, 5, 200, 200),
                                       (8, 16, 2000, 2000)])
def test_beam_select_returns_the_reference_ranking(B, k, V, ldv):
    """Random fp32 logits, tie-free by construction: the values of a row are a permutation of a grid of spacing 2e-4 (far
    above fp32 resolution at these magnitudes) and the test asserts the float64 gaps around the cut.  Same (parent,
    token) order as the reference; no suppressed token.

    Score bound against float64, from V: u = 2^-24.  The sum of exp runs through 8 sequential additions per thread, a
    6-level wave tree, 2 levels over the waves and ceil(V / 2048) sequential chunk additions, each term carrying expf's
    <= 2 ulp, and logf adds <= 2 ulp: a relative error of the sum, hence an absolute error of its log, of at most
    (8 + 6 + 2 + ceil(V / 2048) + 4) u.  The three roundings of ((x - max) - logZ) + run add u times the magnitude of
    each intermediate, and the partial maxima are exact."""
    g = torch.Generator().manual_seed(100 * B + k)
    R = B * k
    logits = torch.zeros(R, ldv)
    for r in range(R):
        logits[r, :V] = (torch.randperm(V, generator=g).float() - V / 2) * 2e-4
    logits[:, V:] = 1e30  # pad columns are never read
    sup = (torch.rand(V, generator=g) < 0.05).to(torch.uint8)
    sup[logits[0, :V].argmax()] = 1  # the best token of a row is masked
    run = -torch.rand(R, generator=g) * 6.0
    run.view(B, k)[0, -1] = -1.0e9
    cs, cp, ct = _select(logits, sup, run, B, k, V)
    acc, order = _reference_ranking(logits, sup, run, B, k, V)
    u = 2.0 ** -24
    for b in range(B):
        top = acc[b, order[b, :2 * k + 1]]
        assert np.all(np.diff(top) < -1e-5), "the fixture has a near-tie at the cut"
        flat = cp[b].astype(np.int64) * V + ct[b]
        assert flat.tolist() == order[b, :2 * k].tolist()
        assert not sup.numpy()[ct[b]].any()
        mag = max(float(np.abs(top).max()), float(logits[:, :V].abs().max()) * 2, float(np.log(V)) + 1)
        bound = (8 + 6 + 2 + -(-V // 2048) + 4) * u + 3 * u * mag
        err = np.abs(cs[b].astype(np.float64) - top[:2 * k]).max()
        print(f"B={B} k={k} V={V} clip {b}: score err {err:.2e} (bound {bound:.2e})")
        assert err <= bound


def test_beam_select_breaks_ties_by_flat_index_and_is_deterministic():
    """Hand-made tables: whole rows of equal logits, equal rows with equal running scores."""
    B, k, V = 2, 3, 4100  # three chunks, the last one ragged
    logits = torch.zeros(B * k, V)
    logits[0, [7, 2049, 4099]] = 1.0
    logits[1] = logits[0]
    logits[2, [5, 6]] = 1.0
    logits[3:] = 0.25  # clip 1: every candidate ties
    run = torch.zeros(B * k)
    run[2] = 0.0
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[[0, 2049]] = 1
    cs, cp, ct = _select(logits, sup, run, B, k, V)
    acc, order = _reference_ranking(logits, sup, run, B, k, V)
    for b in range(B):
        assert (cp[b].astype(np.int64) * V + ct[b]).tolist() == order[b, :2 * k].tolist(), b
    # clip 0: rows 0 and 1 are equal (tokens 7 and 4099 at the top of each), row 2 has two tokens above a lower log-sum-exp
    assert (cp[1] * V + ct[1]).tolist() == [1, 2, 3, 4, 5, 6]  # token 0 is suppressed
    again = _select(logits, sup, run, B, k, V)
    for a, b_ in zip((cs, cp, ct), again):
        assert np.array_equal(a, b_)


# ---- ca_beam_advance --------------------------------------------------------------------------------------------------------
def _advance_on_device(st, cand, eos, lp, early, L):
    """Load the restatement's state into device tables, run ca_beam_advance once, return the tables."""
    from coral_amd import _lib, ops

    B, k, P, cur = st.B, st.k, st.P, st.cur
    R = B * k
    t = lambda x, dt: x.to(dt).to(DEV).contiguous()  # noqa: E731
    g = dict(cand_score=t(cand[0], torch.float32), cand_parent=t(cand[1], torch.int32), cand_token=t(cand[2], torch.int32),
             run_score=t(st.running_scores.reshape(R), torch.float32), tok=torch.zeros(R, dtype=torch.int32, device=DEV),
             pos=torch.full((R,), cur - 1, dtype=torch.int32, device=DEV), klen=torch.full((R,), cur, dtype=torch.int32, device=DEV),
             anc_in=t(torch.arange(R)[:, None].expand(R, L), torch.int32), anc_out=torch.full((R, L), -7, dtype=torch.int32, device=DEV),
             ids_in=t(st.running.reshape(R, L), torch.int32), ids_out=torch.full((R, L), -7, dtype=torch.int32, device=DEV),
             fin_score=t(torch.where(st.finished, st.beam_scores, torch.tensor(-1.0e9)).reshape(R), torch.float32),
             fin_len=t(st.lengths.reshape(R), torch.int32), fin_seq=t(torch.arange(k).repeat(B), torch.int32),
             fin_ids=t(st.sequences.reshape(R, L), torch.int32), fin_count=torch.full((B,), k, dtype=torch.int32, device=DEV),
             heur=t(st.unsat[:, 0], torch.int32), done=torch.zeros(B, dtype=torch.bool, device=DEV),
             tr_parent=torch.zeros(L, B, k, dtype=torch.int32, device=DEV), tr_token=torch.zeros(L, B, k, dtype=torch.int32, device=DEV),
             tr_score=torch.zeros(L, B, k, dtype=torch.float32, device=DEV),
             len_pen=torch.tensor([float(n) ** lp for n in range(L + 1)], dtype=torch.float32).to(DEV))
    d = _lib.CaBeamDesc()
    d.B, d.k, d.max_len, d.prompt_len, d.max_length, d.eos_id, d.early_stopping = B, k, L, P, st.max_length, eos, int(early)
    for n, v in g.items():
        setattr(d, n, v.data_ptr())
    ops.beam_advance(d)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in g.items()}


def _finished_table(scores, lengths, seq, ids):
    """Canonical form of a clip's finished table: entries best first -> [(score, length, ids)]."""
    live = [j for j in range(len(lengths)) if int(lengths[j]) > 0]
    live.sort(key=lambda j: (-float(scores[j]), int(seq[j])))
    return [(float(scores[j]), int(lengths[j]), [int(v) for v in ids[j][:int(lengths[j])]]) for j in live]


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("lp", [1.0, 0.6])
@pytest.mark.parametrize("last", [False, True])
def test_beam_advance_is_the_restatements_single_step(early, lp, last):
    """Constructed states, integer for integer (scores bit for bit): clip 0 - EOS at ranks 0 and 5 (inside and outside the
    first k), table with one entry; clip 1 - already closed (heuristic satisfied, table full); clip 2 - table full, one new
    finisher better than its worst entry and one worse; clip 3 - table full but open, no EOS."""
    B, k, P, eos, pad = 4, 3, 2, 9, 0
    cur = 6
    L = cur + 1 if last else 12
    g = torch.Generator().manual_seed(3)
    st = bref.BeamState([50, 51], B, k, L, pad)
    st.cur = cur
    st.running[:, :, P:cur] = torch.randint(10, 40, (B, k, cur - P), generator=g)
    st.running_scores = -torch.sort(torch.rand(B, k, generator=g) * 3 + 4, dim=1)[0]
    fin = [[-1.5], [-1.2, -1.3, -1.4], [-1.6, -1.9, -2.4], [-3.0, -3.1, -3.2]]
    for b, rows in enumerate(fin):
        for j, sc in enumerate(rows):
            n = 4 + j
            st.sequences[b, j, P:n] = torch.randint(10, 40, (n - P,), generator=g)
            st.sequences[b, j, n - 1] = eos
            st.beam_scores[b, j], st.lengths[b, j], st.finished[b, j] = sc, n, True
    st.unsat[1, 0] = False
    cs = -torch.sort(torch.rand(B, 2 * k, generator=g) * 2 + 7, dim=1)[0]
    cs[2, 0], cs[2, 1] = -8.5, -12.5  # / 5 tokens: -1.7 (enters a full table), -2.5 (does not)
    cp = torch.randint(0, k, (B, 2 * k), generator=g)
    ct = torch.randint(10, 40, (B, 2 * k), generator=g)
    ct[0, 0] = ct[0, 5] = eos
    ct[1, 1] = eos
    ct[2, 0] = ct[2, 1] = eos
    want = bref.BeamState.__new__(bref.BeamState)
    want.__dict__.update({n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.__dict__.items()})
    parent, token, score = bref.advance(want, cs, cp, ct, eos, lp, early)
    got = _advance_on_device(st, (cs, cp, ct), eos, lp, early, L)
    R = B * k
    assert got["tok"].tolist() == token.reshape(R).tolist()
    assert torch.equal(got["run_score"], score.reshape(R))
    assert got["pos"].tolist() == [cur] * R and got["klen"].tolist() == [cur + 1] * R
    step = cur - P
    assert got["tr_parent"][step].tolist() == parent.tolist() and got["tr_token"][step].tolist() == token.tolist()
    assert torch.equal(got["tr_score"][step], score)
    assert got["ids_out"][:, :cur + 1].tolist() == want.running.reshape(R, L)[:, :cur + 1].tolist()
    rows = torch.arange(R).view(B, k)
    for b in range(B):
        for j in range(k):
            src = int(rows[b, int(parent[b, j])])
            assert got["anc_out"][rows[b, j], :cur].tolist() == [src] * cur and int(got["anc_out"][rows[b, j], cur]) == int(rows[b, j])
        mine = _finished_table(got["fin_score"].view(B, k)[b], got["fin_len"].view(B, k)[b], got["fin_seq"].view(B, k)[b],
                               got["fin_ids"].view(B, k, L)[b])
        ref = _finished_table(want.beam_scores[b], want.lengths[b], list(range(k)), want.sequences[b])
        assert [(m[1], m[2]) for m in mine] == [(r[1], r[2]) for r in ref], (b, mine, ref)
        assert [np.float32(m[0]) for m in mine] == [np.float32(r[0]) for r in ref], (b, mine, ref)
    assert got["heur"].tolist() == want.unsat[:, 0].int().tolist()
    assert got["done"].tolist() == bref.clip_done(want, early).tolist()
    if not last and not early and lp == 1.0:  # (the constructed scores keep clips 0, 2 and 3 open at this penalty)
        assert got["done"].tolist() == [False, True, False, False]


# ---- attention through the ancestry table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,H,hd,Lmax", [(6, 4, 64, 40), (10, 6, 16, 24), (128, 4, 64, 72), (5, 16, 64, 448)])
def test_attention_with_key_slot_equals_a_gathered_cache_bit_for_bit(R, H, hd, Lmax):
    """ca_attn_fwd with CaAttnDesc.key_slot == the same kernel over a cache physically gathered on the host by the same
    table; with key_slot NULL == the table that names every row's own cache row (the unchanged kernel)."""
    from coral_amd import ops

    g = torch.Generator().manual_seed(R * 1000 + H)
    d = H * hd
    cache = (torch.randn(R, Lmax, 2 * d, generator=g) * 0.7).to(torch.bfloat16)
    q = torch.randn(R, d, generator=g).to(torch.bfloat16).to(DEV)
    klen = torch.randint(1, Lmax + 1, (R,), generator=g).to(torch.int32)
    klen[0] = Lmax
    slot = torch.randint(0, R, (R, Lmax), generator=g).to(torch.int32)
    gathered = cache[slot.long(), torch.arange(Lmax)[None, :].expand(R, Lmax)]

    def run(c, key_slot):
        c = c.to(DEV).contiguous().view(-1)
        ctx = torch.zeros(R, d, dtype=torch.bfloat16, device=DEV)
        lse = torch.zeros(R * H * 32, dtype=torch.float32, device=DEV)
        ops.attn_fwd(q, c, c, ctx, lse, B=R, H=H, Tq=1, Tk=Lmax, hd=hd, Tqp=32, scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d,
                     ldo=d, sqb=d, skb=Lmax * 2 * d, svb=Lmax * 2 * d, sob=d, k_off=0, v_off=d, klen=klen.to(DEV),
                     key_slot=None if key_slot is None else key_slot.to(DEV).contiguous())
        torch.cuda.synchronize()
        return ctx.cpu(), lse.cpu()

    want, want_lse = run(gathered, None)
    got, got_lse = run(cache, slot)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(got_lse, want_lse)
    own = torch.arange(R, dtype=torch.int32)[:, None].expand(R, Lmax)
    a, b = run(cache, own), run(cache, None)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])
    assert float(got.float().abs().max()) > 0


def test_key_slot_is_refused_outside_the_single_query_decode_form():
    from coral_amd import ops

    R, H, hd, L = 2, 2, 64, 8
    d = H * hd
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    c, lse = z(R * L * 2 * d), torch.zeros(R * H * 32, dtype=torch.float32, device=DEV)
    slot = torch.zeros(R, L, dtype=torch.int32, device=DEV)
    klen = torch.ones(R, dtype=torch.int32, device=DEV)
    kw = dict(B=R, H=H, Tk=L, hd=hd, Tqp=32, scale=1.0, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, skb=L * 2 * d, svb=L * 2 * d,
              k_off=0, v_off=d, key_slot=slot)
    with pytest.raises(ops.CoralAmdError, match="key_slot"):
        ops.attn_fwd(z(R * 2 * d), c, c, z(R * 2 * d), lse, Tq=2, sqb=2 * d, sob=2 * d, klen=klen, **kw)
    with pytest.raises(ops.CoralAmdError, match="key_slot"):
        ops.attn_fwd(z(R * d), c, c, z(R * d), lse, Tq=1, sqb=d, sob=d, klen=None, **kw)


# ---- the engine -------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def _engine(name):
    from coral_amd.whisper import WhisperEngine, WhisperShape

    kw, c, P, feats, prefix, sup, sup_begin = fixture(name)
    if name not in _ENGINES:
        eng = WhisperEngine(WhisperShape(**kw), DEV)
        eng.load_state_dict(P)
        _ENGINES[name] = eng
    return _ENGINES[name], c, P, feats, prefix, sup, sup_begin


def test_new_symbols_are_in_the_library_and_the_signatures():
    from coral_amd import _lib

    lib = _lib.load()
    for sym in ("ca_beam_select_workspace_bytes", "ca_beam_select", "ca_beam_advance"):
        assert sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    assert lib.ca_beam_select_workspace_bytes(8, 5, 51865) > 0


@pytest.mark.parametrize("name", list(FIXTURES))
def test_one_beam_through_the_beam_path_is_the_greedy_launch_sequence(name):
    """num_beams = 1 routed through the beam launches (key_slot self-attention, Tq = k cross-attention, select + advance;
    early_stopping=True: the search of one beam ends at its first EOS, as greedy does) == the greedy launch sequence."""
    eng, c, P, feats, prefix, sup, sup_begin = _engine(name)
    eng._persistent_off = True  # the launch sequence, not the one-launch kernel
    try:
        greedy = eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin)
    finally:
        eng._persistent_off = False
    beam = eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin, num_beams=1,
                        early_stopping=True, _beam_path=True)
    assert beam == greedy


def test_generate_num_beams_5_returns_the_transformers_beam_ids(golden_dir):
    """The clip whose beam result leaves its greedy path (tests/test_whisper_beam_ref.py: clip 0 of whisper_mid): before
    this feature generate(num_beams=5) returned the greedy ids.  (whisper_tiny at 5 beams is no fixture for an exact
    comparison: the fp32 oracle's own margin at the cut-off is 0.005 at position 18 of clip 0 and 0.008 at position 5 of
    clip 1, inside the 2e-2 by which bf16 logits may move; the tie-policy test below covers it.)"""
    z = np.load(golden_dir / "whisper_beam.npz")
    zg = np.load(golden_dir / "whisper_mid.npz")
    eng, c, P, feats, prefix, sup, sup_begin = _engine("mid")
    ids = eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin, num_beams=5)
    want = z["mid:k5:lp1.0:es0:ids"].tolist()
    assert want[0] != zg["greedy_ids"][0].tolist()
    assert ids[0] == want[0]


def test_public_generate_refuses_and_passes_through():
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperForConditionalGeneration

    model = WhisperForConditionalGeneration(WhisperShape(d_model=64, encoder_layers=1, decoder_layers=1, encoder_attention_heads=1,
                                                         decoder_attention_heads=1, encoder_ffn_dim=64, decoder_ffn_dim=64),
                                            device=DEV).eval()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    for kw in (dict(num_return_sequences=2), dict(do_sample=True), dict(early_stopping="never"), dict(temperature=0.5)):
        with pytest.raises(ValueError):
            model.generate(feats, max_length=8, num_beams=2, **kw)
    with pytest.raises(ValueError, match="16"):
        model.generate(feats, max_length=8, num_beams=17)
    with pytest.raises(ValueError, match="128"):
        model.generate(torch.zeros(33, 80, 3000), max_length=8, num_beams=4)
    greedy = model.generate(feats, max_length=8)
    assert model.generate(feats, max_length=8, num_beams=1) == greedy and model.generate(feats, max_length=8, num_beams=None) == greedy
    beam = model.generate(feats, max_length=8, num_beams=3, length_penalty=1.0, early_stopping=False)
    assert len(beam) == 2 and all(r[:4] == greedy[0][:4] and len(r) <= 8 for r in beam)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_search_against_the_oracle_under_the_tie_policy(golden_dir, name):
    """The beam analogue of tests/greedy_check.py.  The engine's own trace is replayed: at every step the fp32 oracle's
    log-probs of the engine's OWN running prefixes give the candidate scores (oracle log-prob + oracle score of the
    prefix); the cut-off is the oracle's k-th best candidate that does not stop.
      1. every running beam the engine kept is within `accept` of the cut-off;
      2. every oracle candidate more than `forced` above the cut-off was kept;
      3. the engine's recorded running scores agree with the oracle's within `accept` x generated tokens;
    the returned sequence is the best hypothesis of the engine's own finished table, whose scores agree likewise; and
    against the transformers ids the first differing position is a step whose oracle margin at the cut-off is at most
    `forced`.  accept / forced: those of the greedy tests of the same fixture and depth."""
    from oracle import whisper_ref as w

    accept, forced = MARGINS[name]
    z = np.load(golden_dir / "whisper_beam.npz")
    eng, c, P, feats, prefix, sup, sup_begin = _engine(name)
    with torch.no_grad():
        enc = w.encoder(feats, P, c)
    B, Pn, eos = 2, len(prefix), c.eos_token_id
    for k, lp, es in CASES:
        key = f"{name}:k{k}:lp{lp}:es{int(es)}"
        ids, tr = eng.generate(feats, prefix, MAX_LENGTH, suppress_tokens=sup, begin_suppress_tokens=sup_begin, num_beams=k,
                               length_penalty=lp, early_stopping=es, return_trace=True)
        prefixes = [[list(prefix) for _ in range(k)] for _ in range(B)]
        osc = torch.full((B, k), -1.0e9, dtype=torch.float64)
        osc[:, 0] = 0.0
        margins = []  # per step, per clip: the oracle's margin at the cut-off
        worst_keep, worst_score = 0.0, 0.0
        for t in range(tr["steps"]):
            cur = Pn + t
            rows = torch.tensor([p for clip in prefixes for p in clip])
            with torch.no_grad():
                lg = w.decoder(rows, enc.repeat_interleave(k, dim=0), P, c)[:, -1]
            lpo = bref.masked_log_probs(lg, cur, Pn, sup, sup_begin).double().reshape(B, k, -1)
            V = lpo.shape[-1]
            acc = lpo + osc[:, :, None]
            last = cur + 1 >= MAX_LENGTH
            new_prefixes, new_osc, step_margin = [], osc.clone(), []
            for b in range(B):
                par, tok, sc = tr["parent"][t, b].tolist(), tr["token"][t, b].tolist(), tr["score"][t, b]
                cand = acc[b].clone()
                if not last:
                    cand[:, eos] = float("-inf")  # candidates that stop are not running beams
                    flat = cand.reshape(-1)
                    top = torch.sort(flat, descending=True)[0]
                    cut, nxt = float(top[k - 1]), float(top[k])
                    step_margin.append(cut - nxt)
                    kept = {p * V + v for p, v in zip(par, tok)}
                    assert len(kept) == k, (key, t, b, "a running beam twice")
                    for p, v in zip(par, tok):
                        worst_keep = max(worst_keep, cut - float(cand[p, v]))
                        assert float(cand[p, v]) >= cut - accept, (key, t, b, p, v, float(cand[p, v]), cut)
                    must = torch.nonzero(flat > cut + forced).flatten().tolist()
                    assert set(must) <= kept, (key, t, b, "a candidate above the forced margin was dropped")
                    for j in range(k):
                        new_osc[b, j] = acc[b, par[j], tok[j]]
                        worst_score = max(worst_score, abs(float(sc[j]) - float(new_osc[b, j])))
                        assert abs(float(sc[j]) - float(new_osc[b, j])) <= accept * (t + 1), (key, t, b, j)
                else:
                    step_margin.append(float("inf"))
                new_prefixes.append([prefixes[b][par[j]] + [tok[j]] for j in range(k)])
            prefixes, osc = new_prefixes, new_osc
            margins.append(step_margin)
        # the finished table: scores against the oracle's, and the returned sequence is its best entry
        for b in range(B):
            table = _finished_table(tr["fin_score"][b], tr["fin_len"][b], tr["fin_seq"][b], tr["fin_ids"][b])
            assert table, (key, b)
            pad = [c.pad_token_id] * (len(ids[b]) - table[0][1])
            assert ids[b] == table[0][2] + pad, (key, b)
            for score, n, seq in table:
                with torch.no_grad():
                    lg = w.decoder(torch.tensor([seq[:-1]]), enc[b:b + 1], P, c)[0]
                tot = 0.0
                for pos in range(Pn, n):
                    row = bref.masked_log_probs(lg[pos - 1], pos, Pn, sup, sup_begin).double()
                    tot += float(row[seq[pos]])
                gen = n - Pn
                assert abs(score - tot / gen ** lp) <= accept * gen / gen ** lp, (key, b, score, tot / gen ** lp)
        want = z[key + ":ids"].tolist()
        first = []
        for b in range(B):
            n = max(len(ids[b]), len(want[b]))
            a_, w_ = ids[b] + [c.pad_token_id] * (n - len(ids[b])), want[b] + [c.pad_token_id] * (n - len(want[b]))
            div = next((i for i in range(n) if a_[i] != w_[i]), None)
            first.append(div)
        print(f"{key}: kept within {worst_keep:.4f} of the cut-off (accept {accept}), running scores within {worst_score:.4f}; "
              f"first difference from the transformers ids at {first}")
        for b, div in enumerate(first):
            if div is not None:
                t = div - Pn
                assert 0 <= t < len(margins), (key, b, div)
                print(f"  clip {b}: position {div}, oracle margin at the cut-off of that step {margins[t][b]:.5f}")
                assert margins[t][b] <= forced, (key, b, div, margins[t][b])


def test_evaluate_with_num_beams_from_the_config(tmp_path, monkeypatch):
    """evaluate() on a saved Whisper checkpoint: num_beams=5 runs and returns ids; without the key the id rows are
    those of greedy decoding."""
    sys.path.insert(0, str(ROOT / "scripts"))
    import finetune_asr_model

    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.whisper_setup import prefix_ids

    monkeypatch.chdir(tmp_path)
    res = finetune_asr_model.main(["model=test-whisper", "datasets=synthetic", f"models_dir={tmp_path}", "model_id=wbeam",
                                   "max_steps=1", "total_batch_size=2", "per_device_batch_size=2",
                                   "max_seconds_per_example=2.0", "min_seconds_per_example=1.0", "logging_steps=1",
                                   "eval_steps=2", "model.max_length=12"])
    shape = res["model"].shape
    over = [f"model_id={tmp_path / 'wbeam'}", "batch_size=3", "generation_max_length=10", "dataset=synthetic",
            "store_results=false"]
    greedy = evaluate(load_config("evaluation", over + ["num_beams=1"]))["token_ids"]
    cfg = load_config("evaluation", over)
    del cfg["num_beams"]
    assert evaluate(cfg)["token_ids"] == greedy
    beam = evaluate(load_config("evaluation", over + ["num_beams=5"]))["token_ids"]
    assert len(beam) == len(greedy) == 6
    for r in beam:
        assert r[:4] == prefix_ids(shape) and 4 < len(r) <= 10 and r[4] not in (220, shape.eos_token_id)
