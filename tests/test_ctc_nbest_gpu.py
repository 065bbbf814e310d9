"""`ca_ctc_beam_decode_ex` on the GPU: n-best output and hotword boosting against brute force over every alignment on the
tiny cases, row 0 against `ca_ctc_beam_decode` bit for bit, the n-best list against the test-side restatement
(tests/ctc_hotword_ref.py) at 8 x 499 frames with and without LM and with hotwords under a narrow beam, ragged lengths
with fewer finals than n_best, argument validation, and end to end through `evaluate`.

Tolerances are those of tests/test_ctc_beam_gpu.py: 1e-4 absolute on the tiny cases; at real size
tol = T * |S| * 2^-23 (one fp32 rounding per frame on a score of magnitude |S|)."""
import functools
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref as ref  # noqa: E402
import ctc_hotword_ref as href  # noqa: E402
from test_ctc_beam_gpu import BLANK, DELIM, FORBIDDEN, V, TinyTok, fixture_lms, gpu_decode, regime  # noqa: E402
from test_ctc_beam_host import ARPA, ARPA_NOUNK, EXHAUSTIVE, TINY, coral_tokenizer, tiny_cases  # noqa: E402
from test_ctc_nbest_cpu import HOT_SETTINGS, N_TINY  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
T_REAL = 499
N_REAL = 10
# the hotword test: in-lexicon words and two the LM has not seen, which are spliced into the label strings; the seed is
# chosen on the CPU with the restatement alone (float32 = float64 on the ranks compared; every utterance's best string
# changes under the hotwords) - both asserted below before the kernel is consulted
HOTWORDS = ["ab", "ba", "cæb", "zyx", "qåq"]
OOV = ["zyx", "qåq"]
HOT_SEED, HOT_BEAM, HOT_N = 1, 16, 4


def gpu_nbest(logits, n_best, in_len=None, lm=None, tok=None, hotwords=None, hotword_weight=10.0, blank=BLANK, delim=DELIM,
              forbidden=FORBIDDEN, beam_width=100, **params):
    """logits [B, T, V] -> (per row the list of (ids tuple, score, logit_score, lm_score) of its real rows, raw host
    arrays) through ops.ctc_beam_decode_ex; the padding rules of the unused rows are asserted here for every call"""
    from coral_amd import ngram, ops

    x = torch.as_tensor(logits, dtype=torch.float32).cuda().contiguous()
    B, T, Vv = x.shape
    ids = torch.full((B, n_best, T), 7, dtype=torch.int32, device="cuda")
    olen = torch.full((B, n_best), 7, dtype=torch.int32, device="cuda")
    split = torch.full((3, B, n_best), 7.0, dtype=torch.float32, device="cuda")
    n_out = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, Vv, beam_width), dtype=torch.uint8, device="cuda")
    forb = torch.zeros(Vv, dtype=torch.uint8)
    forb[list(forbidden)] = 1
    il = None if in_len is None else torch.as_tensor(in_len, dtype=torch.int32).cuda()
    tables = None if lm is None else lm.device_tables(tok, "cuda")
    hot = None if hotwords is None else ngram.hotword_tables(hotwords, tok, "cuda")
    ops.ctc_beam_decode_ex(x, il, ids, olen, split[0], split[1], split[2], n_out, ws, B, T, Vv, Vv, blank, delim, forb.cuda(),
                           tables, n_best=n_best, hotwords=hot, hotword_weight=hotword_weight, beam_width=beam_width,
                           **params)
    torch.cuda.synchronize()
    raw = dict(ids=ids.cpu().numpy(), len=olen.cpu().numpy(), score=split[0].cpu().numpy(), logit=split[1].cpu().numpy(),
               lm=split[2].cpu().numpy(), n_out=n_out.cpu().numpy())
    rows = []
    for b in range(B):
        n = int(raw["n_out"][b])
        assert 0 <= n <= n_best
        assert (raw["len"][b, n:] == -1).all() and (raw["ids"][b, n:] == -1).all()
        for k in ("score", "logit", "lm"):
            assert (raw[k][b, n:] == -np.inf).all()
        assert (raw["len"][b, :n] >= 0).all() and (raw["score"][b, :n] > -np.inf).all()
        for r in range(n):
            assert (raw["ids"][b, r, raw["len"][b, r]:] == -1).all()
        # score = logit_score + lm_score bit for bit, in fp32
        assert (raw["logit"][b, :n] + raw["lm"][b, :n]).tobytes() == raw["score"][b, :n].tobytes()
        rows.append([(tuple(int(c) for c in raw["ids"][b, r, :raw["len"][b, r]]), float(raw["score"][b, r]),
                      float(raw["logit"][b, r]), float(raw["lm"][b, r])) for r in range(n)])
    return rows, raw


@pytest.mark.parametrize("hot", list(HOT_SETTINGS))
@pytest.mark.parametrize("mode", ["lm", "lm_nounk", "plain"])
def test_n_best_against_brute_force_on_tiny_cases(mode, hot):
    from coral_amd.ngram import NGramLM

    path = dict(lm=ARPA, lm_nounk=ARPA_NOUNK, plain=None)[mode]
    lm, rlm = (NGramLM.from_arpa(path), ref.RefLM(path)) if path else (None, None)
    params = dict(alpha=0.0, beta=0.0) if mode == "plain" else {}
    words, weight = HOT_SETTINGS[hot]
    cases = tiny_cases()
    # the 20 cases as one batch: T <= 4, shorter ones through in_len
    x = np.zeros((len(cases), 4, 4), dtype=np.float32)
    for i, c in enumerate(cases):
        x[i, :len(c)] = c
    want = []
    for logits in cases:
        exact = href.brute_force(logits, lm=rlm, hotwords=words, hotword_weight=weight, **TINY, **params)
        order = href.ranked(exact)[:N_TINY + 1]
        gaps = [exact[order[i]] - exact[order[i + 1]] for i in range(N_TINY)]
        assert min(gaps) >= 1e-3  # the cases' own margin among ranks 1..9: ten times the fp32 tolerance below
        want.append([(y, exact[y]) for y in order[:N_TINY]])
    rows, _ = gpu_nbest(x, N_TINY, in_len=[len(c) for c in cases], lm=lm, tok=TinyTok(), hotwords=list(words),
                        hotword_weight=weight, blank=0, delim=3, forbidden=(), **EXHAUSTIVE, **params)
    for i, (got, exp) in enumerate(zip(rows, want)):
        err = max(abs(g[1] - e[1]) for g, e in zip(got, exp))
        print(mode, hot, i, "max score err %.3e" % err)
        assert [g[0] for g in got] == [e[0] for e in exp], i
        assert err <= 1e-4


@pytest.mark.parametrize("use_lm", [True, False], ids=["lm", "nolm"])
@pytest.mark.parametrize("kind", ["confident", "noisy"])
def test_row_0_is_the_answer_of_the_plain_entry_bit_for_bit(kind, use_lm):
    lm, _ = fixture_lms()
    tok = coral_tokenizer()
    x = regime(kind)
    ids, score = gpu_decode(x, lm=lm if use_lm else None, tok=tok)
    for kw in (dict(), dict(hotwords=[]), dict(hotwords=["ab", "zyx"], hotword_weight=0.0)):
        rows, raw = gpu_nbest(x, N_REAL, lm=lm if use_lm else None, tok=tok, **kw)
        assert [r[0][0] for r in rows] == ids
        assert raw["score"][:, 0].tobytes() == score.tobytes()
    rows1, raw1 = gpu_nbest(x, 1, lm=lm if use_lm else None, tok=tok)
    assert [r[0][0] for r in rows1] == ids and raw1["score"][:, 0].tobytes() == score.tobytes()


def ctc_log_likelihoods(x, strings):
    """ln P_ctc of one label string per row of x, from the loss kernel"""
    from coral_amd import ops

    B, T, Vv = x.shape
    Lmax = max(1, max(len(s) for s in strings))
    lab = torch.full((B, Lmax), -100, dtype=torch.int32)
    for b, s in enumerate(strings):
        lab[b, :len(s)] = torch.tensor(s, dtype=torch.int32)
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.ctc_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device="cuda")
    ops.ctc_loss_fwd_bwd(torch.from_numpy(np.ascontiguousarray(x)).cuda(), lab.cuda(),
                         torch.full((B,), T, dtype=torch.int32).cuda(), nll, None, None, ws, B, T, Vv, Vv, Lmax, BLANK,
                         zero_infinity=False)
    torch.cuda.synchronize()
    return -nll.cpu().numpy()


def check_against_restatement(x, rows, want64, n, what):
    """the n-best assertions shared by the tests at real size; want64: the restatement's ranked finals per utterance"""
    B, T, _ = x.shape
    loglik = ctc_log_likelihoods(np.repeat(x, [len(r) for r in rows], axis=0), [h[0] for r in rows for h in r])
    at = 0
    for b, (got, want) in enumerate(zip(rows, want64)):
        finals = {y: (s, lg, lms) for y, s, lg, lms in want}
        assert len(got) == min(n, len(want)), b
        tol = T * abs(want[0][1]) * 2.0 ** -23
        scores = [g[1] for g in got]
        assert all(a >= c for a, c in zip(scores, scores[1:])), b  # non-increasing
        for r, (y, s, lg, lms) in enumerate(got):
            assert y in finals, (b, r, y)
            ws, wl, wm = finals[y]
            print(what, b, r, "same string", y == want[r][0], "score err %.3e logit err %.3e lm err %.3e tol %.3e"
                  % (abs(s - ws), abs(lg - wl), abs(lms - wm), tol), "rank gap %.3e" % (want[r][1] - s))
            assert abs(s - ws) <= tol and abs(lg - wl) <= tol and abs(lms - wm) <= tol
            assert want[r][1] - s <= tol  # rank r of the kernel is no worse than rank r of the restatement
            assert lg <= loglik[at] + T * abs(float(loglik[at])) * 2.0 ** -23  # the beam sums a subset of the alignments
            at += 1


@functools.lru_cache(maxsize=None)
def restated(use_lm, dtype):
    tok = coral_tokenizer()
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    return [href.prefix_beam_search_nbest(u, BLANK, DELIM, id2char, ref.RefLM(ARPA) if use_lm else None, FORBIDDEN,
                                          dtype=getattr(np, dtype)) for u in regime("noisy")]


@pytest.mark.parametrize("use_lm", [True, False], ids=["lm", "nolm"])
def test_n_best_within_rounding_of_the_restatement(use_lm):
    want64, want32 = restated(use_lm, "float64"), restated(use_lm, "float32")
    for a, c in zip(want64, want32):  # seed condition, on the restatement alone
        assert [f[0] for f in a[:N_REAL]] == [f[0] for f in c[:N_REAL]]
    lm, _ = fixture_lms()
    x = regime("noisy")
    rows, _ = gpu_nbest(x, N_REAL, lm=lm if use_lm else None, tok=coral_tokenizer())
    check_against_restatement(x, rows, want64, N_REAL, "nbest lm" if use_lm else "nbest nolm")


@functools.lru_cache(maxsize=None)
def hotword_regime():
    tok = coral_tokenizer()
    words = sorted(w for w in ref.RefLM(ARPA).unigrams if not w.startswith("<")) + OOV
    lex = [[tok.vocab[c] for c in w] for w in words]
    return ref.regime_logits("noisy", HOT_SEED, 8, T_REAL, V, BLANK, lex, DELIM)


def test_hotwords_under_a_narrow_beam_within_rounding_of_the_restatement():
    tok = coral_tokenizer()
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    rlm = ref.RefLM(ARPA)
    assert not set(OOV) & rlm.unigrams and set(HOTWORDS) - set(OOV) <= rlm.unigrams
    x = hotword_regime()
    kw = dict(hotwords=HOTWORDS, hotword_weight=10.0, beam_width=HOT_BEAM)
    want64 = [href.prefix_beam_search_nbest(u, BLANK, DELIM, id2char, rlm, FORBIDDEN, **kw) for u in x]
    want32 = [href.prefix_beam_search_nbest(u, BLANK, DELIM, id2char, rlm, FORBIDDEN, dtype=np.float32, **kw) for u in x]
    plain = [href.prefix_beam_search_nbest(u, BLANK, DELIM, id2char, rlm, FORBIDDEN, beam_width=HOT_BEAM) for u in x]
    for a, c in zip(want64, want32):  # seed condition
        assert [f[0] for f in a[:HOT_N]] == [f[0] for f in c[:HOT_N]]
    flipped = sum(a[0][0] != p[0][0] for a, p in zip(want64, plain))
    assert flipped >= 1  # the bonus decides something: the test cannot pass with it ignored
    lm, _ = fixture_lms()
    rows, _ = gpu_nbest(x, HOT_N, lm=lm, tok=tok, **kw)
    check_against_restatement(x, rows, want64, HOT_N, "hotwords")
    base, _ = gpu_nbest(x, HOT_N, lm=lm, tok=tok, beam_width=HOT_BEAM)
    print("best strings changed by the hotwords: restatement", flipped, "kernel", sum(r[0][0] != q[0][0] for r, q in zip(rows, base)))
    assert sum(r[0][0] != q[0][0] for r, q in zip(rows, base)) >= 1


def test_ragged_lengths_and_fewer_finals_than_n_best():
    lm, _ = fixture_lms()
    tok = coral_tokenizer()
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    rlm = ref.RefLM(ARPA)
    x = regime("noisy")[:4].copy()
    T = x.shape[1]
    in_len = [1, T, 137, 0]
    rng = np.random.RandomState(5)
    y = x.copy()
    for b, n in enumerate(in_len):
        x[b, n:] = 50.0 * rng.randn(T - n, V)
        y[b, n:] = np.float32(-3.0)
    kw = dict(in_len=in_len, lm=lm, tok=tok, token_min_logp=-0.05)
    a_rows, a = gpu_nbest(x, N_REAL, **kw)
    b_rows, b = gpu_nbest(y, N_REAL, **kw)
    c_rows, c = gpu_nbest(x, N_REAL, **kw)
    r_rows, r = gpu_nbest(x[::-1].copy(), N_REAL, **dict(kw, in_len=in_len[::-1]))
    for k in a:  # frames past in_len are ignored; bit-identical from run to run and under batch reversal
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes() == r[k][::-1].tobytes(), k
    # the number of real rows is the number of finals the restatement has, capped at n_best
    want = [href.prefix_beam_search_nbest(x[i], BLANK, DELIM, id2char, rlm, FORBIDDEN, in_len=in_len[i], token_min_logp=-0.05)
            for i in range(4)]
    print("finals", [len(w) for w in want], "n_out", a["n_out"].tolist())
    assert a["n_out"].tolist() == [min(N_REAL, len(w)) for w in want]
    assert any(0 < n < N_REAL for n in a["n_out"])  # the padding rules (asserted in gpu_nbest) are exercised
    assert a_rows[3] == [((), 0.0, 0.0, 0.0)] or (len(a_rows[3]) == 1 and a_rows[3][0][0] == ())
    for i in range(4):
        assert [g[0] for g in a_rows[i]][:1] == [want[i][0][0]]
        assert abs(a_rows[i][0][1] - want[i][0][1]) <= max(1e-4, T * abs(want[i][0][1]) * 2.0 ** -23)


def test_argument_validation_reports_through_last_error():
    from coral_amd._lib import CoralAmdError

    x = np.zeros((1, 4, 8), dtype=np.float32)
    kw = dict(blank=0, delim=3, forbidden=())
    with pytest.raises(CoralAmdError, match="n_best 0 outside 1..beam_width = 100"):
        gpu_nbest(x, 0, **kw)
    with pytest.raises(CoralAmdError, match="n_best 17 outside 1..beam_width = 16"):
        gpu_nbest(x, 17, beam_width=16, **kw)
    with pytest.raises(CoralAmdError, match="hotword_weight must be a finite number"):
        gpu_nbest(x, 2, tok=TinyTok(), hotwords=["ab"], hotword_weight=math.nan, **kw)
    with pytest.raises(CoralAmdError, match="beam_width 129"):
        gpu_nbest(x, 2, beam_width=129, **kw)
    rows, _ = gpu_nbest(x, 16, beam_width=16, **kw)  # the limits themselves are served
    assert len(rows[0]) >= 1


def test_evaluate_with_n_best_and_hotwords(tmp_path, monkeypatch):
    sys.path.insert(0, str(ROOT / "scripts"))
    import finetune_asr_model

    from coral_amd import modeling, ops
    from coral_amd.config import DictConfig, load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.model_setup import load_model_setup
    from coral_amd.ngram import NGramLM
    from coral_amd.processor import Wav2Vec2ProcessorWithLM

    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(modeling.HUB_SHAPES, "facebook/wav2vec2-xls-r-300m",
                        dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=4))
    finetune_asr_model.main(["model=test-wav2vec2", "datasets=synthetic", f"models_dir={tmp_path}", "model_id=nbev",
                             "max_steps=2", "total_batch_size=2", "per_device_batch_size=2",
                             "max_seconds_per_example=2.0", "min_seconds_per_example=1.0", "logging_steps=1",
                             "eval_steps=2"])
    mdir = tmp_path / "nbev"
    saved = load_model_setup(DictConfig(model=DictConfig(type="wav2vec2", sampling_rate=16_000, decoder=None),
                                        model_dir=str(mdir), padding="longest", max_seconds_per_example=10)).load_saved()
    lm = NGramLM.from_arpa(ARPA)
    Wav2Vec2ProcessorWithLM(saved.processor.feature_extractor, saved.processor.tokenizer, lm).save_pretrained(mdir)
    rng = np.random.RandomState(3)
    examples = [dict(audio=(0.1 * rng.randn(int(16_000 * s))).astype(np.float32), text="a ab") for s in (1.0, 1.6, 1.2, 2.0)]

    calls = []
    real = ops.ctc_beam_decode_ex

    def spy(*args, **kw):
        calls.append(dict(n_best=kw["n_best"], weight=kw["hotword_weight"],
                          n_hot=0 if kw["hotwords"] is None else kw["hotwords"]["hot_keys"].numel()))
        return real(*args, **kw)

    monkeypatch.setattr(ops, "ctc_beam_decode_ex", spy)

    def run(*extra):
        import csv

        cfg = load_config("evaluation", [f"model_id={mdir}", "batch_size=2", "dataset=synthetic", "store_results=true",
                                         "error_rates=device", *extra])
        scores = evaluate(cfg, examples)
        return scores, [r[0] for r in list(csv.reader(open(scores["csv"])))[1:]]

    plain, plain_preds = run()
    assert not calls and "n_best" not in plain and "oracle_cer" not in plain  # the defaults: the call of before
    assert not list(tmp_path.glob("*.nbest.jsonl"))
    scores, preds = run("n_best=5")
    assert preds == plain_preds and (scores["cer"], scores["wer"]) == (plain["cer"], plain["wer"])
    assert [c["n_best"] for c in calls] == [5, 5] and all(c["n_hot"] == 0 for c in calls)
    assert scores["oracle_cer"] <= scores["cer"] and scores["oracle_wer"] <= scores["wer"]
    lines = [json.loads(l) for l in open(scores["nbest_jsonl"], encoding="utf-8")]
    assert len(lines) == len(examples)
    for line, pred, hyps in zip(lines, preds, scores["n_best"]):
        assert line["label"] == "a ab" and 1 <= len(line["n_best"]) <= 5 and line["n_best"] == hyps
        assert line["n_best"][0]["text"].lower().strip() == pred
        assert abs(sum(h["posterior"] for h in hyps) - 1.0) < 1e-9
        for h in hyps:
            assert np.float32(h["logit_score"]) + np.float32(h["lm_score"]) == np.float32(h["score"])
    # hotwords from the configuration reach the kernel: the table of the three words' prefixes, the weight of the key
    del calls[:]
    run("hotwords=[ab,Cæb b]", "hotword_weight=4.5")
    assert calls and all(c == dict(n_best=1, weight=4.5, n_hot=len({"a", "ab", "c", "cæ", "cæb", "b"})) for c in calls)

    # ... and decide the result: a logits fixture through the saved model's engine, where the hotword flips the best string
    eng, tok = saved.model.engine, saved.processor.tokenizer
    proc = Wav2Vec2ProcessorWithLM.from_pretrained(mdir)
    Vm, blank, delim = eng.s.vocab_size, eng.s.pad_token_id, tok.vocab["|"]
    x = np.full((1, 6, Vm), -4.0, dtype=np.float32)
    a, b_ = tok.vocab["a"], tok.vocab["z"]
    for t, (c, alt) in enumerate([(a, b_), (blank, blank), (delim, delim), (a, b_), (blank, blank), (blank, blank)]):
        x[0, t, c] = 4.0
        if alt != c:
            x[0, t, alt] = 3.0  # "z" one nat behind "a" in frames 0 and 3
    logits = torch.from_numpy(x).to(eng.device)
    tables = proc.device_tables(eng.device)
    ids0, _ = eng.beam_decode(tables, tokenizer=tok, logits=logits)
    hyp = eng.beam_decode(tables, tokenizer=tok, logits=logits, hotwords=proc.hotword_tables(["z"], eng.device),
                          hotword_weight=30.0, n_best=3)
    assert tok.decode(ids0[0], group_tokens=False).strip() == "a a"
    assert tok.decode(hyp[0][0]["ids"], group_tokens=False).strip() == "z z"
    assert 1 <= len(hyp[0]) <= 3 and [h["score"] for h in hyp[0]] == sorted((h["score"] for h in hyp[0]), reverse=True)
