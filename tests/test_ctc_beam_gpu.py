"""`ca_ctc_beam_decode` on the GPU: against brute force over every alignment on tiny inputs, against the test-side float64
prefix beam search (tests/ctc_beam_ref.py) at real size in three regimes of seeded logits, against `ca_ctc_loss_fwd_bwd`
in no-LM mode, run-to-run determinism, ragged lengths, and end to end through `evaluate`.

Tolerances: 1e-4 absolute on the tiny cases (fp32 log-sum-exp over at most 256 paths of magnitude about 10: a few hundred
roundings of 1.2e-7 relative); at real size tol = T * |S| * 2^-23 (worst-case linear accumulation of one fp32 rounding
per frame on a score of magnitude |S|)."""
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_beam_ref as ref  # noqa: E402
from test_ctc_beam_host import ARPA, ARPA_NOUNK, EXHAUSTIVE, TINY, coral_tokenizer, tiny_cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
V, BLANK, DELIM = 46, 45, 36
FORBIDDEN = (42, 43, 44)  # <s>, </s>, <unk> of the CoRal vocabulary
# seeds chosen on the CPU with the helper alone: "confident" leads by >= 1 nat on every utterance; "noisy" and "flat"
# give the same best string in float32 and float64 (both asserted below before the kernel is consulted)
SEEDS = dict(confident=1, noisy=1, flat=2)
SHAPE = dict(confident=(8, 499), noisy=(8, 499), flat=(8, 60))


def gpu_decode(logits, in_len=None, lm=None, tok=None, blank=BLANK, delim=DELIM, forbidden=FORBIDDEN, beam_width=100, **params):
    """logits np/torch [B, T, V] -> (list of id tuples, scores np fp32 [B]) through ops.ctc_beam_decode"""
    from coral_amd import ops

    x = torch.as_tensor(logits, dtype=torch.float32).cuda().contiguous()
    B, T, Vv = x.shape
    ids = torch.empty(B, T, dtype=torch.int32, device="cuda")
    olen = torch.empty(B, dtype=torch.int32, device="cuda")
    score = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, Vv, beam_width), dtype=torch.uint8, device="cuda")
    forb = torch.zeros(Vv, dtype=torch.uint8)
    forb[list(forbidden)] = 1
    il = None if in_len is None else torch.as_tensor(in_len, dtype=torch.int32).cuda()
    tables = None if lm is None else lm.device_tables(tok, "cuda")
    ops.ctc_beam_decode(x, il, ids, olen, score, ws, B, T, Vv, Vv, blank, delim, forb.cuda(), tables, beam_width=beam_width,
                        **params)
    torch.cuda.synchronize()
    ids, olen = ids.cpu().numpy(), olen.cpu().numpy()
    for b in range(B):
        assert (ids[b, olen[b]:] == -1).all()
    return [tuple(int(c) for c in ids[b, :olen[b]]) for b in range(B)], score.cpu().numpy()


class TinyTok:
    """tokenizer view of the tiny alphabet {blank = 0, a = 1, b = 2, | = 3}"""
    word_delimiter_token = "|"

    def get_vocab(self):
        return {"<pad>": 0, "a": 1, "b": 2, "|": 3}


def fixture_lms():
    from coral_amd.ngram import NGramLM

    return NGramLM.from_arpa(ARPA), ref.RefLM(ARPA)


@functools.lru_cache(maxsize=None)
def regime(kind):
    tok = coral_tokenizer()
    words = sorted(w for w in ref.RefLM(ARPA).unigrams if not w.startswith("<"))
    lex = [[tok.vocab[c] for c in w] for w in words]
    B, T = SHAPE[kind]
    return ref.regime_logits(kind, SEEDS[kind], B, T, V, BLANK, lex, DELIM)


@functools.lru_cache(maxsize=None)
def helper(kind, use_lm, dtype="float64", **params):
    """the helper's (best ids, score, final beams) per utterance of a regime"""
    tok = coral_tokenizer()
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    lm = ref.RefLM(ARPA) if use_lm else None
    return [ref.prefix_beam_search(x, BLANK, DELIM, id2char, lm, FORBIDDEN, dtype=getattr(np, dtype), **params)
            for x in regime(kind)]


@pytest.mark.parametrize("mode", ["lm", "lm_nounk", "plain"])
def test_kernel_against_brute_force_on_tiny_cases(mode):
    from coral_amd.ngram import NGramLM

    path = dict(lm=ARPA, lm_nounk=ARPA_NOUNK, plain=None)[mode]
    lm, rlm = (NGramLM.from_arpa(path), ref.RefLM(path)) if path else (None, None)
    params = dict(alpha=0.0, beta=0.0) if mode == "plain" else {}
    for logits in tiny_cases():
        exact = ref.brute_force(logits, lm=rlm, **TINY, **params)
        order = sorted(exact, key=exact.get, reverse=True)
        assert exact[order[0]] - exact[order[1]] >= 1e-3  # the cases' own margin: ten times the fp32 tolerance below
        ids, score = gpu_decode(logits[None], lm=lm, tok=TinyTok(), blank=0, delim=3, forbidden=(), **EXHAUSTIVE, **params)
        print(mode, "brute-force lead %.3e" % (exact[order[0]] - exact[order[1]]), "score err %.3e" % abs(score[0] - exact[order[0]]))
        assert ids[0] == order[0]
        assert abs(float(score[0]) - exact[order[0]]) <= 1e-4


@pytest.mark.parametrize("use_lm", [True, False], ids=["lm", "nolm"])
def test_kernel_confident_regime_identical_to_helper(use_lm):
    want = helper("confident", use_lm)
    for ids, s, finals in want:  # the seed's own margin, on the helper alone
        top = sorted(finals.values(), reverse=True)
        assert len(top) == 1 or top[0] - top[1] >= 1.0
    lm, _ = fixture_lms()
    ids, score = gpu_decode(regime("confident"), lm=lm if use_lm else None, tok=coral_tokenizer())
    for b, (wi, ws, _) in enumerate(want):
        tol = SHAPE["confident"][1] * abs(ws) * 2.0 ** -23
        print("confident", use_lm, b, "score err %.3e tol %.3e" % (abs(score[b] - ws), tol))
        assert ids[b] == wi
        assert abs(float(score[b]) - ws) <= tol


@pytest.mark.parametrize("use_lm", [True, False], ids=["lm", "nolm"])
@pytest.mark.parametrize("kind", ["noisy", "flat"])
def test_kernel_noisy_and_flat_regimes_within_rounding_of_helper(kind, use_lm):
    want = helper(kind, use_lm)
    for (i64, _, _), (i32, _, _) in zip(want, helper(kind, use_lm, "float32")):
        assert i64 == i32  # seed condition: no cascade at the beam_width cut-off between float32 and float64
    lm, _ = fixture_lms()
    ids, score = gpu_decode(regime(kind), lm=lm if use_lm else None, tok=coral_tokenizer())
    for b, (wi, ws, finals) in enumerate(want):
        tol = SHAPE[kind][1] * abs(ws) * 2.0 ** -23
        assert ids[b] in finals, (b, ids[b])
        print(kind, use_lm, b, "same string", ids[b] == wi, "helper gap %.3e" % (ws - finals[ids[b]]),
              "score err %.3e" % abs(score[b] - finals[ids[b]]), "tol %.3e" % tol)
        assert ws - finals[ids[b]] <= tol
        assert abs(float(score[b]) - finals[ids[b]]) <= tol


@pytest.mark.parametrize("kind", ["confident", "noisy", "flat"])
def test_no_lm_score_is_bounded_by_the_ctc_likelihood(kind):
    from coral_amd import ops

    x = regime(kind)
    B, T = SHAPE[kind]
    ids, score = gpu_decode(x, alpha=0.0, beta=0.0)
    Lmax = max(1, max(len(r) for r in ids))
    lab = torch.full((B, Lmax), -100, dtype=torch.int32)
    for b, r in enumerate(ids):
        lab[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.ctc_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device="cuda")
    ops.ctc_loss_fwd_bwd(torch.from_numpy(x).cuda(), lab.cuda(), torch.full((B,), T, dtype=torch.int32).cuda(), nll, None,
                         None, ws, B, T, V, V, Lmax, BLANK, zero_infinity=False)
    torch.cuda.synchronize()
    nll = nll.cpu().numpy()
    for b in range(B):
        tol = T * abs(float(nll[b])) * 2.0 ** -23
        print(kind, b, "score %.5f -nll %.5f gap %.3e" % (score[b], -nll[b], -nll[b] - score[b]))
        assert score[b] <= -nll[b] + tol  # the beam sums a subset of the alignments
        if kind == "confident":
            assert abs(score[b] + nll[b]) <= 5e-3


def test_bit_identical_from_run_to_run_and_under_batch_reversal():
    lm, _ = fixture_lms()
    tok = coral_tokenizer()
    for kind in ("noisy", "flat"):
        x = regime(kind)
        for use in (lm, None):
            a_ids, a_s = gpu_decode(x, lm=use, tok=tok)
            b_ids, b_s = gpu_decode(x, lm=use, tok=tok)
            r_ids, r_s = gpu_decode(x[::-1].copy(), lm=use, tok=tok)
            assert a_ids == b_ids == r_ids[::-1]
            assert a_s.tobytes() == b_s.tobytes() == r_s[::-1].tobytes()


def test_ragged_lengths_ignore_frames_past_in_len():
    lm, _ = fixture_lms()
    tok = coral_tokenizer()
    x = regime("noisy")[:4].copy()
    T = x.shape[1]
    in_len = [1, T, 137, 0]
    rng = np.random.RandomState(5)
    y = x.copy()
    for b, n in enumerate(in_len):
        x[b, n:] = 50.0 * rng.randn(T - n, V)
        y[b, n:] = np.float32(-3.0)
    a_ids, a_s = gpu_decode(x, in_len=in_len, lm=lm, tok=tok)
    b_ids, b_s = gpu_decode(y, in_len=in_len, lm=lm, tok=tok)
    assert a_ids == b_ids and a_s.tobytes() == b_s.tobytes()
    assert len(a_ids[0]) <= 1 and a_ids[3] == ()
    # the rows equal a decode of the truncated utterance alone
    for b in (0, 1, 2):
        ids, s = gpu_decode(x[b:b + 1, :in_len[b]].copy(), lm=lm, tok=tok)
        assert ids[0] == a_ids[b] and s.tobytes() == a_s[b:b + 1].tobytes()
    rlm = ref.RefLM(ARPA)
    id2char = {i: c for c, i in tok.vocab.items() if len(c) == 1}
    wi, ws, _ = ref.prefix_beam_search(x[0], BLANK, DELIM, id2char, rlm, FORBIDDEN, in_len=1)
    assert a_ids[0] == wi and abs(float(a_s[0]) - ws) <= 1e-4


def test_argument_validation_reports_through_last_error():
    from coral_amd import ops
    from coral_amd._lib import CoralAmdError

    x = np.zeros((1, 4, 80), dtype=np.float32)
    with pytest.raises(CoralAmdError, match="LDS layout holds"):
        gpu_decode(x, blank=0, delim=3, forbidden=(), beam_width=128)
    with pytest.raises(CoralAmdError, match="beam_width 129"):
        gpu_decode(x[:, :, :8].copy(), blank=0, delim=3, forbidden=(), beam_width=129)
    assert ops.ctc_beam_workspace_bytes(16, 499, 46, 100) >= 16 * 499 * 100 * 8


def test_evaluate_decodes_with_the_language_model_unless_no_lm(tmp_path, monkeypatch):
    sys.path.insert(0, str(ROOT / "scripts"))
    import finetune_asr_model

    from coral_amd import modeling
    from coral_amd.config import DictConfig, load_config
    from coral_amd.evaluate import evaluate, transcribe
    from coral_amd.model_setup import load_model_setup
    from coral_amd.ngram import NGramLM
    from coral_amd.processor import Wav2Vec2Processor, Wav2Vec2ProcessorWithLM

    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(modeling.HUB_SHAPES, "facebook/wav2vec2-xls-r-300m",
                        dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=4))
    finetune_asr_model.main(["model=test-wav2vec2", "datasets=synthetic", f"models_dir={tmp_path}", "model_id=lmev",
                             "max_steps=2", "total_batch_size=2", "per_device_batch_size=2",
                             "max_seconds_per_example=2.0", "min_seconds_per_example=1.0", "logging_steps=1",
                             "eval_steps=2"])
    mdir = tmp_path / "lmev"
    rng = np.random.RandomState(3)
    examples = [dict(audio=(0.1 * rng.randn(int(16_000 * s))).astype(np.float32), text="a ab") for s in (1.0, 1.6, 1.2, 2.0)]

    def run(no_lm):
        cfg = load_config("evaluation", [f"model_id={mdir}", "batch_size=2", "dataset=synthetic", "store_results=true",
                                         f"no_lm={str(no_lm).lower()}"])
        scores = evaluate(cfg, examples)
        import csv

        return [r[0] for r in list(csv.reader(open(scores["csv"])))[1:]]

    plain = (run(False), run(True))
    assert plain[0] == plain[1]  # no language_model/: today's greedy output in both settings

    saved = load_model_setup(DictConfig(model=DictConfig(type="wav2vec2", sampling_rate=16_000, decoder=None),
                                        model_dir=str(mdir), padding="longest", max_seconds_per_example=10)).load_saved()
    assert type(saved.processor) is Wav2Vec2Processor
    greedy = [t.lower().strip() for t in transcribe(saved.model, saved.processor, [e["audio"] for e in examples], 2)]
    assert plain[0] == greedy

    lm = NGramLM.from_arpa(ARPA)
    Wav2Vec2ProcessorWithLM(saved.processor.feature_extractor, saved.processor.tokenizer, lm).save_pretrained(mdir)
    with_lm, without = run(False), run(True)
    assert without == greedy
    # the strings of engine.beam_decode with that LM, batch by batch
    want = []
    tok = saved.processor.tokenizer
    for i in (0, 2):
        feats = [saved.processor(e["audio"], sampling_rate=16_000) for e in examples[i:i + 2]]
        batch = saved.processor.feature_extractor.pad(feats, padding="longest")
        with torch.no_grad():
            saved.model(torch.from_numpy(batch["input_values"]), torch.from_numpy(batch["attention_mask"]))
        ids, _ = saved.model.engine.beam_decode(lm, tokenizer=tok)
        want += [tok.decode(r, group_tokens=False).lower().strip() for r in ids]
    assert with_lm == want
