"""ca_edit_counts on the GPU (coral_amd/csrc/edit.hip) against tests/edit_ref.py, exact integer equality throughout: the
wave route and the workgroup route at every length where the code takes another path, route selection, launch order,
determinism, the equality with coral_amd/metrics.py, and `evaluate` with `error_rates: device` on the fixture checkpoint."""
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import edit_ref as eref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
UNWRITTEN = -7  # the kernel writes counts >= 0, or -1 for a pair it cannot serve
TAIL = 64  # tokens behind the last string of each side: a common token, so that reading them would find matches


def _consts():
    from coral_amd import _lib

    return _lib.EDIT_WAVE_MAX, _lib.EDIT_PANEL


def run_raw(refs, hyps, route, order=None, ws_bytes=None):
    """The C entry point on device buffers built here: outputs pre-filled, token tails poisoned.  -> int32 [n, 4]"""
    from coral_amd import _lib, ops

    n = len(refs)
    ref = np.concatenate([np.asarray(r, dtype=np.int32) for r in refs] + [np.zeros(TAIL, dtype=np.int32)])
    hyp = np.concatenate([np.asarray(h, dtype=np.int32) for h in hyps] + [np.zeros(TAIL, dtype=np.int32)])
    ref_off = np.concatenate(([0], np.cumsum([len(r) for r in refs]))).astype(np.int64)
    hyp_off = np.concatenate(([0], np.cumsum([len(h) for h in hyps]))).astype(np.int64)
    if ws_bytes is None:
        ws_bytes = ops.edit_counts_workspace_bytes(n, max(len(r) for r in refs), max(len(h) for h in hyps))
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(ref=ref, hyp=hyp, ref_off=ref_off, hyp_off=hyp_off).items()}
    od = None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda()
    ws = torch.empty(max(8, ws_bytes), dtype=torch.uint8, device="cuda")
    counts = torch.full((n, 4), UNWRITTEN, dtype=torch.int32, device="cuda")
    rc = _lib.load().ca_edit_counts(d["ref"].data_ptr(), d["ref_off"].data_ptr(), d["hyp"].data_ptr(), d["hyp_off"].data_ptr(),
                                    None if od is None else od.data_ptr(), n, counts.data_ptr(), route, ws.data_ptr(),
                                    ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().ca_last_error()
    torch.cuda.synchronize()
    return counts.cpu().numpy()


def _mutate(rng, s, k):
    """s with k random edits (substitutions, deletions, insertions) over the alphabet {0, 1, 2}"""
    s = list(s)
    for _ in range(k):
        op, at = rng.randint(3), rng.randint(len(s) + 1)
        if op == 0 and s:
            s[min(at, len(s) - 1)] = rng.randint(3)
        elif op == 1 and s:
            del s[min(at, len(s) - 1)]
        else:
            s.insert(at, rng.randint(3))
    return s


@pytest.fixture(scope="module")
def small():
    """Pairs both routes accept, with their reference counts (computed once): every length the wave route changes its
    columns per lane or its step count at, crossed, on a 3-letter alphabet so that ties are frequent."""
    wave_max, _ = _consts()
    rng = np.random.RandomState(11)
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, wave_max - 1, wave_max]
    refs, hyps = [], []
    for n in lengths:
        for m in lengths:
            r = rng.randint(0, 3, n).tolist()
            # about half the pairs are related strings (a realistic alignment), the others independent
            h = (_mutate(rng, r, max(1, n // 8)) + rng.randint(0, 3, m).tolist())[:m] if (n + m) % 2 else rng.randint(0, 3, m).tolist()
            refs.append(r), hyps.append(h)
    same = rng.randint(0, 3, 257).tolist()
    extra = [(rng.randint(0, 3, 700).tolist(), [1, 2, 0]), ([2, 0], rng.randint(0, 3, 900).tolist()),  # m << n, n << m
             (same, list(same)), ([0, 1] * 100, [2] * 130)]  # identical; no common token
    for r, h in extra:
        refs.append(r), hyps.append(h)
    assert len(refs) % 4 != 0  # the last workgroup is not full
    return refs, hyps, eref.batch_counts(refs, hyps)


@pytest.fixture(scope="module")
def panels():
    """Pairs for the workgroup route around its panel width."""
    _, panel = _consts()
    rng = np.random.RandomState(12)
    refs, hyps = [], []
    for m in (panel - 1, panel, panel + 1, 2 * panel + 3):
        r = rng.randint(0, 3, 300).tolist()
        refs.append(r), hyps.append((_mutate(rng, r, 40) + rng.randint(0, 3, m).tolist())[:m])
    refs.append(rng.randint(0, 3, panel + 1).tolist()), hyps.append(rng.randint(0, 3, 70).tolist())
    return refs, hyps, eref.batch_counts(refs, hyps)


def _check(got, want, refs, hyps):
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), [(int(b), len(refs[b]), len(hyps[b]), got[b].tolist(), want[b].tolist()) for b in bad[:8]]


def test_wave_route(small):
    refs, hyps, want = small
    _check(run_raw(refs, hyps, route=1), want, refs, hyps)


def test_workgroup_route_small_lengths(small):
    refs, hyps, want = small
    _check(run_raw(refs, hyps, route=2), want, refs, hyps)


def test_workgroup_route_panels(panels):
    refs, hyps, want = panels
    _check(run_raw(refs, hyps, route=2), want, refs, hyps)


def test_route_selection_order_and_determinism(small, panels):
    from coral_amd import ops
    from coral_amd._lib import CoralAmdError

    wave_max, _ = _consts()
    refs, hyps = small[0] + panels[0], small[1] + panels[1]
    want = np.concatenate([small[2], panels[2]])
    n = len(refs)
    assert any(max(len(r), len(h)) > wave_max for r, h in zip(refs, hyps)) and any(
        0 < max(len(r), len(h)) <= wave_max for r, h in zip(refs, hyps))  # route 0 takes both routes here
    first = run_raw(refs, hyps, route=0)
    _check(first, want, refs, hyps)
    assert np.array_equal(run_raw(refs, hyps, route=0), first)  # bit-identical from run to run
    perm = np.random.RandomState(13).permutation(n)
    _check(run_raw(refs, hyps, route=0, order=perm), want, refs, hyps)
    _check(run_raw(refs, hyps, route=0, order=np.arange(n)[::-1].copy()), want, refs, hyps)
    # the two routes agree on everything the wave route accepts
    assert np.array_equal(run_raw(small[0], small[1], route=1), run_raw(small[0], small[1], route=2))
    # the wrapper: its own upload, the largest-first order, a workspace for the long pairs alone
    ref = np.concatenate([np.asarray(r, dtype=np.int32) for r in refs])
    hyp = np.concatenate([np.asarray(h, dtype=np.int32) for h in hyps])
    ref_off = np.concatenate(([0], np.cumsum([len(r) for r in refs])))
    hyp_off = np.concatenate(([0], np.cumsum([len(h) for h in hyps])))
    plan = ops.edit_counts_plan(ref, ref_off, hyp, hyp_off)
    assert plan["ws_bytes"] == sum(16 * (len(r) + 1) for r, h in zip(refs, hyps) if max(len(r), len(h)) > wave_max)
    _check(ops.edit_counts_launch(plan).cpu().numpy(), want, refs, hyps)
    # route 1 with a pair above CA_EDIT_WAVE_MAX: refused where the lengths are known ...
    with pytest.raises(CoralAmdError, match="CA_ERR_ARG"):
        ops.edit_counts(ref, ref_off, hyp, hyp_off, route=1)
    # ... and behind the C entry point, which cannot see them, such a pair is marked and the others are served
    got = run_raw(refs, hyps, route=1)
    long = np.array([max(len(r), len(h)) > wave_max and min(len(r), len(h)) > 0 for r, h in zip(refs, hyps)])
    assert (got[long] == -1).all() and np.array_equal(got[~long], want[~long])
    # a workspace that holds no boundary column: the same mark, no access
    got = run_raw(panels[0], panels[1], route=2, ws_bytes=0)
    assert (got == -1).all()


def _danish(rng, n):
    alphabet = list("abcdefghijklmnopqrstuvwxyzæøå") + [" "] * 6
    return "".join(rng.choice(alphabet, n))


def test_rates_equal_the_existing_metric():
    from coral_amd import error_rates as er, metrics

    rng = np.random.RandomState(14)
    labels, preds = [], []
    for _ in range(40):
        lab = " ".join(_danish(rng, rng.randint(5, 160)).split()) or "a"  # single spaces, stripped: what the pipeline compares
        chars = list(lab)
        for _ in range(max(1, len(chars) // 10)):
            at = rng.randint(len(chars))
            op = rng.randint(3)
            if op == 0:
                chars[at] = _danish(rng, 1)
            elif op == 1:
                del chars[at]
            else:
                chars.insert(at, _danish(rng, 1))
        labels.append(lab)
        preds.append(" ".join("".join(chars).split()))
    assert er.cer(preds, labels, normalise=False) == metrics.cer(preds, labels)
    assert er.wer(preds, labels, normalise=False) == metrics.wer(preds, labels)
    cc = eref.batch_counts([[ord(c) for c in x] for x in labels], [[ord(c) for c in x] for x in preds])
    words = {}
    wc = eref.batch_counts([[words.setdefault(w, len(words)) for w in x.split()] for x in labels],
                           [[words.setdefault(w, len(words)) for w in x.split()] for x in preds])
    assert np.array_equal(er.error_counts(preds, labels, "char"), cc) and np.array_equal(er.error_counts(preds, labels, "word"), wc)
    assert er.cer(preds, labels) == eref.rate(cc, True) and er.wer(preds, labels) == eref.rate(wc, True)
    assert er.cer(preds, labels) <= er.cer(preds, labels, normalise=False)
    assert er.text_rates(preds, labels, "device", False) == dict(cer=metrics.cer(preds, labels), wer=metrics.wer(preds, labels))
    assert er.text_rates(preds, labels, "device", True) == dict(cer=eref.rate(cc, True), wer=eref.rate(wc, True))


def test_in_training_metrics_with_device_error_rates():
    """compute_error_rate_metrics (what the wav2vec2 setup binds, and what finetune.evaluate_split reads its keys from)
    with `error_rates: device`: the host path's floats exactly, and the normalised ones from the restatement."""
    from functools import partial

    from coral_amd.compute_metrics import compute_error_rate_metrics
    from coral_amd.config import load_config
    from coral_amd.processor import CTCTokenizer, Wav2Vec2Processor, WaveformFeatureExtractor

    chars = load_config("evaluation").characters_to_keep
    tok = CTCTokenizer({c: i for i, c in enumerate(sorted(set(chars + "|")))})
    proc = Wav2Vec2Processor(WaveformFeatureExtractor(), tok)
    rng = np.random.RandomState(16)
    n_chars = len(sorted(set(chars + "|")))
    labels = rng.randint(0, n_chars, (6, 40))
    labels[:, 30:] = -100
    labels[2, 12:] = -100
    preds = np.where(rng.rand(6, 40) < 0.8, np.where(labels < 0, tok.pad_token_id, labels), rng.randint(0, n_chars, (6, 40)))
    host = compute_error_rate_metrics(preds, labels, proc)
    assert partial(compute_error_rate_metrics, processor=proc)(preds, labels) == host and 0 < host["cer"] < 1
    dev = compute_error_rate_metrics(preds, labels, proc, error_rates="device")
    assert dev == host and set(dev) == {"cer", "wer"}
    norm = compute_error_rate_metrics(preds, labels, proc, error_rates="device", normalise_error_rates=True)
    assert 0 < norm["cer"] <= host["cer"] and 0 < norm["wer"] <= host["wer"]
    with pytest.raises(ValueError, match="normalise_error_rates"):
        compute_error_rate_metrics(preds, labels, proc, normalise_error_rates=True)


def test_evaluate_with_device_error_rates(tmp_path, monkeypatch):
    import csv

    from coral_amd import error_rates as er
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.processor import dump_vocabulary

    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "ckpt"
    shutil.copytree(GOLDEN / "engine_ckpt_w2v2", mdir)
    dump_vocabulary(load_config("evaluation").characters_to_keep, mdir)
    rng = np.random.RandomState(15)
    texts = ["hej med dig", "det er en god dag", "å", "jeg hedder anna", "to tre fire", "ø æ å", "hvad sker der her", "nej"]
    examples = [dict(audio=(0.1 * rng.randn(int(16_000 * s))).astype(np.float32), text=t, age_group=a, gender=g)
                for s, t, a, g in zip((1.0, 1.5, 0.8, 2.0, 1.2, 0.9, 1.7, 1.1), texts, "yoyyooyo", "ffmmfmff")]

    def run(*overrides):
        return evaluate(load_config("evaluation", [f"model_id={mdir}", "batch_size=4", "dataset=synthetic", *overrides]), examples)

    host = run()
    assert set(host) == {"model_type", "n", "cer", "wer", "csv"}  # the defaults add nothing
    dev = run("error_rates=device", "score_categories=[age_group,gender]")
    assert dev["cer"] == host["cer"] and dev["wer"] == host["wer"]
    assert set(dev) == set(host) | {"error_counts", "score_table", "scores_csv"}
    preds = [r[0] for r in list(csv.reader(open(host["csv"])))[1:]]
    labels = [t.lower().strip() for t in texts]
    cc = eref.batch_counts([[ord(c) for c in x] for x in labels], [[ord(c) for c in er.tokenise(x, "char")] for x in preds])
    words = {}
    wc = eref.batch_counts([[words.setdefault(w, len(words)) for w in er.tokenise(x, "word")] for x in labels],
                           [[words.setdefault(w, len(words)) for w in er.tokenise(x, "word")] for x in preds])
    assert dev["error_counts"] == dict(char=cc.sum(0).tolist(), word=wc.sum(0).tolist())
    assert dev["score_table"] == er.score_table(examples, ["age_group", "gender"], cc, wc, normalise=False)
    assert len(dev["score_table"]) == 9 and dev["score_table"][-1]["cer"] == host["cer"]
    rows = list(csv.DictReader(open(dev["scores_csv"])))
    assert [r["age_group"] for r in rows] == [t["age_group"] or "" for t in dev["score_table"]]
    assert [float(r["cer"]) for r in rows] == [t["cer"] for t in dev["score_table"]]
    norm = run("error_rates=device", "normalise_error_rates=true")
    assert norm["cer"] == eref.rate(cc, True) and norm["wer"] == eref.rate(wc, True) and norm["error_counts"] == dev["error_counts"]
