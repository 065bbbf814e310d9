"""ca_ctc_align on the GPU (coral_amd/csrc/ctc_align.hip): planted paths (exact), the greedy path (exact, against
ca_ctc_collapse_offsets), arbitrary labels on flat logits (score bounds derived from the inputs, against the float64
Viterbi of tests/ctc_align_ref.py), determinism, and the route through transcribe / align on the fixture checkpoint."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_align_ref as aref  # noqa: E402
import longform_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, LDV, BLANK = 46, 48, 45
U = 2.0 ** -24  # fp32 unit roundoff


def _align(logits, in_len, labels, Lmax=None):
    """logits [B, T, V] (NumPy), labels a list of id lists -> (start, end, tok_score [B, Lmax], score [B]) host arrays;
    the output buffers are pre-filled with values the kernel never writes."""
    from coral_amd import ops

    B, T, v = logits.shape
    lg = np.full((B, T, LDV), 1e4, np.float32)  # the padding columns must not be read either
    lg[:, :, :v] = logits
    Lmax = max([len(r) for r in labels] + [1]) if Lmax is None else Lmax
    lab = np.zeros((B, Lmax), np.int32)
    for b, r in enumerate(labels):
        lab[b, :len(r)] = r
    start = torch.full((B, Lmax), -9, dtype=torch.int32, device=DEV)
    end = torch.full((B, Lmax), -9, dtype=torch.int32, device=DEV)
    tok = torch.full((B, Lmax), 9.0, dtype=torch.float32, device=DEV)
    score = torch.full((B,), 9.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.ctc_align_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    il = None if in_len is None else torch.tensor(in_len, dtype=torch.int32, device=DEV)
    ops.ctc_align(torch.from_numpy(lg).to(DEV), il, torch.from_numpy(lab), torch.tensor([len(r) for r in labels]),
                  start, end, tok, score, ws, B, T, v, LDV, Lmax, BLANK)
    return start.cpu().numpy(), end.cpu().numpy(), tok.cpu().numpy(), score.cpu().numpy()


def _need(labels):
    return len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))


def _plant(rng, labels, n):
    """A random frame sequence of n frames that collapses to labels -> (frames, start, end)."""
    L = len(labels)
    extra = n - _need(labels)
    assert extra >= 0
    add = np.bincount(rng.randint(0, 2 * L + 1, extra), minlength=2 * L + 1) if extra else np.zeros(2 * L + 1, int)
    frames, start, end = [], [], []
    for i, c in enumerate(labels):
        gap = int(add[2 * i]) + (1 if i > 0 and labels[i - 1] == c else 0)
        frames += [BLANK] * gap
        start.append(len(frames))
        frames += [int(c)] * (1 + int(add[2 * i + 1]))
        end.append(len(frames))
    frames += [BLANK] * int(add[2 * L])
    assert len(frames) == n
    return frames, start, end


def _planted_logits(rng, T, rows):
    """rows: (labels, in_len, plant?) -> logits [B, T, V] = 0.1 N(0,1) + 6 at the planted symbol, 1e4 beyond in_len."""
    B = len(rows)
    x = (0.1 * rng.randn(B, T, V)).astype(np.float32)
    want = []
    for b, (labels, n, plant) in enumerate(rows):
        if plant:
            frames, start, end = _plant(rng, labels, n)
            x[b, np.arange(n), frames] += 6.0
            want.append((frames, start, end))
        else:
            want.append(None)
        x[b, n:] = 1e4
    return x, want


def _score_bound(lp, n, opt):
    return n * U * (abs(opt) + 8 * np.abs(lp[:n]).max())


def _check_planted(x, rows, want, got):
    start, end, tok, score = got
    for b, (labels, n, plant) in enumerate(rows):
        L = len(labels)
        assert (start[b, L:] == -1).all() and (end[b, L:] == -1).all(), b
        if not plant:
            assert score[b] == -np.inf and (start[b, :L] == -1).all() and (end[b, :L] == -1).all(), b
            continue
        frames, ws_, we = want[b]
        assert start[b, :L].tolist() == ws_ and end[b, :L].tolist() == we, (b, L, n)
        lp = aref.log_softmax64(x[b, :n])
        ps = aref.path_score(lp, frames)
        assert abs(float(score[b]) - ps) <= _score_bound(lp, n, ps), (b, score[b], ps)


def _labels(rng, L):
    return rng.randint(0, V - 1, L).tolist()


def test_planted_paths_small_rows_and_edge_cases():
    rng = np.random.RandomState(0)
    T = 64
    single = _labels(rng, 20) + [7, 7, 7]          # L + repeats == in_len: exactly one alignment
    over = _labels(rng, 30) + [3, 3]               # L + repeats == in_len + 1: none
    rows = [([], 40, True), ([11], 64, True), ([5, 5], 17, True), (_labels(rng, 31), 61, True),
            (single, _need(single), True), (over, _need(over) - 1, False), (_labels(rng, 12), 13, True), ([9], 0, False)]
    assert _need(single) <= T and max(len(r[0]) for r in rows) == 32
    x, want = _planted_logits(rng, T, rows)
    got = _align(x, [r[1] for r in rows], [r[0] for r in rows])
    _check_planted(x, rows, want, got)
    # lab_len = 0: the all-blank path
    lp = aref.log_softmax64(x[0, :40])
    assert abs(float(got[3][0]) - lp[:, BLANK].sum()) <= _score_bound(lp, 40, lp[:, BLANK].sum())


def test_one_and_two_frames():
    """The shortest rows: no recursion step at all (in_len = 1), and one."""
    rng = np.random.RandomState(1)
    rows = [([7], 1, True), ([], 1, True), ([7, 8], 1, False), ([7, 8], 2, True), ([7, 7], 2, False), ([3], 2, True)]
    x, want = _planted_logits(rng, 4, rows)
    _check_planted(x, rows, want, _align(x, [r[1] for r in rows], [r[0] for r in rows]))


@pytest.mark.parametrize("L", [127, 128])
def test_planted_paths_on_both_sides_of_the_regime_switch(L):
    rng = np.random.RandomState(L)
    T = 300
    rows = [(_labels(rng, L), 300, True), (_labels(rng, L - 40) + [4, 4], 251, True), (_labels(rng, L), L - 1, False)]
    x, want = _planted_logits(rng, T, rows)
    _check_planted(x, rows, want, _align(x, [r[1] for r in rows], [r[0] for r in rows]))


def test_planted_path_at_the_label_limit_and_refusal_beyond():
    from coral_amd import _lib, ops

    rng = np.random.RandomState(4095)
    T, L = 8300, 4095
    labels = _labels(rng, L)
    assert _need(labels) <= 8200
    rows = [(labels, 8200, True)]
    x, want = _planted_logits(rng, T, rows)
    _check_planted(x, rows, want, _align(x, [8200], [labels]))
    # one label more is refused by the library, by name
    lib = _lib.load()
    t = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.ca_ctc_align(p, LDV, None, p, p, p, p, p, p, p, t.numel() * 4, 1, 8, V, 4096, BLANK, None) == -1
    assert b"ca_ctc_align" in lib.ca_last_error() and b"4096" in lib.ca_last_error()
    with pytest.raises(ValueError, match="4095"):
        ops.ctc_align(t, None, torch.zeros(1, 4096, dtype=torch.int32), torch.tensor([1]), t, t, t, t, t, 1, 8, V, LDV, 4096,
                      BLANK)
    with pytest.raises(ValueError, match="blank"):
        _align(np.zeros((1, 8, V), np.float32), None, [[3, BLANK]])
    with pytest.raises(ValueError, match="labels"):
        _align(np.zeros((1, 8, V), np.float32), None, [[3, V]])


def _greedy_and_offsets(lg):
    from coral_amd import ops

    B, T, _ = lg.shape
    d = torch.from_numpy(lg).to(DEV)
    raw = torch.empty(B, T, dtype=torch.int32, device=DEV)
    ids = torch.empty(B, T, dtype=torch.int32, device=DEV)
    olen = torch.empty(B, dtype=torch.int32, device=DEV)
    ops.ctc_greedy_decode(d, None, raw, ids, olen, B, T, V, LDV, BLANK)
    outs = [torch.empty(B, T, dtype=torch.int32, device=DEV) for _ in range(3)]
    olen2 = torch.empty(B, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.ctc_collapse_workspace_bytes(B, T), dtype=torch.uint8, device=DEV)
    ops.ctc_collapse_offsets(raw, None, outs[0], outs[1], outs[2], olen2, ws, B, T, BLANK)
    n = olen.cpu().numpy()
    assert np.array_equal(n, olen2.cpu().numpy())
    ids, cs, ce = ids.cpu().numpy(), outs[1].cpu().numpy(), outs[2].cpu().numpy()
    return [ids[b, :n[b]].tolist() for b in range(B)], [cs[b, :n[b]].tolist() for b in range(B)], \
        [ce[b, :n[b]].tolist() for b in range(B)]


@pytest.mark.parametrize("blank_bias", [False, True])
def test_alignment_of_the_greedy_ids_is_the_greedy_path(blank_bias):
    """The argmax path maximises every term of the sum and fp32 addition is monotone, so no path beats it; the enforced
    top-2 gap of 0.5 per frame excludes ties."""
    rng = np.random.RandomState(11 + blank_bias)
    B, T = 4, 499
    x = rng.randn(B, T, V).astype(np.float32)
    if blank_bias:  # blank wins about 80 % of the frames: L ~ 100, the wave regime
        x[:, :, BLANK] += np.where(rng.rand(B, T) < 0.8, 10.0, 0.0).astype(np.float32)
    am = x.argmax(-1)
    np.put_along_axis(x, am[..., None], np.take_along_axis(x, am[..., None], -1) + np.float32(0.5), -1)
    top2 = np.sort(x, -1)[..., -2:]
    assert (top2[..., 1] - top2[..., 0] >= 0.5).all()
    lg = np.zeros((B, T, LDV), np.float32)
    lg[:, :, :V] = x
    ids, cs, ce = _greedy_and_offsets(lg)
    Lmax = max(len(r) for r in ids)
    assert (64 < Lmax <= 127) if blank_bias else Lmax > 400, Lmax
    start, end, tok, score = _align(x, None, ids)
    for b in range(B):
        L = len(ids[b])
        assert start[b, :L].tolist() == cs[b] and end[b, :L].tolist() == ce[b], b
        assert (start[b, L:] == -1).all() and (end[b, L:] == -1).all()


def _check_bounded(x_row, n, labels, start, end, tok, score, what=""):
    """The criterion for labels that are not the greedy ones: the returned start / end define a valid alignment whose
    float64 score lies in [opt - 2e, opt + e], e = n * 2^-24 * (|opt| + 8 max|lp|): the kernel maximises fp32 partial sums
    of non-positive terms, each bounded by the total (n roundings of at most 2^-24 |opt|) over an fp32 log-softmax allowed
    8 ulp per term; so its path's true score is within e of its fp32 score, which is at least the optimum's fp32 score,
    itself within e of opt.  -> (deficit, e)."""
    L = len(labels)
    lp = aref.log_softmax64(x_row[:n])
    opt, _, _ = aref.viterbi(lp, labels, BLANK)
    assert opt > -np.inf
    st, en = start[:L].tolist(), end[:L].tolist()
    aref.check_valid_alignment(st, en, labels, n)
    frames = aref.path_of(st, en, labels, n, BLANK)
    assert aref.collapse(frames, BLANK) == [int(c) for c in labels]
    ps = aref.path_score(lp, frames)
    mx = np.abs(lp).max()
    e = n * U * (abs(opt) + 8 * mx)
    print(f"{what} L={L} n={n}: opt {opt:.6f} path {ps:.6f} deficit {opt - ps:.3e} bound 2e {2 * e:.3e}; "
          f"|score - path| {abs(float(score) - ps):.3e} bound e {e:.3e}")
    assert opt - 2 * e <= ps <= opt + e, (opt, ps, e)
    assert abs(float(score) - ps) <= e, (float(score), ps, e)
    worst = 0.0
    for i, c in enumerate(labels):
        k = en[i] - st[i]
        mean = lp[st[i]:en[i], int(c)].mean()
        tb = (8 + k) * U * mx
        worst = max(worst, abs(float(tok[i]) - mean) / tb)
        assert abs(float(tok[i]) - mean) <= tb, (i, float(tok[i]), mean, tb)
    print(f"{what} tok_score: largest error / bound {worst:.3f}")
    return opt - ps, e


@pytest.mark.parametrize("L", [5, 60, 150])
def test_arbitrary_labels_on_flat_logits_are_within_the_derived_bounds(L):
    rng = np.random.RandomState(100 + L)
    B, T = 2, 200
    x = rng.randn(B, T, V).astype(np.float32)
    in_len = [200, 173]
    labels = [_labels(rng, L), _labels(rng, L - 2) + [8, 8]]
    x[1, 173:] = 1e4
    start, end, tok, score = _align(x, in_len, labels)
    for b in range(B):
        _check_bounded(x[b], in_len[b], labels[b], start[b], end[b], tok[b], score[b], f"flat row {b}")


@pytest.mark.parametrize("L", [60, 150])
def test_bit_identical_from_run_to_run_and_under_batch_reversal(L):
    rng = np.random.RandomState(7 + L)
    B, T = 5, 200
    x = rng.randn(B, T, V).astype(np.float32)
    in_len = [200, 150, 0, 199, 64]
    labels = [_labels(rng, L), _labels(rng, L // 2), _labels(rng, 3), [], _labels(rng, 64) + [1]]
    Lmax = max(len(r) for r in labels)
    a = _align(x, in_len, labels, Lmax)
    b = _align(x, in_len, labels, Lmax)
    c = _align(x[::-1].copy(), in_len[::-1], labels[::-1], Lmax)
    for u, v, w in zip(a, b, c):
        assert u.tobytes() == v.tobytes()
        assert u.tobytes() == w[::-1].tobytes()
    assert a[3][2] == -np.inf and a[3][4] == -np.inf and np.isfinite(a[3][[0, 1, 3]]).all()


# ---- through the engine: transcribe(timestamp_source="alignment") and align --------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from coral_amd.modeling import Wav2Vec2ForCTC
    from coral_amd.ngram import NGramLM, load_attrs
    from coral_amd.processor import (CTCTokenizer, Wav2Vec2Processor, Wav2Vec2ProcessorWithLM,
                                     WaveformFeatureExtractor)

    model = Wav2Vec2ForCTC.from_pretrained(str(lref.GOLDEN / "hf_ckpt_w2v2")).eval()
    proc = Wav2Vec2Processor(WaveformFeatureExtractor(), CTCTokenizer(lref.load_fixture()[0]["vocab"]))
    lm_dir = lref.GOLDEN / "lm_tiny"
    plm = Wav2Vec2ProcessorWithLM(proc.feature_extractor, proc.tokenizer, NGramLM.from_arpa(lm_dir / "3gram.arpa"),
                                  load_attrs(lm_dir))
    return model, proc, plm


def _frames(chunks):
    return [(int(round(c["timestamp"][0] * 50)), int(round(c["timestamp"][1] * 50))) for c in chunks]


def _check_chunks(res, text, duration):
    assert res["text"] == text
    assert [c["text"] for c in res["chunks"]] == text.split()
    prev = 0.0
    for c in res["chunks"]:
        a, b = c["timestamp"]
        assert prev <= a <= b <= duration + 1e-9, (c, prev, duration)
        prev = b


def test_word_times_under_lm_decoding_chunked(tiny):
    from coral_amd import longform as lf
    from coral_amd.evaluate import transcribe

    model, proc, plm = tiny
    wave = lref.fixture_waveform()
    waves = [wave, wave[:40000]]
    texts = transcribe(model, plm, waves, 3, chunk_length_s=2.0)
    words = transcribe(model, plm, waves, 3, chunk_length_s=2.0, return_timestamps="word", timestamp_source="alignment")
    chars = transcribe(model, plm, waves, 3, chunk_length_s=2.0, return_timestamps="char", timestamp_source="alignment")
    assert [r["text"] for r in words] == texts == [r["text"] for r in chars] and any(len(t) > 0 for t in texts)
    with pytest.raises(ValueError, match="return_timestamps.*LM"):
        transcribe(model, plm, waves, 3, chunk_length_s=2.0, return_timestamps="word")
    with pytest.raises(ValueError, match="timestamp_source"):
        transcribe(model, plm, waves, 3, chunk_length_s=2.0, return_timestamps="word", timestamp_source="beam")
    # the criterion on the stitched logits, for the ids the beam search returned
    st = lf.stitch_long(model, waves, 2.0, None, batch_size=3, want_logits=True)
    eng = model.engine
    ids, _ = eng.beam_decode(plm.device_tables(eng.device), tokenizer=plm.tokenizer, in_len=st["in_len"],
                             logits=st["logits"], **plm.decoder_params)
    rows, score = eng.align(ids, in_len=st["in_len"], logits=st["logits"])
    lg = st["logits"].cpu().numpy()[:, :, :eng.s.vocab_size]
    blank = eng.s.pad_token_id
    assert blank == BLANK and eng.s.vocab_size == V
    delim = plm.tokenizer.vocab[plm.tokenizer.word_delimiter_token]
    for r, w in enumerate(waves):
        n = st["lengths"][r]
        start, end, tok = (np.asarray(a) for a in rows[r])
        _check_bounded(lg[r], n, ids[r], start, end, tok, score[r], f"stitched row {r}")
        _check_chunks(words[r], texts[r], len(w) / 16000)
        # the chunks carry these frames: every character's, and a word's first start / last end
        assert _frames(chars[r]["chunks"]) == list(zip(start.tolist(), end.tolist()))
        assert "".join(c["text"] for c in chars[r]["chunks"]).strip() == texts[r]
        spans, cur = [], None
        for i, s, e in zip(ids[r], start.tolist(), end.tolist()):
            if i == delim:
                cur = None
            elif cur is None:
                cur = [s, e]
                spans.append(cur)
            else:
                cur[1] = e
        assert _frames(words[r]["chunks"]) == [tuple(s) for s in spans]


def test_whole_clips_both_levels_with_and_without_the_lm_and_align(tiny):
    from coral_amd import ctc_align as ca
    from coral_amd.evaluate import transcribe

    model, proc, plm = tiny
    wave = lref.fixture_waveform()
    waves = [wave[:48000], wave[:32000]]
    for p in (proc, plm):
        texts = transcribe(model, p, waves)
        for level in ("word", "char"):
            res = transcribe(model, p, waves, return_timestamps=level, timestamp_source="alignment")
            assert [r["text"] for r in res] == texts
            for r, t in zip(res, texts):
                if level == "word":
                    _check_chunks(r, t, 3.0)
                else:
                    assert "".join(c["text"] for c in r["chunks"]).strip() == t
                    ts = [x for c in r["chunks"] for x in c["timestamp"]]
                    assert ts == sorted(ts) and 0 <= ts[0] and ts[-1] <= 3.0
    # greedy decoding, chunked, from the alignment: the same texts as from the emission frames
    emis = transcribe(model, proc, [wave], chunk_length_s=2.0, return_timestamps="word")
    alig = transcribe(model, proc, [wave], chunk_length_s=2.0, return_timestamps="word", timestamp_source="alignment")
    assert emis[0]["text"] == alig[0]["text"] and [c["text"] for c in emis[0]["chunks"]] == [c["text"] for c in alig[0]["chunks"]]
    # align(): a transcript the caller brings
    text = transcribe(model, proc, [wave])[0]
    want = transcribe(model, proc, [wave], return_timestamps="word", timestamp_source="alignment")[0]
    got = ca.align(model, proc, [wave], [text])[0]
    assert got["text"] == text and np.isfinite(got["score"]) and got["score"] < 0
    assert [{"text": c["text"], "timestamp": c["timestamp"]} for c in got["chunks"]] == want["chunks"]
    assert all(np.isfinite(c["score"]) and c["score"] <= 0 for c in got["chunks"])
    chunked = ca.align(model, proc, [wave, wave[:40000]], [text, "ab"], batch_size=3, chunk_length_s=2.0, level="char")
    assert [c["text"] for c in chunked[0]["chunks"]] == list(text) and [c["text"] for c in chunked[1]["chunks"]] == ["a", "b"]
    # a text that cannot be aligned, and one beyond the limit
    n_frames = len(wave[:8000]) // 320
    res = ca.align(model, proc, [wave[:8000]], ["ab" * n_frames])[0]
    assert res["score"] == -math.inf and res["chunks"] is None
    with pytest.raises(ValueError, match="4095"):
        ca.align(model, proc, [wave], ["ab " * 1366])
