"""Long-form wav2vec2 transcription on the GPU: `ca_ctc_stitch` and `ca_ctc_collapse_offsets` against NumPy
restatements (tests/longform_ref.py), the `transformers` ASR pipeline's chunked CTC semantics reproduced exactly from its
recorded logits (tests/golden/w2v2_longform.*, tools/gen_longform_goldens.py), the engine end to end on the fixture
waveform, clips beyond the greedy kernel's 4096 frames, and the LM route."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import longform_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, LDV, BLANK = 46, 48, 45
TILE = 4096


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _stitch(logits, seg, R, Tout, want_logits=True, raw_fill=-7, logits_fill=-3.5):
    from coral_amd import ops

    C, T, ldv = logits.shape
    raw = torch.full((R, Tout), raw_fill, dtype=torch.int32, device=DEV)
    lo = torch.full((R, Tout, ldv), logits_fill, dtype=torch.float32, device=DEV) if want_logits else None
    ops.ctc_stitch(_dev(logits, torch.float32), _dev(np.asarray(seg, np.int32).reshape(-1, 4), torch.int32), raw, lo,
                   C, T, V, ldv, R, Tout)
    return raw, lo


def _collapse(raw, in_len):
    """-> (ids, start, end, out_len) as host arrays, full [B, T] buffers."""
    from coral_amd import ops

    B, T = raw.shape
    d = _dev(raw, torch.int32)
    outs = [torch.full((B, T), -9, dtype=torch.int32, device=DEV) for _ in range(3)]
    olen = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.ctc_collapse_workspace_bytes(B, T), dtype=torch.uint8, device=DEV)
    il = None if in_len is None else _dev(np.asarray(in_len, np.int32), torch.int32)
    ops.ctc_collapse_offsets(d, il, outs[0], outs[1], outs[2], olen, ws, B, T, BLANK)
    return [o.cpu().numpy() for o in outs] + [olen.cpu().numpy()]


def _check_collapse(raw, in_len):
    B, T = raw.shape
    ids, start, end, olen = _collapse(raw, in_len)
    for b in range(B):
        n = T if in_len is None else int(in_len[b])
        wi, ws_, we = lref.collapse_ref_fast(raw[b], n, BLANK)
        k = len(wi)
        assert int(olen[b]) == k, (b, int(olen[b]), k)
        assert ids[b, :k].tolist() == wi and start[b, :k].tolist() == ws_ and end[b, :k].tolist() == we
        assert (ids[b, k:] == -1).all() and (start[b, k:] == -1).all() and (end[b, k:] == -1).all()
    return ids, start, end, olen


def _runs(rng, T, mean_run, p_blank=0.4):
    """A row of T frames made of random runs (geometric lengths, mean `mean_run`), blank with probability p_blank;
    neighbouring runs may carry the same id, which merges them - as in real argmax rows."""
    out = np.empty(T + 64 * mean_run, np.int32)
    t = 0
    while t < T:
        n = int(rng.geometric(1.0 / mean_run))
        out[t:t + n] = BLANK if rng.rand() < p_blank else rng.randint(0, V - 1)
        t += n
    return out[:T]


# ---- 1. stitch ---------------------------------------------------------------------------------
def test_stitch_kernel_matches_numpy_bit_for_bit():
    rng = np.random.RandomState(3)
    C, T, R, Tout = 5, 49, 2, 90
    logits = rng.randn(C, T, LDV).astype(np.float32)
    logits[:, :, V:] = 99.0  # the padding columns must never win the argmax (they are copied, though)
    logits[1, 7, :V] = np.minimum(logits[1, 7, :V], 1.0)
    logits[1, 7, [11, 30]] = 2.5  # two equal maxima: the lower index wins
    logits[3, 40, :V] = -np.inf   # a frame of -inf: index 0
    # (row, offset, first kept frame, kept frames): one chunk keeps nothing, the last is cut short by T (45 + 9 > 49)
    seg = [(0, 0, 0, 40), (0, 40, 5, 30), (1, 3, 8, 0), (1, 3, 8, 41), (1, 44, 45, 9)]
    raw, lo = _stitch(logits, seg, R, Tout)
    want_raw, want_lo = lref.stitch_ref(logits, seg, R, Tout, V, -7, -3.5)
    assert want_raw[0, 42] == 11 and (want_raw[0, 70:] == -7).all() and (want_raw[1, :3] == -7).all()
    assert (want_raw[1, 44:48] != -7).all() and (want_raw[1, 48:] == -7).all()
    assert np.array_equal(raw.cpu().numpy(), want_raw)
    assert np.array_equal(lo.cpu().numpy().view(np.uint32), want_lo.view(np.uint32))
    # without the logits copy, and on an ldv that is no multiple of 4 (the scalar path): the same ids
    raw2, _ = _stitch(logits, seg, R, Tout, want_logits=False)
    assert np.array_equal(raw2.cpu().numpy(), want_raw)
    odd = np.ascontiguousarray(logits[:, :, :47])
    raw3, lo3 = _stitch(odd, seg, R, Tout)
    assert np.array_equal(raw3.cpu().numpy(), want_raw)
    assert np.array_equal(lo3.cpu().numpy(), lref.stitch_ref(odd, seg, R, Tout, V, -7, -3.5)[1])
    # segments that point outside the destination are skipped, not written
    raw4, _ = _stitch(logits, [(2, 0, 0, 5), (0, 88, 0, 10), (-1, 0, 0, 5), (0, 0, 0, 0), (0, 0, 0, 0)], R, Tout)
    w4 = np.full((R, Tout), -7, np.int32)
    w4[0, 88:90] = logits[1, 0:2, :V].argmax(-1)
    assert np.array_equal(raw4.cpu().numpy(), w4)


# ---- 2. collapse -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4096, 4097, 3 * TILE + 5, 70001])
def test_collapse_kernel_matches_numpy(T):
    from coral_amd import ops

    rng = np.random.RandomState(T)
    raw = np.stack([_runs(rng, T, 3), _runs(rng, T, 40, 0.7), _runs(rng, T, 1, 0.1)])
    for edge in range(TILE, T, TILE):  # runs that straddle every tile boundary, blank and not
        raw[0, max(0, edge - 6):edge + 9] = 5
        raw[1, max(0, edge - 2):edge + 1] = BLANK
        raw[2, edge - 1], raw[2, min(T - 1, edge)] = 7, 8  # ... and a run that starts exactly on the boundary
    ids, _, _, olen = _check_collapse(raw, None)
    lens = [T, T // 2, max(0, T - 1)]
    _check_collapse(raw, lens)
    _check_collapse(raw, [0, 1, T + 100] if T > 1 else [0, 1, 5])  # nothing, one frame, longer than the row
    again = _collapse(raw, lens)
    for a, b in zip(again, _collapse(raw, lens)):
        assert np.array_equal(a, b)  # the same bits on every run
    if T <= 4096:  # ids and out_len of the greedy kernel, on one-hot logits of the same rows
        B = raw.shape[0]
        onehot = np.zeros((B, T, LDV), np.float32)
        np.put_along_axis(onehot, raw[:, :, None].astype(np.int64), 1.0, axis=2)
        for in_len in (None, lens):
            r2, i2 = (torch.empty(B, T, dtype=torch.int32, device=DEV) for _ in range(2))
            o2 = torch.empty(B, dtype=torch.int32, device=DEV)
            il = None if in_len is None else _dev(np.asarray(in_len, np.int32), torch.int32)
            ops.ctc_greedy_decode(_dev(onehot, torch.float32), il, r2, i2, o2, B, T, V, LDV, BLANK)
            mine = _collapse(raw, in_len)
            assert np.array_equal(r2.cpu().numpy(), raw)
            assert np.array_equal(i2.cpu().numpy(), mine[0]) and np.array_equal(o2.cpu().numpy(), mine[3])


def test_collapse_kernel_silence_and_one_long_run():
    T = 70001
    rng = np.random.RandomState(8)
    raw = np.stack([np.full(T, BLANK, np.int32), _runs(rng, T, 4), _runs(rng, T, 4)])
    raw[1, 5000:65000] = 9     # one 60 000-frame non-blank run, tokens in front of it and behind it
    raw[1, 4999], raw[1, 65000] = BLANK, 3
    raw[2, :] = 12             # a single run over the whole row
    ids, start, end, olen = _check_collapse(raw, None)
    assert int(olen[0]) == 0 and int(olen[2]) == 1 and (start[2, 0], end[2, 0]) == (0, T)
    k = int(np.flatnonzero(start[1] == 5000)[0])
    assert (int(ids[1, k]), int(end[1, k]), int(start[1, k + 1])) == (9, 65000, 65000)
    ids, start, end, olen = _check_collapse(raw, [T, 64000, 0])
    assert (int(end[1, int(olen[1]) - 1]), int(olen[2])) == (64000, 0)  # the open run ends at in_len


def test_collapse_restatement_reproduces_the_tokenizer_cases_and_the_kernel_agrees():
    meta, _ = lref.load_fixture()
    cases = meta["tokenizer_cases"]
    T = max(len(c["ids"]) for c in cases)
    raw = np.full((len(cases), T), BLANK, np.int32)
    for b, c in enumerate(cases):
        raw[b, :len(c["ids"])] = c["ids"]
    lens = [len(c["ids"]) for c in cases]
    ids, start, end, olen = _check_collapse(raw, lens)
    for b, c in enumerate(cases):
        wi, ws_, we = lref.collapse_ref(c["ids"], lens[b], BLANK)
        assert [[s, e] for s, e in zip(ws_, we)] == [o[1:] for o in c["char_offsets"]]
        k = int(olen[b])
        assert (ids[b, :k].tolist(), start[b, :k].tolist(), end[b, :k].tolist()) == (wi, ws_, we)


# ---- 3. the pipeline's semantics, exactly --------------------------------------------------------
def _tokenizer():
    from coral_amd.processor import CTCTokenizer

    return CTCTokenizer(lref.load_fixture()[0]["vocab"])


def _padded(lg):
    out = np.zeros(lg.shape[:2] + (LDV,), np.float32)
    out[:, :, :V] = lg
    return out


@pytest.mark.parametrize("k", range(4))
def test_recorded_pipeline_logits_decode_to_the_recorded_pipeline_output(k):
    from coral_amd import longform as lf

    meta, z = lref.load_fixture()
    s = meta["settings"][k]
    al, sr = meta["align_to"], meta["sampling_rate"]
    sl = tuple(s["stride_length_s"]) if isinstance(s["stride_length_s"], list) else s["stride_length_s"]
    plan = lf.chunk_plan(meta["n_samples"], s["chunk_length_s"], sl, sr, al)
    lg = _padded(z[f"logits_{k}"])
    seg, total = lf.frame_segments(plan, lg.shape[1], al)
    assert total == s["stitched_len"]
    raw, _ = _stitch(lg, seg, 1, total, want_logits=False)
    rows = lf.collapse_rows(raw, None, BLANK)
    tok = _tokenizer()
    for mode, want in (("char", s["char_chunks"]), ("word", s["word_chunks"])):
        got = lf.decode_rows(rows, tok, mode, al, sr)[0]
        assert got["text"] == s["text"]
        assert [{"text": c["text"], "timestamp": list(c["timestamp"])} for c in got["chunks"]] == want
    assert lf.decode_rows(rows, tok, None, al, sr) == [{"text": s["text"]}]


# ---- 4. engine end to end ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from coral_amd.modeling import Wav2Vec2ForCTC
    from coral_amd.processor import Wav2Vec2Processor, WaveformFeatureExtractor

    model = Wav2Vec2ForCTC.from_pretrained(str(lref.GOLDEN / "hf_ckpt_w2v2")).eval()
    return model, Wav2Vec2Processor(WaveformFeatureExtractor(), _tokenizer())


def test_engine_end_to_end_on_the_fixture_waveform(tiny):
    from coral_amd import longform as lf

    model, proc = tiny
    meta, z = lref.load_fixture()
    s = meta["settings"][1]  # (2.0, (0.5, 0.25)): 5 chunks in batches of 2, 2, 1
    wave = lref.fixture_waveform()
    seen = []
    st = lf.stitch_long(model, [wave], 2.0, (0.5, 0.25), batch_size=2, want_logits=True,
                        on_batch=lambda c0, lg, seg: seen.append((c0, lg.cpu().numpy().copy(), seg)))
    assert [c0 for c0, _, _ in seen] == [0, 2, 4] and st["lengths"] == [s["stitched_len"]]
    n = st["lengths"][0]
    # against the HF logits stitched the same way; the tolerance tests/test_ckpt_gpu.py applies to this checkpoint's logits
    _, want = lref.stitch_ref(_padded(z["logits_1"]), st["segs"][0], 1, n, V, -1, 0.0)
    got = st["logits"][0, :n, :V].cpu().numpy()
    err = np.abs(got - want[0, :, :V]).max()
    print(f"stitched logits max-abs err vs HF: {err:.3e}")
    assert err <= 3e-2, err
    # the stitched ids are the argmax of the chunk logits buffers read back, stitched on the host, exactly
    raw = np.full((1, n), -1, np.int32)
    for c0, lg, seg in seen:
        r, _ = lref.stitch_ref(lg, seg, 1, n, V, -1, 0.0)
        raw = np.where(r >= 0, r, raw)
    assert (raw >= 0).all() and np.array_equal(st["raw"].cpu().numpy()[:, :n], raw)
    ids, start, end = lref.collapse_ref(raw[0], n, BLANK)
    res = lf.transcribe_long(model, proc, [wave], 2.0, (0.5, 0.25), batch_size=2, return_timestamps="char")
    assert res[0]["text"] == proc.tokenizer.decode(ids, group_tokens=False)
    assert [c["timestamp"] for c in res[0]["chunks"]] == [(a * 320 / 16000, b * 320 / 16000) for a, b in zip(start, end)]


# ---- 5. long clips -------------------------------------------------------------------------------
def _monotone(chunks, limit):
    t = 0.0
    for c in chunks:
        a, b = c["timestamp"]
        assert t <= a < b <= limit, (t, a, b)
        t = b
    return True


def test_long_clips(tiny):
    from coral_amd.evaluate import transcribe

    model, proc = tiny
    rng = np.random.RandomState(90)
    w90 = np.clip(0.1 * rng.randn(90 * 16000), -1, 1).astype(np.float32)
    w37 = lref.fixture_waveform(seed=37, seconds=37.0)
    whole = transcribe(model, proc, [w90], chunk_length_s=0)  # T = 4499 frames: beyond the greedy kernel's 4096
    assert model.engine._saved["w"]["T"] == 4499
    assert len(whole) == 1 and isinstance(whole[0], str) and len(whole[0]) > 0
    kw = dict(chunk_length_s=10, batch_size=4)
    words = transcribe(model, proc, [w90], return_timestamps="word", **kw)
    chars = transcribe(model, proc, [w90], return_timestamps="char", **kw)
    assert words[0]["text"] == chars[0]["text"] and len(words[0]["text"]) > 0 and words[0]["chunks"]
    assert _monotone(words[0]["chunks"], 90.0) and _monotone(chars[0]["chunks"], 90.0)
    assert transcribe(model, proc, [w90], **kw) == [chars[0]["text"]]
    # two recordings of different lengths in one call == each alone
    both = transcribe(model, proc, [w37, w90], return_timestamps="char", **kw)
    alone = transcribe(model, proc, [w37], return_timestamps="char", **kw)
    assert both[1] == chars[0] and both[0] == alone[0]
    assert _monotone(both[0]["chunks"], 37.0)
    # timestamps on the whole-clip path too
    short = transcribe(model, proc, [w37[:48000], w37[:32000]], return_timestamps="word")
    assert all(_monotone(r["chunks"], 3.0) for r in short)
    assert [r["text"] for r in short] == transcribe(model, proc, [w37[:48000], w37[:32000]])


# ---- 6. LM route and refusals ----------------------------------------------------------------------
def test_lm_route_and_refusals(tiny):
    from coral_amd import longform as lf
    from coral_amd.config import DictConfig
    from coral_amd.evaluate import evaluate, transcribe
    from coral_amd.ngram import NGramLM, load_attrs
    from coral_amd.processor import Wav2Vec2ProcessorWithLM

    model, proc = tiny
    lm_dir = lref.GOLDEN / "lm_tiny"
    plm = Wav2Vec2ProcessorWithLM(proc.feature_extractor, proc.tokenizer, NGramLM.from_arpa(lm_dir / "3gram.arpa"),
                                  load_attrs(lm_dir))
    wave = lref.fixture_waveform()
    got = lf.transcribe_long(model, plm, [wave, wave[:40000]], 2.0, batch_size=3)
    st = lf.stitch_long(model, [wave, wave[:40000]], 2.0, None, batch_size=3, want_logits=True)
    eng = model.engine
    ids, _ = eng.beam_decode(plm.device_tables(eng.device), tokenizer=plm.tokenizer, in_len=st["in_len"],
                             logits=st["logits"], **plm.decoder_params)
    assert [g["text"] for g in got] == [plm.tokenizer.decode(r, group_tokens=False) for r in ids]
    assert set(got[0]) == {"text"} and len(got[0]["text"]) > 0
    assert transcribe(model, plm, [wave, wave[:40000]], 3, chunk_length_s=2.0) == [g["text"] for g in got]
    with pytest.raises(ValueError, match="return_timestamps"):
        transcribe(model, plm, [wave], chunk_length_s=2.0, return_timestamps="word")
    with pytest.raises(ValueError, match="return_timestamps"):
        transcribe(model, proc, [wave], chunk_length_s=2.0, return_timestamps="sentence")
    with pytest.raises(ValueError, match="chunk_length_s"):
        evaluate(DictConfig(model_dir=str(lref.GOLDEN / "hf_ckpt_whisper"), model_id="x", chunk_length_s=10.0))

    class NotCTC:
        engine = object()

    with pytest.raises(ValueError, match="chunk_length_s"):
        lf.transcribe_long(NotCTC(), proc, [wave], 2.0)
