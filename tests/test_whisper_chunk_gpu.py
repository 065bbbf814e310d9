"""Chunked Whisper long-form decoding on a real MI355X: ca_overlap_merge against the plain-Python restatement
(tests/whisper_chunk_ref.py) by exact integer equality - merged ids, lengths and cuts -, and `transcribe_chunked` end to
end on the fixture checkpoint (tests/golden/hf_ckpt_whisper, which decodes noise to special ids only: its merges are of
empty rows) and on the timestamp fixture of tests/whisper_ts_ref.py (which gives text, so that cuts happen)."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_chunk_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN_DIR = Path(__file__).resolve().parent / "golden"


def _launch(groups, skip_ids=None, n_bits=None, row_start=None, ld=None, filler=7):
    """groups: [[rows]] -> (merged per group, out_len, cuts) from one ca_overlap_merge launch.  row_start: one offset per
    row; the cells outside a row hold `filler`, which must never come out."""
    from coral_amd import ops

    rows = [r for g in groups for r in g]
    starts = [0] * len(rows) if row_start is None else list(row_start)
    ld = ld or max(1, max(s + len(r) for s, r in zip(starts, rows)))
    table = np.full((len(rows), ld), filler, dtype=np.int32)
    for i, (s, r) in enumerate(zip(starts, rows)):
        table[i, s:s + len(r)] = r
    skip = None if skip_ids is None else ops.skip_bitmap(skip_ids, n_bits, DEV)
    res = ops.overlap_merge(torch.from_numpy(table).to(DEV), [len(r) for r in rows],
                            np.concatenate([[0], np.cumsum([len(g) for g in groups])]), row_start=row_start and starts,
                            skip=skip, want_cuts=True)
    torch.cuda.synchronize()
    return ops.overlap_merge_read(res)


def _expect(groups, skip_ids=()):
    """The restatement over the rows without the skipped ids -> (merged per group, cuts [rows, 2], wins per group)."""
    skip = set(skip_ids)
    merged, cuts, wins = [], [], []
    for g in groups:
        m, c, w = C.merge_sequences([[t for t in r if t not in skip] for r in g])
        merged.append(m)
        cuts += ([(-1, -1)] + c) if g else []
        wins.append(w)
    return merged, np.array(cuts, dtype=np.int32).reshape(-1, 2), wins


def _check(groups, **kw):
    want, want_cuts, wins = _expect(groups, kw.get("skip_ids") or ())
    got, out_len, cuts = _launch(groups, **kw)
    assert out_len.tolist() == [len(m) for m in want]
    assert got == want
    assert np.array_equal(cuts, want_cuts), (cuts.tolist(), want_cuts.tolist())
    return wins


def _stream_rows(rng, n_rows, length, vocab, overlap, noise=0.1):
    """Rows cut from one token stream, each overlapping the one before by about `overlap` tokens, with substitutions."""
    stream = [rng.randrange(vocab) for _ in range(n_rows * length + overlap)]
    rows = []
    for j in range(n_rows):
        lo = max(0, j * (length - overlap) - rng.randint(0, 2))
        rows.append([t if rng.random() > noise else rng.randrange(vocab) for t in stream[lo:lo + length]])
    return rows


def test_small_cases_equal_the_restatement():
    groups = [
        [[1, 2, 3]],                                           # one row: nothing to merge
        [[], [1, 2, 3], [2, 3, 4]], [[1, 2, 3], [], [2, 3, 4]], [[1, 2, 3], [2, 3, 4], []], [[], []], [[]],
        [[1, 2, 3], [4, 5, 6]],                                # no diagonal with two matches: concatenation
        [[1, 2, 3], [3, 9, 8]], [[1, 2, 3, 4], [9, 4, 8, 7]],  # exactly one match: not accepted
        # two diagonals with the same matches / i ratio (2 / 2 and 4 / 4): the longer wins through i / 10000
        [[9, 9, 5, 6, 5, 6], [5, 6, 5, 6, 7, 7]],
        [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [11, 12, 13]],          # right shorter than left (i > R)
        [[11, 12], [1, 2, 3, 11, 12, 13, 14, 15, 16, 17]],                 # right longer than left (i > L)
        [[3, 4, 5], [1, 2, 3, 4, 5, 6, 7, 8, 9]],
        [[7] * 9, [7] * 5, [7] * 12], [[7] * 64, [7] * 65], [[7, 7], [7, 7], [7, 7], [7]],  # one repeated token
        [[1, 2, 3, 4, 5], [4, 5, 6, 7, 8], [7, 8, 9, 10, 11]],            # three rows: a cut changes the next left side
        [[1, 2, 3, 4, 5, 6], [5, 6, 7, 8], [1, 2, 7, 8, 9], [8, 9, 10, 11], [10, 11, 12]],  # five rows
    ]
    wins = _check(groups)
    assert wins[6] == [None] and wins[7] == [None] and wins[8] == [None]
    left, right = groups[9]
    assert C.diagonal(left, right, 2)[0] == 2 and C.diagonal(left, right, 4)[0] == 4 and wins[9] == [4]
    assert wins[10][0] is not None and wins[11][0] is not None and wins[16] == [2, 2] and all(w is not None for w in wins[17])


def test_equal_float64_scores_keep_the_earlier_diagonal():
    """Diagonals 100 and 200 land in different waves of the workgroup: the tie crosses the workgroup reduction."""
    left, right = C.equal_score_pair()
    s1, s2 = C.diagonal(left, right, 100)[1], C.diagonal(left, right, 200)[1]
    assert s1 == s2 and C.diagonal(left, right, 100)[0] == C.diagonal(left, right, 200)[0] == 2
    wins = _check([[left, right], [right[::-1], left[::-1]]])
    assert wins[0] == [100]


@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 255, 256, 257, 448])
def test_row_lengths_around_the_wave_and_workgroup_sizes(length):
    rng = random.Random(length)
    rows = _stream_rows(rng, 3, length, 60, overlap=max(1, length // 6))
    other = _stream_rows(rng, 2, length, 5, overlap=max(1, length // 3))
    wins = _check([rows, other, [rows[0], rows[0]], [rows[1][: length // 2 + 1], rows[1]]])
    if length >= 63:
        assert all(w is not None for w in wins[0]), wins[0]


def test_the_bitmap_drops_ids_while_a_row_is_loaded():
    """Skipped ids at the start, in the middle and at the end of a row, across the 256-token rounds of the load; an id
    outside the bitmap's range is kept."""
    rng = random.Random(5)
    skip_ids, n_bits = [50, 51, 52, 53, 63] + list(range(64, 100)), 100
    rows = []
    for row in _stream_rows(rng, 4, 300, 40, overlap=50):
        row = [51, 52, 53] + row[:100] + [70] + row[100:290] + [71, 64] + row[290:] + [50, 50, 50]
        rows.append(row)
    rows[2][5] = 150  # above n_bits: kept
    only_skipped = [[51, 52, 53, 50], [1, 2, 3], [51, 2, 3, 4, 50]]
    _check([rows, only_skipped, [[1, 2, 3, 63, 99]]], skip_ids=skip_ids, n_bits=n_bits)
    # bit 31 / 32 / 33: the word boundary of the bitmap
    _check([[[31, 32, 33, 1, 2, 3], [32, 2, 3, 31, 4, 33]]], skip_ids=[31, 33], n_bits=34)


def test_row_start_and_a_leading_dimension_larger_than_the_row():
    rng = random.Random(9)
    groups = [_stream_rows(rng, 3, 40, 30, overlap=8), _stream_rows(rng, 2, 17, 30, overlap=5)]
    n = sum(len(g) for g in groups)
    _check(groups, row_start=[rng.randint(1, 9) for _ in range(n)], ld=64, filler=groups[0][0][-1])


def test_more_workgroups_than_compute_units():
    rng = random.Random(300)
    groups = [_stream_rows(rng, rng.randint(2, 4), rng.randint(3, 20), 15, overlap=3) for _ in range(300)]
    _check(groups)


def test_random_groups_over_a_small_vocabulary():
    rng = random.Random(12)
    groups = [[[rng.randrange(12) for _ in range(rng.choice((0, 1, 3, 8, 20, 45, 90)))] for _ in range(rng.randint(1, 6))]
              for _ in range(200)]
    wins = _check(groups)
    assert sum(1 for w in wins if any(i is not None for i in w)) >= 100, "overlaps must be common in this test"


def test_a_row_above_the_limit_is_refused_without_a_launch():
    from coral_amd import _lib, ops

    assert _lib.CHUNK_MERGE_MAX_TOKENS == 1024
    ok = torch.zeros(2, 1024, dtype=torch.int32, device=DEV)
    res = ops.overlap_merge(ok, [1024, 1024], [0, 2], want_cuts=True)
    merged, out_len, cuts = ops.overlap_merge_read(res)  # at the limit: all zeros, the full overlap wins, cut in its middle
    want, want_cuts, _ = C.merge_sequences([[0] * 1024, [0] * 1024])
    assert merged == [want] and out_len.tolist() == [1024] and cuts.tolist() == [[-1, -1], [512, 512]] == [[-1, -1]] + [list(c) for c in want_cuts]
    ids = torch.zeros(2, 1025, dtype=torch.int32, device=DEV)
    out = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    args = torch.tensor([3, 1025, 0, 2, 0, 1028], dtype=torch.int32, device=DEV)
    rc = ops.lib().ca_overlap_merge(ids.data_ptr(), 1025, None, args.data_ptr(), 2, 1025, None, 0, args.data_ptr() + 8,
                                    args.data_ptr() + 16, 1, out.data_ptr(), 4, out.data_ptr() + 16, None,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"CA_CHUNK_MERGE_MAX_TOKENS" in ops.lib().ca_last_error()
    assert out.cpu().tolist() == [-7] * 8, "CA_ERR_ARG must come back before anything is launched"
    with pytest.raises(ops.CoralAmdError, match="CA_CHUNK_MERGE_MAX_TOKENS"):
        ops.overlap_merge(ids, [3, 1025], [0, 2])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
MAX_LENGTH = 64


def _ts_fixture_model():
    """The timestamp fixture of tests/whisper_ts_ref.py: 50 text ids, eos 50, timestamps from 64; its weights are made so
    that text and timestamps both come out."""
    import whisper_ts_ref as R

    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperForConditionalGeneration

    model = WhisperForConditionalGeneration(WhisperShape(**R.CONFIG), device=DEV).eval()
    model.engine.load_state_dict(R.fixture_params())
    model.engine.refresh_derived()
    model.generation_config = dict(no_timestamps_token_id=R.NO_TIMESTAMPS, lang_to_id={"<|da|>": R.LANG},
                                   task_to_id={"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE},
                                   max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)
    return model


@pytest.fixture(scope="module", params=["hf_ckpt_whisper", "timestamp_fixture"])
def fixture_model(request):
    """(model, processor, a recording of 70.3 s, a clip of 12 s, the forced prefix, eos, the first timestamp id).
    hf_ckpt_whisper: the checkpoint directory transformers wrote (150 text ids, eos 150, timestamps from 164)."""
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

    if request.param == "hf_ckpt_whisper":
        model = WhisperForConditionalGeneration.from_pretrained(str(GOLDEN_DIR / "hf_ckpt_whisper"), device=DEV).eval()
        model.generation_config = dict(no_timestamps_token_id=163, lang_to_id={"<|da|>": 152},
                                       task_to_id={"transcribe": 153, "translate": 154})
        assert model.shape.vocab_size == 200
        prefix, eos = [151, 152, 153, 163], 150
    else:
        model = _ts_fixture_model()
        prefix, eos = [51, 52, 53, 63], 50
    assert model.forced_prefix() == prefix and model.shape.eos_token_id == eos
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    g = np.random.RandomState(70)
    long_ = np.clip(0.1 * g.randn(70 * 16000 + 4800), -1, 1).astype(np.float32)
    short = np.clip(0.1 * g.randn(12 * 16000), -1, 1).astype(np.float32)
    return model, proc, long_, short, prefix, eos, prefix[-1] + 1


def _chunks_of(wave):
    return [wave[s:s + n] for s, n, _, _ in C.chunk_strides(len(wave), 480000, 80000, 80000)]


def test_chunked_transcription_equals_the_restatement_on_its_own_chunk_ids(fixture_model):
    from coral_amd.chunked_whisper import special_ids, transcribe_chunked
    from coral_amd.evaluate import transcribe_whisper

    model, proc, long_, short, prefix, eos, tb = fixture_model
    assert special_ids(model, proc) == list(range(eos, tb))
    res = transcribe_chunked(model, proc, [long_, short], chunk_length_s=30, batch_size=16, max_length=MAX_LENGTH)
    assert [len(r["chunk_ids"]) for r in res] == [4, 1]  # 0, 20, 40 and 60 s: the last chunk is 10.3 s long
    # the per-chunk ids are those of one generate call on the same chunk batch
    clips = _chunks_of(long_) + _chunks_of(short)
    plain = model.generate(proc.feature_extractor(clips), max_length=MAX_LENGTH)
    plain = plain.tolist() if hasattr(plain, "tolist") else [list(map(int, r)) for r in plain]
    assert res[0]["chunk_ids"] + res[1]["chunk_ids"] == plain
    assert all(r[:4] == prefix for r in plain)
    # text and ids: the restatement applied to those ids
    for r in res:
        text_rows = [[t for t in row if t < eos] for row in r["chunk_ids"]]
        want = C.merge_sequences(text_rows)[0]
        print("text tokens per chunk", [len(t) for t in text_rows], "merged", len(want))
        assert r["ids"] == want and r["text"] == proc.batch_decode([want])[0]
    if eos == 50:  # the timestamp fixture gives text: the long recording's chunks overlap and are cut
        n_text = sum(1 for row in res[0]["chunk_ids"] for t in row if t < eos)
        assert 0 < len(res[0]["ids"]) < n_text
    # a recording of one chunk is a clip: what plain transcribe_whisper gives
    texts, rows = transcribe_whisper(model, proc, [short], max_length=MAX_LENGTH)
    alone = transcribe_chunked(model, proc, [short], chunk_length_s=30, max_length=MAX_LENGTH)
    assert alone[0]["chunk_ids"] == rows
    assert alone[0]["text"] == proc.batch_decode([[t for t in rows[0] if t < eos]])[0]
    if eos >= 50257:  # (the offline rendering skips special ids from 50257 upward only: a toy vocabulary's stay in `texts`)
        assert alone[0]["text"] == texts[0]
    assert res[1]["chunk_ids"][0][:len(rows[0])] == rows[0] and res[1]["ids"] == alone[0]["ids"]
    # through the public entry
    texts2, rows2 = transcribe_whisper(model, proc, [long_, short], max_length=MAX_LENGTH, long_form="chunked")
    assert texts2 == [r["text"] for r in res] and rows2 == [r["ids"] for r in res]
    # beams on a long recording: the sequential loop refuses them, chunks are clips
    with pytest.raises(ValueError, match="num_beams"):
        transcribe_whisper(model, proc, [long_], max_length=MAX_LENGTH, num_beams=2)
    beam = transcribe_chunked(model, proc, [long_], chunk_length_s=30, max_length=MAX_LENGTH, num_beams=2)
    assert isinstance(beam[0]["text"], str) and len(beam[0]["chunk_ids"]) == 4
    assert beam[0]["ids"] == C.merge_sequences([[t for t in row if t < eos] for row in beam[0]["chunk_ids"]])[0]


def test_chunked_timestamps_equal_the_restated_state_machine(fixture_model):
    from coral_amd.chunked_whisper import transcribe_chunked

    model, proc, long_, short, prefix, eos, tb = fixture_model
    clips = _chunks_of(long_)
    assert len(clips) == 4 and len(clips[-1]) < 480000
    res = transcribe_chunked(model, proc, [long_, short], chunk_length_s=30, batch_size=len(clips), max_length=MAX_LENGTH,
                             return_timestamps=True)
    plain = model.generate(proc.feature_extractor(clips), max_length=MAX_LENGTH, return_timestamps=True)
    assert res[0]["chunk_ids"] == [list(map(int, r)) for r in plain]
    assert all(r[:3] == prefix[:3] and r[3] >= tb for r in res[0]["chunk_ids"])
    for r, wave in zip(res, (long_, short)):
        plan = C.chunk_strides(len(wave), 480000, 80000, 80000)
        outs = [dict(tokens=row, stride=(n / 16000, left / 16000, right / 16000)) for row, (_, n, left, right) in
                zip(r["chunk_ids"], plan)]
        want = C.transcript(outs, lambda ids: proc.batch_decode([ids])[0], timestamp_begin=tb,
                            special_ids=range(eos, tb), time_precision=0.02)
        print("segments", [(c["timestamp"], len(m)) for c, m in zip(want["chunks"], want["merged"])])
        assert [(c["text"], c["timestamp"]) for c in r["chunks"]] == [(c["text"], c["timestamp"]) for c in want["chunks"]]
        assert r["ids"] == [t for m in want["merged"] for t in m]
        assert r["text"] == " ".join(c["text"] for c in want["chunks"] if c["text"])
        assert r["chunks"], "a chunk that starts with a timestamp opens a segment"
    with pytest.raises(ValueError, match="num_beams"):
        transcribe_chunked(model, proc, [long_], num_beams=2, return_timestamps=True)


def test_sequential_long_form_issues_the_parents_launches(monkeypatch, tmp_path):
    """long_form="sequential" (the default) on the timestamp fixture of tests/whisper_ts_ref.py, a short and a long
    clip: not one ca_overlap_merge launch and not one step into the chunked module, and the results are the parent
    commit's pieces called directly - one `generate` for the short clip, the window loop for the long one."""
    import whisper_ts_ref as R

    from coral_amd import chunked_whisper, evaluate as E, ops
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperProcessor

    model = _ts_fixture_model()
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    short, long_ = R.short_waves()[1], R.long_waves()[0]

    def boom(*a, **k):
        raise AssertionError("a chunked-mode launch on the sequential path")

    monkeypatch.setattr(ops, "overlap_merge", boom)
    monkeypatch.setattr(ops, "skip_bitmap", boom)
    monkeypatch.setattr(chunked_whisper, "transcribe_chunked", boom)
    texts, rows = E.transcribe_whisper(model, proc, [short, long_], batch_size=2, max_length=R.MAX_LENGTH, long_form="sequential")
    plain = model.generate(proc.feature_extractor([short]), max_length=R.MAX_LENGTH)
    assert rows[0] == [int(v) for v in plain[0]] and texts[0] == proc.batch_decode([rows[0]], skip_special_tokens=True)[0]
    looped, looped_rows = E._transcribe_whisper_windows(model, proc, [long_], 2, R.MAX_LENGTH, False)
    assert texts[1] == looped[0] and rows[1] == looped_rows[0]
    with pytest.raises(ValueError, match="without it"):
        E.transcribe_whisper(model, proc, [short], chunk_length_s=30.0)
