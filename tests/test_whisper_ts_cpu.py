"""Whisper timestamps without a GPU: the restated rules against the recorded output of transformers' own
WhisperTimeStampLogitsProcessor, the segment cutter and the long-form loop against transformers' recorded long-form
generations (tests/golden/whisper_ts.npz, tools/gen_whisper_ts_goldens.py), and what stays refused."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_ts_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def test_restated_rules_give_the_processors_mask_exactly():
    z = R.load_golden()
    n = len(z["proc_seed"])
    assert n >= 30
    sides = set()
    for i in range(n):
        scores, hist, cap, mask = R.processor_case(z, i)
        row, info = R.timestamp_rules(scores, hist, R.TIMESTAMP_BEGIN, R.EOS, cap, detail=True)
        assert np.array_equal(np.isneginf(row), mask), (i, hist, cap)
        if np.isfinite(info["lse"]) and np.isfinite(info["text_max"]):
            # the processor decides in fp32: the recorded cases are not near-ties of the log-prob rule
            assert abs(info["lse"] - info["text_max"]) > 1e-3, (i, info["lse"], info["text_max"])
            sides.add(info["forced"])
    assert sides == {True, False}


def test_recorded_generations_take_every_branch_and_obey_the_grammar():
    """Five of the seven branches show in the ids and are re-derived here.  Two need the scores of the step, which the
    fixture does not hold: that a timestamp after text was forced by the log-prob rule (a text token scored higher), and
    that the monotonic mask removed the otherwise-best timestamp.  For those the test rests on the counts the tool
    took from transformers' own scores and recorded (it asserts every count > 0 before it writes the file); from the ids
    only `timestamp_after_text`, a necessary condition of the first, is checked."""
    z = R.load_golden()
    counts = dict(zip(R.BRANCHES, z["branch_counts"].tolist()))
    assert len(z["branch_counts"]) == len(R.BRANCHES)
    for name in R.BRANCHES:
        assert counts[name] > 0, name
    P = len(R.PREFIX)
    rows = [r for r in z["short_ids"].tolist()]
    for n in range(len(R.LONG_SECONDS)):
        rows += [R.PREFIX + ids[:k].tolist() + [R.EOS] for ids, k in zip(z[f"long{n}_ids"], z[f"long{n}_len"])]
    seen = R.branches_from_ids(rows, P, R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX)
    assert seen >= {"initial_cap", "text_while_open", "timestamp_after_text", "pair_closed", "text_after_pair",
                    "eos_after_single"}, seen
    for r in z["short_ids"].tolist():
        assert r[:P] == R.PREFIX
        assert R.grammar_ok(R.strip_row(r, P, R.EOS, R.EOS), R.TIMESTAMP_BEGIN, R.EOS), r


@pytest.mark.parametrize("n", range(len(R.LONG_SECONDS)))
def test_longform_loop_replays_the_recorded_windows_to_the_recorded_segments(n):
    from coral_amd.longform_whisper import run_longform, segments_of

    z = R.load_golden()
    P = len(R.PREFIX)
    windows = {int(s): ids[:k].tolist() for s, ids, k in zip(z[f"long{n}_seek"], z[f"long{n}_ids"], z[f"long{n}_len"])}
    asked = []

    def window_generate(batch):
        asked.append(batch)
        # rows as generate returns them: prefix, ids, EOS, padded to a common length
        rows = [R.PREFIX + windows[seek] + [R.EOS] for _, seek in batch]
        L = max(len(r) for r in rows) + 2
        return [r + [R.EOS] * (L - len(r)) for r in rows]

    frames = int(z[f"long{n}_frames"])
    assert frames == int(R.LONG_SECONDS[n] * 100) > 3000
    res = run_longform(window_generate, [frames], R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS)[0]
    assert [s for s, _ in res["windows"]] == z[f"long{n}_seek"].tolist()
    assert [g for _, g in res["windows"]] == [windows[s] for s in z[f"long{n}_seek"].tolist()]
    want_ids = [ids[:k].tolist() for ids, k in zip(z[f"long{n}_seg_ids"], z[f"long{n}_seg_len"])]
    assert [s[2] for s in res["segments"]] == want_ids
    assert [s[0] for s in res["segments"]] == z[f"long{n}_seg_start"].tolist()  # equal as floats
    assert [s[1] for s in res["segments"]] == z[f"long{n}_seg_end"].tolist()
    # one window alone, offset 0
    first = segments_of(windows[0], R.TIMESTAMP_BEGIN)
    assert first == [s for s in res["segments"][:len(first)]]


def test_two_recordings_share_the_rounds_and_batches_are_capped():
    from coral_amd.longform_whisper import run_longform

    z = R.load_golden()
    P = len(R.PREFIX)
    tables = [{int(s): ids[:k].tolist() for s, ids, k in zip(z[f"long{n}_seek"], z[f"long{n}_ids"], z[f"long{n}_len"])}
              for n in range(2)]
    sizes = []

    def window_generate(batch):
        sizes.append(len(batch))
        return [R.PREFIX + tables[c][seek] + [R.EOS] for c, seek in batch]

    frames = [int(z[f"long{n}_frames"]) for n in range(2)]
    both = run_longform(window_generate, frames, R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS)
    for n in range(2):
        assert [s for s, _ in both[n]["windows"]] == z[f"long{n}_seek"].tolist()
    assert sizes[0] == 2 and sizes[-1] == 1
    sizes.clear()
    run_longform(window_generate, frames, R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS, batch_size=1)
    assert set(sizes) == {1}


def test_segments_of_hand_made_windows():
    from coral_amd.longform_whisper import segments_of

    tb = 100
    # two closed pairs, then an unfinished rest: advance to the last closed pair (index 50 -> 100 frames)
    segs, adv = segments_of([100, 5, 6, 120, 120, 7, 150, 150, 8, 9], tb, return_advance=True)
    assert [(s, e) for s, e, _ in segs] == [(0.0, 20 * 0.02), (20 * 0.02, 50 * 0.02)] and adv == 100
    assert segs[0][2] == [100, 5, 6, 120] and segs[1][2] == [120, 7, 150, 150]
    # a single closing timestamp: the whole window is consumed
    segs, adv = segments_of([100, 5, 120, 120, 7, 140], tb, num_frames=3000, time_offset=30.0, return_advance=True)
    assert [(s, e) for s, e, _ in segs] == [(30.0, 30.0 + 20 * 0.02), (30.0 + 20 * 0.02, 30.0 + 40 * 0.02)] and adv == 3000
    # no pair: one segment up to the last timestamp, or to the end of the window without one
    segs, adv = segments_of([100, 5, 6, 130], tb, return_advance=True)
    assert [(s, e) for s, e, _ in segs] == [(0.0, 30 * 0.02)] and adv == 3000
    segs, adv = segments_of([100, 5, 6], tb, num_frames=500, return_advance=True)
    assert [(s, e) for s, e, _ in segs] == [(0.0, 250 * 0.02)] and adv == 500


def test_what_stays_refused():
    from coral_amd.longform_whisper import run_longform
    from coral_amd.whisper import check_beam_arguments

    with pytest.raises(ValueError, match="return_timestamps"):
        check_beam_arguments(2, 5, 1.0, False, dict(return_timestamps=True))
    for kw in (dict(temperature=(0.0, 0.2, 0.4)), dict(condition_on_prev_tokens=True), dict(no_speech_threshold=0.6),
               dict(logprob_threshold=-1.0), dict(compression_ratio_threshold=1.35), dict(num_beams=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            run_longform(lambda batch: [], [4000], 100, 3, 0, 0, **kw)
    run_longform(lambda batch: [[1, 2, 3, 100, 5, 140, 0]] * len(batch), [2500], 100, 3, 0, 0, temperature=None,
                 condition_on_prev_tokens=False)


def test_evaluate_still_refuses_chunk_length_for_whisper(tmp_path):
    import json

    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate

    (tmp_path / "config.json").write_text(json.dumps(dict(architectures=["WhisperForConditionalGeneration"], model_type="whisper")))
    cfg = load_config("evaluation", [f"model_id={tmp_path}", "chunk_length_s=10"])
    assert cfg.get("return_timestamps", None) is False
    with pytest.raises(ValueError, match="without it"):
        evaluate(cfg)


def test_engine_and_wrapper_refuse_beams_with_timestamps_by_name():
    """Argument checks run before any device work (no GPU needed: the engine is never built)."""
    from coral_amd.whisper import WhisperEngine
    from coral_amd.whisper_setup import WhisperForConditionalGeneration

    class Shape:
        vocab_size, eos_token_id, max_target_positions = 1565, 50, 64

    eng = WhisperEngine.__new__(WhisperEngine)
    eng.s, eng.device = Shape(), "cpu"
    with pytest.raises(ValueError, match="return_timestamps"):
        eng.generate(None, [51, 52, 53], 20, num_beams=2, return_timestamps=True, timestamp_begin=64)
    with pytest.raises(ValueError, match="timestamp_begin"):
        eng.generate(None, [51, 52, 53], 20, return_timestamps=True)
    model = WhisperForConditionalGeneration.__new__(WhisperForConditionalGeneration)
    model.generation_config, model.shape = {}, type("S", (), dict(vocab_size=51865, decoder_start_token_id=50258))()
    import torch

    with pytest.raises(ValueError, match="return_timestamps"):
        model.generate(torch.zeros(2, 80, 3000), num_beams=2, return_timestamps=True)
    assert model.forced_prefix() == [50258, 50285, 50359, 50363] and model.forced_prefix(True) == [50258, 50285, 50359]
    model.generation_config = dict(lang_to_id={"<|da|>": 52}, task_to_id={"transcribe": 53}, no_timestamps_token_id=63)
    model.shape.decoder_start_token_id = 51
    assert model.forced_prefix(True) == R.PREFIX and model.forced_prefix() == R.PREFIX_NO_TS


def test_new_symbols_are_declared_on_both_sides():
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym in ("ca_argmax_timestamps", "ca_argmax_timestamps_advance"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    assert callable(ops.argmax_timestamps) and callable(ops.argmax_timestamps_advance)
    # argument validation needs no GPU: eos_id must lie below timestamp_begin, timestamp_begin inside the vocabulary
    assert lib.ca_argmax_timestamps(None, None, None, 1, 8, 8, None, 1, None, 0, 4, 1, -1, None) == -1
    assert b"ca_argmax_timestamps" in lib.ca_last_error()
