"""Whisper word timestamps without a GPU: the restatements (tests/whisper_word_ref.py, coral_amd/whisper_align.py, the
long-form carrier of coral_amd/longform_whisper.py) against what transformers recorded in tests/golden/whisper_word.npz,
the refusals by name, and the C ABI additions."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_ts_ref as R  # noqa: E402
import whisper_word_ref as W  # noqa: E402

from coral_amd import whisper_align as A  # noqa: E402

P = len(R.PREFIX)


def test_restated_dtw_reproduces_every_recorded_path_and_time():
    z = W.load_golden()
    ids, times = z["short_ids"], z["short_times"]
    Ltot = ids.shape[1]
    frames = W.frames_of(z["short_num_frames"].tolist(), len(ids))
    assert frames == [200, 575, 1350] and A.frames_of(z["short_num_frames"].tolist(), 3) == frames
    for b in range(len(ids)):
        m, path = z[f"short_cost{b}"], z[f"short_path{b}"]
        assert m.shape == (Ltot - 1 - P, frames[b])
        text, time = W.dtw(m)
        assert np.array_equal(text, path[0]) and np.array_equal(time, path[1])
        jump = W.jump_frames(text, time)
        assert np.array_equal(W.token_times(jump, P, Ltot), times[b])
        assert np.array_equal(A.times_from_jumps(jump[None], P, Ltot)[0], times[b])
        assert (np.diff(times[b]) >= 0).all() and times[b].max() <= frames[b] * 0.02
    for name in W.DTW_CASES:
        text, time = W.dtw(W.dtw_case(name))
        assert np.array_equal(text, z[f"dtw_{name}"][0]) and np.array_equal(time, z[f"dtw_{name}"][1]), name
    br = json.loads(str(z["dtw_branches"]))["ties"]
    assert br == W.dtw_branches(W.dtw_case("ties")) and all(v > 0 for v in br.values())
    text, time = W.dtw(np.full((1, 6), np.nan))
    assert np.array_equal(text, z["dtw_nan"][0]) and np.array_equal(time, z["dtw_nan"][1])
    assert W.token_times(W.jump_frames(text, time), P, P + 2).tolist() == [0.0] * (P + 2)
    # no DTW tokens at all: every time is 0
    assert A.times_from_jumps(np.zeros((2, 0), dtype=np.int32), P, P + 1).tolist() == [[0.0] * (P + 1)] * 2


def test_oracle_cost_is_the_matrix_transformers_fed_its_dtw():
    """The fp32 oracle's matrix on the recorded ids against transformers' (two fp32 evaluations of one formula: they
    differ by rounding only; the standardised weights are O(1), 1e-3 is a loose bound on that)."""
    z = W.load_golden()
    costs = W.oracle_costs(z["short_ids"], R.short_features(), R.fixture_params(), R.fixture_config(),
                           z["short_num_frames"].tolist())
    for b, c in enumerate(costs):
        assert c.shape == z[f"short_cost{b}"].shape
        assert float(np.abs(c - z[f"short_cost{b}"]).max()) <= 1e-3


def test_median_filter_is_skipped_on_short_inputs_and_sorts_nan_last():
    x = torch.tensor([[[3.0, 1.0, 2.0]]])
    assert torch.equal(W.median_filter(x, 7), x)                      # 3 <= 7 // 2
    y = torch.tensor([[[5.0, 1.0, 4.0, 2.0, 3.0, 9.0]]])
    assert W.median_filter(y, 3)[0, 0].tolist() == [1.0, 4.0, 2.0, 3.0, 3.0, 3.0]
    n = torch.tensor([[[1.0, float("nan"), 0.0, 2.0]]])
    got = W.median_filter(n, 3)[0, 0]
    assert torch.isnan(got[0]) and got[1].item() == 1.0 and got[2].item() == 2.0 and got[3].item() == 0.0
    with pytest.raises(ValueError, match="odd number"):
        W.median_filter(y, 4)


def test_word_grouping_equals_transformers():
    z = W.load_golden()
    words = json.loads(str(z["words"]))
    assert len(words) == len(W.WORD_CASES)
    for case, want in zip(W.WORD_CASES, words):
        w, wt, wi = A.combine_tokens_into_words(W.word_decode, case, W.WORD_EOS)
        assert dict(words=w, tokens=wt, indices=wi) == want, case
    for (ids, tt), want in zip(W.ASR_CASES, json.loads(str(z["asr"]))):
        got = A.word_chunks(W.word_decode, ids, tt, W.WORD_TIMESTAMP_BEGIN, W.WORD_EOS, special_ids=[W.WORD_EOS, 41, 42])
        assert [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in got] == want["chunks"]
        assert "".join(c["text"] for c in got) == want["text"]
    # the offline rendering: every text token is its own word, its interval (the token in front's time, its own)
    got = A.word_chunks(A.offline_decode, [64, 5, 6, 80, 80, 7, 90], [0.0, 0.1, 0.26, 0.4, 0.4, 0.5, 0.62], 64, 50)
    assert got == [dict(text=" t5", timestamp=(0.0, 0.1)), dict(text=" t6", timestamp=(0.1, 0.26)),
                   dict(text=" t7", timestamp=(0.4, 0.5))]
    with pytest.raises(ValueError, match="token times"):
        A.word_chunks(A.offline_decode, [64, 5], [0.0], 64, 50)
    assert A.cap_token_times(np.array([0.0, 11.48, 11.5, 12.0, 26.2], dtype=np.float32), 11.5) == [0.0, float(np.float32(11.48)),
                                                                                                  11.5, 11.5, 11.5]


def test_longform_carries_the_recorded_token_times():
    from coral_amd.longform_whisper import run_longform, segments_of

    z = W.load_golden()
    table = {int(s): (ids[:n].tolist(), tt[:n]) for s, ids, tt, n in zip(z["long_seek"], z["long_ids"], z["long_times"], z["long_len"])}
    asked = []

    def window_generate(batch):
        asked.append([s for _, s in batch])
        return [table[s][0] for _, s in batch], [table[s][1] for _, s in batch]

    res = run_longform(window_generate, [int(z["long_frames"])], R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS,
                       return_token_timestamps=True)[0]
    assert [s for (s,) in asked] == z["long_seek"].tolist()
    assert len(res["segments"]) == len(z["long_seg_len"])
    for seg, n, ids, tt in zip(res["segments"], z["long_seg_len"], z["long_seg_ids"], z["long_seg_times"]):
        assert seg[2] == ids[:n].tolist()
        assert seg[3].dtype == np.float32 and np.array_equal(seg[3], tt[:n])
    # a window past the first: its times are shifted by its offset
    assert res["segments"][-1][3].min() >= np.float32(z["long_seek"][-1] * 0.01) > 60
    for w in res["windows"]:
        assert len(w) == 3 and len(w[1]) == len(w[2])
    # without token times the carrier is what it was
    plain = run_longform(lambda batch: [table[s][0] for _, s in batch], [int(z["long_frames"])], R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS)[0]
    assert [s[:3] for s in res["segments"]] == plain["segments"] and all(len(w) == 2 for w in plain["windows"])
    with pytest.raises(ValueError, match="token times"):
        segments_of([R.TIMESTAMP_BEGIN, 5, R.TIMESTAMP_BEGIN + 9], R.TIMESTAMP_BEGIN, token_times=[0.0, 0.1])
    with pytest.raises(ValueError, match="condition_on_prev_tokens"):  # the other refusals stay
        run_longform(window_generate, [3000], R.TIMESTAMP_BEGIN, P, R.EOS, R.EOS, condition_on_prev_tokens=True)


def test_refusals_are_raised_by_name():
    from coral_amd import _lib

    with pytest.raises(ValueError, match="alignment_heads"):
        A.check_alignment_heads(None, 2, 4)
    with pytest.raises(ValueError, match="no `alignment_heads`"):
        A.check_alignment_heads(None, 2, 4)
    with pytest.raises(ValueError, match=r"alignment_heads: \(2, 0\)"):
        A.check_alignment_heads([(0, 1), (2, 0)], 2, 4)
    with pytest.raises(ValueError, match="alignment_heads: 33 heads"):
        A.check_align_limits(_lib.ALIGN_MAX_HEADS + 1, 10, 100, 64)
    with pytest.raises(ValueError, match="448 tokens"):
        A.check_align_limits(4, _lib.ALIGN_MAX_TOKENS + 1, 100, 64)
    with pytest.raises(ValueError, match="1501 encoder positions"):
        A.check_align_limits(4, 10, 1501, 64)
    for hd in (4, 12, 136):
        with pytest.raises(ValueError, match="head_dim"):
            A.check_align_limits(4, 10, 100, hd)
    with pytest.raises(ValueError, match="odd number"):
        A.check_align_limits(4, 10, 100, 64, 1500, 6)
    with pytest.raises(ValueError, match="median_filter_width 33"):
        A.check_align_limits(4, 10, 100, 64, 1500, 33)
    A.check_align_limits(32, 447, 1500, 128, 1500, 31)
    A.check_align_limits(1, 1, 1, 8, 1500, 1)
    with pytest.raises(ValueError, match="num_frames"):
        A.frames_of([3000, 3000], 3)
    assert A.frames_of(None, 2) == [1500, 1500] and A.frames_of(401, 2) == [200, 200] and A.frames_of([0, 1, 9000], 3) == [1, 1, 1500]
    # beams: refused by name before any device work
    from coral_amd.whisper import check_beam_arguments

    with pytest.raises(ValueError, match="return_token_timestamps=True is not implemented with beam search"):
        check_beam_arguments(1, 2, 1.0, False, dict(return_token_timestamps=True))


def test_evaluation_config_mode():
    from coral_amd.evaluate import _whisper_timestamp_mode

    assert _whisper_timestamp_mode("word") == "word"
    assert _whisper_timestamp_mode(True) is True and _whisper_timestamp_mode(False) is False
    assert _whisper_timestamp_mode(None) is False


def test_c_abi_has_the_two_entries():
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym in ("ca_whisper_align_cost", "ca_dtw_token_times"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
        code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % sym, code)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[sym][1]), sym
    for name, val in (("TOKENS", _lib.ALIGN_MAX_TOKENS), ("FRAMES", _lib.ALIGN_MAX_FRAMES), ("HEADS", _lib.ALIGN_MAX_HEADS),
                      ("HEAD_DIM", _lib.ALIGN_MAX_HEAD_DIM), ("FILTER_WIDTH", _lib.ALIGN_MAX_FILTER_WIDTH)):
        assert re.search(rf"#define CA_ALIGN_MAX_{name} {val}\b", hdr), name
    assert _lib.align_ws_bytes_per_clip(10, 448, 1500) == 10 * 1500 * 452 * 4
    assert callable(ops.whisper_align_cost) and callable(ops.dtw_token_times)
