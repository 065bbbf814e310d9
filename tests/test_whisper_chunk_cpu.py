"""Chunked Whisper long-form decoding, the parts that need no GPU: the restatement (tests/whisper_chunk_ref.py) against
what transformers' own `_find_longest_common_sequence`, `_decode_asr` and `chunk_iter` gave
(tests/golden/whisper_chunk.npz, tools/gen_whisper_chunk_goldens.py), the library's host state machine against the
same goldens, and the argument checks that run before any device work."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_chunk_ref as C  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def test_the_restated_merge_equals_transformers(golden):
    cut = 0
    for case in golden["merge"]:
        merged, cuts, wins = C.merge_sequences(case["seqs"])
        assert merged == case["merged"], case["seqs"]
        assert len(cuts) == len(case["seqs"]) - 1
        # the cuts, through where every kept token comes from (transformers returns that, not the indices)
        assert [list(o) for o in C.origins(case["seqs"], cuts)] == case["origins"], (case["seqs"], cuts)
        cut += sum(1 for w in wins if w is not None)
    assert cut >= 40, "the goldens must hold accepted diagonals"


def test_the_restated_state_machine_equals_transformers(golden):
    timed = open_ended = merged_runs = 0
    for case in golden["asr"]:
        got = C.transcript(case["outputs"], C.stand_in_decode)
        assert got["text"] == case["text"]
        if not case["timestamps"]:
            assert len(got["chunks"]) <= 1 and all(c["timestamp"] == (None, None) for c in got["chunks"])
            continue
        assert [dict(text=c["text"], timestamp=list(c["timestamp"])) for c in got["chunks"]] == case["chunks"]
        timed += len(case["chunks"])
        open_ended += bool(case["chunks"]) and case["chunks"][-1]["timestamp"][1] is None
        merged_runs += sum(1 for seg in C.segments_of(case["outputs"]) if len(seg["runs"]) > 1)
    assert timed > 100 and open_ended >= 3 and merged_runs >= 10, (timed, open_ended, merged_runs)


def test_the_library_state_machine_equals_transformers(golden):
    """`plan_segments` is what `transcribe_chunked` runs on the host; the text of a segment is the merge of its runs."""
    from coral_amd.chunked_whisper import plan_segments

    for case in golden["asr"]:
        segs = plan_segments(case["outputs"], C.TIMESTAMP_BEGIN, C.SPECIAL_IDS, C.TIME_PRECISION)
        assert segs == C.segments_of(case["outputs"])
        texts = [C.stand_in_decode(C.merge_sequences(s["runs"])[0]) for s in segs]
        assert "".join(texts) == case["text"]
        if case["timestamps"]:
            assert [dict(text=t, timestamp=[s["start"], s["end"]]) for t, s in zip(texts, segs)] == case["chunks"]


def test_a_decreasing_timestamp_inside_one_chunk_raises():
    from coral_amd.chunked_whisper import plan_segments

    tb = C.TIMESTAMP_BEGIN
    outs = [dict(tokens=[C.SOT, tb + 100, 1, 2, tb + 200, tb + 50, 3, tb + 80, C.EOS], stride=(30.0, 0.0, 0.0))]
    with pytest.raises(ValueError, match="timestamp"):
        plan_segments(outs, tb, C.SPECIAL_IDS)
    with pytest.raises(ValueError, match="timestamp"):
        C.segments_of(outs)


def test_chunk_plan_gives_the_pipelines_strides(golden):
    from coral_amd.longform import chunk_plan

    short_last = 0
    for case in golden["strides"]:
        plan = chunk_plan(case["n"], case["chunk_length_s"], case["stride_length_s"], C.SAMPLING_RATE, align_to=1)
        assert [list(c[1:]) for c in plan["chunks"]] == case["strides"], case["n"]
        assert [c[0] for c in plan["chunks"]] == [i * plan["step"] for i in range(len(plan["chunks"]))]
        short_last += len(case["strides"]) > 1 and case["strides"][-1][0] < case["strides"][0][0]
    assert short_last >= 3
    # the default stride is a sixth of the chunk each side, in whole samples
    plan = chunk_plan(70 * 16000, 30.0, None, 16000, align_to=1)
    assert (plan["chunk_len"], plan["stride_left"], plan["stride_right"], plan["step"]) == (480000, 80000, 80000, 320000)


class _Boom:
    """A model and processor that fail on any use: the checks below must raise before they are touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device work before the argument checks ({name})")


@pytest.mark.parametrize("kw,word", [
    (dict(return_timestamps="word"), "word"),
    (dict(temperature=(0.0, 0.2)), "temperature"),
    (dict(logprob_threshold=-1.0), "logprob_threshold"),
    (dict(compression_ratio_threshold=1.35), "compression_ratio_threshold"),
    (dict(no_speech_threshold=0.6), "no_speech_threshold"),
    (dict(prompt_ids=[62, 1, 2]), "prompt_ids"),
    (dict(prompt="Aarhus"), "prompt"),
    (dict(condition_on_prev_tokens=True), "condition_on_prev_tokens"),
    (dict(prompt_condition_type="all-segments"), "prompt_condition_type"),
    (dict(num_beams=2, return_timestamps=True), "num_beams"),
    (dict(chunk_length_s=30.5), "chunk_length_s"),
    (dict(chunk_length_s=-1.0), "chunk_length_s"),
])
def test_what_chunked_decoding_refuses_by_name(kw, word):
    from coral_amd.chunked_whisper import transcribe_chunked
    from coral_amd.evaluate import transcribe_whisper

    wave = [np.zeros(16000, dtype=np.float32)]
    with pytest.raises(ValueError, match=word):
        transcribe_chunked(_Boom(), _Boom(), wave, **kw)
    with pytest.raises(ValueError, match=word):
        transcribe_whisper(_Boom(), _Boom(), wave, long_form="chunked", **kw)


def test_neutral_values_of_the_refused_keys_pass_the_checks():
    from coral_amd.chunked_whisper import check_chunked_arguments

    check_chunked_arguments(30.0, 1, False, dict(temperature=None, logprob_threshold=None, prompt_ids=None,
                                                 condition_on_prev_tokens=False, prompt_condition_type=None))
    check_chunked_arguments(12.5, 4, False, dict(temperature=0.0))
    check_chunked_arguments(30.0, 1, True, {})
    with pytest.raises(TypeError, match="beam_width"):
        check_chunked_arguments(30.0, 1, True, dict(beam_width=3))


def test_sequential_still_refuses_chunk_length_and_chunked_is_a_config_key(tmp_path):
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate, transcribe_whisper

    (tmp_path / "config.json").write_text(json.dumps(dict(architectures=["WhisperForConditionalGeneration"], model_type="whisper")))
    cfg = load_config("evaluation", [f"model_id={tmp_path}", "chunk_length_s=10"])
    assert cfg.get("whisper_long_form", None) == "sequential"
    with pytest.raises(ValueError, match="without it") as e:
        evaluate(cfg)
    assert "chunk_length_s" in str(e.value) and "whisper_long_form: chunked" in str(e.value)
    with pytest.raises(ValueError, match="without it"):
        transcribe_whisper(_Boom(), _Boom(), [np.zeros(16000, dtype=np.float32)], chunk_length_s=10.0)
    with pytest.raises(ValueError, match="whisper_long_form"):
        evaluate(load_config("evaluation", [f"model_id={tmp_path}", "whisper_long_form=overlapped"]))
    with pytest.raises(ValueError, match="long_form"):
        transcribe_whisper(_Boom(), _Boom(), [], long_form="overlapped")
    # chunked + a chunk above 30 s: refused before the model is loaded (the directory holds no weights)
    with pytest.raises(ValueError, match="chunk_length_s"):
        evaluate(load_config("evaluation", [f"model_id={tmp_path}", "whisper_long_form=chunked", "chunk_length_s=45"]))


def test_the_equal_score_pair_of_the_gpu_test_is_equal_in_float64():
    """Diagonals 100 and 200 with two matches each: 2/100 + 100/10000 and 2/200 + 200/10000 are the same two float64
    numbers added in the other order, so the scores are equal bit for bit and the earlier diagonal wins."""
    left, right = C.equal_score_pair()
    m1, s1, _ = C.diagonal(left, right, 100)
    m2, s2, _ = C.diagonal(left, right, 200)
    assert (m1, m2) == (2, 2) and s1 == s2
    assert all(C.diagonal(left, right, i)[0] <= 1 for i in range(1, len(left) + len(right)) if i not in (100, 200))
    assert C.best_diagonal(left, right)[0] == 100

