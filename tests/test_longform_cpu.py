"""Host side of long-form wav2vec2 transcription (no GPU): `chunk_plan` / `frame_segments` against the chunk lists,
rescaled strides and stitched lengths the `transformers` ASR pipeline produced (tests/golden/w2v2_longform.*, written by
tools/gen_longform_goldens.py), word offsets and seconds against its recorded word chunks, the tokenizer cases against
the host restatements, and the C ABI additions."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import longform_ref as lref  # noqa: E402

from coral_amd import longform as lf  # noqa: E402


def _sl(s):
    sl = s["stride_length_s"]
    return tuple(sl) if isinstance(sl, list) else sl


def test_fixture_covers_the_settings_and_the_waveform_is_the_seeded_one():
    meta, z = lref.load_fixture()
    got = [(s["chunk_length_s"], _sl(s)) for s in meta["settings"]]
    assert got[:3] == [(2.0, None), (2.0, (0.5, 0.25)), (1.0, 0.3)] and len(got) >= 4
    # the edge setting: its last chunk is one alignment unit longer than left + right, chunk_iter's shortest
    e = meta["settings"][3]
    assert e["strides"][-1][0] == e["stride_left"] + e["stride_right"] + meta["align_to"]
    w = lref.fixture_waveform()
    assert len(w) == meta["n_samples"] == 100800 and w.dtype.name == "float32"
    assert [float(x) for x in w[:8]] == meta["wave_head"] and float(w.astype("float64").sum()) == meta["wave_sum"]
    for k, s in enumerate(meta["settings"]):
        assert z[f"logits_{k}"].shape == (len(s["strides"]), max(s["frames"]), 46)


@pytest.mark.parametrize("k", range(4))
def test_chunk_plan_and_frame_segments_reproduce_the_pipeline(k):
    meta, _ = lref.load_fixture()
    s = meta["settings"][k]
    plan = lf.chunk_plan(meta["n_samples"], s["chunk_length_s"], _sl(s), meta["sampling_rate"], meta["align_to"])
    assert (plan["chunk_len"], plan["stride_left"], plan["stride_right"]) == (s["chunk_len"], s["stride_left"],
                                                                            s["stride_right"])
    assert [c[0] for c in plan["chunks"]] == s["starts"]
    assert [list(c[1:]) for c in plan["chunks"]] == s["strides"]
    assert [list(lf.rescale_stride(*c[1:], meta["align_to"])) for c in plan["chunks"]] == s["rescaled"]
    assert [lf.conv_frames(c[1]) for c in plan["chunks"]] == s["frames"]
    seg, total = lf.frame_segments(plan, max(s["frames"]), meta["align_to"], row=3)
    assert total == s["stitched_len"]
    off = 0
    for (row, o, l, keep), (tn, rl, rr), T_b in zip(seg, s["rescaled"], s["frames"]):
        assert (row, o, l) == (3, off, rl) and keep == len(range(T_b)[rl:tn - rr])  # NumPy's slice clipping
        off += keep


def test_chunk_plan_edges():
    with pytest.raises(ValueError, match="stride_length_s"):
        lf.chunk_plan(100_000, 1.0, 0.5)  # step == 0
    with pytest.raises(ValueError, match="stride_length_s"):
        lf.chunk_plan(100_000, 1.0, (0.7, 0.5))  # step < 0
    with pytest.raises(ValueError, match="chunk_length_s"):
        lf.chunk_plan(100_000, 0)
    # default stride = chunk / 6 on both sides, each length rounded to the alignment
    p = lf.chunk_plan(100_000, 10.0)
    assert (p["chunk_len"], p["stride_left"], p["stride_right"], p["step"]) == (160000, 26560, 26560, 106880)
    assert p["chunks"] == [(0, 100000, 0, 0)]  # one chunk: first and last at once
    assert lf.chunk_plan(0, 1.0)["chunks"] == []
    # a recording that ends exactly with a chunk: that chunk is the last, nothing follows it
    p = lf.chunk_plan(32000 + 2 * 21120, 2.0)
    assert [c[0] for c in p["chunks"]] == [0, 21120, 42240] and p["chunks"][-1] == (42240, 32000, 5440, 0)
    # token_n is round(n / 320), one more than the conv stack's frames for a full 10 s chunk
    assert lf.rescale_stride(160000, 26560, 26560)[0] == 500 and lf.conv_frames(160000) == 499
    # the last chunk is cut short by its own frame count; a chunk too short for a frame keeps nothing
    seg, total = lf.frame_segments(dict(chunks=[(0, 32000, 0, 5440), (21120, 32000, 5440, 0), (42240, 300, 0, 0)]), 99)
    assert seg == [(0, 0, 0, 83), (0, 83, 17, 82), (0, 165, 0, 0)] and total == 165


def test_word_offsets_and_seconds_reproduce_the_recorded_word_chunks():
    meta, _ = lref.load_fixture()
    al, sr = meta["align_to"], meta["sampling_rate"]
    for s in meta["settings"]:
        # seconds -> frame offsets is exact here (offset * 320 / 16000 = offset / 50, offsets below 2^24)
        chars = [{"char": c["text"], "start_offset": round(c["timestamp"][0] * sr / al),
                  "end_offset": round(c["timestamp"][1] * sr / al)} for c in s["char_chunks"]]
        assert [list(c["timestamp"]) for c in lf.timestamp_chunks(chars, "char", al, sr)] == \
            [c["timestamp"] for c in s["char_chunks"]]
        words = lf.timestamp_chunks(lf.word_offsets(chars), "word", al, sr)
        assert [{"text": w["text"], "timestamp": list(w["timestamp"])} for w in words] == s["word_chunks"]


def test_tokenizer_cases_match_the_host_restatements():
    from coral_amd.processor import CTCTokenizer

    meta, _ = lref.load_fixture()
    tok = CTCTokenizer(meta["vocab"])
    blank = tok.pad_token_id
    cases = meta["tokenizer_cases"]
    assert len(cases) >= 36
    assert any(not c["char_offsets"] for c in cases) and any(len(c["word_offsets"]) > 2 for c in cases)
    for c in cases:
        for collapse in (lref.collapse_ref, lref.collapse_ref_fast):
            ids, start, end = collapse(c["ids"], len(c["ids"]), blank)
            offs = lf.char_offsets(ids, start, end, tok)
            assert [[o["char"], o["start_offset"], o["end_offset"]] for o in offs] == c["char_offsets"]
        assert [[o["word"], o["start_offset"], o["end_offset"]] for o in lf.word_offsets(offs)] == c["word_offsets"]
        assert tok.decode(ids, group_tokens=False) == c["text"]


def test_refusals_name_the_argument():
    with pytest.raises(ValueError, match="return_timestamps"):
        lf.check_timestamp_mode("words", False)
    with pytest.raises(ValueError, match="return_timestamps"):
        lf.check_timestamp_mode(True, False)
    with pytest.raises(ValueError, match="return_timestamps.*LM"):
        lf.check_timestamp_mode("word", True)
    lf.check_timestamp_mode(None, True)
    lf.check_timestamp_mode("char", False)


def test_c_abi_additions_and_config_keys():
    from coral_amd import _lib, ops
    from coral_amd.config import load_config

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    lib = _lib.load()
    for sym in ("ca_ctc_stitch", "ca_ctc_collapse_workspace_bytes", "ca_ctc_collapse_offsets"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    assert int(re.search(r"#define CA_CTC_COLLAPSE_TILE (\d+)", hdr).group(1)) == _lib.CTC_COLLAPSE_TILE
    for fn in ("ctc_stitch", "ctc_collapse_workspace_bytes", "ctc_collapse_offsets"):
        assert callable(getattr(ops, fn))
    # argument validation needs no GPU
    assert lib.ca_ctc_stitch(None, None, None, None, 1, 1, 1, 1, 1, 1, None) == -1
    assert b"ca_ctc_stitch" in lib.ca_last_error()
    assert lib.ca_ctc_collapse_offsets(None, None, None, None, None, None, None, 0, 1, 1, 0, None) == -1
    assert b"ca_ctc_collapse_offsets" in lib.ca_last_error()
    assert lib.ca_ctc_collapse_workspace_bytes(3, 1 << 24) >= 4 * 3 * 4096 * 4
    cfg = load_config("evaluation")
    assert cfg.get("chunk_length_s", None) == 0 and cfg.get("stride_length_s", 1) is None
