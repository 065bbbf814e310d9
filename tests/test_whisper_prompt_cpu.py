"""Previous-text conditioning and prompts of the Whisper long-form loop against transformers' own runs
(tests/golden/whisper_prompt.npz, written by tools/gen_whisper_prompt_goldens.py; fixture and reference decoder in
tests/whisper_prompt_ref.py).  No GPU: the decoder inputs the restated loop prepares, the fp32 restated masked decoder,
the loop itself replaying the recorded windows, and the argument checks."""
import json

import numpy as np
import pytest
import torch

import whisper_prompt_ref as PR
import whisper_ts_ref as R
from coral_amd.longform_whisper import (FallbackPolicy, PromptPolicy, grown_max_length, prepare_decoder_inputs, run_longform)

V = R.CONFIG["vocab_size"]


@pytest.fixture(scope="module")
def z():
    return PR.load_golden()


@pytest.fixture(scope="module")
def model():
    return PR.fixture_params(), PR.fixture_config(), PR.features()


def _fallback(z):
    return FallbackPolicy(PR.FALLBACK_TEMPERATURES, float(z["fallback_logprob_threshold"]), None, None, None, 0)


def _replay(z, run, batch_size=None):
    """run_longform(conditioning=...) fed with the recorded attempts -> (result, the decoder inputs it handed out)."""
    atts = PR.rounds_of(z, run)
    it = iter(atts)
    handed = []

    def rows_of(batch, inputs):
        att = next(it)
        assert list(batch) == att["batch"]
        handed.append((att, inputs))
        return [inputs["rows"][i] + ids for i, ids in enumerate(att["ids"])], att

    def plain(batch, inputs):
        return rows_of(batch, inputs)[0]

    def scored(batch, temperature, uniforms, inputs):
        rows, att = rows_of(batch, inputs)
        assert temperature == att["T"] and (uniforms is None) == (temperature == 0)
        return rows, dict(sum_logprob=(att["avg_logprob"] * att["n_scored"]).tolist(), n_scored=att["n_scored"].tolist(),
                          no_speech_prob=None)

    fb = _fallback(z) if run == "fallback" else None
    out = run_longform(scored if fb else plain, z["frames"].tolist(), R.TIMESTAMP_BEGIN, len(R.PREFIX), R.EOS, R.EOS,
                       fallback=fb, vocab_size=V, max_length=R.MAX_LENGTH, conditioning=PR.policy_of(run),
                       init_tokens=R.PREFIX, max_target_positions=PR.MAX_TARGET_POSITIONS, batch_size=batch_size)
    assert next(it, None) is None, "the restated loop asked for fewer attempts than transformers ran"
    return out, handed


def test_golden_holds_every_branch(z):
    assert set(json.loads(str(z["branches"]))) >= set(PR.BRANCHES)
    ok, other = z["position_check"]
    assert ok <= 1e-5 and other > 1e-3  # positions count the padding: the other reading misses transformers' logits


@pytest.mark.parametrize("run", list(PR.RUNS))
def test_decoder_inputs_and_loop_reproduce_transformers(z, run):
    out, handed = _replay(z, run)
    two_pads = cut = False
    for att, inputs in handed:
        assert inputs["rows"] == att["rows"].tolist(), (run, att["round"], att["attempt"])
        assert inputs["masked"] == att["masked"] and inputs["max_length"] == att["max_length"]
        assert inputs["no_speech_index"] == att["rows"].shape[1] - len(R.PREFIX)
        if att["masked"]:
            assert inputs["start"] == att["start"].tolist()
            mask = np.arange(att["rows"].shape[1])[None, :] >= np.asarray(inputs["start"])[:, None]
            assert (mask == att["mask"]).all(), "the padding is one left run: the mask by value is the mask by count"
            two_pads |= len({s for s in inputs["start"] if s > 0}) >= 2
            cut |= any(s == 0 and att["rows"].shape[1] - len(R.PREFIX) >= PR.CUT_OFF + 1 for s in inputs["start"])
        else:
            assert inputs["start"] == [0] * len(att["batch"])
    if run == "fallback":
        assert two_pads and cut
    for b in range(len(z["frames"])):
        n = z[f"{run}_clip{b}_seg_len"]
        toks = [z[f"{run}_clip{b}_seg_ids"][i, :int(k)].tolist() for i, k in enumerate(n)]
        assert [s[2] for s in out[b]["segments"]] == toks
        assert [s[0] for s in out[b]["segments"]] == z[f"{run}_clip{b}_seg_start"].tolist()
        assert [s[1] for s in out[b]["segments"]] == z[f"{run}_clip{b}_seg_end"].tolist()
        seeks = [k[1] for a in PR.rounds_of(z, run) if a["attempt"] == 0 for k in a["batch"] if k[0] == b]
        assert [w[0] for w in out[b]["windows"]] == seeks
        # transformers' final sequences: the segments' tokens, right-padded (a first-segment prompt dropped)
        flat = [t for s in out[b]["segments"] for t in s[2]]
        want = z[f"{run}_sequences"][b]
        assert want[:len(flat)].tolist() == flat and (want[len(flat):] == R.EOS).all()


def test_rounds_are_padded_alike_however_they_are_cut_into_calls(z):
    """batch_size = 1: every call gets its rows of the ROUND's inputs - the same rows, the same padding."""
    atts = [a for a in PR.rounds_of(z, "prev")]
    it = iter([(a, j) for a in atts for j in range(len(a["batch"]))])

    def one(batch, inputs):
        att, j = next(it)
        assert list(batch) == [att["batch"][j]] and inputs["rows"] == [att["rows"][j].tolist()]
        assert inputs["start"] == [int(att["start"][j])] or not att["masked"]
        return [inputs["rows"][0] + att["ids"][j]]

    out = run_longform(one, z["frames"].tolist(), R.TIMESTAMP_BEGIN, len(R.PREFIX), R.EOS, R.EOS, max_length=R.MAX_LENGTH,
                       conditioning=PR.policy_of("prev"), init_tokens=R.PREFIX, max_target_positions=PR.MAX_TARGET_POSITIONS,
                       batch_size=1)
    assert out == _replay(z, "prev")[0]


def test_restated_masked_decoder_reproduces_the_first_step_logits_and_the_ids(z, model):
    from oracle import whisper_ref as w

    params, cfg, mels = model
    checked = greedy = 0
    for run in PR.RUNS:
        for att in PR.rounds_of(z, run):
            if att["logits"] is None:
                continue
            enc = w.encoder(PR.window_batch(mels, att["batch"]), params, cfg)
            ids, mask = torch.from_numpy(att["rows"]), torch.from_numpy(att["mask"] if att["masked"] else np.ones_like(att["mask"]))
            with torch.no_grad():
                lg = PR.masked_decoder(ids, mask, enc, params, cfg)[:, -1].numpy()
            assert np.abs(lg - att["logits"]).max() <= 1e-5, (run, att["round"])
            checked += len(att["batch"])
            if att["T"] == 0 and run in ("prev", "fallback") and att["round"] == 1:
                with torch.no_grad():
                    gen = PR.greedy_rows(ids, mask, enc, params, cfg, att["max_length"])
                assert gen == att["ids"], (run, att["round"])
                greedy += len(gen)
    assert checked >= 30 and greedy >= 6


def test_loose_arguments_stay_refused_and_name_the_policy():
    for kw in (dict(condition_on_prev_tokens=True), dict(prompt_ids=[1, 2]), dict(prompt_condition_type="all-segments")):
        with pytest.raises(ValueError, match=r"conditioning=PromptPolicy"):
            run_longform(lambda b: [], [10], R.TIMESTAMP_BEGIN, 3, R.EOS, R.EOS, **kw)
    with pytest.raises(ValueError, match="needs init_tokens"):
        run_longform(lambda b, i: [], [10], R.TIMESTAMP_BEGIN, 3, R.EOS, R.EOS, conditioning=PromptPolicy(condition_on_prev_tokens=True))
    with pytest.raises(ValueError, match="return_token_timestamps"):
        run_longform(lambda b, i: [], [10], R.TIMESTAMP_BEGIN, 3, R.EOS, R.EOS, return_token_timestamps=True, init_tokens=R.PREFIX,
                     max_target_positions=64, max_length=64, conditioning=PromptPolicy(condition_on_prev_tokens=True))


def test_prompt_policy_checks():
    assert PromptPolicy().prompt_condition_type == "first-segment" and not PromptPolicy().active
    assert PromptPolicy(prompt_ids=[5, 6]).prompt_ids == (5, 6) and PromptPolicy(prompt_ids=[5]).active
    with pytest.raises(ValueError, match="does not exist"):
        PromptPolicy(prompt_condition_type="every-segment")
    with pytest.raises(ValueError, match="needs condition_on_prev_tokens=True"):
        PromptPolicy(prompt_ids=[5, 6], prompt_condition_type="all-segments")
    with pytest.raises(ValueError, match="True or False"):
        PromptPolicy(condition_on_prev_tokens=None)
    with pytest.raises(ValueError, match="non-empty"):
        PromptPolicy(prompt_ids=[])
    # <|startofprev|>: the configured id, else suppress_tokens[-2], else none
    assert PromptPolicy(prev_sot_token_id=55).prev_sot([1, 2, 3]) == 55
    assert PromptPolicy().prev_sot([1, 2, 3]) == 2 and PromptPolicy().prev_sot([1]) is None and PromptPolicy().prev_sot() is None
    # a first-segment prompt seeds every clip, without its leading <|startofprev|> where that id is configured
    assert PromptPolicy(prompt_ids=[55, 7, 8], prev_sot_token_id=55).first_segments(2) == [[[7, 8]], [[7, 8]]]
    assert PromptPolicy(prompt_ids=[55, 7, 8]).first_segments(1, suppress_tokens=[55, 9]) == [[[55, 7, 8]]]
    assert PromptPolicy(prompt_ids=[55, 7], condition_on_prev_tokens=True, prompt_condition_type="all-segments").first_segments(1) == [[]]


def test_decoder_input_details():
    pol = PromptPolicy(condition_on_prev_tokens=True, prev_sot_token_id=55)
    tb = 64
    # a segment ending in two timestamps gives its text and the first of them; the cut-off keeps the LAST tokens
    segs = [[[64, 1, 2, 70, 70]], [[64, 3, 80]], []]
    rows, start, masked = prepare_decoder_inputs([51, 52], segs, [0, 1, 2], [True, True, True], pol, 50, 12, tb)
    assert masked and rows == [[55, 64, 1, 2, 70, 51, 52], [50, 55, 64, 3, 80, 51, 52], [50, 50, 50, 50, 55, 51, 52]]
    assert start == [0, 1, 4]
    rows, start, _ = prepare_decoder_inputs([51], [[[64, 1, 2, 3, 4, 5, 6, 70]]], [0], [True], pol, 50, 8, tb)
    assert rows == [[55, 5, 6, 70, 51]] and start == [0]  # cut-off 8 // 2 - 1 = 3
    # the branch looks at clip 0's segments whoever is in the batch; a row whose flag is off gets <|startofprev|> alone
    rows, start, masked = prepare_decoder_inputs([51], [[], [[64, 3, 80]]], [1], [True, True], pol, 50, 12, tb)
    assert not masked and rows == [[51]]
    rows, start, masked = prepare_decoder_inputs([51], segs, [0, 1], [True, False], pol, 50, 12, tb)
    assert masked and rows == [[55, 64, 1, 2, 70, 51], [50, 50, 50, 50, 55, 51]] and start == [0, 4]
    # every row unconditioned while a flag further back is still set: the rows are cut to nothing
    rows, start, masked = prepare_decoder_inputs([51], segs, [0], [False, True, True], pol, 50, 12, tb)
    assert masked and rows == [[51]] and start == [0]
    # max_length grows round by round, up to the target positions
    assert grown_max_length(64, 3, 128) == 67 and grown_max_length(67, 67, 128) == 128 and grown_max_length(72, 8, 128) == 80
    assert grown_max_length(64, 40, 128, max_new_tokens=20) == 64
    with pytest.raises(ValueError, match="exceed"):
        grown_max_length(64, 120, 128, max_new_tokens=20)
