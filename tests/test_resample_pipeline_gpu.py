"""Audio at other sampling rates through the device input pipeline and its callers (coral_amd/resample.py in front of
ca_pcm_prepare): against the host featurisation of the float64-reference resampling (tests/resample_ref.py) where
numbers are compared, and bit for bit where both sides resample with the same kernel."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import longform_ref as lref  # noqa: E402
import resample_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = [48_000, 16_000, 44_100, 8_000]
LENGTHS = [43_201, 4_800, 66_150, 4_803]  # 0.9, 0.3, 1.5 and 0.6 s


def _batch(dtype, seed=1):
    rng = np.random.RandomState(seed)
    out = []
    for n in LENGTHS:
        x = np.clip(0.2 * rng.randn(n), -1, 1)
        out.append((x * 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32))
    return out


_REF: dict = {}


def _reference(dtype):
    """Per row (y float64, the resampling bound over the row's standard deviation), computed once."""
    name = np.dtype(dtype).name
    if name not in _REF:
        rows = []
        for x, r in zip(_batch(dtype), RATES):
            if r == 16_000:
                y = x.astype(np.float64) / (32768.0 if dtype == np.int16 else 1.0)
                rows.append((y, 0.0))
            else:
                y, A, K = rref.resample(x, r, 16_000, 32, 0.99, int16=dtype == np.int16)
                rows.append((y, float(rref.bound(A, K).max() / y.std())))
        _REF[name] = rows
    return _REF[name]


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
@pytest.mark.parametrize("padding", ["longest", "max_length"])
def test_wav2vec2_pipeline_mixed_rates_match_host_featurisation_of_the_reference(dtype, padding):
    from coral_amd.input_pipeline import DeviceInputPipeline
    from coral_amd.processor import WaveformFeatureExtractor

    fe = WaveformFeatureExtractor()
    pipe = DeviceInputPipeline(DEV, batch=4, max_samples=32_000, dtype=dtype, padding=padding, max_source_rate=48_000)
    assert pipe.host[0].shape == (4, 96_000)
    ref = _reference(dtype)
    want = fe.pad([fe(y) for y, _ in ref], padding=padding, max_length=32_000)
    pipe.submit(_batch(dtype), sampling_rate=RATES)
    got = pipe.get()
    torch.cuda.synchronize()
    assert got["sample_lengths"] == [len(y) for y, _ in ref] == [rref.out_length(n, r, 16_000) for n, r in zip(LENGTHS, RATES)]
    assert got["input_values"].shape == want["input_values"].shape
    assert np.array_equal(got["attention_mask"].cpu().numpy(), want["attention_mask"])
    diff = np.abs(got["input_values"].cpu().numpy() - want["input_values"]).max(axis=1)
    for i, (_, tol) in enumerate(ref):
        print(f"row {i} ({RATES[i]} Hz): max difference {diff[i]:.3e}, tolerance {3e-5 + tol:.3e}")
        assert diff[i] <= 3e-5 + tol


def test_long_clips_are_cut_at_the_source_length_of_max_samples():
    from coral_amd.input_pipeline import DeviceInputPipeline

    pipe = DeviceInputPipeline(DEV, batch=2, max_samples=2_000, dtype=np.float32, max_source_rate=48_000)
    x = _batch(np.float32)
    pipe.submit([x[0], x[2]], sampling_rate=[48_000, 44_100])
    got = pipe.get()
    assert got["sample_lengths"] == [2_000, 2_000] and got["input_values"].shape == (2, 2_000)
    y, A, K = rref.resample(x[2][:5512], 44_100, 16_000, 32, 0.99)  # floor(2000 * 441 / 160) source samples
    assert len(y) == 2_000
    want = (y - y.mean()) / np.sqrt(y.var() + 1e-7)
    assert np.abs(got["input_values"][1].cpu().numpy() - want).max() <= 3e-5 + float(rref.bound(A, K).max() / y.std())


def test_whisper_pipeline_equals_the_pipeline_fed_the_resampled_audio():
    from coral_amd import resample as rs
    from coral_amd.input_pipeline import DeviceInputPipeline
    from coral_amd.whisper import N_SAMPLES, WhisperEngine, WhisperShape

    eng = WhisperEngine(WhisperShape(d_model=64, encoder_layers=1, decoder_layers=1, encoder_attention_heads=4,
                                     decoder_attention_heads=4, encoder_ffn_dim=128, decoder_ffn_dim=128), DEV)
    audios = _batch(np.int16, seed=4)
    kw = dict(batch=4, max_samples=N_SAMPLES, kind="whisper", mel_filters=eng.mel_filters)
    pipe = DeviceInputPipeline(DEV, dtype=np.int16, max_source_rate=48_000, **kw)
    pipe.submit(audios, sampling_rate=48_000)
    got = pipe.get()["input_features"]
    # (the resampled audio is float32: the second pipeline stages float32 rows)
    plain = DeviceInputPipeline(DEV, dtype=np.float32, **kw)
    plain.submit(rs.resample(audios, 48_000, device=DEV))
    want = plain.get()["input_features"]
    torch.cuda.synchronize()
    assert got.shape == want.shape == (4, 80, 3000) and torch.equal(got, want)
    assert float(got.std()) > 0


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
def test_batches_at_the_target_rate_are_untouched_and_other_rates_need_max_source_rate(dtype):
    from coral_amd.input_pipeline import DeviceInputPipeline

    audios = _batch(dtype, seed=6)
    plain = DeviceInputPipeline(DEV, batch=4, max_samples=32_000, dtype=dtype)
    wide = DeviceInputPipeline(DEV, batch=4, max_samples=32_000, dtype=dtype, max_source_rate=48_000)
    plain.submit(audios)
    want = plain.get()
    for rate in (None, 16_000, [16_000] * 4, [None, 16_000, None, 16_000]):
        wide.submit(audios, sampling_rate=rate)
        got = wide.get()
        assert got["sample_lengths"] == want["sample_lengths"]
        assert torch.equal(got["input_values"], want["input_values"]) and torch.equal(got["attention_mask"], want["attention_mask"])
    plain.submit(audios, sampling_rate=16_000)  # naming the target rate is fine without max_source_rate
    assert torch.equal(plain.get()["input_values"], want["input_values"])
    with pytest.raises(ValueError, match="max_source_rate"):
        plain.submit(audios, sampling_rate=48_000)
    with pytest.raises(ValueError, match="max_source_rate"):
        plain.submit(audios, sampling_rate=[16_000, 16_000, 8_000, 16_000])
    with pytest.raises(ValueError, match="96000 Hz is above the pipeline's max_source_rate 48000"):
        wide.submit(audios, sampling_rate=[16_000, 96_000, 8_000, 16_000])
    with pytest.raises(ValueError, match="max_source_rate"):
        DeviceInputPipeline(DEV, batch=4, max_samples=32_000, max_source_rate=8_000)
    plain.submit(audios)  # a refused submit took no staging slot
    plain.submit(audios)


# ---- callers: both sides resample with the same kernel, so the comparison is exact ---------------------------------
@pytest.fixture(scope="module")
def tiny():
    from coral_amd.modeling import Wav2Vec2ForCTC
    from coral_amd.processor import CTCTokenizer, Wav2Vec2Processor, WaveformFeatureExtractor

    model = Wav2Vec2ForCTC.from_pretrained(str(lref.GOLDEN / "hf_ckpt_w2v2")).eval()
    proc = Wav2Vec2Processor(WaveformFeatureExtractor(), CTCTokenizer(lref.load_fixture()[0]["vocab"]))
    return model, proc


def test_transcribe_and_align_with_a_sampling_rate(tiny):
    from coral_amd import ctc_align as ca
    from coral_amd import resample as rs
    from coral_amd.evaluate import transcribe

    model, proc = tiny
    wave = lref.fixture_waveform()
    waves, rates = [wave, wave[:60_000], wave[:30_000]], [8_000, 48_000, 16_000]  # 12.6 s, 1.25 s and 1.9 s at 16 kHz
    at16 = rs.resample(waves, rates, device=DEV)
    assert [len(a) for a in at16] == [201_600, 20_000, 30_000] and np.array_equal(at16[2], waves[2])
    assert transcribe(model, proc, waves, sampling_rate=rates) == transcribe(model, proc, at16)
    got = transcribe(model, proc, waves, 3, chunk_length_s=2.0, return_timestamps="word", sampling_rate=rates)
    want = transcribe(model, proc, at16, 3, chunk_length_s=2.0, return_timestamps="word")
    assert got == want and got[0]["chunks"]
    assert max(c["timestamp"][1] for c in got[0]["chunks"]) > 6.3  # seconds of the resampled recording, not of the source
    one = transcribe(model, proc, waves[:1], sampling_rate=8_000)  # one rate for all
    assert one == transcribe(model, proc, at16[:1])
    assert transcribe(model, proc, waves, sampling_rate=16_000) == transcribe(model, proc, waves)
    texts = [t or "ab" for t in transcribe(model, proc, at16)]
    got = ca.align(model, proc, waves, texts, sampling_rate=rates)
    assert got == ca.align(model, proc, at16, texts) and all(r["chunks"] for r in got)
    with pytest.raises(ValueError, match="3 sampling rates for 1"):
        transcribe(model, proc, waves[:1], sampling_rate=rates)


def test_transcribe_whisper_with_a_sampling_rate():
    import whisper_ts_ref as R
    from coral_amd import resample as rs
    from coral_amd.evaluate import transcribe_whisper
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_setup import WhisperFeatureExtractorGPU, WhisperForConditionalGeneration, WhisperProcessor

    model = WhisperForConditionalGeneration(WhisperShape(**R.CONFIG), device=DEV).eval()
    model.engine.load_state_dict(R.fixture_params())
    model.engine.refresh_derived()
    model.generation_config = dict(no_timestamps_token_id=R.NO_TIMESTAMPS, lang_to_id={"<|da|>": R.LANG},
                                   task_to_id={"transcribe": R.TRANSCRIBE, "translate": R.TRANSLATE},
                                   max_initial_timestamp_index=R.MAX_INITIAL_TIMESTAMP_INDEX)
    proc = WhisperProcessor(WhisperFeatureExtractorGPU(model.engine))
    waves, rates = R.short_waves()[:2], [8_000, 48_000]  # 8 s and 3.8 s at 16 kHz
    at16 = rs.resample(waves, rates, device=DEV)
    got = transcribe_whisper(model, proc, waves, batch_size=2, max_length=R.MAX_LENGTH, sampling_rate=rates)
    want = transcribe_whisper(model, proc, at16, batch_size=2, max_length=R.MAX_LENGTH)
    assert got == want and all(len(r) >= 4 for r in got[1])
    timed = transcribe_whisper(model, proc, waves, batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True,
                               sampling_rate=rates)
    assert timed == transcribe_whisper(model, proc, at16, batch_size=2, max_length=R.MAX_LENGTH, return_timestamps=True)


def test_evaluate_reads_a_sampling_rate_per_example(tmp_path, monkeypatch):
    import shutil

    from coral_amd import resample as rs
    from coral_amd.config import load_config
    from coral_amd.evaluate import evaluate
    from coral_amd.processor import dump_vocabulary

    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "ckpt"
    shutil.copytree(lref.GOLDEN / "engine_ckpt_w2v2", mdir)
    dump_vocabulary(load_config("evaluation").characters_to_keep, mdir)
    rng = np.random.RandomState(15)
    texts, rates = ["hej med dig", "det er en god dag", "å", "jeg hedder anna"], [48_000, 16_000, 8_000, 44_100]
    waves = [(0.1 * rng.randn(int(r * s))).astype(np.float32) for r, s in zip(rates, (1.0, 1.5, 0.8, 1.2))]
    config = load_config("evaluation", [f"model_id={mdir}", "batch_size=4", "dataset=synthetic", "store_results=false"])
    got = evaluate(config, [dict(audio=w, text=t, sampling_rate=r) for w, t, r in zip(waves, texts, rates)])
    # (the example at the target rate may leave its rate out)
    same = evaluate(config, [dict(audio=w, text=t, **({} if r == 16_000 else {"sampling_rate": r}))
                             for w, t, r in zip(waves, texts, rates)])
    want = evaluate(config, [dict(audio=w, text=t) for w, t in zip(rs.resample(waves, rates, device=DEV), texts)])
    assert got == want == same and got["n"] == 4


def test_npz_shards_keep_their_sampling_rate(tmp_path):
    from coral_amd import resample as rs
    from coral_amd.data import _npz_examples
    from coral_amd.processor import CTCTokenizer, Wav2Vec2Processor, WaveformFeatureExtractor

    proc = Wav2Vec2Processor(WaveformFeatureExtractor(), CTCTokenizer(lref.load_fixture()[0]["vocab"]))
    rng = np.random.RandomState(2)
    a, b = (0.1 * rng.randn(9_000)).astype(np.float32), (0.1 * rng.randn(7_000)).astype(np.float32)
    np.savez(tmp_path / "0.npz", audio=a, text="ab", sampling_rate=48_000)
    np.savez(tmp_path / "1.npz", audio=b, text="ba")
    raw = list(_npz_examples(tmp_path, proc, "text", 16_000, raw=True))
    assert [e["audio"]["sampling_rate"] for e in raw] == [48_000, 16_000] and np.array_equal(raw[0]["audio"]["array"], a)
    host = list(_npz_examples(tmp_path, proc, "text", 16_000, raw=False))
    want = proc(rs.resample([a], 48_000, device=DEV)[0], sampling_rate=16_000)["input_values"]
    assert np.array_equal(host[0]["input_values"], want) and len(want) == 3_000
    assert np.array_equal(host[1]["input_values"], proc(b, sampling_rate=16_000)["input_values"])
    assert raw[0]["labels"] == host[0]["labels"]


def _two_losses(tmp_path, monkeypatch, examples, extra):
    from coral_amd import modeling
    from coral_amd.config import load_config
    from coral_amd.data import ExampleStream
    from coral_amd.model_setup import load_model_setup

    monkeypatch.setitem(modeling.HUB_SHAPES, "facebook/wav2vec2-xls-r-300m",
                        dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=4))
    config = load_config("asr_finetuning", ["model=test-wav2vec2", "datasets=synthetic", f"models_dir={tmp_path}",
                                            "model_id=t", "max_steps=2", "total_batch_size=2", "per_device_batch_size=2",
                                            "max_seconds_per_example=2.0", "min_seconds_per_example=0.5", "logging_steps=1",
                                            "eval_steps=100", "augment_audio=false", *extra])
    np.random.seed(0)
    torch.manual_seed(0)
    setup = load_model_setup(config)
    processor = setup.load_processor()
    model = setup.load_model()
    trainer = setup.load_trainer_class()(model=model, data_collator=setup.load_data_collator(),
                                         args=setup.load_training_arguments(), compute_metrics=setup.load_compute_metrics(),
                                         train_dataset=ExampleStream(lambda: iter(examples)), eval_dataset=[],
                                         processing_class=processor.tokenizer)
    trainer._it = iter(trainer.train_dataset)
    losses = []
    for _ in range(2):
        losses.append(float(trainer.train_step([trainer.next_micro_batch()])))
    trainer.finish()
    torch.cuda.synchronize()
    assert trainer.pipeline_batches == 2
    return losses


def test_trainer_resamples_raw_examples_and_refuses_them_without_the_key(tmp_path, monkeypatch):
    from coral_amd import resample as rs

    rng = np.random.RandomState(3)
    waves = [np.clip(0.1 * rng.randn(n), -1, 1).astype(np.float32) for n in (30_000, 41_111, 52_345, 24_001, 36_000, 47_999)]
    labels = [[5, 6, 7], [8, 9], [10, 11, 12, 13], [6], [7, 8, 9], [12, 5]]
    at48 = [dict(audio=dict(array=w, sampling_rate=48_000), labels=l) for w, l in zip(waves, labels)]
    at16 = [dict(audio=dict(array=w), labels=l) for w, l in zip(rs.resample(waves, 48_000, device=DEV), labels)]  # no rate: the model's
    got = _two_losses(tmp_path / "a", monkeypatch, at48, ["max_source_sampling_rate=48000"])
    want = _two_losses(tmp_path / "b", monkeypatch, at16, [])
    print("losses", got, want)
    assert got == want and all(np.isfinite(got)) and got[0] != got[1]
    with pytest.raises(ValueError, match="max_source_rate"):
        _two_losses(tmp_path / "c", monkeypatch, at48, [])
