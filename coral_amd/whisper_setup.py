"""`WhisperModelSetup` — mirror of R/src/coral/whisper.py:30-267 over `WhisperEngine`.

The byte-level BPE vocabulary of Whisper ships with the checkpoints on the HuggingFace hub, which
is unreachable here, so `load_processor` builds the feature-extraction half (GPU log-mel) and loads
the tokenizer files only from a local model directory (`tokenizers` library, `tokenizer.json`);
token-id level training / evaluation (`labels` already encoded) works without it."""

from __future__ import annotations

import json
import logging
import os
from pathlib import Path

import numpy as np
import torch

from .model_setup import ModelSetup, PreTrainedModelData, _training_args
from .coral_trainer import CoralTrainer
from . import specaugment
from .autograd import attach_backward
from .whisper import CORAL_WHISPER_SHAPES, HOP, N_SAMPLES, WhisperEngine, WhisperShape, sinusoid_positions
from .whisper_train import WhisperTrainEngine

logger = logging.getLogger(__package__)

HUB_SHAPES = {"openai/whisper-tiny": "whisper-xxsmall", "openai/whisper-base": "whisper-xsmall",
              "openai/whisper-small": "whisper-small", "openai/whisper-medium": "whisper-medium",
              "openai/whisper-large-v3": "whisper-large", "openai/whisper-large-v3-turbo": "whisper-large-turbo"}

# <|startoftranscript|><|da|><|transcribe|><|notimestamps|> in the multilingual vocabulary
# (language="danish", task="transcribe": R/src/coral/evaluate.py:59, R/src/coral/whisper.py:51-55)
DANISH_TRANSCRIBE_PREFIX = [50258, 50285, 50359, 50363]
DANISH_TRANSCRIBE_PREFIX_V3 = [50258, 50285, 50360, 50364]  # large-v3 vocabulary (51866 entries)


# generation_config.json of the openai/whisper-* checkpoints
HUB_MAX_INITIAL_TIMESTAMP_INDEX = 50


def prefix_ids(shape: WhisperShape):
    return DANISH_TRANSCRIBE_PREFIX_V3 if shape.vocab_size == 51866 else DANISH_TRANSCRIBE_PREFIX


class WhisperFeatureExtractorGPU:
    """pad/truncate to 30 s on the host, log-mel on the GPU (ca_logmel)."""

    def __init__(self, engine: WhisperEngine, sampling_rate: int = 16_000):
        self.engine = engine
        self.sampling_rate = sampling_rate

    def __call__(self, audios, sampling_rate: int | None = None) -> torch.Tensor:
        if sampling_rate is not None and sampling_rate != self.sampling_rate:
            raise ValueError(f"expected {self.sampling_rate} Hz audio, got {sampling_rate}")
        if isinstance(audios, np.ndarray) and audios.ndim == 1:
            audios = [audios]
        batch = np.zeros((len(audios), N_SAMPLES), dtype=np.float32)
        for i, a in enumerate(audios):
            a = np.asarray(a, dtype=np.float32)[:N_SAMPLES]
            batch[i, : len(a)] = a
        return self.engine.log_mel(torch.from_numpy(batch))

    def whole(self, audio) -> torch.Tensor:
        """One recording of any length -> log-mel [mels, frames] on the GPU, not cut to 30 s: what the transformers
        extractor gives with truncation=False (the clamp max(x, max - 8) takes the recording's maximum, not a window's).
        ca_logmel takes any whole number of hops (frames = N / 160, reflect padding at the true ends, one maximum per
        row).  Deviation for a length that is no multiple of 160: the trailing part-hop (< 10 ms) is cut BEFORE the
        transform.  The frame count is the extractor's (len // 160), but the extractor reflect-pads at the true last
        sample, so the last two frames (whose 400-sample windows reach past the cut) differ slightly from its values;
        for whole-hop lengths (every pinned fixture) the two agree to the log-mel tolerance."""
        a = np.asarray(audio, dtype=np.float32)
        n = max(len(a) // HOP, 3) * HOP
        buf = np.zeros(n, dtype=np.float32)
        buf[:min(n, len(a))] = a[:n]
        return self.engine.log_mel(torch.from_numpy(buf[None]))[0]


class WhisperProcessor:
    def __init__(self, feature_extractor, tokenizer=None):
        self.feature_extractor = feature_extractor
        self.tokenizer = tokenizer

    def batch_decode(self, ids, skip_special_tokens=True):
        if self.tokenizer is None:
            # no byte-level BPE files offline: render every text token as the word "t<id>", so WER on
            # the rendered strings is the token error rate (special tokens >= 50257 are skipped)
            return [" ".join(f"t{int(i)}" for i in r if not (skip_special_tokens and int(i) >= 50257)) for r in ids]
        return self.tokenizer.decode_batch([list(map(int, r)) for r in ids], skip_special_tokens=skip_special_tokens)

    def save_pretrained(self, model_dir):
        model_dir = Path(model_dir)
        model_dir.mkdir(parents=True, exist_ok=True)
        s = self.feature_extractor.engine.s
        (model_dir / "preprocessor_config.json").write_text(json.dumps(dict(
            feature_extractor_type="WhisperFeatureExtractor", feature_size=s.num_mel_bins, sampling_rate=self.feature_extractor.sampling_rate,
            hop_length=160, chunk_length=30, n_fft=400, padding_value=0.0, return_attention_mask=False), indent=2))
        if self.tokenizer is not None:
            self.tokenizer.save(str(model_dir / "tokenizer.json"))


class WhisperForConditionalGeneration:
    """HF-shaped wrapper: `model(input_features, labels)` and `model.generate(...)`.

    In training mode the call draws SpecAugment masks on the input features
    ($TF/models/whisper/modeling_whisper.py:821-862: time spans over the 3000 frames, then feature
    spans over the mel bins, zero fill) and LayerDrop decisions (:626-634, :771-779) on the host, in
    the reference's order, and runs the training forward (activations saved for `backward`)."""

    def __init__(self, shape: WhisperShape, device=None, activation_dropout: float = 0.0, freeze_base: bool = False,
                 spec=None, layerdrop: float = 0.0, dropout: float = 0.0, attention_dropout: float = 0.0):
        device = device or f"cuda:{torch.cuda.current_device() if torch.cuda.is_available() else 0}"
        self.engine = WhisperTrainEngine(shape, device, activation_dropout=activation_dropout, freeze_base=freeze_base,
                                         dropout=dropout, attention_dropout=attention_dropout)
        self.shape = shape
        self.spec = spec or dict(apply_spec_augment=False, mask_time_prob=0.0, mask_time_length=10,
                                 mask_feature_prob=0.0, mask_feature_length=64)
        self.layerdrop = layerdrop
        # what `generate` reads of a checkpoint's generation_config.json: no_timestamps_token_id, lang_to_id, task_to_id,
        # max_initial_timestamp_index (absent keys: the multilingual vocabulary's ids, no cap - as transformers)
        self.generation_config: dict = {}
        self.median_filter_width = 7  # config.json's `median_filter_width` (token timestamps)
        self.training = False
        self.engine.training = False
        self._rng = np.random

    def train(self, mode: bool = True):
        self.training = mode
        self.engine.training = mode
        return self

    def eval(self):
        return self.train(False)

    @classmethod
    def from_pretrained(cls, name_or_path: str, device=None, seed: int = 4242, **overrides):
        spec = {k: overrides.pop(k) for k in ("apply_spec_augment", "mask_time_prob", "mask_time_length",
                                              "mask_feature_prob", "mask_feature_length") if k in overrides}
        kw = dict(activation_dropout=float(overrides.pop("activation_dropout", 0.0)),
                  dropout=float(overrides.pop("dropout", 0.0)),
                  attention_dropout=float(overrides.pop("attention_dropout", 0.0)),
                  freeze_base=bool(overrides.pop("freeze_base", False)), spec=spec or None,
                  layerdrop=float(overrides.pop("encoder_layerdrop", overrides.pop("layerdrop", 0.0))))
        path = Path(name_or_path)
        if path.is_dir() and (path / "config.json").exists():
            cfg = json.loads((path / "config.json").read_text())
            fields = WhisperShape.__dataclass_fields__
            model = cls(WhisperShape(**{k: cfg[k] for k in fields if k in cfg}), device, **kw)
            model.median_filter_width = int(cfg.get("median_filter_width", 7))
            from .modeling import load_checkpoint_tensors

            sd = load_checkpoint_tensors(path)
            sd = {(k if k.startswith("model.") else "model." + k): v for k, v in sd.items() if k != "proj_out.weight"}
            model.engine.load_state_dict(sd)
            model.engine.refresh_derived()
            if (path / "generation_config.json").exists():
                model.generation_config = json.loads((path / "generation_config.json").read_text())
            return model
        if name_or_path not in HUB_SHAPES:
            raise ValueError(f"unknown model {name_or_path!r}")
        model = cls(WhisperShape(**CORAL_WHISPER_SHAPES[HUB_SHAPES[name_or_path]]), device, **kw)
        model.generation_config = dict(no_timestamps_token_id=prefix_ids(model.shape)[-1],
                                       max_initial_timestamp_index=HUB_MAX_INITIAL_TIMESTAMP_INDEX)
        logger.warning("no network / hub cache here: %s is instantiated with seeded random weights", name_or_path)
        g = torch.Generator(device=model.engine.device).manual_seed(seed)
        for n in model.engine.exported_names():
            v = model.engine.store.view(n)
            if n.endswith("layer_norm.weight"):
                v.fill_(1.0)
            elif n.endswith(".bias"):
                v.zero_()
            elif n.endswith("encoder.embed_positions.weight"):  # fixed sinusoid table (:55-64, requires_grad False)
                v.copy_(sinusoid_positions(*v.shape).to(v.device))
            else:
                v.normal_(0.0, 0.02, generator=g)
        model.engine.refresh_compute_weights()
        model.engine.refresh_derived()
        return model

    def save_pretrained(self, model_dir):
        from safetensors.torch import save_file

        model_dir = Path(model_dir)
        model_dir.mkdir(parents=True, exist_ok=True)
        cfg = dict(architectures=["WhisperForConditionalGeneration"], model_type="whisper", **self.shape.__dict__,
                   median_filter_width=int(self.median_filter_width))
        (model_dir / "config.json").write_text(json.dumps(cfg, indent=2))
        if self.generation_config:
            (model_dir / "generation_config.json").write_text(json.dumps(self.generation_config, indent=2))
        save_file({k: v.cpu().contiguous() for k, v in self.engine.state_dict().items()},
                  str(model_dir / "model.safetensors"), metadata={"format": "pt"})

    def sample_spec_masks(self, B: int):
        sp = self.spec
        if not (self.training and sp.get("apply_spec_augment", False)):
            return None, None
        mt, mf = specaugment.sample_masks(B, 2 * self.shape.max_source_positions, self.shape.num_mel_bins, None,
                                          sp["mask_time_prob"], sp["mask_time_length"], sp["mask_feature_prob"],
                                          sp["mask_feature_length"], rng=self._rng)
        return (None if mt is None else torch.from_numpy(mt)), (None if mf is None else torch.from_numpy(mf))

    def sample_layer_keep(self):
        if not self.training or self.layerdrop <= 0:
            return None, None
        draw = lambda n: [bool(float(torch.rand([])) >= self.layerdrop) for _ in range(n)]  # noqa: E731
        return draw(self.shape.encoder_layers), draw(self.shape.decoder_layers)

    def __call__(self, input_features, labels=None, decoder_input_ids=None, mask_time=None, mask_feature=None,
                 enc_keep=None, dec_keep=None):
        if self.training and labels is not None:
            if mask_time is None and mask_feature is None:
                mask_time, mask_feature = self.sample_spec_masks(input_features.shape[0])
            if enc_keep is None and dec_keep is None:
                enc_keep, dec_keep = self.sample_layer_keep()
            out = self.engine(input_features, labels, mask_time, mask_feature, enc_keep, dec_keep)
            if out.get("loss") is not None:  # `out["loss"].backward()` runs the engine's backward (coral_amd/autograd.py)
                out["loss"] = attach_backward(self, out["loss"])
            return out
        return self.engine.forward(input_features, labels, decoder_input_ids)

    backward_kwargs: dict | None = None

    def backward(self, **kw):
        return self.engine.backward(**kw)

    def forced_prefix(self, return_timestamps: bool = False) -> list[int]:
        """<|sot|><|da|><|transcribe|><|notimestamps|> from the checkpoint's generation config where it names the ids
        (lang_to_id, task_to_id, no_timestamps_token_id: `_retrieve_init_tokens`), else the multilingual vocabulary's;
        return_timestamps=True drops <|notimestamps|>."""
        gc = self.generation_config
        prefix = list(prefix_ids(self.shape))
        if "lang_to_id" in gc and "task_to_id" in gc and "no_timestamps_token_id" in gc:
            prefix = [self.shape.decoder_start_token_id, int(gc["lang_to_id"]["<|da|>"]), int(gc["task_to_id"]["transcribe"]),
                      int(gc["no_timestamps_token_id"])]
        return prefix[:-1] if return_timestamps else prefix

    def generate(self, input_features, language="danish", task="transcribe", max_length: int = 225, num_beams: int | None = 1,
                 length_penalty: float = 1.0, early_stopping=False, return_timestamps: bool | None = False,
                 return_token_timestamps: bool | None = False, num_frames=None, temperature=None, logprob_threshold=None,
                 compression_ratio_threshold=None, no_speech_threshold=None, sample_seed: int = 0,
                 return_fallback_stats: bool = False, prompt_ids=None, condition_on_prev_tokens=None,
                 prompt_condition_type=None, **other):
        """Greedy (num_beams 1 / None: other keyword arguments are ignored, as before) or beam search (num_beams >= 2,
        transformers' semantics; every generation argument this build does not implement is then refused by name).
        return_timestamps=True (greedy only): the prefix drops <|notimestamps|> and every pick obeys Whisper's timestamp
        rules (timestamp_begin = that id + 1, max_initial_timestamp_index from the generation config).
        return_token_timestamps=True (with return_timestamps=True, greedy only): -> (ids, float32 seconds per token) from
        the cross-attention of the generation config's `alignment_heads` (absent: transformers' error) and dynamic time
        warping; num_frames: valid log-mel frames per clip; `median_filter_width` is the checkpoint config's (default 7).
        temperature (a number or a tuple tried in order), logprob_threshold, compression_ratio_threshold,
        no_speech_threshold, sample_seed: transformers' temperature fallback for clips of one window (greedy only, no token
        timestamps): `decode_with_fallback` of coral_amd/longform_whisper.py with one window per clip, the encoder run once.
        A clip skipped as silence comes back as the prefix and EOS.  return_fallback_stats=True: -> (ids, per clip
        dict(temperature, avg_logprob, compression_ratio, no_speech_prob, skipped)).
        prompt_ids (the ids `get_prompt_ids` returns, <|startofprev|> first), condition_on_prev_tokens,
        prompt_condition_type: transformers' arguments of the same names (coral_amd/longform_whisper.py `PromptPolicy`).
        Here every clip is one window, so what they change is the decoder input in front of the forced prefix: the
        prompt (behind a mask when conditioning is on, as `_prepare_decoder_input_ids` builds it); max_length grows by
        its length as `_set_max_new_tokens_and_length` grows it.  The rows returned start with the forced prefix, the
        prompt is stripped.  Greedy only, not with token timestamps or the fallback arguments (`transcribe_whisper`
        takes all of them together, and recordings of any length)."""
        if language not in ("danish", "da") or task != "transcribe":
            raise ValueError("only language='danish', task='transcribe' (CoRal's evaluation call) is wired up")
        prefix = self.forced_prefix()
        num_beams = 1 if num_beams is None else num_beams
        kw = {}
        policy = None
        prompting = self.prompt_policy(prompt_ids, condition_on_prev_tokens, prompt_condition_type)
        if prompting is not None:
            if num_beams != 1:
                raise ValueError(f"generate(num_beams={num_beams}): prompt_ids / condition_on_prev_tokens / "
                                 "prompt_condition_type are not implemented with beam search")
            if return_token_timestamps:
                raise ValueError("prompt_ids / condition_on_prev_tokens are not implemented with return_token_timestamps=True")
            if self.fallback_policy(temperature, logprob_threshold, compression_ratio_threshold, no_speech_threshold) is not None:
                raise ValueError("prompt_ids / condition_on_prev_tokens together with temperature fallback: "
                                 "coral_amd.evaluate.transcribe_whisper runs the two in one loop, generate() does not")
        if num_beams != 1:  # with beams they are refused by name below, their neutral values pass as before
            given = dict(temperature=temperature, logprob_threshold=logprob_threshold,
                         compression_ratio_threshold=compression_ratio_threshold, no_speech_threshold=no_speech_threshold)
            other = dict(other, **{k: v for k, v in given.items() if v is not None})
        else:
            policy = self.fallback_policy(temperature, logprob_threshold, compression_ratio_threshold, no_speech_threshold,
                                          sample_seed)
        if policy is not None and return_token_timestamps:
            raise ValueError("return_token_timestamps=True is not implemented with temperature fallback")
        if policy is None and return_fallback_stats:
            raise ValueError("return_fallback_stats=True needs temperature= or a threshold (greedy only)")
        if return_timestamps:
            if num_beams != 1:
                other = dict(other, return_timestamps=return_timestamps)  # refused by name below
            else:
                no_ts, prefix = prefix[-1], prefix[:-1]
                kw = dict(return_timestamps=True, timestamp_begin=no_ts + 1,
                          max_initial_timestamp_index=self.generation_config.get("max_initial_timestamp_index", None))
        if return_token_timestamps:
            from .whisper_align import check_alignment_heads

            if num_beams != 1:
                other = dict(other, return_token_timestamps=return_token_timestamps)  # refused by name below
            else:
                heads = check_alignment_heads(self.generation_config.get("alignment_heads"), self.shape.decoder_layers,
                                              self.shape.decoder_attention_heads)
                kw.update(return_token_timestamps=True, alignment_heads=heads, num_frames=num_frames,
                          median_filter_width=int(self.median_filter_width))
        if num_beams != 1:
            from .whisper import check_beam_arguments

            check_beam_arguments(int(input_features.shape[0]), num_beams, length_penalty, early_stopping, other)
            kw = dict(num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping)
        # CoRal clears `suppress_tokens`; the default begin-suppress set (blank ' ' = 220, eos) stays
        if prompting is not None:
            from .longform_whisper import grown_max_length, prepare_decoder_inputs

            s, n = self.shape, int(input_features.shape[0])
            rows, start, masked = prepare_decoder_inputs(prefix, prompting.first_segments(n), list(range(n)),
                                                         [prompting.condition_on_prev_tokens] * n, prompting, s.pad_token_id,
                                                         s.max_target_positions, self.forced_prefix()[-1] + 1)
            inputs = dict(rows=rows, start=start, masked=masked,
                          max_length=grown_max_length(max_length, len(rows[0]), s.max_target_positions))
            out = self.prompted_window(input_features, inputs, bool(return_timestamps))
            return [list(prefix) + [int(t) for t in r[len(rows[0]):]] for r in out]
        if policy is not None:
            from .longform_whisper import decode_with_fallback

            s = self.shape
            n = int(input_features.shape[0])
            attempt = self.fallback_attempts(policy, max_length, bool(return_timestamps))
            feats = {(i, 0): input_features[i] for i in range(n)}
            kept, skipped = decode_with_fallback(lambda batch, t, u: attempt(batch, t, u, feats), [(i, 0) for i in range(n)],
                                                 policy, torch.Generator().manual_seed(int(policy.seed)), len(prefix),
                                                 s.pad_token_id, s.eos_token_id, s.vocab_size, max_length)
            rows = [list(prefix) + [s.eos_token_id] if sk else [int(t) for t in k["row"]] for k, sk in zip(kept, skipped)]
            width = max(len(r) for r in rows)
            rows = [r + [s.pad_token_id] * (width - len(r)) for r in rows]
            if not return_fallback_stats:
                return rows
            return rows, [dict(skipped=bool(sk), **{a: v for a, v in k.items() if a != "row"}) for k, sk in zip(kept, skipped)]
        return self.engine.generate(input_features, prefix, max_length, suppress_tokens=None,
                                    begin_suppress_tokens=self.begin_suppress(), **kw)

    def begin_suppress(self) -> list[int]:
        """The begin-suppress set: blank ' ' = 220 and eos.  An id the vocabulary does not hold is left out (a toy
        vocabulary of fewer than 221 ids has no 220 to suppress; the mask has one entry per id)."""
        return [t for t in (220, self.shape.eos_token_id) if t < self.shape.vocab_size]

    def prompt_policy(self, prompt_ids=None, condition_on_prev_tokens=None, prompt_condition_type=None):
        """The PromptPolicy of these generate arguments, or None where they leave decoding as it is.  <|startofprev|> is
        the generation config's prev_sot_token_id (CoRal clears suppress_tokens, transformers' other source of it); without
        it previous text stands in front of the forced prefix with no token before it, as in transformers."""
        from .longform_whisper import PromptPolicy

        if prompt_ids is None and not condition_on_prev_tokens and prompt_condition_type is None:
            return None
        if prompt_ids is not None:
            prompt_ids = tuple(int(t) for t in (prompt_ids.tolist() if hasattr(prompt_ids, "tolist") else prompt_ids))
        prev = self.generation_config.get("prev_sot_token_id")
        policy = PromptPolicy(prompt_ids, prompt_condition_type, bool(condition_on_prev_tokens), None if prev is None else int(prev))
        return policy if policy.active else None

    def prompted_window(self, input_features, inputs: dict, return_timestamps: bool, cross_kv=None, **scoring):
        """One batch of windows decoded from the decoder inputs of `prepare_decoder_inputs` / `run_longform` (dict(rows,
        start, max_length[, no_speech_index])): `engine.generate(prefix_rows=, prefix_start=)`.  -> what that returns."""
        s = self.shape
        kw = {}
        if return_timestamps:
            kw = dict(return_timestamps=True, timestamp_begin=self.forced_prefix()[-1] + 1,
                      max_initial_timestamp_index=self.generation_config.get("max_initial_timestamp_index", None))
        return self.engine.generate(input_features, None, int(inputs["max_length"]), suppress_tokens=None,
                                    begin_suppress_tokens=self.begin_suppress(),
                                    prefix_rows=torch.tensor(inputs["rows"], dtype=torch.int64),
                                    prefix_start=torch.tensor(inputs["start"], dtype=torch.int32), cross_kv=cross_kv,
                                    no_speech_index=int(inputs.get("no_speech_index", 0)), **kw, **scoring)

    def fallback_policy(self, temperature=None, logprob_threshold=None, compression_ratio_threshold=None,
                        no_speech_threshold=None, sample_seed: int = 0):
        """The FallbackPolicy of these generate arguments, or None where they leave decoding as it is (temperature None
        / 0 / (0,) and no threshold).  <|nospeech|> is the id in front of <|notimestamps|>, as transformers takes it."""
        from .longform_whisper import FallbackPolicy

        ts = (0.0,) if temperature is None else temperature
        ts = (ts,) if isinstance(ts, (int, float)) and not isinstance(ts, bool) else tuple(ts)
        if all(t == 0 for t in ts) and len(ts) <= 1 and logprob_threshold is None and compression_ratio_threshold is None \
                and no_speech_threshold is None:
            return None
        return FallbackPolicy(ts, logprob_threshold, compression_ratio_threshold, no_speech_threshold,
                              self.forced_prefix()[-1] - 1 if no_speech_threshold is not None else None, int(sample_seed))

    def fallback_attempts(self, policy, max_length: int, return_timestamps: bool):
        """-> attempt(batch, temperature, uniforms, feats[, inputs]): the `window_generate` of `decode_with_fallback` on this
        model.  batch: keys of `feats` (key -> log-mel [mels, 3000]).  The encoder and the cross K|V run when a batch
        brings keys that the last encoded batch did not hold; a later attempt decodes its rows against a gather of that
        K|V.  inputs: the attempt's decoder inputs under a PromptPolicy (`run_longform(conditioning=)`), in place of the
        forced prefix."""
        eng, s = self.engine, self.shape
        prefix = self.forced_prefix(return_timestamps)
        kw = {}
        if return_timestamps:
            kw = dict(return_timestamps=True, timestamp_begin=self.forced_prefix()[-1] + 1,
                      max_initial_timestamp_index=self.generation_config.get("max_initial_timestamp_index", None))
        held = dict(keys={}, kv=None)

        def attempt(batch, temperature, uniforms, feats, inputs=None):
            if held["kv"] is None or any(k not in held["keys"] for k in batch):
                held["kv"] = eng.cross_kv(eng.encode(torch.stack([torch.as_tensor(feats[k]) for k in batch])))
                held["keys"] = {k: i for i, k in enumerate(batch)}
            rows = [held["keys"][k] for k in batch]
            kv = held["kv"] if rows == list(range(len(held["keys"]))) else eng.gather_cross_kv(held["kv"], rows)
            if inputs is not None:
                return self.prompted_window(None, inputs, return_timestamps, cross_kv=kv, temperature=float(temperature),
                                            sample_uniforms=uniforms, return_stats=True, no_speech_token=policy.no_speech_token)
            return eng.generate(None, prefix, max_length, suppress_tokens=None,
                                begin_suppress_tokens=self.begin_suppress(), temperature=float(temperature),
                                sample_uniforms=uniforms, return_stats=True, no_speech_token=policy.no_speech_token,
                                cross_kv=kv, **kw)

        return attempt


class WhisperModelSetup(ModelSetup):
    def __init__(self, config) -> None:
        self.config = config
        self.processor = None
        self.model = None
        self.is_main_process = os.getenv("RANK", "0") == "0"

    def load_model(self):
        m = self.config.model
        self.model = WhisperForConditionalGeneration.from_pretrained(
            m.pretrained_model_id, seed=self.config.seed, dropout=m.dropout, activation_dropout=m.activation_dropout,
            attention_dropout=m.attention_dropout, apply_spec_augment=True, mask_time_prob=m.mask_time_prob,
            mask_time_length=m.mask_time_length, mask_feature_prob=m.mask_feature_prob,
            mask_feature_length=m.mask_feature_length, encoder_layerdrop=m.layerdrop, decoder_layerdrop=m.layerdrop,
            freeze_base=bool(m.freeze_feature_encoder))
        return self.model

    def load_processor(self):
        if self.model is None:
            self.load_model()
        tok = None
        tj = Path(self.config.model_dir) / "tokenizer.json"
        if tj.exists():
            from tokenizers import Tokenizer

            tok = Tokenizer.from_file(str(tj))
        self.processor = WhisperProcessor(WhisperFeatureExtractorGPU(self.model.engine, self.config.model.sampling_rate), tok)
        return self.processor

    def load_data_collator(self):
        def collate(features):
            """DataCollatorSpeechSeq2SeqWithPadding (R/src/coral/data_collators.py:130-187): stack
            input_features, pad labels with -100, strip a leading BOS present in every row."""
            feats = torch.stack([torch.as_tensor(f["input_features"]) for f in features])
            L = max(len(f["labels"]) for f in features)
            labels = torch.full((len(features), L), -100, dtype=torch.int64)
            for i, f in enumerate(features):
                labels[i, : len(f["labels"])] = torch.as_tensor(f["labels"])
            start = self.model.shape.decoder_start_token_id
            if bool((labels[:, 0] == start).all()):
                labels = labels[:, 1:]
            return dict(input_features=feats, labels=labels)

        return collate

    def load_trainer_class(self):
        return CoralTrainer

    def load_compute_metrics(self):
        def compute(pred_ids, label_ids):
            from .error_rates import text_rates

            labels = np.array(label_ids, copy=True)
            labels[labels == -100] = self.model.shape.pad_token_id
            preds = self.processor.batch_decode(pred_ids, skip_special_tokens=True)
            labs = self.processor.batch_decode(labels, skip_special_tokens=True)
            preds = [p.lower().strip() for p in preds]
            labs = [x.lower().strip() for x in labs]
            return text_rates(preds, labs, self.config.get("error_rates", "host") or "host",
                              bool(self.config.get("normalise_error_rates", False) or False))

        return compute

    def load_training_arguments(self):
        args = _training_args(self.config, self.config.model.learning_rate)
        args.generation_max_length = self.config.model.max_length  # predict_with_generate (whisper.py:221-222)
        return args

    def load_saved(self) -> PreTrainedModelData:
        model_dir = Path(self.config.model_dir)
        if not model_dir.exists():
            raise FileNotFoundError(f"{model_dir} does not exist (no hub access in this environment)")
        self.model = WhisperForConditionalGeneration.from_pretrained(str(model_dir))
        self.load_processor()
        return PreTrainedModelData(model=self.model, processor=self.processor,
                                   data_collator=self.load_data_collator(), compute_metrics=self.load_compute_metrics())
