"""MI355X-native Whisper engine behind CoRal's `model=whisper-*` keys: log-mel front end on the
GPU, encoder, teacher-forced decoder with the tied LM head + cross-entropy, and greedy generation.

Mirrors what `WhisperModelSetup` gives CoRal (R/src/coral/whisper.py:49-109) and what the ASR
pipeline calls (R/src/coral/evaluate.py:56-60 -> `model.generate`):
  WhisperFeatureExtractor            $TF/models/whisper/feature_extraction_whisper.py:135-168  -> ca_logmel
  WhisperEncoder.forward             $TF/models/whisper/modeling_whisper.py:592-646
  WhisperDecoder(.Layer).forward     :448-505, 690-795
  WhisperForConditionalGeneration    :994-1099 (shift_tokens_right, tied proj_out, CE ignore -100)
  greedy generate                    $TF/models/whisper/generation_whisper.py:383,1455,1774-1812

Forward paths (inference, evaluation loss, greedy decode).  The conv stem runs as overlapping-row GEMMs
over a time-padded channels-last buffer (Conv1d k=3, p=1, stride 1 / 2), the sinusoidal positions are
added in the second conv's epilogue.  The encoder and decoder layers are the pre-LN blocks of blocks.py,
run on inference workspaces; the training engine (whisper_train.py) runs the same blocks, stem and head
with saved activations.  Greedy decoding appends one token at a time against a self-attention K|V cache
(decode_step, or the graph-replayed / persistent token step), the cross-attention K|V computed once per clip.
Beam search (`generate(num_beams=k)`, `_generate_beam`): the launch-sequence step over clips x k rows, the K|V cache read
through an ancestry table (CaAttnDesc.key_slot), candidates ranked and beams kept on the device (csrc/beam.hip), with the
semantics of $TF/generation/utils.py:3208-3508 (GenerationMixin._beam_search).
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .blocks import LN_IN_GEMM, CrossAttnBlock, FFNBlock, SelfAttnBlock, zeros_on
from .ops import EPI_GELU, EPI_GELU_RESIDUAL, EPI_RESIDUAL
from .wav2vec2 import ParamStore, _r8


@dataclass
class WhisperShape:
    d_model: int = 384
    encoder_layers: int = 4
    decoder_layers: int = 4
    encoder_attention_heads: int = 6
    decoder_attention_heads: int = 6
    encoder_ffn_dim: int = 1536
    decoder_ffn_dim: int = 1536
    num_mel_bins: int = 80
    vocab_size: int = 51865
    max_source_positions: int = 1500
    max_target_positions: int = 448
    pad_token_id: int = 50257
    decoder_start_token_id: int = 50258
    eos_token_id: int = 50257
    layer_norm_eps: float = 1e-5


# CoRal model keys -> architectures (R/config/model/whisper-*.yaml:3-5; public config.json values)
CORAL_WHISPER_SHAPES = {
    "whisper-xxsmall": dict(d_model=384, encoder_layers=4, decoder_layers=4, encoder_attention_heads=6,
                            decoder_attention_heads=6, encoder_ffn_dim=1536, decoder_ffn_dim=1536),
    "whisper-xsmall": dict(d_model=512, encoder_layers=6, decoder_layers=6, encoder_attention_heads=8,
                           decoder_attention_heads=8, encoder_ffn_dim=2048, decoder_ffn_dim=2048),
    "whisper-small": dict(d_model=768, encoder_layers=12, decoder_layers=12, encoder_attention_heads=12,
                          decoder_attention_heads=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072),
    "whisper-medium": dict(d_model=1024, encoder_layers=24, decoder_layers=24, encoder_attention_heads=16,
                           decoder_attention_heads=16, encoder_ffn_dim=4096, decoder_ffn_dim=4096),
    "whisper-large": dict(d_model=1280, encoder_layers=32, decoder_layers=32, encoder_attention_heads=20,
                          decoder_attention_heads=20, encoder_ffn_dim=5120, decoder_ffn_dim=5120,
                          num_mel_bins=128, vocab_size=51866),
    "whisper-large-turbo": dict(d_model=1280, encoder_layers=32, decoder_layers=4, encoder_attention_heads=20,
                                decoder_attention_heads=20, encoder_ffn_dim=5120, decoder_ffn_dim=5120,
                                num_mel_bins=128, vocab_size=51866),
}

N_FFT, HOP, N_SAMPLES = 400, 160, 480_000


def mel_filter_bank(n_mels: int, n_freq: int = 201, sr: int = 16_000, fmin=0.0, fmax=8000.0) -> np.ndarray:
    """Slaney-scale, Slaney-normalised triangular filters [n_freq, n_mels]
    (`mel_filter_bank(201, n_mels, 0, 8000, 16000, "slaney", "slaney")`, $TF/audio_utils.py:638-731)."""
    def hz2mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-10) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)

    def mel2hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)

    hz = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), n_mels + 2))
    freqs = np.linspace(0, sr // 2, n_freq)
    slopes = hz[None, :] - freqs[:, None]
    d = np.diff(hz)
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / d[:-1], slopes[:, 2:] / d[1:]))
    return (fb * (2.0 / (hz[2:n_mels + 2] - hz[:n_mels]))[None, :]).astype(np.float32)


def whisper_param_list(s: WhisperShape):
    """(HF name, shape, bucket); q,k,v weights adjacent, and a zero `k_proj.bias` slot (HF has none)
    so the fused [3d] bias vector exists.  Names ending in `__zero` are internal and never exported."""
    d = s.d_model
    out = [("model.encoder.conv1.weight", (d, s.num_mel_bins, 3), "front"), ("model.encoder.conv1.bias", (d,), "front"),
           ("model.encoder.conv2.weight", (d, d, 3), "front"), ("model.encoder.conv2.bias", (d,), "front"),
           ("model.encoder.embed_positions.weight", (s.max_source_positions, d), "front")]

    for l in range(s.encoder_layers):
        p, b = f"model.encoder.layers.{l}.", f"enc{l}"
        a = p + "self_attn."
        # small tensors first, the weight matrices (read through the bf16 compute copy only) at the end of the bucket:
        # the part a sharded optimiser splits over the ranks (WhisperTrainEngine.shard_ranges, trainer.py zero_stage)
        out += [(p + "self_attn_layer_norm.weight", (d,), b), (p + "self_attn_layer_norm.bias", (d,), b),
                (p + "final_layer_norm.weight", (d,), b), (p + "final_layer_norm.bias", (d,), b),
                # the Linear biases are contiguous (q|k|v, out, fc1, fc2 = 5d + f floats): their gradients are partial
                # column sums out of the grouped weight-gradient launch, added in one pass (whisper_train.backward)
                (a + "q_proj.bias", (d,), b), (a + "k_proj.bias__zero", (d,), b), (a + "v_proj.bias", (d,), b),
                (a + "out_proj.bias", (d,), b), (p + "fc1.bias", (s.encoder_ffn_dim,), b), (p + "fc2.bias", (d,), b)]
        out += [(a + n + ".weight", (d, d), b) for n in ("q_proj", "k_proj", "v_proj")]
        out += [(a + "out_proj.weight", (d, d), b),
                (p + "fc1.weight", (s.encoder_ffn_dim, d), b), (p + "fc2.weight", (d, s.encoder_ffn_dim), b)]
    out += [("model.encoder.layer_norm.weight", (d,), "encf"), ("model.encoder.layer_norm.bias", (d,), "encf"),
            ("model.decoder.embed_tokens.weight", (s.vocab_size, d), "emb"),
            ("model.decoder.embed_positions.weight", (s.max_target_positions, d), "emb")]
    for l in range(s.decoder_layers):
        p, b = f"model.decoder.layers.{l}.", f"dec{l}"
        sa, ca = p + "self_attn.", p + "encoder_attn."
        # small tensors first (the three norms, then ALL Linear biases as one contiguous vector of 9d + f floats in the
        # order self q|k|v, self out, cross q, cross k|v, cross out, fc1, fc2: the fused bias gradients of the layer's
        # grouped weight-gradient launch are added in one pass), the weight matrices at the end of the bucket
        for n in ("self_attn_layer_norm", "encoder_attn_layer_norm", "final_layer_norm"):
            out += [(p + n + ".weight", (d,), b), (p + n + ".bias", (d,), b)]
        out += [(sa + "q_proj.bias", (d,), b), (sa + "k_proj.bias__zero", (d,), b), (sa + "v_proj.bias", (d,), b),
                (sa + "out_proj.bias", (d,), b),
                (ca + "q_proj.bias", (d,), b), (ca + "k_proj.bias__zero", (d,), b), (ca + "v_proj.bias", (d,), b),
                (ca + "out_proj.bias", (d,), b),
                (p + "fc1.bias", (s.decoder_ffn_dim,), b), (p + "fc2.bias", (d,), b)]
        for a in (sa, ca):
            out += [(a + n + ".weight", (d, d), b) for n in ("q_proj", "k_proj", "v_proj", "out_proj")]
        out += [(p + "fc1.weight", (s.decoder_ffn_dim, d), b), (p + "fc2.weight", (d, s.decoder_ffn_dim), b)]
    out += [("model.decoder.layer_norm.weight", (d,), "decf"), ("model.decoder.layer_norm.bias", (d,), "decf")]
    return out


def shift_tokens_right(labels: torch.Tensor, pad_token_id: int, decoder_start_token_id: int) -> torch.Tensor:
    """Decoder inputs of teacher forcing ($TF/models/whisper/modeling_whisper.py, shift_tokens_right): the labels one
    position to the right behind the start token, -100 replaced by the pad token."""
    lab = labels.to(torch.int64)
    dec = lab.new_zeros(lab.shape)
    dec[:, 1:] = lab[:, :-1]
    dec[:, 0] = decoder_start_token_id
    return dec.masked_fill(dec == -100, pad_token_id)


def sinusoid_positions(length: int, channels: int, max_timescale: float = 10000.0) -> torch.Tensor:
    """The encoder's fixed position table ($TF/models/whisper/modeling_whisper.py:55-64): [sin | cos] of
    position x geometric timescales."""
    import math

    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2, dtype=torch.float32))
    t = torch.arange(length, dtype=torch.float32).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1)


# generation arguments of transformers' `generate` that change what beam search returns and that this build does not
# implement: refused by name, never swallowed (values that leave the search as it is - None, or the neutral value - pass)
_BEAM_REFUSED = {"num_return_sequences": (None, 1), "do_sample": (None, False), "temperature": (None, 1.0), "top_k": (None,),
                 "top_p": (None, 1.0), "typical_p": (None, 1.0), "num_beam_groups": (None, 1), "diversity_penalty": (None, 0.0),
                 "repetition_penalty": (None, 1.0), "no_repeat_ngram_size": (None, 0), "penalty_alpha": (None,),
                 "return_timestamps": (None, False), "return_token_timestamps": (None, False), "low_memory": (None, False), "constraints": (None,),
                 "force_words_ids": (None,), "bad_words_ids": (None,), "min_length": (None, 0), "min_new_tokens": (None,),
                 "max_new_tokens": (None,), "logits_processor": (None,), "stopping_criteria": (None,),
                 "prefix_allowed_tokens_fn": (None,), "assistant_model": (None,), "no_speech_threshold": (None,),
                 "compression_ratio_threshold": (None,), "logprob_threshold": (None,), "prompt_ids": (None,),
                 "return_dict_in_generate": (None, False), "output_scores": (None, False)}


def check_beam_arguments(clips: int, num_beams, length_penalty, early_stopping, other: dict):
    """The limits of generate(num_beams=k): raises ValueError for what the beam search here does not do."""
    if not isinstance(num_beams, int) or isinstance(num_beams, bool) or num_beams < 1:
        raise ValueError(f"num_beams must be a positive integer, got {num_beams!r}")
    if num_beams > _lib.BEAM_MAX_BEAMS:
        raise ValueError(f"num_beams={num_beams} exceeds the limit of {_lib.BEAM_MAX_BEAMS} beams")
    if clips * num_beams > _lib.BEAM_MAX_ROWS:
        raise ValueError(f"{clips} clips x num_beams={num_beams} = {clips * num_beams} decoder rows exceed the limit of "
                         f"{_lib.BEAM_MAX_ROWS} (clips x num_beams <= {_lib.BEAM_MAX_ROWS}): decode fewer clips at a time")
    if early_stopping not in (True, False):
        raise ValueError(f"early_stopping={early_stopping!r} is not implemented (True and False are; \"never\" is not)")
    if not isinstance(length_penalty, (int, float)) or isinstance(length_penalty, bool) or not math.isfinite(length_penalty):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
    for name, val in other.items():
        neutral = _BEAM_REFUSED.get(name)
        if neutral is None:
            raise ValueError(f"generate(num_beams={num_beams}): argument {name}={val!r} is not known to this build")
        if not any(val is n or (n is not None and type(val) is type(n) and val == n) for n in neutral):
            raise ValueError(f"generate(num_beams={num_beams}): {name}={val!r} is not implemented with beam search")


class WhisperEngine:
    """Forward paths of WhisperForConditionalGeneration as sequences of HIP kernels."""

    def __init__(self, shape: WhisperShape, device="cuda:0"):
        ops.lib()
        if not torch.cuda.is_available():
            raise ops.CoralAmdError("WhisperEngine needs a GPU: there is no CPU path")
        self.s = shape
        self.device = torch.device(device)
        assert shape.d_model % 8 == 0 and shape.num_mel_bins % 8 == 0
        self.store = ParamStore(whisper_param_list(shape), self.device)
        d = shape.d_model
        self.conv1_wr = torch.zeros(d * 3 * shape.num_mel_bins, dtype=torch.bfloat16, device=self.device)
        self.conv2_wr = torch.zeros(d * 3 * d, dtype=torch.bfloat16, device=self.device)
        self.mel_filters = torch.from_numpy(mel_filter_bank(shape.num_mel_bins)).to(self.device)
        self.zero_mel = torch.zeros(shape.num_mel_bins, dtype=torch.bfloat16, device=self.device)  # SpecAugment's fill
        st, eps = self.store, shape.layer_norm_eps

        def self_attn_ffn(p, H, f, causal):  # the self-attention and feed-forward blocks of layer `p`
            return (SelfAttnBlock(st, p + "self_attn_layer_norm", p + "self_attn.", H, d, eps, causal, p + "self_attn.q_proj.bias"),
                    FFNBlock(st, p + "final_layer_norm", p + "fc1", p + "fc2", d, f, eps))

        self.enc_blocks = [self_attn_ffn(f"model.encoder.layers.{l}.", shape.encoder_attention_heads, shape.encoder_ffn_dim,
                                         False) for l in range(shape.encoder_layers)]
        self.dec_blocks = []
        for l in range(shape.decoder_layers):
            p = f"model.decoder.layers.{l}."
            sa, ff = self_attn_ffn(p, shape.decoder_attention_heads, shape.decoder_ffn_dim, True)
            ca = CrossAttnBlock(st, p + "encoder_attn_layer_norm", p + "encoder_attn.", shape.decoder_attention_heads, d, eps)
            # a decoder layer's bias vector (whisper_param_list): self q|k|v, self out, cross q, cross k|v, cross out, fc1, fc2
            sa.cs_qkv, sa.cs_o, ca.cs, ff.cs_fc1, ff.cs_fc2 = 0, 3 * d, (4 * d, 7 * d), 8 * d, 8 * d + shape.decoder_ffn_dim
            self.dec_blocks.append((sa, ca, ff))
        self._enc_ws = {}
        self._dec_ws = {}

    # The trainer may still be updating parameter buckets on its optimiser stream (trainer.py); every
    # path that reads weights waits for the bucket events first.
    weights_ready: dict | None = None

    def _await(self, bucket: str):
        ev = self.weights_ready.get(bucket) if self.weights_ready else None
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def _await_all(self):
        if self.weights_ready:
            for ev in self.weights_ready.values():
                torch.cuda.current_stream().wait_event(ev)

    # ---- parameters ------------------------------------------------------------------------
    def exported_names(self):
        return [n for n in self.store.names() if not n.endswith("__zero")]

    def load_state_dict(self, P: dict):
        missing = [n for n in self.exported_names() if n not in P]
        if missing:
            raise KeyError(f"missing parameters: {missing[:4]}...")
        for n in self.exported_names():
            self.store.view(n).copy_(P[n].to(self.device, torch.float32).reshape(self.store.index[n][1]))
        self.refresh_compute_weights()

    def state_dict(self):
        self._await_all()
        return {n: self.store.view(n).detach().clone() for n in self.exported_names()}

    def refresh_compute_weights(self):
        s, st = self.s, self.store
        st.refresh_bf16()
        ops.conv_weight_reorder(st.p32, self.conv1_wr, s.d_model, s.num_mel_bins, 3, w_off=st.off("model.encoder.conv1.weight"))
        ops.conv_weight_reorder(st.p32, self.conv2_wr, s.d_model, s.d_model, 3, w_off=st.off("model.encoder.conv2.weight"))

    # ---- front end ---------------------------------------------------------------------------
    def log_mel(self, waves: torch.Tensor) -> torch.Tensor:
        """waves f32 [B, N] (480000 = PCM padded / truncated to 30 s; any multiple of 160 for a whole recording) ->
        input_features f32 [B, mels, N / 160] on the GPU."""
        B, N = waves.shape
        x = waves.to(self.device, torch.float32).contiguous()
        out = torch.empty(B, self.s.num_mel_bins, N // HOP, dtype=torch.float32, device=self.device)
        ws = torch.empty(ops.logmel_workspace_bytes(B), dtype=torch.uint8, device=self.device)
        ops.logmel(x, self.mel_filters, out, ws, B, N, self.s.num_mel_bins)
        return out

    # ---- shared pieces -----------------------------------------------------------------------
    def encoder_stem(self, x, w, h, pre=(None, None), mask_time=None, mask_feature=None):
        """x f32 [B, mels, 3000] -> h = gelu(conv2(gelu(conv1(x)))) + positions, bf16 [B*1500, d].  w["xin"] / w["c1"]:
        the time-padded channels-last input and conv1's output ([B, 3002, mels | d] + 64).  pre: where the training
        forward keeps the two pre-activations (None: not written); mask_time / mask_feature: SpecAugment masks on the
        device, u8 [B, 3000] / [B, mels]."""
        s, st = self.s, self.store
        o = st.off
        B, mels, Tin = x.shape
        T, d = s.max_source_positions, s.d_model
        # channels-last, time-padded input: rows 1..3000 of each clip hold the frames
        for b in range(B):
            ops.transpose_f32_bf16(x[b], w["xin"][(b * (Tin + 2) + 1) * mels:], mels, Tin)
            if mask_time is not None or mask_feature is not None:  # SpecAugment on the input features
                tm = mask_time[b:b + 1].contiguous() if mask_time is not None else None
                fm = mask_feature[b:b + 1].contiguous() if mask_feature is not None else None
                ops.mask_frames(w["xin"][(b * (Tin + 2) + 1) * mels:], tm, fm, self.zero_mel, None, 1, Tin, mels)
        # conv1 (k=3, p=1) + GELU -> padded [B, 3002, d]
        ops.gemm(w["xin"], self.conv1_wr, pre[0], C2=w["c1"], c_off=d, c2_off=d, M=Tin, N=d, K=3 * mels, lda=mels,
                 ldb=3 * mels, ldc=d, bias=st.p32, bias_off=o("model.encoder.conv1.bias"), epilogue=EPI_GELU, batch2=B,
                 sA=(0, (Tin + 2) * mels), sC=(0, (Tin + 2) * d))
        # conv2 (k=3, s=2, p=1) + GELU + sinusoidal positions
        ops.gemm(w["c1"], self.conv2_wr, pre[1], C2=h, M=T, N=d, K=3 * d, lda=2 * d, ldb=3 * d, ldc=d, bias=st.p32,
                 bias_off=o("model.encoder.conv2.bias"), epilogue=EPI_GELU_RESIDUAL, R=st.p16,
                 r_off=o("model.encoder.embed_positions.weight"), ldr=d, batch2=B, sA=(0, (Tin + 2) * d), sC=(0, T * d),
                 sR=(0, 0))

    def _embed(self, ids, pos, h, M):
        """The decoder's input rows: token + position embeddings of int32 ids / positions on the device."""
        p16, o = self.store.p16, self.store.off
        ops.embed_tokens(p16[o("model.decoder.embed_tokens.weight"):], p16[o("model.decoder.embed_positions.weight"):],
                         ids, pos, h, M, self.s.d_model)

    def _head(self, h, hf, M, logits=None, stats=None, last_of=None):
        """The decoder's final LayerNorm (h -> hf, M rows) and the tied output projection: fp32 logits [rows, Vp] of every
        row, or with last_of=B of the last row of each of B sequences, into `logits` (default: a fresh buffer)."""
        s, st = self.s, self.store
        d, V, Vp = s.d_model, s.vocab_size, _r8(s.vocab_size)
        ops.layernorm_fwd(h, st.view("model.decoder.layer_norm.weight"), st.view("model.decoder.layer_norm.bias"), hf, stats,
                          M, d, s.layer_norm_eps)
        rows, n = (hf, M) if last_of is None else (hf.view(last_of, M // last_of, d)[:, -1, :].contiguous(), last_of)
        if logits is None:
            # (torch.empty: the GEMM writes all V columns, the Vp - V pad columns are never read - no fill kernel per call)
            logits = torch.empty(n, Vp, dtype=torch.float32, device=self.device)
        ops.gemm(rows, st.p16, logits, M=n, N=V, K=d, lda=d, ldb=d, ldc=Vp, b_off=st.off("model.decoder.embed_tokens.weight"))
        return logits

    # ---- encoder -----------------------------------------------------------------------------
    def _encoder_ws(self, B):
        """The stem's buffers, the residual stream and one inference workspace that every layer's blocks reuse."""
        if B in self._enc_ws:
            return self._enc_ws[B]
        s = self.s
        d, T = s.d_model, s.max_source_positions
        z = zeros_on(self.device)
        w = dict(xin=z(B * (2 * T + 2) * s.num_mel_bins + 64), c1=z(B * (2 * T + 2) * d + 64), h=[z(B * T * d), z(B * T * d)],
                 out=z(B * T * d))
        for sa, ff in self.enc_blocks[:1]:  # (every layer's blocks have the same shapes)
            w.update(sa=sa.alloc(B, T, z, train=False), ff=ff.alloc(B * T, z, train=False))
        self._enc_ws[B] = w
        return w

    # ---- fp8 encoder weights (BASELINE.json configs[4]) ------------------------------------------------
    _fp8 = None

    def enable_fp8_encoder(self, on: bool = True):
        """Inference: keep the encoder's q|k|v and fc1 weights as OCP fp8 e4m3 (one scale per matrix) and run those
        two projections of every layer on the fp8 matrix instruction; their inputs are the LayerNorm outputs, which
        ca_layernorm_fwd_fp8 quantises per row in the pass that produces them.  (out_proj and fc2 stay bf16: their
        inputs come out of the attention kernel / the GELU epilogue, where a row is spread over many workgroups.)
        Call again after the weights change."""
        if not on:
            self._fp8 = None
            return
        s, st, dev = self.s, self.store, self.device
        d, f = s.d_model, s.encoder_ffn_dim
        p8 = torch.zeros(st.numel, dtype=torch.uint8, device=dev)
        scales = torch.zeros(2 * s.encoder_layers, dtype=torch.float32, device=dev)
        ws = torch.zeros(1, dtype=torch.float32, device=dev)
        for l in range(s.encoder_layers):
            p = f"model.encoder.layers.{l}."
            for k, (name, n) in enumerate(((p + "self_attn.q_proj.weight", 3 * d * d), (p + "fc1.weight", f * d))):
                off = st.off(name)
                ops.quantize_fp8(st.p16[off:off + n], p8[off:off + n], scales[2 * l + k:2 * l + k + 1], ws, n=n)
        self._fp8 = dict(p8=p8, scales=scales)

    def encode(self, input_features: torch.Tensor) -> torch.Tensor:
        """input_features f32 [B, mels, 3000] -> encoder states bf16 [B, 1500, d]."""
        self._await_all()
        s, st = self.s, self.store
        x = input_features.to(self.device, torch.float32).contiguous()
        B, mels, Tin = x.shape
        T, d = s.max_source_positions, s.d_model
        if mels != s.num_mel_bins or Tin != 2 * T:
            raise ValueError(f"Whisper expects the mel input features to be of shape [B, {s.num_mel_bins}, {2 * T}], "
                             f"but found {tuple(x.shape)}")
        M = B * T
        w = self._encoder_ws(B)
        f8 = self._fp8
        if f8 is not None and "x8" not in w:
            w["x8"] = torch.zeros(M * d, dtype=torch.uint8, device=self.device)
            w["rs"] = torch.zeros(M, dtype=torch.float32, device=self.device)

        def w8(i):  # enable_fp8_encoder's operands of weight matrix i: q|k|v (2l) or fc1 (2l + 1) of layer l
            return dict(w=(f8["p8"], f8["scales"][i:i + 1], w["x8"], w["rs"])) if f8 is not None else None

        h, hmid = w["h"]
        self.encoder_stem(x, w, h)
        for l, (sa, ff) in enumerate(self.enc_blocks):
            sa.forward(h, hmid, w["sa"], B, T, fp8=w8(2 * l))
            ff.forward(hmid, h, w["ff"], M, fp8=w8(2 * l + 1))  # result back in `h`
        ops.layernorm_fwd(h, st.view("model.encoder.layer_norm.weight"), st.view("model.encoder.layer_norm.bias"),
                          w["out"], None, M, d, s.layer_norm_eps)
        return w["out"].view(B, T, d)

    # ---- decoder -----------------------------------------------------------------------------
    def cross_kv(self, enc: torch.Tensor) -> list[torch.Tensor]:
        """Per decoder layer: K|V projections of the encoder states, bf16 [B*1500, 2d] (computed once
        per clip, like the cross-attention cache at $TF/models/whisper/modeling_whisper.py:312-335)."""
        self._await_all()
        B, T, _ = enc.shape
        n = B * T * 2 * self.s.d_model
        return [ca.project_kv(enc, dict(kv=torch.empty(n, dtype=torch.bfloat16, device=self.device)), B, T)
                for _, ca, _ in self.dec_blocks]

    def _decoder_ws(self, B, L):
        key = (B, L)
        if key in self._dec_ws:
            return self._dec_ws[key]
        s = self.s
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        z = zeros_on(self.device)
        w = dict(h=[z(B * L * d), z(B * L * d)], hf=z(B * L * d))
        for sa, ca, ff in self.dec_blocks[:1]:  # (every layer's blocks have the same shapes)
            w.update(sa=sa.alloc(B, L, z, train=False), ca=ca.alloc(B, L, Te, z, train=False), ff=ff.alloc(B * L, z, train=False))
        # one decoded token per clip: the cross-attention may deal a (clip, head)'s 1500 keys to several workgroups
        # (CaAttnDesc.split_ws; it decides by B x H against the CU count)
        w["split"] = ops.attn_split_workspace(B, H, self.device) if L == 1 else None
        self._dec_ws[key] = w
        return w

    def decode(self, input_ids: torch.Tensor, enc: torch.Tensor, kv: list | None = None, last_only: bool = False):
        """Teacher-forced decoder: input_ids [B, L] -> fp32 logits [B, L, V] (or [B, 1, V] for the
        last position only)."""
        self._await_all()
        s, dev = self.s, self.device
        B, L = input_ids.shape
        if L > s.max_target_positions:
            raise ValueError(f"sequence length {L} cannot exceed the maximum allowed length of {s.max_target_positions} tokens")
        M, Te = B * L, s.max_source_positions
        w = self._decoder_ws(B, L)
        kv = kv if kv is not None else self.cross_kv(enc)
        ids = input_ids.to(dev, torch.int32).contiguous().view(-1)
        pos = torch.arange(L, dtype=torch.int32, device=dev).repeat(B)
        h0, h1 = w["h"]
        self._embed(ids, pos, h0, M)
        for l, (sa, ca, ff) in enumerate(self.dec_blocks):
            sa.forward(h0, h1, w["sa"], B, L)
            ca.forward(h1, h0, w["ca"], B, L, Te, kv=kv[l])
            ff.forward(h0, h1, w["ff"], M)
            h0, h1 = h1, h0
        V, Vp = s.vocab_size, _r8(s.vocab_size)
        if last_only:
            return self._head(h0, w["hf"], M, last_of=B).view(B, 1, Vp)[:, :, :V]
        logits = self._last_logits = self._head(h0, w["hf"], M)
        return logits.view(B, L, Vp)[:, :, :V]

    # ---- incremental decoding (self-attention K|V cache) ----------------------------------------
    def new_decode_cache(self, B: int, max_len: int):
        """Per decoder layer a bf16 [B, max_len, 2d] buffer holding K|V of the tokens decoded so far — the
        self-attention half of the cache HF keeps in `EncoderDecoderCache`
        ($TF/models/whisper/modeling_whisper.py:312-335, generation with use_cache)."""
        d = self.s.d_model
        return dict(kv=[torch.zeros(B * max_len * 2 * d, dtype=torch.bfloat16, device=self.device)
                        for _ in range(self.s.decoder_layers)], max_len=max_len, pos=0, B=B)

    def decode_step(self, new_ids: torch.Tensor, cross_kv: list, cache: dict) -> torch.Tensor:
        """Feed `new_ids` [B, n] (the forced prefix at position 0, then one token per call) through the
        decoder, appending their K|V to `cache`; returns fp32 logits [B, V] of the last position.
        Same arithmetic as `decode(...)[:, -1]`: each new query attends to all cached keys."""
        self._await_all()
        s, st = self.s, self.store
        p32, p16, o = st.p32, st.p16, st.off
        dev = self.device
        B, n = new_ids.shape
        pos0, Lmax = cache["pos"], cache["max_len"]
        if B != cache["B"] or pos0 + n > Lmax or pos0 + n > s.max_target_positions:
            raise ValueError("decode cache too small / batch mismatch")
        if pos0 > 0 and n != 1:
            raise ValueError("after the first call tokens are appended one at a time")
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd = d // H
        M = B * n
        w = self._decoder_ws(B, n)
        x, q, ctx, lse = w["ca"]["x"], w["ca"]["q"], w["ca"]["ctx"], w["ca"]["lse"]
        ids = new_ids.to(dev, torch.int32).contiguous().view(-1)
        pos = (torch.arange(n, dtype=torch.int32, device=dev) + pos0).repeat(B)
        h0, h1 = w["h"]
        self._embed(ids, pos, h0, M)
        Lk = pos0 + n
        nqp = (n + 31) // 32 * 32
        for l, (_, _, ff) in enumerate(self.dec_blocks):
            p = f"model.decoder.layers.{l}."
            ckv = cache["kv"][l]
            ops.layernorm_fwd(h0, st.view(p + "self_attn_layer_norm.weight"), st.view(p + "self_attn_layer_norm.bias"),
                              x, None, M, d, s.layer_norm_eps)
            ops.gemm(x, p16, q, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "self_attn.q_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.q_proj.bias"))
            # K|V of the new tokens go straight into the cache rows (batch b, position pos0..)
            ops.gemm(x, p16, ckv, M=n, N=2 * d, K=d, lda=d, ldb=d, ldc=2 * d, c_off=pos0 * 2 * d,
                     b_off=o(p + "self_attn.k_proj.weight"), bias=p32, bias_off=o(p + "self_attn.k_proj.bias__zero"),
                     batch2=B, sA=(0, n * d), sC=(0, Lmax * 2 * d))
            ops.attn_fwd(q, ckv, ckv, ctx, lse, B=B, H=H, Tq=n, Tk=Lk, hd=hd, Tqp=nqp,
                         scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=n * d, skb=Lmax * 2 * d,
                         svb=Lmax * 2 * d, sob=n * d, k_off=0, v_off=d, causal=(n > 1))
            ops.gemm(ctx, p16, h1, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "self_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h0, ldr=d)
            ops.layernorm_fwd(h1, st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                              x, None, M, d, s.layer_norm_eps)
            ops.gemm(x, p16, q, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "encoder_attn.q_proj.weight"),
                     bias=p32, bias_off=o(p + "encoder_attn.q_proj.bias"))
            ops.attn_fwd(q, cross_kv[l], cross_kv[l], ctx, lse, B=B, H=H, Tq=n, Tk=Te, hd=hd,
                         Tqp=nqp, scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=n * d, skb=Te * 2 * d,
                         svb=Te * 2 * d, sob=n * d, k_off=0, v_off=d)
            ops.gemm(ctx, p16, h0, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "encoder_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "encoder_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h1, ldr=d)
            ff.forward(h0, h1, w["ff"], M)
            h0, h1 = h1, h0
        logits = self._head(h0, w["hf"], M, last_of=B)
        cache["pos"] = Lk
        return logits[:, :s.vocab_size]

    # ---- one-token step with static shapes and pointers (capturable in a HIP graph) -----------------
    def _graph_state(self, cache: dict, cross_kv: list, pad_id: int, eos_id: int):
        """Static buffers of the per-token step: everything that changes from token to token (position,
        cached length, token ids, finished flags) lives in device memory, so the launch sequence is
        identical for every token and can be replayed as one graph."""
        B, Lmax, dev = cache["B"], cache["max_len"], self.device
        s = self.s
        st = dict(
            tok=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev),
            klen=torch.zeros(B, dtype=torch.int32, device=dev), cur=torch.zeros(1, dtype=torch.int64, device=dev),
            done=torch.zeros(B, dtype=torch.bool, device=dev), nxt=torch.zeros(B, dtype=torch.int32, device=dev),
            out=torch.full((B, Lmax), pad_id, dtype=torch.int64, device=dev),
            logits=torch.zeros(B, _r8(s.vocab_size), dtype=torch.float32, device=dev),
            kvnew=torch.zeros(B * 2 * s.d_model, dtype=torch.bfloat16, device=dev),
            rows=torch.arange(B, device=dev), pad=torch.full((B,), pad_id, dtype=torch.int32, device=dev), pad_id=pad_id,
            eos=eos_id, cross=cross_kv)
        return st

    def _persistent_state(self, cache: dict, g: dict, suppress: torch.Tensor):
        """Descriptor + device tables of ca_whisper_decode_token for this decode state, or None where the launch
        sequence stays (shape / device outside the kernel's limits, CA_DECODE_PERSISTENT=0).  Decoding with timestamps
        (g["ts"]) always keeps the launch sequence: the one-launch kernel's pick is the plain masked argmax
        (csrc/decode.hip), the timestamp rules live in ca_argmax_timestamps_advance."""
        if "persist" in g:
            return g["persist"]
        if g.get("ts") is not None or g.get("scored") is not None:  # (the scored pick is a launch of its own as well)
            g["persist"] = None
            return None
        s, st = self.s, self.store
        B, Lmax = cache["B"], cache["max_len"]
        d, f, H, V = s.d_model, s.decoder_ffn_dim, s.decoder_attention_heads, s.vocab_size
        g["persist"] = None
        if os.environ.get("CA_DECODE_PERSISTENT", "1") == "0" or d != 64 * H or getattr(self, "_persistent_off", False):
            return None
        if not ops.whisper_decode_token_supported(B, d, f, H, V):
            return None
        p16, p32, o = st.p16.data_ptr(), st.p32.data_ptr(), st.off
        w16 = lambda n: p16 + 2 * o(n)  # noqa: E731
        w32 = lambda n: p32 + 4 * o(n)  # noqa: E731
        # the encoder K|V head-major for the launch's cross-attention: a (clip, head)'s keys / values as two contiguous
        # strips instead of 128-byte columns of 4 KB rows (one copy per generate: ~1 ms at 16 clips; CA_DECODE_CROSS_HM=0
        # keeps the [B, Te, 2d] buffers)
        Te = s.max_source_positions
        hm = os.environ.get("CA_DECODE_CROSS_HM", "1") != "0"
        cross = [c.view(B, Te, 2, H, 64).permute(0, 2, 3, 1, 4).contiguous() for c in g["cross"]] if hm else g["cross"]
        rows = []
        for l in range(s.decoder_layers):
            p = f"model.decoder.layers.{l}."
            rows.append([
                w32(p + "self_attn_layer_norm.weight"), w32(p + "self_attn_layer_norm.bias"),
                w16(p + "self_attn.q_proj.weight"), w32(p + "self_attn.q_proj.bias"),
                w16(p + "self_attn.out_proj.weight"), w32(p + "self_attn.out_proj.bias"),
                w32(p + "encoder_attn_layer_norm.weight"), w32(p + "encoder_attn_layer_norm.bias"),
                w16(p + "encoder_attn.q_proj.weight"), w32(p + "encoder_attn.q_proj.bias"),
                w16(p + "encoder_attn.out_proj.weight"), w32(p + "encoder_attn.out_proj.bias"),
                w32(p + "final_layer_norm.weight"), w32(p + "final_layer_norm.bias"),
                w16(p + "fc1.weight"), w32(p + "fc1.bias"), w16(p + "fc2.weight"), w32(p + "fc2.bias"),
                cache["kv"][l].data_ptr(), cross[l].data_ptr()])
        assert len(rows[0]) == len(_lib.CaDecodeLayer.FIELDS)
        table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        nbytes = _lib.decode_ws_bytes(B, d, f, H, s.decoder_layers)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        status = torch.zeros(4, dtype=torch.int32, device=self.device)
        dsc = _lib.CaDecodeDesc()
        dsc.layers, dsc.n_layers, dsc.B, dsc.d, dsc.f, dsc.H = table.data_ptr(), s.decoder_layers, B, d, f, H
        dsc.Te, dsc.max_len, dsc.V = s.max_source_positions, Lmax, V
        dsc.embed, dsc.embed_pos = w16("model.decoder.embed_tokens.weight"), w16("model.decoder.embed_positions.weight")
        dsc.lnf_g, dsc.lnf_b = w32("model.decoder.layer_norm.weight"), w32("model.decoder.layer_norm.bias")
        dsc.eps = s.layer_norm_eps
        dsc.logits, dsc.ld_logits = g["logits"].data_ptr(), g["logits"].stride(0)
        dsc.suppress = suppress.data_ptr()
        dsc.out, dsc.done, dsc.ids, dsc.ld_ids = g["nxt"].data_ptr(), g["done"].data_ptr(), g["out"].data_ptr(), g["out"].stride(0)
        dsc.tok, dsc.pos, dsc.klen = g["tok"].data_ptr(), g["pos"].data_ptr(), g["klen"].data_ptr()
        dsc.pad_id, dsc.eos_id = g["pad_id"], g["eos"]
        dsc.ws, dsc.ws_bytes, dsc.status = ws.data_ptr(), nbytes, status.data_ptr()
        dsc.cross_head_major = 1 if hm else 0
        g["persist"] = dict(desc=dsc, table=table, ws=ws, status=status, suppress=suppress, cross=cross)
        return g["persist"]

    def _token_step(self, cache: dict, g: dict, suppress: torch.Tensor):
        """Decode the token in g["tok"] at position g["pos"], pick the next one (masked argmax), record it.
        Up to 16 clips: ONE persistent launch (ca_whisper_decode_token, csrc/decode.hip; bit-identical to the launch
        sequence below, which larger batches keep)."""
        ps = self._persistent_state(cache, g, suppress)
        if ps is not None:
            ops.whisper_decode_token(ps["desc"])
            return
        self._token_step_launches(cache, g, suppress)

    def _token_step_launches(self, cache: dict, g: dict, suppress: torch.Tensor):
        """The same step as a sequence of ~7 launches per layer."""
        s, st = self.s, self.store
        p32, p16, o = st.p32, st.p16, st.off
        B, Lmax = cache["B"], cache["max_len"]
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd = d // H
        w = self._decoder_ws(B, 1)
        x, q, ctx, lse = w["ca"]["x"], w["ca"]["q"], w["ca"]["ctx"], w["ca"]["lse"]
        # LayerNorm + query projection inside the cross-attention launch: every (clip, head) workgroup streams its head's
        # 64 x d slice of Wq in its prologue (128 KB at d = 1024, a third of the K|V it then streams) - worth it while the
        # launch is short of workgroups (32 clips x 16 heads = 2 per CU: 3.05 against 3.14 ms per token), not above (64
        # clips: 4.17 against 4.02, 128: 7.34 against 6.96; round 5).  CA_DECODE_FUSED = 0 / 1 forces either.
        fz = os.environ.get("CA_DECODE_FUSED")
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
        fused = (fz != "0" if fz is not None else B * H <= 2 * ncu) and hd <= 64 and d <= 2048
        h0, h1 = w["h"]
        self._embed(g["tok"], g["pos"], h0, B)
        for l, (_, _, ff) in enumerate(self.dec_blocks):
            p = f"model.decoder.layers.{l}."
            ckv = cache["kv"][l]
            ln_in = LN_IN_GEMM and B <= 128 and d <= 2048
            if not ln_in:
                ops.layernorm_fwd(h0, st.view(p + "self_attn_layer_norm.weight"), st.view(p + "self_attn_layer_norm.bias"),
                                  x, None, B, d, s.layer_norm_eps)
            # q and the new K|V rows from one launch over the adjacent q|k|v weights: q to its buffer, K|V straight
            # into the cache at the device-side position (CaGemmDesc.c_split_n / c_row_index: the position is data,
            # not a launch argument, so the launch sequence can be replayed as a graph); the LayerNorm in front of it
            # in the same launch's prologue (CaGemmDesc.a_ln_gamma)
            ops.gemm(h0 if ln_in else x, p16, q, M=B, N=3 * d, K=d, lda=d, ldb=d, ldc=d,
                     b_off=o(p + "self_attn.q_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.q_proj.bias"), c_split_n=d, C_hi=ckv, ldc_hi=2 * d,
                     c_row_index=g["pos"], c_row_mul=Lmax,
                     a_ln=(st.view(p + "self_attn_layer_norm.weight"), st.view(p + "self_attn_layer_norm.bias"),
                           s.layer_norm_eps) if ln_in else None)
            ops.attn_fwd(q, ckv, ckv, ctx, lse, B=B, H=H, Tq=1, Tk=Lmax, hd=hd, Tqp=32,
                         scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=d, skb=Lmax * 2 * d,
                         svb=Lmax * 2 * d, sob=d, k_off=0, v_off=d, klen=g["klen"])
            ops.gemm(ctx, p16, h1, M=B, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "self_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h0, ldr=d)
            if fused:
                # LayerNorm + query projection + attention over the cached encoder K|V: one launch (bit-identical to
                # the three below; CA_DECODE_FUSED=0 keeps them)
                ops.decode_attn_qproj(h1, st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                                      p16, p32, g["cross"][l], g["cross"][l], ctx, d_model=d, eps=s.layer_norm_eps,
                                      ldx=d, ldw=d, w_off=o(p + "encoder_attn.q_proj.weight"),
                                      bias_off=o(p + "encoder_attn.q_proj.bias"), B=B, H=H, Tk=Te, hd=hd,
                                      scale=hd ** -0.5, ldk=2 * d, ldv=2 * d, ldo=d, skb=Te * 2 * d, svb=Te * 2 * d,
                                      sob=d, k_off=0, v_off=d, split_ws=w["split"])
            else:
                if not ln_in:
                    ops.layernorm_fwd(h1, st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                                      x, None, B, d, s.layer_norm_eps)
                ops.gemm(h1 if ln_in else x, p16, q, M=B, N=d, K=d, lda=d, ldb=d, ldc=d,
                         b_off=o(p + "encoder_attn.q_proj.weight"), bias=p32, bias_off=o(p + "encoder_attn.q_proj.bias"),
                         a_ln=(st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                               s.layer_norm_eps) if ln_in else None)
                ops.attn_fwd(q, g["cross"][l], g["cross"][l], ctx, lse, B=B, H=H, Tq=1, Tk=Te,
                             hd=hd, Tqp=32, scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=d, skb=Te * 2 * d,
                             svb=Te * 2 * d, sob=d, k_off=0, v_off=d, split_ws=w["split"])
            ops.gemm(ctx, p16, h0, M=B, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "encoder_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "encoder_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h1, ldr=d)
            ff.forward(h0, h1, w["ff"], B)
            h0, h1 = h1, h0
        self._head(h0, w["hf"], B, logits=g["logits"])
        V, Vp = s.vocab_size, _r8(s.vocab_size)
        # argmax + the step's bookkeeping in one launch: out[b, pos + 1] = the token (pad for finished rows), done |= eos,
        # tok = the token, pos += 1, klen += 1
        if g.get("scored") is not None:  # greedy or sampled, with the token's log-probability (csrc/sample.hip)
            sc = g["scored"]
            ops.pick_scored_advance(g["logits"], suppress, g["nxt"], B, V, Vp, sc["inv_t"], sc["uniforms"], sc["sum_logprob"],
                                    sc["n_scored"], g["done"], g["out"], g["tok"], g["pos"], g["klen"], g["pad_id"], g["eos"],
                                    timestamps=g.get("ts"))
            return
        if g.get("ts") is not None:  # the same step under the timestamp rules (history: g["out"] up to g["pos"])
            begin, tb, cap = g["ts"]
            ops.argmax_timestamps_advance(g["logits"], suppress, g["nxt"], B, V, Vp, g["done"], g["out"], g["tok"], g["pos"],
                                          g["klen"], g["pad_id"], g["eos"], begin, tb, cap)
            return
        ops.argmax_advance(g["logits"], suppress, g["nxt"], B, V, Vp, g["done"], g["out"], g["tok"], g["pos"], g["klen"],
                           g["pad_id"], g["eos"])

    # ---- model-level API -------------------------------------------------------------------------
    def forward(self, input_features, labels=None, decoder_input_ids=None):
        """-> dict(loss, logits): `WhisperForConditionalGeneration.forward(input_features, labels)`."""
        s = self.s
        enc = self.encode(input_features)
        if decoder_input_ids is None:
            if labels is None:
                raise ValueError("either labels or decoder_input_ids is required")
            decoder_input_ids = shift_tokens_right(labels, s.pad_token_id, s.decoder_start_token_id)
        logits = self.decode(decoder_input_ids, enc)
        out = dict(logits=logits, loss=None, encoder_last_hidden_state=enc)
        if labels is not None:
            B, L = labels.shape
            lab = labels.to(self.device, torch.int32).contiguous().view(-1)
            loss_sum = torch.zeros(1, dtype=torch.float32, device=self.device)
            count = torch.zeros(1, dtype=torch.int32, device=self.device)
            ops.cross_entropy_fwd_bwd(self._last_logits, lab, loss_sum, count, None, B * L, s.vocab_size,
                                      _r8(s.vocab_size), -100)
            out["loss"] = (loss_sum / count.clamp(min=1).to(torch.float32))[0]
        return out

    def generate(self, input_features, prefix: list[int], max_length: int, suppress_tokens=None,
                 begin_suppress_tokens=None, use_cache: bool = True, use_graph: bool = True, num_beams: int = 1,
                 length_penalty: float = 1.0, early_stopping: bool = False, return_trace: bool = False,
                 _beam_path: bool = False, return_timestamps: bool = False, timestamp_begin: int | None = None,
                 max_initial_timestamp_index: int | None = None, return_token_timestamps: bool = False,
                 alignment_heads=None, num_frames=None, median_filter_width: int = 7, temperature: float = 0.0,
                 sample_uniforms=None, return_stats: bool = False, no_speech_token: int | None = None, cross_kv=None):
        """Greedy decoding with a forced prefix (<|sot|><|da|><|transcribe|><|notimestamps|> in CoRal's
        evaluation): masked argmax on the GPU (ca_argmax_masked), stop at EOS / max_length.
        num_beams = k >= 2: beam search (`_generate_beam`; length_penalty, early_stopping True / False as in
        transformers); return_trace=True then returns (ids, trace).  num_beams = 1 is the greedy code, untouched
        (_beam_path=True routes it through the beam launches instead: a test switch).
        return_timestamps=True: greedy decoding under WhisperTimeStampLogitsProcessor's rules (ca_argmax_timestamps; the
        prefix then has no <|notimestamps|>, `timestamp_begin` is that token's id + 1, `max_initial_timestamp_index` the
        generation config's or None).  Not with beams; the one-launch-per-token kernel is bypassed.
        return_token_timestamps=True (with return_timestamps=True, greedy only): -> (ids, times), times float32 seconds
        [B, len(ids[0])] from the cross-attention of `alignment_heads` [(layer, head)] and dynamic time warping
        (`token_timestamps`); num_frames: valid log-mel frames per clip (None: all).
        temperature > 0: every pick is sampled by inverse CDF at that temperature on `sample_uniforms` (float32
        [B, max_length], the uniform of position p in column p; ca_pick_scored_advance).  return_stats=True: -> (ids,
        dict(sum_logprob, n_scored, no_speech_prob)) per clip: the log-probabilities of the generated tokens (EOS included)
        under the processed distribution at temperature 1 and their count; with `no_speech_token`, the probability of that
        id at the first prefix position.  Either keeps the launch sequence (graph-captured per token); not with beams.
        cross_kv: the result of `cross_kv(encode(...))` (or `gather_cross_kv` of it) - the encoder is then not run and
        input_features may be None."""
        s, dev = self.s, self.device
        beam = num_beams != 1 or _beam_path
        ts = None
        scored = None
        if temperature is None or not isinstance(temperature, (int, float)) or isinstance(temperature, bool) \
                or not math.isfinite(temperature) or temperature < 0:
            raise ValueError(f"temperature must be a non-negative finite number, got {temperature!r}")
        if temperature > 0 or return_stats or no_speech_token is not None:
            if beam:
                what = f"temperature={temperature}" if temperature > 0 else "return_stats=True"
                raise ValueError(f"generate(num_beams={num_beams}): {what} is not implemented with beam search")
            if return_token_timestamps:
                raise ValueError("return_token_timestamps=True is not implemented with temperature > 0 / return_stats=True")
            if not use_cache:
                raise ValueError("temperature > 0 / return_stats=True need use_cache=True")
            if max_length <= len(prefix) or max_length > s.max_target_positions:
                raise ValueError(f"temperature > 0 / return_stats=True need len(prefix) < max_length <= "
                                 f"{s.max_target_positions}, got {max_length}")
            if temperature > 0:
                if sample_uniforms is None:
                    raise ValueError(f"temperature={temperature} needs sample_uniforms, float32 [clips, max_length]")
                if sample_uniforms.dim() != 2 or sample_uniforms.shape[1] < max_length:
                    raise ValueError(f"sample_uniforms must be [clips, >= max_length], got {tuple(sample_uniforms.shape)}")
            if no_speech_token is not None and not 0 <= no_speech_token < s.vocab_size:
                raise ValueError(f"no_speech_token={no_speech_token} lies outside the vocabulary")
            scored = dict(inv_t=float(np.float32(1.0 / temperature)) if temperature > 0 else 0.0,
                          uniforms=sample_uniforms if temperature > 0 else None, no_speech_token=no_speech_token,
                          use_graph=use_graph)
        if return_token_timestamps:
            from .whisper_align import check_alignment_heads

            if beam:
                raise ValueError(f"generate(num_beams={num_beams}): return_token_timestamps=True is not implemented with beam "
                                 "search")
            if not return_timestamps:
                raise ValueError("return_token_timestamps=True needs return_timestamps=True (the word mode of the ASR pipeline "
                                 "sets both)")
            alignment_heads = check_alignment_heads(alignment_heads, s.decoder_layers, s.decoder_attention_heads)
        if return_timestamps:
            if beam:
                raise ValueError(f"generate(num_beams={num_beams}): return_timestamps=True is not implemented with beam search")
            if timestamp_begin is None or not 0 <= s.eos_token_id < timestamp_begin <= s.vocab_size:
                raise ValueError(f"return_timestamps=True needs timestamp_begin (<|notimestamps|> + 1) with eos_token_id < "
                                 f"timestamp_begin <= vocab_size, got {timestamp_begin!r}")
            if max_initial_timestamp_index is not None and max_initial_timestamp_index < 0:
                raise ValueError(f"max_initial_timestamp_index must be None or >= 0, got {max_initial_timestamp_index}")
            if max_length > s.max_target_positions:
                raise ValueError(f"max_length {max_length} exceeds the {s.max_target_positions} target positions")
            ts = (len(prefix), int(timestamp_begin), max_initial_timestamp_index)
        if beam:
            check_beam_arguments(int(input_features.shape[0]), num_beams, length_penalty, early_stopping, {})
            if max_length <= len(prefix) or max_length > s.max_target_positions:
                raise ValueError(f"beam search needs len(prefix) < max_length <= {s.max_target_positions}, got {max_length}")
            if s.d_model // s.decoder_attention_heads > 64:
                raise ValueError("beam search needs head_dim <= 64 (the single-query attention kernel reads the cache "
                                 "through CaAttnDesc.key_slot)")
        elif return_trace:
            raise ValueError("return_trace is a beam search option (num_beams >= 2)")
        if cross_kv is not None:
            if not use_cache:
                raise ValueError("cross_kv= needs use_cache=True (the pass without a cache reads the encoder states)")
            kv, enc = cross_kv, None
            B = kv[0].numel() // (s.max_source_positions * 2 * s.d_model)
        else:
            enc = self.encode(input_features)
            kv = self.cross_kv(enc)
            B = enc.shape[0]
        V = s.vocab_size
        sup = torch.zeros(V, dtype=torch.uint8, device=dev)
        if suppress_tokens:
            sup[torch.tensor(list(suppress_tokens), device=dev)] = 1
        sup_begin = sup.clone()
        if begin_suppress_tokens:
            sup_begin[torch.tensor(list(begin_suppress_tokens), device=dev)] = 1
        if beam:
            return self._generate_beam(kv, prefix, max_length, sup, sup_begin, num_beams, float(length_penalty),
                                       bool(early_stopping), return_trace, use_graph)
        if scored is not None:
            if temperature > 0 and sample_uniforms.shape[0] != B:
                raise ValueError(f"sample_uniforms has {sample_uniforms.shape[0]} rows for {B} clips")
            rows = self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts, scored)
            stats = dict(sum_logprob=scored["sum_logprob"].cpu().tolist(), n_scored=scored["n_scored"].cpu().tolist(),
                         no_speech_prob=scored["no_speech_prob"].cpu().tolist() if no_speech_token is not None else None)
            return (rows, stats) if return_stats else rows
        if use_cache and use_graph and max_length > len(prefix) + 2:
            rows = self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts)
            if return_token_timestamps:
                return rows, self.token_timestamps(rows, kv, len(prefix), alignment_heads, num_frames, median_filter_width)
            return rows
        ids = torch.tensor([prefix] * B, dtype=torch.int64, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        nxt = torch.empty(B, dtype=torch.int32, device=dev)
        cache = self.new_decode_cache(B, max_length) if use_cache else None
        feed = ids
        while ids.shape[1] < max_length and not bool(done.all()):
            if use_cache:
                base = self.decode_step(feed, kv, cache).contiguous()  # fp32 [B, V]
            else:
                base = self.decode(ids, enc, kv, last_only=True)[:, 0, :].contiguous()
            mask = sup_begin if ids.shape[1] == len(prefix) else sup
            if ts is None:
                ops.argmax_masked(base, mask, nxt, B, V, V)
            else:
                pos = torch.full((B,), ids.shape[1] - 1, dtype=torch.int32, device=dev)
                ops.argmax_timestamps(base, mask, nxt, B, V, V, ids, pos, ts[0], ts[1], s.eos_token_id, ts[2])
            step = torch.where(done, torch.full_like(nxt, s.pad_token_id), nxt).to(torch.int64)
            ids = torch.cat([ids, step[:, None]], 1)
            feed = step[:, None]
            done |= step == s.eos_token_id
        if return_token_timestamps:
            rows = ids.tolist()
            return rows, self.token_timestamps(rows, kv, len(prefix), alignment_heads, num_frames, median_filter_width)
        return ids.tolist()

    # ---- token timestamps (cross-attention alignment + DTW) ------------------------------------------------------------
    def alignment_queries(self, ids, kv: list, heads: list, prefix_len: int) -> torch.Tensor:
        """One teacher-forced decoder pass over ids [B, L] with `decode`'s launch sequence, up to the last alignment
        layer's cross-attention: -> bf16 [A, B, L - prefix_len, head_dim], the queries of the alignment heads at the
        positions that consume tokens prefix_len .. L-1 (w["ca"]["q"] after CrossAttnBlock.forward of their layer)."""
        self._await_all()
        s, dev = self.s, self.device
        ids = torch.as_tensor(ids)
        B, L = ids.shape
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd, M = d // H, B * L
        # L changes from batch to batch: a workspace made for this pass is not kept (`_dec_ws` never evicts)
        fresh = (B, L) not in self._dec_ws
        w = self._decoder_ws(B, L)
        if fresh:
            del self._dec_ws[(B, L)]
        flat = ids.to(dev, torch.int32).contiguous().view(-1)
        pos = torch.arange(L, dtype=torch.int32, device=dev).repeat(B)
        h0, h1 = w["h"]
        self._embed(flat, pos, h0, M)
        q = torch.empty(len(heads), B, L - prefix_len, hd, dtype=torch.bfloat16, device=dev)
        last = max(l for l, _ in heads)
        for l, (sa, ca, ff) in enumerate(self.dec_blocks):
            sa.forward(h0, h1, w["sa"], B, L)
            ca.forward(h1, h0, w["ca"], B, L, Te, kv=kv[l])
            ql = w["ca"]["q"][:M * d].view(B, L, H, hd)
            for a, (la, h) in enumerate(heads):
                if la == l:
                    q[a].copy_(ql[:, prefix_len:, h, :])
            if l == last:
                break
            ff.forward(h0, h1, w["ff"], M)
            h0, h1 = h1, h0
        return q

    def token_timestamps(self, rows, kv: list, prefix_len: int, alignment_heads, num_frames=None,
                         median_filter_width: int = 7, return_parts: bool = False):
        """`WhisperGenerationMixin._extract_token_timestamps` for generated id rows [B, Ltot] (prefix included, padded as
        `generate` pads): the DTW tokens are the input positions prefix_len .. Ltot-2.  -> float32 seconds [B, Ltot];
        return_parts: (times, dict(cost, jump, frames)) with the device tensors of the two kernels."""
        from .whisper_align import check_align_limits, check_alignment_heads, frames_of, times_from_jumps

        s, dev = self.s, self.device
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd = d // H
        heads = check_alignment_heads(alignment_heads, s.decoder_layers, H)
        ids = torch.as_tensor(rows)
        B, Ltot = ids.shape
        Lw = Ltot - 1 - prefix_len
        frames = frames_of(num_frames, B, Te)
        Fmax = max(frames)
        check_align_limits(len(heads), Lw, Fmax, hd, Te, median_filter_width)
        if Lw <= 0:
            times = times_from_jumps(np.zeros((B, 0), dtype=np.int32), prefix_len, Ltot)
            return (times, dict(cost=None, jump=None, frames=frames)) if return_parts else times
        q = self.alignment_queries(ids[:, :Ltot - 1], kv, heads, prefix_len)
        fdev = torch.tensor(frames, dtype=torch.int32).to(dev)
        cost = ops.whisper_align_cost(q, kv, heads, B, Lw, Te, H, hd, 2 * d, Te * 2 * d, fdev, Fmax, hd ** -0.5,
                                      median_filter_width)
        jump = ops.dtw_token_times(cost, fdev)
        times = times_from_jumps(jump.cpu().numpy(), prefix_len, Ltot)
        return (times, dict(cost=cost, jump=jump, frames=frames)) if return_parts else times

    def gather_cross_kv(self, kv: list, rows) -> list:
        """The cross K|V of a subset of the clips of `cross_kv`'s result (a fallback attempt decodes the rows that failed
        against the K|V of the window's one encoder pass)."""
        n = self.s.max_source_positions * 2 * self.s.d_model
        idx = torch.as_tensor(list(rows), dtype=torch.int64, device=self.device)
        return [c.view(-1, n).index_select(0, idx).reshape(-1) for c in kv]

    def _generate_graph(self, kv, prefix, max_length, sup, sup_begin, ts=None, scored=None):
        """Greedy loop with the per-token step captured once in a HIP graph and replayed: the ~350 small
        launches of a token (24-32 layers x 14 kernels) cost one graph launch instead of 350 host calls."""
        s, dev = self.s, self.device
        B, V, P = kv[0].shape[0] // (s.max_source_positions * 2 * s.d_model), s.vocab_size, len(prefix)
        cache = self.new_decode_cache(B, max_length)
        g = self._graph_state(cache, kv, s.pad_token_id, s.eos_token_id)
        g["ts"] = ts  # (begin_index, timestamp_begin, max_initial_timestamp_index) or None
        # the forced prefix and the first free token run eagerly (different shapes / begin-suppress mask)
        ids0 = torch.tensor([prefix] * B, dtype=torch.int64, device=dev)
        base = self.decode_step(ids0, kv, cache).contiguous()
        if scored is not None:
            g["scored"] = scored
            scored["sum_logprob"] = torch.zeros(B, dtype=torch.float32, device=dev)
            scored["n_scored"] = torch.zeros(B, dtype=torch.int32, device=dev)
            if scored["uniforms"] is not None:
                scored["uniforms"] = scored["uniforms"].to(dev, torch.float32).contiguous()
            if scored["no_speech_token"] is not None:
                # WhisperNoSpeechDetection: the softmax of the raw logits at the start-of-transcript position, i.e. the
                # head on prefix position 0 (decode_step left the final LayerNorm of every prefix row in the workspace)
                hf0 = self._decoder_ws(B, P)["hf"][:B * P * s.d_model].view(B, P, s.d_model)[:, 0, :].contiguous()
                lg0 = torch.empty(B, _r8(V), dtype=torch.float32, device=dev)
                ops.gemm(hf0, self.store.p16, lg0, M=B, N=V, K=s.d_model, lda=s.d_model, ldb=s.d_model, ldc=_r8(V),
                         b_off=self.store.off("model.decoder.embed_tokens.weight"))
                scored["no_speech_prob"] = torch.empty(B, dtype=torch.float32, device=dev)
                ops.row_token_prob(lg0, scored["no_speech_prob"], B, V, _r8(V), scored["no_speech_token"])
            # the first free token through the scored pick as well (its log-probability counts): the books stand at the
            # last prefix token
            g["out"][:, :P] = ids0
            g["pos"].fill_(P - 1)
            g["klen"].fill_(P)
            ops.pick_scored_advance(base, sup_begin, g["nxt"], B, V, V, scored["inv_t"], scored["uniforms"],
                                    scored["sum_logprob"], scored["n_scored"], g["done"], g["out"], g["tok"], g["pos"], g["klen"],
                                    s.pad_token_id, s.eos_token_id, timestamps=ts)
        elif ts is None:
            ops.argmax_masked(base, sup_begin, g["nxt"], B, V, V)
        else:  # (an empty history: only the prefix length matters)
            ops.argmax_timestamps(base, sup_begin, g["nxt"], B, V, V, ids0, torch.full((B,), P - 1, dtype=torch.int32, device=dev),
                                  ts[0], ts[1], s.eos_token_id, ts[2])
        if scored is None:
            g["out"][:, :P] = ids0
            g["out"][:, P] = g["nxt"].long()
            g["done"] |= g["nxt"] == s.eos_token_id
            g["tok"].copy_(g["nxt"])
            g["pos"].fill_(P)
            g["klen"].fill_(P + 1)
        g["cur"].fill_(P + 1)
        n_done = P + 1
        if n_done < max_length and not bool(g["done"].all()):
            self._token_step(cache, g, sup)  # eager warm-up of the captured sequence (allocations, attributes)
            n_done += 1
        graphs = {}

        def replay(n):  # n token steps as ONE graph (capture records the launches without running them)
            if scored is not None and not scored["use_graph"]:
                return self._token_step(cache, g, sup)
            if n not in graphs:
                torch.cuda.synchronize()
                graphs[n] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[n]):
                    for _ in range(n):
                        self._token_step(cache, g, sup)
            graphs[n].replay()

        # with one launch per token a graph of eight tokens is 8 kernels + 8 memset nodes: the gap between two graph
        # launches (~10-16 us) is paid once per eight tokens, like the host's all-finished check
        persist = g.get("persist") is not None
        chunk = 8 if persist else 1
        # The all-finished check.  Launch sequence: synchronous, every 8 tokens (the host waits, looks, launches).  One launch
        # per token: the check of a chunk is an asynchronous copy to pinned memory behind it, looked at one chunk LATER, so
        # the next chunk is already queued while the host waits - the device never idles between chunks (the synchronous
        # form cost ~50 us per token at 16 clips).  What the host sees late costs nothing: a launch that finds every clip
        # finished only records pad and returns (decode.hip), and the trimming below cuts those columns off.
        flags = torch.zeros(2, dtype=torch.bool).pin_memory() if persist else None
        pending = []  # (event, slot) of the chunks whose flag has not been looked at
        k = 0
        while n_done < max_length:
            if not persist and (n_done - P) % 8 == 2 and bool(g["done"].all()):  # host check every 8 tokens
                break
            n = chunk if (chunk > 1 and (n_done - P) % 8 == 2 and n_done + chunk <= max_length) else 1
            replay(n)
            n_done += n
            if persist and (n_done - P) % 8 == 2:
                flags[k & 1:(k & 1) + 1].copy_(g["done"].all().view(1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((ev, k & 1))
                k += 1
                if len(pending) == 2:  # the chunk before the one just queued
                    ev0, slot = pending.pop(0)
                    ev0.synchronize()
                    if bool(flags[slot]):
                        break
        out = g["out"][:, :n_done]
        if g.get("persist") is not None:
            code = int(g["persist"]["status"][0])  # (synchronises)
            if code != 0:
                msg = (f"ca_whisper_decode_token gave up at the seam in front of phase {code - 1}: the launch needs every "
                       "CU of the device (nothing else may run beside it)")
                if os.environ.get("CA_DECODE_STRICT") == "1":
                    raise ops.CoralAmdError(msg + "; CA_DECODE_PERSISTENT=0 keeps the launch sequence")
                # a launch that gave up has written no token: the ids above are not a generation.  This engine keeps
                # the launch sequence from here on (same bits) and decodes the batch again.
                import warnings

                warnings.warn("coral_amd: " + msg + "; decoding this batch again as a launch sequence and keeping that "
                              "path for this engine (CA_DECODE_STRICT=1 raises instead)")
                self._persistent_off = True
                return self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts, scored)
        # trim like the eager loop: stop at the first column where every row had already finished
        fin = (out == s.eos_token_id).cumsum(1) > 0
        allfin = fin.all(0)
        keep = n_done
        if bool(allfin.any()):
            keep = int(torch.nonzero(allfin)[0]) + 1
        return out[:, :keep].tolist()

    # ---- beam search ---------------------------------------------------------------------------------------------------
    def _beam_state(self, B, k, Lmax, P, max_length, length_penalty, early_stopping, cross_kv):
        """Device state of the beam search: like `_graph_state`, everything that changes between tokens lives in device
        memory.  The ancestry table `anc` (the cache row that holds position t of beam row r: CaAttnDesc.key_slot) and
        the running ids are double-buffered: step n reads buffer n & 1 and ca_beam_advance writes the other."""
        s, dev = self.s, self.device
        R, V, Vp = B * k, s.vocab_size, _r8(s.vocab_size)
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)  # noqa: E731
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        g = dict(B=B, k=k, tok=i32(R), pos=i32(R), klen=i32(R), run_score=f32(R), logits=f32(R, Vp),
                 anc=[i32(R, Lmax), i32(R, Lmax)], ids=[i32(R, Lmax), i32(R, Lmax)],
                 cand_score=f32(B, 2 * k), cand_parent=i32(B, 2 * k), cand_token=i32(B, 2 * k),
                 fin_score=torch.full((R,), -1.0e9, dtype=torch.float32, device=dev), fin_len=i32(R), fin_seq=i32(R),
                 fin_ids=i32(R, Lmax), fin_count=i32(B), heur=torch.ones(B, dtype=torch.int32, device=dev),
                 done=torch.zeros(B, dtype=torch.bool, device=dev),
                 tr_parent=i32(Lmax, B, k), tr_token=i32(Lmax, B, k), tr_score=f32(Lmax, B, k),
                 len_pen=torch.tensor([float(n) ** length_penalty for n in range(Lmax + 1)], dtype=torch.float32).to(dev),
                 select_ws=torch.zeros(ops.beam_select_workspace_bytes(B, k, V), dtype=torch.uint8, device=dev),
                 # the cross-attention runs with B = clips and Tq = k: the key split is that of B x H items, as in greedy
                 split=ops.attn_split_workspace(B, s.decoder_attention_heads, dev), cross=cross_kv)
        g["desc"] = []
        for par in (0, 1):
            dsc = _lib.CaBeamDesc()
            dsc.B, dsc.k, dsc.max_len, dsc.prompt_len, dsc.max_length = B, k, Lmax, P, max_length
            dsc.eos_id, dsc.early_stopping = s.eos_token_id, int(early_stopping)
            for n in ("len_pen", "cand_score", "cand_parent", "cand_token", "run_score", "tok", "pos", "klen", "fin_score",
                      "fin_len", "fin_seq", "fin_ids", "fin_count", "heur", "done", "tr_parent", "tr_token", "tr_score"):
                setattr(dsc, n, g[n].data_ptr())
            dsc.anc_in, dsc.anc_out = g["anc"][par].data_ptr(), g["anc"][1 - par].data_ptr()
            dsc.ids_in, dsc.ids_out = g["ids"][par].data_ptr(), g["ids"][1 - par].data_ptr()
            g["desc"].append(dsc)
        return g

    def _beam_pick(self, g: dict, suppress: torch.Tensor, par: int):
        """Rank the k x V continuations of every clip and take the step's decisions (tables: buffer par -> 1 - par)."""
        V, Vp = self.s.vocab_size, _r8(self.s.vocab_size)
        ops.beam_select(g["logits"], suppress, g["run_score"], g["B"], g["k"], V, Vp, g["cand_score"], g["cand_parent"],
                        g["cand_token"], g["select_ws"])
        ops.beam_advance(g["desc"][par])

    def _beam_token_step(self, cache: dict, g: dict, suppress: torch.Tensor, par: int):
        """`_token_step_launches` over clips x beams rows with three changes: the self-attention reads the K|V cache through
        the ancestry table (rows are written once, by the beam slot that produced them, and never copied); the
        cross-attention takes a clip's k beams as k queries against the clip's ONE encoder K|V; ca_beam_select +
        ca_beam_advance stand where ca_argmax_advance stood."""
        s, st = self.s, self.store
        p32, p16, o = st.p32, st.p16, st.off
        B, k, Lmax = g["B"], g["k"], cache["max_len"]
        R = B * k
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd = d // H
        w = self._decoder_ws(R, 1)
        x, q, ctx, lse = w["ca"]["x"], w["ca"]["q"], w["ca"]["ctx"], w["ca"]["lse"]
        h0, h1 = w["h"]
        self._embed(g["tok"], g["pos"], h0, R)
        ln_in = LN_IN_GEMM and R <= 128 and d <= 2048
        for l, (_, _, ff) in enumerate(self.dec_blocks):
            p = f"model.decoder.layers.{l}."
            ckv = cache["kv"][l]
            if not ln_in:
                ops.layernorm_fwd(h0, st.view(p + "self_attn_layer_norm.weight"), st.view(p + "self_attn_layer_norm.bias"),
                                  x, None, R, d, s.layer_norm_eps)
            ops.gemm(h0 if ln_in else x, p16, q, M=R, N=3 * d, K=d, lda=d, ldb=d, ldc=d,
                     b_off=o(p + "self_attn.q_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.q_proj.bias"), c_split_n=d, C_hi=ckv, ldc_hi=2 * d,
                     c_row_index=g["pos"], c_row_mul=Lmax,
                     a_ln=(st.view(p + "self_attn_layer_norm.weight"), st.view(p + "self_attn_layer_norm.bias"),
                           s.layer_norm_eps) if ln_in else None)
            ops.attn_fwd(q, ckv, ckv, ctx, lse, B=R, H=H, Tq=1, Tk=Lmax, hd=hd, Tqp=32,
                         scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=d, skb=Lmax * 2 * d,
                         svb=Lmax * 2 * d, sob=d, k_off=0, v_off=d, klen=g["klen"], key_slot=g["anc"][par])
            ops.gemm(ctx, p16, h1, M=R, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "self_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "self_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h0, ldr=d)
            if not ln_in:
                ops.layernorm_fwd(h1, st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                                  x, None, R, d, s.layer_norm_eps)
            ops.gemm(h1 if ln_in else x, p16, q, M=R, N=d, K=d, lda=d, ldb=d, ldc=d,
                     b_off=o(p + "encoder_attn.q_proj.weight"), bias=p32, bias_off=o(p + "encoder_attn.q_proj.bias"),
                     a_ln=(st.view(p + "encoder_attn_layer_norm.weight"), st.view(p + "encoder_attn_layer_norm.bias"),
                           s.layer_norm_eps) if ln_in else None)
            ops.attn_fwd(q, g["cross"][l], g["cross"][l], ctx, lse, B=B, H=H, Tq=k, Tk=Te, hd=hd, Tqp=32,
                         scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=k * d, skb=Te * 2 * d,
                         svb=Te * 2 * d, sob=k * d, k_off=0, v_off=d, split_ws=g["split"])
            ops.gemm(ctx, p16, h0, M=R, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(p + "encoder_attn.out_proj.weight"),
                     bias=p32, bias_off=o(p + "encoder_attn.out_proj.bias"), epilogue=EPI_RESIDUAL, R=h1, ldr=d)
            ff.forward(h0, h1, w["ff"], R)
            h0, h1 = h1, h0
        self._head(h0, w["hf"], R, logits=g["logits"])
        self._beam_pick(g, suppress, par)

    def _generate_beam(self, kv, prefix, max_length, sup, sup_begin, k, length_penalty, early_stopping, return_trace,
                       use_graph=True):
        """Beam search as GenerationMixin._beam_search states it ($TF/generation/utils.py:3208-3508; restated in
        tests/whisper_beam_ref.py), on the launch-sequence path.  The forced prefix runs once per clip into beam slot 0;
        the ancestry table makes it visible to all k slots.  The token step is captured once per table parity and
        replayed; the host looks at the per-clip done flags every 8 tokens, as greedy does.  The ids of the running and
        the finished hypotheses are kept on the device as [clips x k, max_length] tables that ca_beam_advance re-gathers
        with the ancestry rows (the same few KB per step): a finished hypothesis needs its ids at the moment it finishes,
        when its beam may not survive the step, so back-pointers alone would have to keep every step's parents and be
        walked at the end for nothing saved."""
        s, dev = self.s, self.device
        d, Te = s.d_model, s.max_source_positions
        B, V, Vp, P = kv[0].shape[0] // (Te * 2 * d), s.vocab_size, _r8(s.vocab_size), len(prefix)
        R, Lmax = B * k, max_length
        cache = self.new_decode_cache(R, Lmax)
        g = self._beam_state(B, k, Lmax, P, max_length, length_penalty, early_stopping, kv)
        # the forced prefix, eagerly, on B rows: clip b's K|V go to cache row b * k (beam slot 0 of the clip)
        ids0 = torch.tensor([prefix] * B, dtype=torch.int64, device=dev)
        base = self.decode_step(ids0, kv, dict(kv=cache["kv"], max_len=k * Lmax, pos=0, B=B))
        g["logits"].view(B, k, Vp)[:, :, :V] = base[:, None, :]
        slot0 = (torch.arange(R, device=dev, dtype=torch.int32) // k) * k
        g["anc"][0][:, :P] = slot0[:, None]  # no copy: every beam's prefix positions name the clip's slot 0
        g["ids"][0][:, :P] = ids0[0].to(torch.int32)
        g["run_score"].view(B, k)[:, 1:] = -1.0e9  # the first step expands one beam ($TF/generation/utils.py:3332-3333)
        g["pos"].fill_(P - 1)
        g["klen"].fill_(P)
        self._beam_pick(g, sup_begin, 0)  # the first free position: begin-suppress set
        n_done, par = P + 1, 1
        if n_done < max_length and not bool(g["done"].all()):
            self._beam_token_step(cache, g, sup, par)  # eager warm-up of the captured sequence
            n_done, par = n_done + 1, par ^ 1
        graphs = {}

        def replay(par):
            if not use_graph:
                return self._beam_token_step(cache, g, sup, par)
            if par not in graphs:
                torch.cuda.synchronize()
                graphs[par] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[par]):
                    self._beam_token_step(cache, g, sup, par)
            graphs[par].replay()

        while n_done < max_length:
            if (n_done - P) % 8 == 2 and bool(g["done"].all()):  # host check every 8 tokens
                break
            replay(par)
            n_done, par = n_done + 1, par ^ 1
        # the best finished hypothesis of every clip: highest score, of equal scores the one that entered first
        fs, fl = g["fin_score"].view(B, k).cpu(), g["fin_len"].view(B, k).cpu()
        fq, fi = g["fin_seq"].view(B, k).cpu(), g["fin_ids"].view(B, k, Lmax).cpu()
        out, best = [], []
        for b in range(B):
            live = [j for j in range(k) if int(fl[b, j]) > 0]
            if not live:
                raise ops.CoralAmdError("beam search ended without a finished hypothesis")
            j = min(live, key=lambda j: (-float(fs[b, j]), int(fq[b, j])))
            best.append(j)
            out.append(fi[b, j, :int(fl[b, j])].tolist())
        n = max(len(r) for r in out)
        out = [r + [s.pad_token_id] * (n - len(r)) for r in out]
        if not return_trace:
            return out
        steps = n_done - P
        trace = dict(parent=g["tr_parent"][:steps].cpu(), token=g["tr_token"][:steps].cpu(), score=g["tr_score"][:steps].cpu(),
                     fin_score=fs, fin_len=fl, fin_seq=fq, fin_ids=fi, best=best, steps=steps,
                     sequence_scores=[float(fs[b, j]) for b, j in enumerate(best)])
        return out, trace
