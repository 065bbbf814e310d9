"""MI355X-native Whisper engine behind CoRal's `model=whisper-*` keys: log-mel front end on the
GPU, encoder, teacher-forced decoder with the tied LM head + cross-entropy, and greedy generation.

Mirrors what `WhisperModelSetup` gives CoRal (R/src/coral/whisper.py:49-109) and what the ASR
pipeline calls (R/src/coral/evaluate.py:56-60 -> `model.generate`):
  WhisperFeatureExtractor            $TF/models/whisper/feature_extraction_whisper.py:135-168  -> ca_logmel
  WhisperEncoder.forward             $TF/models/whisper/modeling_whisper.py:592-646
  WhisperDecoder(.Layer).forward     :448-505, 690-795
  WhisperForConditionalGeneration    :994-1099 (shift_tokens_right, tied proj_out, CE ignore -100)
  greedy generate                    $TF/models/whisper/generation_whisper.py:383,1455,1774-1812

Forward paths (inference, evaluation loss).  The conv stem runs as overlapping-row GEMMs
over a time-padded channels-last buffer (Conv1d k=3, p=1, stride 1 / 2), the sinusoidal positions are
added in the second conv's epilogue.  The encoder and decoder layers are the pre-LN blocks of blocks.py,
run on inference workspaces; the training engine (whisper_train.py) runs the same blocks, stem and head
with saved activations.  This module holds the shape, the parameters, the front end, the encoder, the teacher-forced
decoder and the head.  Generation - `generate`, the self-attention K|V cache and its token step, greedy, timestamp,
scored and beam search, token timestamps - is whisper_decode.py: `WhisperDecoding`, the engine's base class.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .blocks import CrossAttnBlock, FFNBlock, SelfAttnBlock, zeros_on
from .engine import Engine
from .ops import EPI_GELU, EPI_GELU_RESIDUAL
from .stem_blocks import LMHead, StridedConvBlock
from .wav2vec2 import ParamStore, _r8
from .whisper_decode import WhisperDecoding, check_beam_arguments  # noqa: F401  (check_beam_arguments: imported from here)


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


class WhisperEngine(WhisperDecoding, Engine):
    """Forward paths of WhisperForConditionalGeneration as sequences of HIP kernels (generation: WhisperDecoding)."""

    def __init__(self, shape: WhisperShape, device="cuda:0"):
        ops.lib()
        if not torch.cuda.is_available():
            raise ops.CoralAmdError("WhisperEngine needs a GPU: there is no CPU path")
        self.s = shape
        self.device = torch.device(device)
        assert shape.d_model % 8 == 0 and shape.num_mel_bins % 8 == 0
        self.store = ParamStore(whisper_param_list(shape), self.device)
        d = shape.d_model
        # the stem on time-padded clips of 2 T + 2 rows: conv1 (k 3, padding 1) writes rows 1 .. 2 T, conv2 (k 3, stride 2,
        # padding 1) reads all of them
        rows = 2 * shape.max_source_positions + 2
        self.conv1 = StridedConvBlock(self.store, "model.encoder.conv1.weight", "model.encoder.conv1.bias", shape.num_mel_bins,
                                      d, 3, 1, rows_in=rows, rows_out=rows, y_off=1)
        self.conv2 = StridedConvBlock(self.store, "model.encoder.conv2.weight", "model.encoder.conv2.bias", d, d, 3, 2,
                                      rows_in=rows)
        self.head = LMHead(self.store, "model.decoder.layer_norm", "model.decoder.embed_tokens.weight", None, d,
                           shape.vocab_size, shape.layer_norm_eps)
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

    # (Engine.weights_ready: every path that reads weights waits for the trainer's bucket events first)

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
        self.store.refresh_bf16()
        self.refresh_derived()

    def refresh_derived(self, part: str | None = None):
        """The conv stem's weights are consumed in the reordered [Co][k][Ci] layout."""
        self.conv1.refresh()
        self.conv2.refresh()

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
        B, mels, Tin = x.shape
        # channels-last, time-padded input: rows 1..3000 of each clip hold the frames
        for b in range(B):
            ops.transpose_f32_bf16(x[b], w["xin"][(b * (Tin + 2) + 1) * mels:], mels, Tin)
            if mask_time is not None or mask_feature is not None:  # SpecAugment on the input features
                tm = mask_time[b:b + 1].contiguous() if mask_time is not None else None
                fm = mask_feature[b:b + 1].contiguous() if mask_feature is not None else None
                ops.mask_frames(w["xin"][(b * (Tin + 2) + 1) * mels:], tm, fm, self.zero_mel, None, 1, Tin, mels)
        # conv1 (k=3, p=1) + GELU -> padded [B, 3002, d]
        self.conv1.forward(w["xin"], pre[0], B, C2=w["c1"], epilogue=EPI_GELU)
        # conv2 (k=3, s=2, p=1) + GELU + sinusoidal positions
        self.conv2.forward(w["c1"], pre[1], B, C2=h, epilogue=EPI_GELU_RESIDUAL, R=st.p16,
                           r_off=st.off("model.encoder.embed_positions.weight"), ldr=s.d_model, sR=(0, 0))

    def _embed(self, ids, pos, h, M):
        """The decoder's input rows: token + position embeddings of int32 ids / positions on the device."""
        p16, o = self.store.p16, self.store.off
        ops.embed_tokens(p16[o("model.decoder.embed_tokens.weight"):], p16[o("model.decoder.embed_positions.weight"):],
                         ids, pos, h, M, self.s.d_model)

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
        w = dict(h=[z(B * L * d), z(B * L * d)], **self.head.alloc(B * L, z, train=False))  # (the head's: "hf")
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
            return self.head.forward(h0, w, M, last_of=B).view(B, 1, Vp)[:, :, :V]
        logits = self._last_logits = self.head.forward(h0, w, M)
        return logits.view(B, L, Vp)[:, :, :V]

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
