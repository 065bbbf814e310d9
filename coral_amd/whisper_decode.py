"""Cached Whisper decoding: `WhisperDecoding`, the base class that gives `WhisperEngine` (whisper.py: shape, parameters,
decoder blocks, `_decoder_ws`, `_embed`, `_head`, `encode`, `cross_kv`, `decode`) everything `generate` runs behind the encoder.
`decode_step` feeds the forced prefix into the self-attention K|V cache.  `_decode_rows` is the decoder layer of every
cached token step, spelled once: `_token_step_launches` (greedy, timestamp or scored pick) and `_beam_token_step` (clips x k
rows, the cache read through an ancestry table, CaAttnDesc.key_slot) run it and end with their pick; `_token_step` is the
greedy step as ONE persistent launch where the shape allows (csrc/decode.hip).  `_step_loop` owns warm-up, graph capture and
the host's all-finished check of both searches.  Beam search has the semantics of $TF/generation/utils.py:3208-3508
(GenerationMixin._beam_search); candidates are ranked and beams kept on the device (csrc/beam.hip).
"""

from __future__ import annotations

import functools
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .blocks import LN_IN_GEMM
from .ops import EPI_RESIDUAL
from .wav2vec2 import _r8


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


class Scoring(NamedTuple):  # the scored pick of a request (temperature > 0 / return_stats / no_speech_token)
    inv_t: float  # 1 / temperature as float32, 0 = greedy
    uniforms: torch.Tensor | None  # float32 [clips, >= max_length] with temperature > 0
    no_speech_token: int | None
    use_graph: bool


class DecodeRequest(NamedTuple):  # what `generate`'s arguments ask for, checked (`check_generate_arguments`)
    beam: bool
    ts: tuple | None  # timestamp rules: (begin_index, timestamp_begin, max_initial_timestamp_index)
    scoring: Scoring | None
    alignment_heads: list | None  # [(layer, head)], checked, with return_token_timestamps


def check_generate_arguments(s, input_features, prefix, max_length, use_cache, use_graph, num_beams, length_penalty,
                             early_stopping, return_trace, _beam_path, return_timestamps, timestamp_begin,
                             max_initial_timestamp_index, return_token_timestamps, alignment_heads, temperature,
                             sample_uniforms, return_stats, no_speech_token, cross_kv, prefix_rows=None,
                             prefix_start=None, no_speech_index=0) -> DecodeRequest:
    """Every refusal of `generate`, before any device work (s: the WhisperShape)."""
    beam = num_beams != 1 or _beam_path
    if prefix_rows is not None:
        check_prefix_rows(s, prefix, prefix_rows, prefix_start, max_length, use_cache, num_beams, _beam_path,
                          return_token_timestamps)
        prefix = [s.pad_token_id] * int(prefix_rows.shape[1])  # (below only its length is looked at)
    elif prefix_start is not None:
        raise ValueError("prefix_start= comes with prefix_rows=")
    if not isinstance(no_speech_index, int) or not 0 <= no_speech_index < len(prefix):
        raise ValueError(f"no_speech_index={no_speech_index!r} lies outside the {len(prefix)} prefix positions")
    ts = None
    scoring = None
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
        scoring = Scoring(float(np.float32(1.0 / temperature)) if temperature > 0 else 0.0,
                          sample_uniforms if temperature > 0 else None, no_speech_token, use_graph)
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
    if cross_kv is not None and not use_cache:
        raise ValueError("cross_kv= needs use_cache=True (the pass without a cache reads the encoder states)")
    return DecodeRequest(beam, ts, scoring, alignment_heads if return_token_timestamps else None)


def check_prefix_rows(s, prefix, prefix_rows, prefix_start, max_length, use_cache, num_beams, beam_path,
                      return_token_timestamps) -> None:
    """The limits of generate(prefix_rows=, prefix_start=): left-padded decoder inputs, one row per clip."""
    if prefix is not None:
        raise ValueError("prefix_rows= replaces prefix=: pass prefix=None with it")
    if not isinstance(prefix_rows, torch.Tensor) or prefix_rows.dim() != 2 or prefix_rows.dtype != torch.int64 \
            or prefix_rows.shape[1] < 1:
        raise ValueError("prefix_rows must be an int64 tensor [clips, P] with P >= 1")
    B, P = prefix_rows.shape
    if not isinstance(prefix_start, torch.Tensor) or prefix_start.dtype != torch.int32 or tuple(prefix_start.shape) != (B,):
        raise ValueError(f"prefix_rows needs prefix_start, int32 [{B}]: the number of leading pad positions of every row")
    if num_beams != 1 or beam_path:
        raise ValueError(f"generate(num_beams={num_beams}): prefix_rows is not implemented with beam search")
    if return_token_timestamps:
        raise ValueError("prefix_rows is not implemented with return_token_timestamps=True")
    if not use_cache:
        raise ValueError("prefix_rows needs use_cache=True (the pass without a cache knows no left padding)")
    if P >= max_length or max_length > s.max_target_positions:
        raise ValueError(f"prefix_rows needs P < max_length <= {s.max_target_positions}, got P = {P}, max_length = "
                         f"{max_length}")
    start = prefix_start.cpu()
    if int(start.min()) < 0 or int(start.max()) >= P:
        raise ValueError(f"prefix_start must lie in [0, P = {P}): every row keeps at least one token")
    rows = prefix_rows.cpu()
    if int(rows.min()) < 0 or int(rows.max()) >= s.vocab_size:
        raise ValueError("prefix_rows holds ids outside the vocabulary")
    valid = torch.arange(P)[None, :] >= start[:, None].long()
    if bool(((rows == s.pad_token_id) & valid).any()):
        raise ValueError(f"prefix_rows: pad id {s.pad_token_id} inside a row's valid part.  transformers masks decoder "
                         "inputs by value (ids != pad_token_id); only the left run of padding it produces is supported")


@functools.lru_cache(maxsize=None)
def decoder_layer_names(l: int) -> dict:
    """The parameters of decoder layer l, HF names under the field names of `CaDecodeLayer` (its parameter fields, in its
    order; wqkv / bqkv name the first of the three adjacent q|k|v tensors), then the K|V half of the self-attention
    projection on its own (wkv / bkv: what the prefill writes into the cache)."""
    p = f"model.decoder.layers.{l}."
    sa, ca = p + "self_attn.", p + "encoder_attn."
    return dict(ln1_g=p + "self_attn_layer_norm.weight", ln1_b=p + "self_attn_layer_norm.bias",
                wqkv=sa + "q_proj.weight", bqkv=sa + "q_proj.bias", wo=sa + "out_proj.weight", bo=sa + "out_proj.bias",
                ln2_g=p + "encoder_attn_layer_norm.weight", ln2_b=p + "encoder_attn_layer_norm.bias",
                wq2=ca + "q_proj.weight", bq2=ca + "q_proj.bias", wo2=ca + "out_proj.weight", bo2=ca + "out_proj.bias",
                ln3_g=p + "final_layer_norm.weight", ln3_b=p + "final_layer_norm.bias",
                w1=p + "fc1.weight", b1=p + "fc1.bias", w2=p + "fc2.weight", b2=p + "fc2.bias",
                wkv=sa + "k_proj.weight", bkv=sa + "k_proj.bias__zero")


class WhisperDecoding:
    """Incremental decoding of a `WhisperEngine` (module docstring)."""

    # ---- incremental decoding (self-attention K|V cache) ----------------------------------------
    def new_decode_cache(self, B: int, max_len: int):
        """Per decoder layer a bf16 [B, max_len, 2d] buffer holding K|V of the tokens decoded so far — the
        self-attention half of the cache HF keeps in `EncoderDecoderCache`
        ($TF/models/whisper/modeling_whisper.py:312-335, generation with use_cache)."""
        d = self.s.d_model
        return dict(kv=[torch.zeros(B * max_len * 2 * d, dtype=torch.bfloat16, device=self.device)
                        for _ in range(self.s.decoder_layers)], max_len=max_len, pos=0, B=B)

    def _prefill_self_attn(self, l, h0, h1, w, ckv, B, n, pos0, Lmax, kstart=None, klen=None):
        """The self-attention half of layer l for n new tokens per clip at the HOST-side position pos0 (h0 -> h1): unlike
        the token step's, K|V go into the cache rows pos0.. of every clip by a batched GEMM and the attention is causal.
        kstart (int32 [B] on the device, or None): the first key of every row - the left padding of `prefix_rows`
        (CaAttnDesc.kstart); a single token then comes with klen = pos0 + 1 per row, the single-query form's key count."""
        s, st = self.s, self.store
        p32, p16, o = st.p32, st.p16, st.off
        d, H, M = s.d_model, s.decoder_attention_heads, B * n
        hd = d // H
        x, q, ctx, lse = w["ca"]["x"], w["ca"]["q"], w["ca"]["ctx"], w["ca"]["lse"]
        nm = decoder_layer_names(l)
        ops.layernorm_fwd(h0, st.view(nm["ln1_g"]), st.view(nm["ln1_b"]), x, None, M, d, s.layer_norm_eps)
        ops.gemm(x, p16, q, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wqkv"]), bias=p32, bias_off=o(nm["bqkv"]))
        # K|V of the new tokens go straight into the cache rows (batch b, position pos0..)
        ops.gemm(x, p16, ckv, M=n, N=2 * d, K=d, lda=d, ldb=d, ldc=2 * d, c_off=pos0 * 2 * d, b_off=o(nm["wkv"]), bias=p32,
                 bias_off=o(nm["bkv"]), batch2=B, sA=(0, n * d), sC=(0, Lmax * 2 * d))
        ops.attn_fwd(q, ckv, ckv, ctx, lse, B=B, H=H, Tq=n, Tk=pos0 + n, hd=hd, Tqp=w["ca"]["Tqp"],
                     scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, sqb=n * d, skb=Lmax * 2 * d,
                     svb=Lmax * 2 * d, sob=n * d, k_off=0, v_off=d, causal=(n > 1), kstart=kstart, klen=klen)
        ops.gemm(ctx, p16, h1, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wo"]), bias=p32, bias_off=o(nm["bo"]),
                 epilogue=EPI_RESIDUAL, R=h0, ldr=d)

    def decode_step(self, new_ids: torch.Tensor, cross_kv: list, cache: dict, kstart=None) -> torch.Tensor:
        """Feed `new_ids` [B, n] (the forced prefix at position 0, then one token per call) through the
        decoder, appending their K|V to `cache`; returns fp32 logits [B, V] of the last position.
        Same arithmetic as `decode(...)[:, -1]`: each new query attends to all cached keys.
        kstart (int32 [B] on the device): cache positions in front of kstart[b] are left padding, attended to by no query
        of clip b.  Positions count the padding, as in transformers (`WhisperDecoder.forward`: arange over the padded row)."""
        self._await_all()
        s, dev = self.s, self.device
        B, n = new_ids.shape
        pos0, Lmax = cache["pos"], cache["max_len"]
        if B != cache["B"] or pos0 + n > Lmax or pos0 + n > s.max_target_positions:
            raise ValueError("decode cache too small / batch mismatch")
        if pos0 > 0 and n != 1:
            raise ValueError("after the first call tokens are appended one at a time")
        M, Te = B * n, s.max_source_positions
        w = self._decoder_ws(B, n)
        ids = new_ids.to(dev, torch.int32).contiguous().view(-1)
        pos = (torch.arange(n, dtype=torch.int32, device=dev) + pos0).repeat(B)
        h0, h1 = w["h"]
        self._embed(ids, pos, h0, M)
        klen = torch.full((B,), pos0 + 1, dtype=torch.int32, device=dev) if kstart is not None and n == 1 else None
        for l, (_, ca, ff) in enumerate(self.dec_blocks):
            self._prefill_self_attn(l, h0, h1, w, cache["kv"][l], B, n, pos0, Lmax, kstart, klen)
            ca.forward(h1, h0, w["ca"], B, n, Te, kv=cross_kv[l])
            ff.forward(h0, h1, w["ff"], M)
            h0, h1 = h1, h0
        logits = self.head.forward(h0, w, M, last_of=B)
        cache["pos"] = pos0 + n
        return logits[:, :s.vocab_size]

    # ---- one-token step with static shapes and pointers (capturable in a HIP graph) -----------------
    def _graph_state(self, cache: dict, cross_kv: list, pad_id: int, eos_id: int, kstart=None):
        """Static buffers of the per-token step: everything that changes from token to token (position,
        cached length, token ids, finished flags) lives in device memory, so the launch sequence is
        identical for every token and can be replayed as one graph.  kstart (int32 [B] on the device, or None): the first
        key of every row, which does not change from token to token."""
        B, Lmax, dev = cache["B"], cache["max_len"], self.device
        i32 = lambda: torch.zeros(B, dtype=torch.int32, device=dev)  # noqa: E731
        return dict(tok=i32(), pos=i32(), klen=i32(), nxt=i32(), done=torch.zeros(B, dtype=torch.bool, device=dev),
                    out=torch.full((B, Lmax), pad_id, dtype=torch.int64, device=dev),
                    logits=torch.zeros(B, _r8(self.s.vocab_size), dtype=torch.float32, device=dev),
                    pad_id=pad_id, eos=eos_id, cross=cross_kv, kstart=kstart)

    def _persistent_state(self, cache: dict, g: dict, suppress: torch.Tensor):
        """Descriptor + device tables of ca_whisper_decode_token for this decode state, or None where the launch
        sequence stays (shape / device outside the kernel's limits, CA_DECODE_PERSISTENT=0).  Decoding with timestamps
        (g["ts"]) always keeps the launch sequence: the one-launch kernel's pick is the plain masked argmax
        (csrc/decode.hip), the timestamp rules live in ca_argmax_timestamps_advance.  So does decoding from left-padded
        prefix rows (g["kstart"]): the one-launch kernel's self-attention knows no first key."""
        if "persist" in g:
            return g["persist"]
        if g.get("kstart") is not None:
            g["persist"] = None
            return None
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
        # a layer's record: its parameters in the order of CaDecodeLayer (weight matrices bf16, the rest fp32), its caches
        fields = _lib.CaDecodeLayer.FIELDS
        assert fields[-2:] == ("self_kv", "cross_kv") and tuple(decoder_layer_names(0))[:len(fields) - 2] == fields[:-2]
        rows = [[(w16 if fld[0] == "w" else w32)(decoder_layer_names(l)[fld]) for fld in fields[:-2]]
                + [cache["kv"][l].data_ptr(), cross[l].data_ptr()] for l in range(s.decoder_layers)]
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

    def _decode_rows(self, cache: dict, g: dict, R: int, key_slot=None, cross=None, may_fuse: bool = True):
        """One token per row, g["tok"] at position g["pos"] (both in device memory), through the decoder against the
        self-attention cache: ~7 launches per layer, the R rows' logits into g["logits"].  A row's K|V go to cache row
        r * max_len + pos[r]; it attends to g["klen"][r] keys of its own cache row - from key g["kstart"][r] on, where the
        state has one - or with key_slot (int32 [R, max_len]) to the cache rows that table names.  cross = (B, Tq,
        split_ws): the cross-attention's view of the R = B * Tq rows as Tq queries of each of B clips and its key-split
        workspace; default (R, 1, the decoder workspace's).  may_fuse:
        whether LayerNorm + q projection + cross-attention may run as one launch (Tq = 1 only)."""
        s, st = self.s, self.store
        p32, p16, o = st.p32, st.p16, st.off
        Lmax, eps = cache["max_len"], s.layer_norm_eps
        d, H, Te = s.d_model, s.decoder_attention_heads, s.max_source_positions
        hd = d // H
        w = self._decoder_ws(R, 1)
        x, q, ctx, lse = w["ca"]["x"], w["ca"]["q"], w["ca"]["ctx"], w["ca"]["lse"]
        cB, cT, split = cross if cross is not None else (R, 1, w["split"])
        ln_in = LN_IN_GEMM and R <= 128 and d <= 2048  # the LayerNorms in the following projection's prologue
        fused = False
        if may_fuse:
            # LayerNorm + query projection inside the cross-attention launch: every (clip, head) workgroup streams its
            # head's 64 x d slice of Wq in its prologue (128 KB at d = 1024, a third of the K|V it then streams) - worth it
            # while the launch is short of workgroups (32 clips x 16 heads = 2 per CU: 3.05 against 3.14 ms per token), not
            # above (64 clips: 4.17 against 4.02, 128: 7.34 against 6.96; round 5).  CA_DECODE_FUSED = 0 / 1 forces either.
            fz = os.environ.get("CA_DECODE_FUSED")
            ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
            fused = (fz != "0" if fz is not None else R * H <= 2 * ncu) and hd <= 64 and d <= 2048
        h0, h1 = w["h"]
        self._embed(g["tok"], g["pos"], h0, R)
        for l, (_, _, ff) in enumerate(self.dec_blocks):
            nm = decoder_layer_names(l)
            ckv, ckx = cache["kv"][l], g["cross"][l]
            ln1, ln2 = (st.view(nm["ln1_g"]), st.view(nm["ln1_b"])), (st.view(nm["ln2_g"]), st.view(nm["ln2_b"]))
            if not ln_in:
                ops.layernorm_fwd(h0, *ln1, x, None, R, d, eps)
            # q and the new K|V rows from one launch over the adjacent q|k|v weights: q to its buffer, K|V straight
            # into the cache at the device-side position (CaGemmDesc.c_split_n / c_row_index: the position is data,
            # not a launch argument, so the launch sequence can be replayed as a graph); the LayerNorm in front of it
            # in the same launch's prologue (CaGemmDesc.a_ln_gamma)
            ops.gemm(h0 if ln_in else x, p16, q, M=R, N=3 * d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wqkv"]), bias=p32,
                     bias_off=o(nm["bqkv"]), c_split_n=d, C_hi=ckv, ldc_hi=2 * d, c_row_index=g["pos"], c_row_mul=Lmax,
                     a_ln=(*ln1, eps) if ln_in else None)
            ops.attn_fwd(q, ckv, ckv, ctx, lse, B=R, H=H, Tq=1, Tk=Lmax, hd=hd, Tqp=32, scale=hd ** -0.5, ldq=d, ldk=2 * d,
                         ldv=2 * d, ldo=d, sqb=d, skb=Lmax * 2 * d, svb=Lmax * 2 * d, sob=d, k_off=0, v_off=d,
                         klen=g["klen"], key_slot=key_slot, kstart=g.get("kstart"))
            ops.gemm(ctx, p16, h1, M=R, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wo"]), bias=p32, bias_off=o(nm["bo"]),
                     epilogue=EPI_RESIDUAL, R=h0, ldr=d)
            if fused:
                # LayerNorm + query projection + attention over the cached encoder K|V: one launch (bit-identical to
                # the three below; CA_DECODE_FUSED=0 keeps them)
                ops.decode_attn_qproj(h1, *ln2, p16, p32, ckx, ckx, ctx, d_model=d, eps=eps, ldx=d, ldw=d,
                                      w_off=o(nm["wq2"]), bias_off=o(nm["bq2"]), B=cB, H=H, Tk=Te, hd=hd, scale=hd ** -0.5,
                                      ldk=2 * d, ldv=2 * d, ldo=d, skb=Te * 2 * d, svb=Te * 2 * d, sob=d, k_off=0, v_off=d,
                                      split_ws=split)
            else:
                if not ln_in:
                    ops.layernorm_fwd(h1, *ln2, x, None, R, d, eps)
                ops.gemm(h1 if ln_in else x, p16, q, M=R, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wq2"]), bias=p32,
                         bias_off=o(nm["bq2"]), a_ln=(*ln2, eps) if ln_in else None)
                ops.attn_fwd(q, ckx, ckx, ctx, lse, B=cB, H=H, Tq=cT, Tk=Te, hd=hd, Tqp=32, scale=hd ** -0.5, ldq=d,
                             ldk=2 * d, ldv=2 * d, ldo=d, sqb=cT * d, skb=Te * 2 * d, svb=Te * 2 * d, sob=cT * d, k_off=0,
                             v_off=d, split_ws=split)
            ops.gemm(ctx, p16, h0, M=R, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=o(nm["wo2"]), bias=p32, bias_off=o(nm["bo2"]),
                     epilogue=EPI_RESIDUAL, R=h1, ldr=d)
            ff.forward(h0, h1, w["ff"], R)
            h0, h1 = h1, h0
        self.head.forward(h0, w, R, logits=g["logits"])

    def _pick_advance(self, g: dict, logits: torch.Tensor, ldv: int, suppress: torch.Tensor):
        """The pick of a greedy step and the step's bookkeeping in one launch: out[b, pos + 1] = the token (pad for
        finished rows), done |= eos, tok = the token, pos += 1, klen += 1."""
        B, V = g["tok"].numel(), self.s.vocab_size
        books = (g["done"], g["out"], g["tok"], g["pos"], g["klen"], g["pad_id"], g["eos"])
        if g.get("scored") is not None:  # greedy or sampled, with the token's log-probability (csrc/pick.hip)
            sc = g["scored"]
            ops.pick_scored_advance(logits, suppress, g["nxt"], B, V, ldv, sc["inv_t"], sc["uniforms"], sc["sum_logprob"],
                                    sc["n_scored"], *books, timestamps=g.get("ts"))
        elif g.get("ts") is not None:  # the same step under the timestamp rules (history: g["out"] up to g["pos"])
            ops.argmax_timestamps_advance(logits, suppress, g["nxt"], B, V, ldv, *books, *g["ts"])
        else:
            ops.argmax_advance(logits, suppress, g["nxt"], B, V, ldv, *books)

    def _token_step_launches(self, cache: dict, g: dict, suppress: torch.Tensor):
        """The same step as a sequence of ~7 launches per layer."""
        self._decode_rows(cache, g, cache["B"])
        self._pick_advance(g, g["logits"], _r8(self.s.vocab_size), suppress)

    def _step_loop(self, step, done, P, n_done, max_length, use_graph=True, by_parity=False, persistent=lambda: False):
        """The token steps of a search from position n_done (the first free token is picked) to max_length or until every
        row has finished; -> n_done.  step(i) issues the launches of step i = n_done - P.  One eager step warms the sequence
        up (allocations, attributes); then the steps are captured in HIP graphs and replayed, use_graph=False: issued.
        by_parity: a graph per parity of i, one step each (beam search's double-buffered tables); else a graph per chunk
        length, 8 steps where persistent() - looked at after the warm-up - says a step is ONE launch, else 1."""
        due = lambda: (n_done - P) % 8 == 2  # noqa: E731  (the host looks at `done` every 8 tokens)
        if n_done < max_length and not bool(done.all()):
            step(n_done - P)
            n_done += 1
        graphs = {}

        def run(n):  # n token steps as ONE graph (capture records the launches without running them)
            i = n_done - P
            if not use_graph:
                for j in range(n):
                    step(i + j)
                return
            key = i & 1 if by_parity else n
            if key not in graphs:
                torch.cuda.synchronize()
                graphs[key] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[key]):
                    for j in range(n):
                        step(i + j)
            graphs[key].replay()

        # with one launch per token a graph of eight tokens is 8 kernels + 8 memset nodes: the gap between two graph
        # launches (~10-16 us) is paid once per eight tokens, like the host's all-finished check
        late = persistent()
        chunk = 8 if late else 1
        # The all-finished check.  Launch sequence: synchronous, every 8 tokens (the host waits, looks, launches).  One launch
        # per token: the check of a chunk is an asynchronous copy to pinned memory behind it, looked at one chunk LATER, so
        # the next chunk is already queued while the host waits - the device never idles between chunks (the synchronous
        # form cost ~50 us per token at 16 clips).  What the host sees late costs nothing: a launch that finds every clip
        # finished only records pad and returns (decode.hip), and the caller's trimming cuts those columns off.
        flags = torch.zeros(2, dtype=torch.bool).pin_memory() if late else None
        pending = []  # (event, slot) of the chunks whose flag has not been looked at
        k = 0
        while n_done < max_length:
            if not late and due() and bool(done.all()):
                break
            n = chunk if (chunk > 1 and due() and n_done + chunk <= max_length) else 1
            run(n)
            n_done += n
            if late and due():
                flags[k & 1:(k & 1) + 1].copy_(done.all().view(1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((ev, k & 1))
                k += 1
                if len(pending) == 2:  # the chunk before the one just queued
                    ev0, slot = pending.pop(0)
                    ev0.synchronize()
                    if bool(flags[slot]):
                        break
        return n_done

    # ---- model-level API -------------------------------------------------------------------------
    def generate(self, input_features, prefix: list[int], max_length: int, suppress_tokens=None,
                 begin_suppress_tokens=None, use_cache: bool = True, use_graph: bool = True, num_beams: int = 1,
                 length_penalty: float = 1.0, early_stopping: bool = False, return_trace: bool = False,
                 _beam_path: bool = False, return_timestamps: bool = False, timestamp_begin: int | None = None,
                 max_initial_timestamp_index: int | None = None, return_token_timestamps: bool = False,
                 alignment_heads=None, num_frames=None, median_filter_width: int = 7, temperature: float = 0.0,
                 sample_uniforms=None, return_stats: bool = False, no_speech_token: int | None = None, cross_kv=None,
                 prefix_rows=None, prefix_start=None, no_speech_index: int = 0):
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
        input_features may be None.
        prefix_rows (with prefix=None): int64 [B, P], a decoder input row per clip - previous text or a prompt in front of
        the forced prefix, as `_prepare_decoder_input_ids` of transformers' long-form loop builds them - LEFT-padded with
        the pad id; prefix_start int32 [B]: the number of leading pad positions of every row.  The padding is attended to
        by nothing (CaAttnDesc.kstart) and counts as positions, as in transformers; the timestamp rules begin at P; the
        returned rows start with the P columns given.  Greedy or sampled, with or without timestamps; not with beams or
        token timestamps; the one-launch-per-token kernel is bypassed.  no_speech_index: the prefix position whose logits
        give the no-speech probability (<|startoftranscript|>: P minus the forced tokens)."""
        s, dev = self.s, self.device
        req = check_generate_arguments(
            s, input_features, prefix, max_length, use_cache, use_graph, num_beams, length_penalty, early_stopping,
            return_trace, _beam_path, return_timestamps, timestamp_begin, max_initial_timestamp_index,
            return_token_timestamps, alignment_heads, temperature, sample_uniforms, return_stats, no_speech_token, cross_kv,
            prefix_rows, prefix_start, no_speech_index)
        ts = req.ts
        rows0 = kstart = None  # left-padded prefix rows on the device and their first keys; None wherever no prompt is in play
        if prefix_rows is not None:
            rows0, kstart = prefix_rows.to(dev).contiguous(), prefix_start.to(dev).contiguous()
            prefix = [s.pad_token_id] * rows0.shape[1]  # (a stand-in where only the length P is looked at)
        if cross_kv is not None:
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

        def with_times(rows):
            if not return_token_timestamps:
                return rows
            return rows, self.token_timestamps(rows, kv, len(prefix), req.alignment_heads, num_frames, median_filter_width)

        if rows0 is not None and rows0.shape[0] != B:
            raise ValueError(f"prefix_rows has {rows0.shape[0]} rows for {B} clips")
        if req.beam:
            return self._generate_beam(kv, prefix, max_length, sup, sup_begin, num_beams, float(length_penalty),
                                       bool(early_stopping), return_trace, use_graph)
        if req.scoring is not None:
            if temperature > 0 and sample_uniforms.shape[0] != B:
                raise ValueError(f"sample_uniforms has {sample_uniforms.shape[0]} rows for {B} clips")
            rows, sc = self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts, req.scoring, rows0, kstart,
                                            no_speech_index)
            stats = dict(sum_logprob=sc["sum_logprob"].cpu().tolist(), n_scored=sc["n_scored"].cpu().tolist(),
                         no_speech_prob=sc["no_speech_prob"].cpu().tolist() if no_speech_token is not None else None)
            return (rows, stats) if return_stats else rows
        if use_cache and use_graph and max_length > len(prefix) + 2:
            return with_times(self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts, None, rows0, kstart)[0])
        ids = torch.tensor([prefix] * B, dtype=torch.int64, device=dev) if rows0 is None else rows0
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        nxt = torch.empty(B, dtype=torch.int32, device=dev)
        cache = self.new_decode_cache(B, max_length) if use_cache else None
        feed = ids
        while ids.shape[1] < max_length and not bool(done.all()):
            if use_cache:
                base = self.decode_step(feed, kv, cache, kstart).contiguous()  # fp32 [B, V]
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
        return with_times(ids.tolist())

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

    # ---- greedy search on the cache --------------------------------------------------------------------------------------
    def _generate_graph(self, kv, prefix, max_length, sup, sup_begin, ts=None, scoring: Scoring | None = None,
                        prefix_rows=None, kstart=None, no_speech_index: int = 0):
        """Greedy loop with the per-token step captured once in a HIP graph and replayed: the ~350 small
        launches of a token (24-32 layers x 14 kernels) cost one graph launch instead of 350 host calls.
        -> (id rows, the scored pick's state or None: dict(sum_logprob, n_scored, no_speech_prob, ...) on the device).
        prefix_rows int64 [B, P] / kstart int32 [B], both on the device: a left-padded row per clip in place of `prefix`
        (then only P long) and its first key - a static array, so the per-token graph replays unchanged."""
        s, dev = self.s, self.device
        B, V, P = kv[0].shape[0] // (s.max_source_positions * 2 * s.d_model), s.vocab_size, len(prefix)
        cache = self.new_decode_cache(B, max_length)
        g = self._graph_state(cache, kv, s.pad_token_id, s.eos_token_id, kstart)
        g["ts"] = ts  # (begin_index, timestamp_begin, max_initial_timestamp_index) or None
        # the forced prefix and the first free token run eagerly (different shapes / begin-suppress mask)
        ids0 = torch.tensor([prefix] * B, dtype=torch.int64, device=dev) if prefix_rows is None else prefix_rows
        base = self.decode_step(ids0, kv, cache, kstart).contiguous()
        if scoring is not None:
            g["scored"] = sc = dict(inv_t=scoring.inv_t, uniforms=scoring.uniforms, no_speech_prob=None,
                                    sum_logprob=torch.zeros(B, dtype=torch.float32, device=dev),
                                    n_scored=torch.zeros(B, dtype=torch.int32, device=dev))
            if sc["uniforms"] is not None:
                sc["uniforms"] = sc["uniforms"].to(dev, torch.float32).contiguous()
            if scoring.no_speech_token is not None:
                # WhisperNoSpeechDetection: the softmax of the raw logits at the start-of-transcript position, i.e. the
                # head on prefix position 0 (decode_step left the final LayerNorm of every prefix row in the workspace);
                # behind previous text or a prompt that token stands at no_speech_index
                hf0 = self._decoder_ws(B, P)["hf"][:B * P * s.d_model].view(B, P, s.d_model)[:, no_speech_index, :].contiguous()
                lg0 = self.head.project(hf0, B)
                sc["no_speech_prob"] = torch.empty(B, dtype=torch.float32, device=dev)
                ops.row_token_prob(lg0, sc["no_speech_prob"], B, V, _r8(V), scoring.no_speech_token)
        # the first free token through the step's own pick (a scored one counts its log-probability): the books stand at
        # the last prefix token
        g["out"][:, :P] = ids0
        g["pos"].fill_(P - 1)
        g["klen"].fill_(P)
        self._pick_advance(g, base, V, sup_begin)
        n_done = self._step_loop(lambda i: self._token_step(cache, g, sup), g["done"], P, P + 1, max_length,
                                 use_graph=scoring is None or scoring.use_graph,
                                 persistent=lambda: g.get("persist") is not None)
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
                return self._generate_graph(kv, prefix, max_length, sup, sup_begin, ts, scoring, prefix_rows, kstart,
                                            no_speech_index)
        # trim like the eager loop: stop at the first column where every row had already finished
        fin = (out == s.eos_token_id).cumsum(1) > 0
        allfin = fin.all(0)
        keep = int(torch.nonzero(allfin)[0]) + 1 if bool(allfin.any()) else n_done
        return out[:, :keep].tolist(), g.get("scored")

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
        """The token step over clips x beams rows: the self-attention reads the K|V cache through the ancestry table (rows
        are written once, by the beam slot that produced them, and never copied); the cross-attention takes a clip's k
        beams as k queries against the clip's ONE encoder K|V; ca_beam_select + ca_beam_advance stand where
        ca_argmax_advance stood."""
        B, k = g["B"], g["k"]
        self._decode_rows(cache, g, B * k, key_slot=g["anc"][par], cross=(B, k, g["split"]), may_fuse=False)
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
        # (step i reads the tables of buffer i & 1: the pick above was step 0)
        n_done = self._step_loop(lambda i: self._beam_token_step(cache, g, sup, i & 1), g["done"], P, P + 1, max_length,
                                 use_graph=use_graph, by_parity=True)
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
