"""fp32 restatement of `Wav2Vec2ForCTC.forward` (stable-LayerNorm encoder) in training mode, with every dropout given as
an explicit mask (test helper, not collected).

Built from oracle/wav2vec2_ref.py (feature encoder, positional conv, CTC loss, parameter names).  A mask is the factor
the dropped tensor is multiplied by: 0 where an element is dropped, 1 / (1 - p) where it is kept.  Sites
($TF = transformers/models/wav2vec2/modeling_wav2vec2.py):

  "feat_proj"           [B, T, d]     after the feature projection, before SpecAugment / padding   ($TF:433)
  "pos_conv"            [B, T, d]     on h0 + pos_conv(h0), before layer 0                         ($TF:765)
  "layer{l}.attn_probs" [B, H, T, T]  on the softmax probabilities of layer l                      ($TF:458)
  "layer{l}.attn_out"   [B, T, d]     on the attention output, before its residual add             ($TF:642)
  "layer{l}.ffn_out"    [B, T, d]     on the FFN output, before its residual add                   ($TF:571)
  "final"               [B, T, d]     after the encoder's final LayerNorm, before lm_head          ($TF:1698)

A site without a mask is not dropped.  layer_keep: LayerDrop decisions (a dropped layer is the identity).  Without masks
and layer_keep this is `oracle.wav2vec2_ref.forward_loss`, operation for operation.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import wav2vec2_ref as ref


def _drop(x, masks, key):
    m = masks.get(key)
    return x if m is None else x * m


def attention(x, P, pre, cfg: ref.W2V2Config, key_mask, probs_mask=None):
    B, T, d = x.shape
    H, hd = cfg.num_attention_heads, cfg.head_dim
    q = F.linear(x, P[pre + "q_proj.weight"], P[pre + "q_proj.bias"]).view(B, T, H, hd).transpose(1, 2)
    k = F.linear(x, P[pre + "k_proj.weight"], P[pre + "k_proj.bias"]).view(B, T, H, hd).transpose(1, 2)
    v = F.linear(x, P[pre + "v_proj.weight"], P[pre + "v_proj.bias"]).view(B, T, H, hd).transpose(1, 2)
    s = torch.matmul(q, k.transpose(-1, -2)) * (hd ** -0.5)
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :], torch.finfo(s.dtype).min)
    p = torch.softmax(s, dim=-1)
    if probs_mask is not None:
        p = p * probs_mask
    o = torch.matmul(p, v).transpose(1, 2).reshape(B, T, d)
    return F.linear(o, P[pre + "out_proj.weight"], P[pre + "out_proj.bias"])


def encoder_layer(h, P, l: int, cfg: ref.W2V2Config, key_mask, masks):
    p = f"wav2vec2.encoder.layers.{l}."
    eps = cfg.layer_norm_eps
    x = F.layer_norm(h, (h.shape[-1],), P[p + "layer_norm.weight"], P[p + "layer_norm.bias"], eps)
    a = attention(x, P, p + "attention.", cfg, key_mask, masks.get(f"layer{l}.attn_probs"))
    h = h + _drop(a, masks, f"layer{l}.attn_out")
    x = F.layer_norm(h, (h.shape[-1],), P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"], eps)
    x = F.gelu(F.linear(x, P[p + "feed_forward.intermediate_dense.weight"], P[p + "feed_forward.intermediate_dense.bias"]))
    x = F.linear(x, P[p + "feed_forward.output_dense.weight"], P[p + "feed_forward.output_dense.bias"])
    return h + _drop(x, masks, f"layer{l}.ffn_out")


def forward_logits(input_values, attention_mask, P, cfg: ref.W2V2Config, masks=None, layer_keep=None, mask_time=None,
                   mask_feature=None):
    """-> logits f32 [B, T, V] (see the module docstring for masks / layer_keep)."""
    masks = masks or {}
    eps = cfg.layer_norm_eps
    feats = ref.feature_encoder(input_values, P, cfg)
    B, T, _ = feats.shape
    frame_mask = None
    if attention_mask is not None:
        flen = ref.feat_extract_output_lengths(attention_mask.sum(-1), cfg)
        frame_mask = torch.arange(T)[None, :] < flen[:, None]
    x = F.layer_norm(feats, (feats.shape[-1],), P["wav2vec2.feature_projection.layer_norm.weight"],
                     P["wav2vec2.feature_projection.layer_norm.bias"], eps)
    h = F.linear(x, P["wav2vec2.feature_projection.projection.weight"], P["wav2vec2.feature_projection.projection.bias"])
    h = _drop(h, masks, "feat_proj")
    if mask_time is not None:
        h = torch.where(mask_time[:, :, None], P["wav2vec2.masked_spec_embed"].to(h.dtype), h)
    if mask_feature is not None:
        h = h.masked_fill(mask_feature[:, None, :], 0.0)
    if frame_mask is not None:
        h = h * frame_mask[:, :, None].to(h.dtype)
    h = h + ref.pos_conv_embed(h, P, cfg)
    h = _drop(h, masks, "pos_conv")
    for l in range(cfg.num_hidden_layers):
        if layer_keep is None or layer_keep[l]:
            h = encoder_layer(h, P, l, cfg, frame_mask, masks)
    h = F.layer_norm(h, (h.shape[-1],), P["wav2vec2.encoder.layer_norm.weight"], P["wav2vec2.encoder.layer_norm.bias"],
                     eps)
    h = _drop(h, masks, "final")
    return F.linear(h, P["lm_head.weight"], P["lm_head.bias"])


def forward_loss(input_values, attention_mask, labels, P, cfg: ref.W2V2Config, masks=None, layer_keep=None, **kw):
    """-> (loss, logits, per-utterance nll) like oracle.wav2vec2_ref.forward_loss."""
    logits = forward_logits(input_values, attention_mask, P, cfg, masks=masks, layer_keep=layer_keep, **kw)
    am = attention_mask if attention_mask is not None else torch.ones_like(input_values, dtype=torch.long)
    in_len = ref.feat_extract_output_lengths(am.sum(-1), cfg)
    loss, nll = ref.ctc_loss(logits, labels, in_len, cfg)
    return loss, logits, nll
