"""CPU checks of the wav2vec2 dropouts: the masked restatement (tests/w2v2_dropout_ref.py) against HF Transformers'
own `Wav2Vec2ForCTC` in training mode with the same masks injected, and the resolution of the five dropout keys that
`Wav2Vec2ForCTC.from_pretrained` takes (coral_amd/modeling.py: resolve_dropouts, hf_config)."""
import json

import numpy as np
import pytest
import torch

import w2v2_dropout_ref as dref
from oracle import wav2vec2_ref as ref


def _batch(lens, lab_lens, seed=4242):
    g = torch.Generator().manual_seed(seed)
    waves = [(0.1 * torch.randn(int(n), generator=g)).clamp(-1, 1).numpy() for n in lens]
    labels = torch.full((len(lens), max(lab_lens)), -100, dtype=torch.long)
    for b, L in enumerate(lab_lens):
        labels[b, :L] = torch.randint(0, 42, (L,), generator=g)
    iv, am = ref.zero_mean_unit_var_norm(waves)
    return torch.from_numpy(iv), torch.from_numpy(am).long(), labels


def _mask(shape, p, g):
    return (torch.rand(shape, generator=g) >= p).float() / (1.0 - p)


def _all_masks(B, T, d, H, L, p, seed):
    g = torch.Generator().manual_seed(seed)
    m = {k: _mask((B, T, d), p, g) for k in ("feat_proj", "pos_conv", "final")}
    for l in range(L):
        m[f"layer{l}.attn_probs"] = _mask((B, H, T, T), p, g)
        m[f"layer{l}.attn_out"] = _mask((B, T, d), p, g)
        m[f"layer{l}.ffn_out"] = _mask((B, T, d), p, g)
    return m


def test_restatement_without_masks_is_the_oracle():
    kw = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128)
    cfg = ref.W2V2Config(**kw)
    P = ref.synth_params(cfg)
    iv, am, labels = _batch([4000, 3100], [4, 3])
    loss_a, logits_a, _ = ref.forward_loss(iv, am, labels, P, cfg)
    loss_b, logits_b, _ = dref.forward_loss(iv, am, labels, P, cfg)
    assert torch.equal(logits_a, logits_b) and torch.equal(loss_a, loss_b)
    # a dropped layer is the identity: layer_keep [False, True] == the restatement with layer 0 skipped
    masks = _all_masks(2, logits_a.shape[1], 64, 4, 2, 0.2, 3)
    la, _, _ = dref.forward_loss(iv, am, labels, P, cfg, masks=masks, layer_keep=[False, True])
    lb, _, _ = dref.forward_loss(iv, am, labels, P, cfg, masks={k: v for k, v in masks.items() if "layer0" not in k},
                                 layer_keep=[False, True])
    assert torch.equal(la, lb)


class _FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def test_restatement_matches_hf_train_mode_with_the_same_masks(golden_dir, monkeypatch):
    """HF's `Wav2Vec2ForCTC` (tiny golden checkpoint, train mode) with every nn.Dropout replaced by a fixed-mask module
    and the eager attention's `nn.functional.dropout` patched per layer: loss, logits and the gradients wrt the inputs
    and parameters equal the restatement's.  This pins the placement of every site to HF itself."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.wav2vec2 import modeling_wav2vec2 as mw

    d_ = golden_dir / "hf_ckpt_w2v2"
    model = transformers.Wav2Vec2ForCTC.from_pretrained(str(d_), attn_implementation="eager", dtype=torch.float32)
    hcfg = model.config
    assert hcfg.do_stable_layer_norm and not hcfg.apply_spec_augment and hcfg.layerdrop == 0.0
    cfg = ref.W2V2Config(
        hidden_size=hcfg.hidden_size, num_hidden_layers=hcfg.num_hidden_layers,
        num_attention_heads=hcfg.num_attention_heads, intermediate_size=hcfg.intermediate_size,
        conv_dim=tuple(hcfg.conv_dim), conv_kernel=tuple(hcfg.conv_kernel), conv_stride=tuple(hcfg.conv_stride),
        num_conv_pos_embeddings=hcfg.num_conv_pos_embeddings,
        num_conv_pos_embedding_groups=hcfg.num_conv_pos_embedding_groups, vocab_size=hcfg.vocab_size,
        pad_token_id=hcfg.pad_token_id, layer_norm_eps=hcfg.layer_norm_eps,
        ctc_loss_reduction=hcfg.ctc_loss_reduction, ctc_zero_infinity=hcfg.ctc_zero_infinity)
    z = np.load(golden_dir / "hf_ckpt_w2v2.npz")
    iv, am, labels = _batch(z["lens"], [4, 3])
    B = iv.shape[0]
    T = int(ref.feat_extract_output_lengths(torch.tensor([iv.shape[1]]), cfg)[0])
    d, H, L = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
    masks = _all_masks(B, T, d, H, L, 0.25, 7)

    # HF side
    enc = model.wav2vec2.encoder
    assert type(enc).__name__ == "Wav2Vec2EncoderStableLayerNorm"
    model.wav2vec2.feature_projection.dropout = _FixedMask(masks["feat_proj"])
    enc.dropout = _FixedMask(masks["pos_conv"])
    model.dropout = _FixedMask(masks["final"])
    current = {}
    for l, layer in enumerate(enc.layers):
        layer.dropout = _FixedMask(masks[f"layer{l}.attn_out"])
        layer.feed_forward.output_dropout = _FixedMask(masks[f"layer{l}.ffn_out"])
        layer.feed_forward.intermediate_dropout = torch.nn.Identity()
        layer.attention.register_forward_pre_hook(lambda mod, args, l=l: current.__setitem__("l", l))
    calls = []

    def attn_dropout(x, p=0.5, training=True, inplace=False):
        calls.append(current["l"])
        return x * masks[f"layer{current['l']}.attn_probs"]

    monkeypatch.setattr(mw.nn.functional, "dropout", attn_dropout)
    model.train()
    # (HF's feature encoder sets requires_grad on its input view in training; with an input that already requires grad
    # that is an error, and skipping it changes nothing else: the conv weights still require grad)
    model.wav2vec2.feature_extractor._requires_grad = False
    iv_h = iv.clone().requires_grad_(True)
    out = model(iv_h, attention_mask=am, labels=labels)
    out.loss.backward()
    monkeypatch.undo()
    assert calls == list(range(L))  # one probability dropout per layer, in layer order

    # restatement side, with HF's own weights
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items() if k in ref.param_shapes(cfg)}
    assert set(P) == set(ref.param_shapes(cfg))
    iv_r = iv.clone().requires_grad_(True)
    loss, logits, _ = dref.forward_loss(iv_r, am, labels, P, cfg, masks=masks)
    loss.backward()
    loss_plain, _, _ = ref.forward_loss(iv, am, labels, {k: v.detach() for k, v in P.items()}, cfg)

    assert abs(float(loss) - float(loss_plain)) > 1e-3 * abs(float(loss_plain))  # the masks change the forward
    assert abs(float(loss) - float(out.loss)) <= 1e-4 * abs(float(out.loss)), (float(loss), float(out.loss))
    assert (logits.detach() - out.logits.detach()).abs().max() <= 1e-4
    ga, gb = iv_r.grad.double(), iv_h.grad.double()
    assert float((ga - gb).norm() / gb.norm()) <= 1e-3
    named = dict(model.named_parameters())
    for k in ("wav2vec2.feature_projection.projection.weight", "wav2vec2.encoder.pos_conv_embed.conv.bias",
              "wav2vec2.encoder.layers.0.attention.v_proj.weight", "wav2vec2.encoder.layers.1.feed_forward.output_dense.bias",
              "wav2vec2.encoder.layer_norm.weight", "lm_head.weight"):
        a, b = P[k].grad.double(), named[k].grad.double()
        assert float((a - b).norm() / b.norm()) <= 1e-3, k


def test_resolve_dropouts_precedence_and_range():
    from coral_amd.modeling import resolve_dropouts

    keys = ("activation_dropout", "attention_dropout", "hidden_dropout", "feat_proj_dropout", "final_dropout")
    assert resolve_dropouts({}, None) == {k: 0.0 for k in keys}
    assert resolve_dropouts({}, {}) == {k: 0.0 for k in keys}
    ckpt = {"hidden_dropout": 0.1, "attention_dropout": 0.05, "final_dropout": 0.2, "activation_dropout": 0.3}
    got = resolve_dropouts({"hidden_dropout": 0.0, "feat_proj_dropout": 0.15, "final_dropout": None}, ckpt)
    # explicit argument > config.json > 0.0; None counts as not given
    assert got == dict(activation_dropout=0.3, attention_dropout=0.05, hidden_dropout=0.0, feat_proj_dropout=0.15,
                       final_dropout=0.2)
    # feat_quantizer_dropout is accepted and ignored (Wav2Vec2ForCTC has no quantizer)
    assert resolve_dropouts({"feat_quantizer_dropout": 0.3}, {}) == {k: 0.0 for k in keys}
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            resolve_dropouts({"attention_dropout": bad}, {})
        with pytest.raises(ValueError):
            resolve_dropouts({}, {"hidden_dropout": bad})


def test_from_pretrained_rejects_a_bad_dropout_before_building_anything(tmp_path, monkeypatch):
    from coral_amd import modeling

    def no_engine(*a, **k):
        raise AssertionError("the model must not be built")

    monkeypatch.setattr(modeling, "Wav2Vec2CTCEngine", no_engine)
    with pytest.raises(ValueError):
        modeling.Wav2Vec2ForCTC.from_pretrained("facebook/wav2vec2-xls-r-300m", final_dropout=1.0)
    (tmp_path / "config.json").write_text(json.dumps(dict(
        hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=[512] * 7,
        conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=16,
        num_conv_pos_embedding_groups=4, vocab_size=46, pad_token_id=45, hidden_dropout=1.2)))
    with pytest.raises(ValueError):
        modeling.Wav2Vec2ForCTC.from_pretrained(str(tmp_path))


def test_save_pretrained_config_keeps_the_five_dropouts():
    from coral_amd.modeling import hf_config, resolve_dropouts
    from coral_amd.wav2vec2 import Wav2Vec2Shape

    drops = dict(activation_dropout=0.1, attention_dropout=0.05, hidden_dropout=0.1, feat_proj_dropout=0.02,
                 final_dropout=0.2)
    shape = Wav2Vec2Shape(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, **drops)
    cfg = json.loads(json.dumps(hf_config(shape, {"mask_time_prob": 0.5})))  # what config.json holds
    assert {k: cfg[k] for k in drops} == drops
    assert resolve_dropouts({}, cfg) == drops  # ... and what loading it back gives
    # the HF side reads the same keys
    transformers = pytest.importorskip("transformers")
    hc = transformers.Wav2Vec2Config(**{k: v for k, v in cfg.items() if k not in ("architectures", "model_type")})
    assert {k: getattr(hc, k) for k in drops} == drops
