"""The wav2vec2 dropouts on the engine: attention, hidden (three sites), feat_proj and final dropout.

The engine draws every mask from a hash of (seed, element); `Wav2Vec2CTCEngine.dropout_site` gives a site's (p, seed).
The masks are taken out of the engine's own kernels (`ops.dropout` on a matrix of ones for the hidden-state sites) or
restated in NumPy (`_keep_mask_np`, the attention probabilities) and injected into the fp32 restatement
tests/w2v2_dropout_ref.py, itself pinned to HF's Wav2Vec2ForCTC by tests/test_w2v2_dropout_ref.py: loss, logits and
every gradient must agree - forward placement, the 1 / (1 - p) scale and the backward's regenerated masks all at once.
Tolerances as in tests/test_w2v2_gpu.py."""
import json

import numpy as np
import pytest
import torch

import w2v2_dropout_ref as dref
from test_whisper_gpu import _keep_mask_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256)
KEYS = ("attention_dropout", "hidden_dropout", "feat_proj_dropout", "final_dropout")


def _batch(lens, lab_lens, seed=4242):
    from oracle import wav2vec2_ref as ref

    g = torch.Generator().manual_seed(seed)
    waves = []
    for n in lens:
        x = (0.1 * torch.randn(int(n), generator=g)).clamp(-1, 1)
        waves.append((x / x.abs().max()).numpy())
    labels = torch.full((len(lens), max(lab_lens)), -100, dtype=torch.long)
    for b, L in enumerate(lab_lens):
        labels[b, :L] = torch.randint(0, 42, (L,), generator=g)
    iv, am = ref.zero_mean_unit_var_norm(waves)
    return torch.from_numpy(iv), torch.from_numpy(am).long(), labels


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _hidden_mask(eng, site, l, B, T):
    """The engine's mask of a hidden-state site ([B*T, d] rows) as factors 0 | 1 / (1 - p), [B, T, d]."""
    from coral_amd import ops

    d = eng.s.hidden_size
    p, seed = eng.dropout_site(site, l)
    ones = torch.ones(B * T * d, dtype=torch.bfloat16, device=DEV)
    out = torch.empty_like(ones)
    ops.dropout(ones, out, B * T * d, p, seed)
    return (out.float().cpu() != 0).float().view(B, T, d) * (1.0 / (1.0 - p))


def _probs_mask(eng, l, B, T):
    p, seed = eng.dropout_site("attention", l)
    H = eng.s.num_attention_heads
    keep = _keep_mask_np(seed, B * H * T, T, p)
    return torch.from_numpy(keep.reshape(B, H, T, T).astype(np.float32)) * (1.0 / (1.0 - p))


def engine_masks(eng, B, T, layer_keep=None):
    """Every mask the engine draws in a training forward (sites with p > 0, kept layers only), restatement keys."""
    s, m = eng.s, {}
    keep = layer_keep or [True] * s.num_hidden_layers
    if s.feat_proj_dropout > 0:
        m["feat_proj"] = _hidden_mask(eng, "feat_proj", 0, B, T)
    if s.hidden_dropout > 0:
        m["pos_conv"] = _hidden_mask(eng, "pos_conv", 0, B, T)
    if s.final_dropout > 0:
        m["final"] = _hidden_mask(eng, "final", 0, B, T)
    for l in range(s.num_hidden_layers):
        if not keep[l]:
            continue
        if s.attention_dropout > 0:
            m[f"layer{l}.attn_probs"] = _probs_mask(eng, l, B, T)
        if s.hidden_dropout > 0:
            m[f"layer{l}.attn_out"] = _hidden_mask(eng, "attn_out", l, B, T)
            m[f"layer{l}.ffn_out"] = _hidden_mask(eng, "ffn_out", l, B, T)
    return m


def _run(kw, drops, lens, lab_lens, step_seed=3, layer_keep=None):
    """Engine (training, given dropouts) vs the restatement with the engine's masks: returns (engine, masks)."""
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    cfg = ref.W2V2Config(**kw)
    P = ref.synth_params(cfg)
    iv, am, labels = _batch(lens, lab_lens)
    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**kw, **drops), DEV).train()
    eng.load_state_dict(P)
    eng.step_seed = step_seed
    eng.zero_grad()
    out = eng(iv, am, labels, layer_keep=layer_keep)
    eng.backward()
    torch.cuda.synchronize()
    B, T = out.logits.shape[:2]
    masks = engine_masks(eng, B, T, layer_keep)
    assert masks, "no site is dropped"
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref, _ = dref.forward_loss(iv, am, labels, Pr, cfg, masks=masks, layer_keep=layer_keep)
    loss_ref.backward()
    loss_eval, _, _ = dref.forward_loss(iv, am, labels, P, cfg, layer_keep=layer_keep)
    loss_ref = float(loss_ref.detach())
    assert abs(loss_ref - float(loss_eval)) > 1e-3 * abs(float(loss_eval))  # the masks really change the forward
    assert abs(float(out.loss) - loss_ref) <= 1e-2 * abs(loss_ref), (float(out.loss), loss_ref)
    assert (out.logits.float().cpu() - logits_ref.detach()).abs().max() <= 6e-2
    bad = []
    for name, g in eng.grad_dict().items():
        gr = Pr[name].grad
        if gr is None:  # unused here (masked_spec_embed without SpecAugment, a dropped layer)
            assert float(g.abs().sum()) == 0.0, name
            continue
        if name.endswith("k_proj.bias"):  # d/d(b_k) == 0 exactly: both sides hold rounding noise (tests/test_w2v2_gpu.py)
            gq = Pr[name.replace("k_proj", "q_proj")].grad.norm()
            assert float(g.norm()) <= 3e-2 * float(gq), name
            continue
        c = _cos(g.cpu(), gr)
        ratio = float(g.norm().cpu() / (gr.norm() + 1e-30))
        if not (c >= 0.99 and 0.94 <= ratio <= 1.06):
            bad.append((name, round(c, 4), round(ratio, 4)))
    assert not bad, bad
    return eng, masks


@pytest.mark.parametrize("key", KEYS + ("all",))
def test_dropout_matches_restatement_with_the_same_masks(key):
    drops = {k: 0.2 for k in KEYS} if key == "all" else {key: 0.2}
    _run(TINY, drops, [4000, 3100], [4, 3])


@pytest.mark.parametrize("d,lens", [(320, [33000, 31500]), (480, [33000, 31500]), (480, [20000, 17000])],
                         ids=["hd80-wide", "hd120-wide", "hd120-narrow"])
def test_head_dim_80_and_120(d, lens):
    """The HDPV = 128 instantiations of the attention kernels with DROP (XLS-R-1B / 2B head sizes): >= 100 frames take the
    128-query kernels, fewer the 64-query ones.  T = 102 / 62: key counts that are not multiples of 4."""
    kw = dict(hidden_size=d, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
              num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=4)
    _run(kw, dict(attention_dropout=0.2, hidden_dropout=0.2), lens, [12, 9])


@pytest.mark.parametrize("side_stream", ["1", "0"])
def test_layerdrop_with_every_dropout(side_stream, monkeypatch):
    """Dropped layers draw no masks; the gradient reaching the kept layer 1 is masked with its FFN-output seed, the one
    leaving it with the seed of the dropout on h0 + pos_conv(h0).  With and without the weight-gradient side stream."""
    monkeypatch.setenv("CA_WGRAD_STREAM", side_stream)
    kw = {**TINY, "num_hidden_layers": 3}
    eng, masks = _run(kw, {k: 0.2 for k in KEYS}, [4000, 3100], [4, 3], layer_keep=[False, True, False])
    assert not any(k.startswith(("layer0", "layer2")) for k in masks)


@pytest.mark.parametrize("C,xf32", [(1024, False), (1280, False), (1920, False), (1024, True)],
                         ids=["1024-bf16x", "1280-bf16x", "1920-bf16x", "1024-f32x"])
def test_layernorm_bwd_dropout_is_layernorm_bwd_then_dropout_bit_for_bit(C, xf32):
    """ca_layernorm_bwd_dropout == ca_layernorm_bwd + ca_dropout_bf16 on dx, dropout(dx) and the d gamma | d beta
    partials, bit for bit (odd row count; the fp32-x form serves C <= 1024)."""
    from coral_amd import ops

    rows, p, seed = 999, 0.15, 123456789012
    g = torch.Generator().manual_seed(C)
    x = torch.randn(rows, C, generator=g).to(DEV, torch.float32 if xf32 else torch.bfloat16)
    dy = torch.randn(rows, C, generator=g).to(DEV, torch.bfloat16)
    dres = torch.randn(rows, C, generator=g).to(DEV, torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    xc = x.float().cpu()
    st = torch.stack([xc.mean(-1), (xc.var(-1, unbiased=False) + 1e-5).rsqrt()], -1).flatten().to(DEV)
    nparts = ops.layernorm_bwd_partial_floats(rows, C)
    dx_a, dx_b, dd = (torch.empty(rows, C, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    dd_a = torch.empty_like(dd)
    part_a = torch.zeros(nparts, dtype=torch.float32, device=DEV)
    part_b = torch.zeros_like(part_a)
    ops.layernorm_bwd(dy, x, gamma, None, st, dres, dx_a, None, None, part_a, rows, C)
    ops.dropout(dx_a, dd_a, rows * C, p, seed)
    ops.layernorm_bwd_dropout(dy, x, gamma, None, st, dres, dx_b, dd, p, seed, None, None, part_b, rows, C)
    torch.cuda.synchronize()
    assert torch.equal(dx_a.view(torch.int16), dx_b.view(torch.int16))
    assert torch.equal(dd_a.view(torch.int16), dd.view(torch.int16))
    assert torch.equal(part_a.view(torch.int32), part_b.view(torch.int32))
    keep = float((dd != 0).float().mean())
    assert abs(keep - (1 - p)) < 0.01
    # ... and with the d gamma | d beta reduction done inside the call
    dgb_a = torch.zeros(2 * C, dtype=torch.float32, device=DEV)
    dgb_b = torch.zeros_like(dgb_a)
    ops.layernorm_bwd(dy, x, gamma, None, st, dres, dx_a, dgb_a[:C], dgb_a[C:], part_a, rows, C)
    ops.layernorm_bwd_dropout(dy, x, gamma, None, st, dres, dx_b, dd, p, seed, dgb_b[:C], dgb_b[C:], part_b, rows, C)
    torch.cuda.synchronize()
    assert torch.equal(dgb_a.view(torch.int32), dgb_b.view(torch.int32))


def test_dropout_properties():
    """Keep rates, distinct masks per site and layer (and apart from the activation dropout's seeds), the same step seed
    reproducing the step bit for bit and another one changing it, and eval() == an engine without dropout."""
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    P = ref.synth_params(ref.W2V2Config(**TINY))
    iv, am, labels = _batch([4000, 3100], [4, 3])
    drops = {k: 0.1 for k in KEYS}
    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**TINY, activation_dropout=0.1, **drops), DEV).train()
    eng.load_state_dict(P)
    eng.step_seed = 9
    B, T = 2, eng.conv_lengths(iv.shape[1])[-1]
    m = engine_masks(eng, B, T)
    kept = sum(float((v != 0).sum()) for v in m.values()) / sum(v.numel() for v in m.values())
    assert abs(kept - 0.9) < 0.01, kept
    hidden = [v for k, v in m.items() if "probs" not in k]
    for i in range(len(hidden)):
        for j in range(i):
            assert not torch.equal(hidden[i], hidden[j])
    seeds = {eng.dropout_site(site, l)[1] for site in ("attention", "attn_out", "ffn_out") for l in range(2)}
    seeds |= {eng.dropout_site(site)[1] for site in ("feat_proj", "pos_conv", "final")}
    assert len(seeds) == 9 and not seeds & {eng.step_seed * 1000 + l for l in range(2)}

    def step(seed):
        eng.step_seed = seed
        eng.zero_grad()
        out = eng(iv, am, labels)
        eng.backward()
        torch.cuda.synchronize()
        return float(out.loss), eng.store.g32.clone()

    l1, g1 = step(9)
    l2, g2 = step(9)
    l3, g3 = step(10)
    assert l1 == l2 and torch.equal(g1, g2)
    assert l3 != l1 and not torch.equal(g1, g3)

    eng.eval()
    ref_eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**TINY), DEV)
    ref_eng.load_state_dict(P)
    for e in (eng, ref_eng):
        e.step_seed = 9
        e.zero_grad()
    oa, ob = eng(iv, am, labels), ref_eng(iv, am, labels)
    eng.backward()
    ref_eng.backward()
    torch.cuda.synchronize()
    assert torch.equal(oa.logits, ob.logits) and float(oa.loss) == float(ob.loss)
    assert torch.equal(eng.store.g32, ref_eng.store.g32)


def test_finetune_with_every_dropout(tmp_path, monkeypatch):
    """CoRal's command line with the four dropouts set (model.* keys): trains, and the saved config.json keeps them."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "scripts"))
    import finetune_asr_model

    from coral_amd import modeling

    monkeypatch.setitem(modeling.HUB_SHAPES, "facebook/wav2vec2-xls-r-300m",
                        dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=4))
    res = finetune_asr_model.main(["model=test-wav2vec2", "datasets=synthetic", f"models_dir={tmp_path}",
                                   "model_id=drop", "max_steps=2", "total_batch_size=2", "per_device_batch_size=2",
                                   "max_seconds_per_example=2.0", "min_seconds_per_example=1.0",
                                   "logging_steps=1", "eval_steps=2", "model.attention_dropout=0.1",
                                   "model.hidden_dropout=0.1", "model.feat_proj_dropout=0.1", "model.final_dropout=0.1"])
    losses = [h["loss"] for h in res["history"] if "loss" in h]
    assert losses and all(np.isfinite(losses))
    s = res["model"].engine.s
    assert (s.attention_dropout, s.hidden_dropout, s.feat_proj_dropout, s.final_dropout) == (0.1, 0.1, 0.1, 0.1)
    cfg = json.loads((tmp_path / "drop" / "config.json").read_text())
    assert all(cfg[k] == 0.1 for k in KEYS)
