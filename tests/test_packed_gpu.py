"""Packed mode of the wav2vec2 training step: the valid frames of a batch laid end to end through the encoder.

Kernel level (CaAttnDesc.row_off, ca_pack_rows / ca_unpack_rows), then the engine against the oracle, the dropout
restatement, the trainer and the evaluation forward.  Every tolerance is the one of the existing test it restates:
tests/test_kernels_gpu.py::test_fused_attention_fwd_bwd (O, lse 2e-2; dQ / dK / dV 3e-2 max(1, max|want|)),
tests/test_w2v2_gpu.py (logits 6e-2 / cosine 0.999, loss 1e-2 rel, gradients cosine 0.99 / norm ratio 5 %) and
tests/test_w2v2_dropout_gpu.py (cosine 0.99, ratio 0.94-1.06)."""
import numpy as np
import pytest
import torch

import w2v2_dropout_ref as dref
from test_w2v2_dropout_gpu import KEYS, TINY, _hidden_mask, _probs_mask
from test_w2v2_gpu import _batch, _cos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0  # sentinel (exact in bf16)
SLACK = 128  # rows behind the packed ones: one tile of the widest kernel


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    return o


def bf(x):
    return x.to(torch.bfloat16)


def _attn_ref(qkv, dO, H, hd):
    """fp32 torch statement of one utterance: qkv [T, 3d], dO [T, d] -> O, lse [H, T], dq, dk, dv [T, d]."""
    T, d = dO.shape

    def heads(x):
        return x.float().view(T, H, hd).transpose(0, 1)

    q, k, v = [heads(qkv[:, i * d:(i + 1) * d]).clone().requires_grad_(True) for i in range(3)]
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    o = torch.softmax(s, -1) @ v
    o.backward(heads(dO))
    un = lambda x: x.transpose(0, 1).reshape(T, d)
    return un(o.detach()), torch.logsumexp(s.detach(), -1), un(q.grad), un(k.grad), un(v.grad)


def _launch(ops, qkv, dO, row_off, Tmax, H, hd, rows):
    """Forward + backward over the packed buffers with sentinel-filled outputs -> (O, lse, dqkv) on the device."""
    d = H * hd
    B = len(row_off) - 1
    Tqp = (Tmax + 31) // 32 * 32
    O = torch.full((rows, d), SENT, dtype=torch.bfloat16, device=DEV)
    dqkv = torch.full((rows, 3 * d), SENT, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, H, Tqp, device=DEV)
    Dq = torch.zeros(B, H, Tqp, device=DEV)
    ro = torch.tensor(row_off, dtype=torch.int32, device=DEV)
    common = dict(B=B, H=H, Tq=Tmax, Tk=Tmax, hd=hd, Tqp=Tqp, scale=hd ** -0.5, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d,
                  sqb=0, skb=0, svb=0, sob=0, q_off=0, k_off=d, v_off=2 * d, row_off=ro)
    ops.attn_fwd(qkv, qkv, qkv, O, lse, **common)
    ops.attn_bwd(qkv, qkv, qkv, O, lse, dO, Dq, dqkv, dqkv, dqkv, lddo=d, sdob=0, lddq=3 * d, lddk=3 * d, lddv=3 * d,
                 sdqb=0, sdkb=0, sdvb=0, dq_off=0, dk_off=d, dv_off=2 * d, **common)
    torch.cuda.synchronize()
    return O, lse, dqkv


LEN_SETS = {"tiles": [499, 1, 31, 33, 64, 65, 250], "edges": [130, 129, 127], "small": [12, 5], "wide": [100, 257, 128, 191]}


@pytest.mark.parametrize("hd", [64, 80, 120, 128])
@pytest.mark.parametrize("name", list(LEN_SETS))
def test_varlen_attention_and_neighbours(ops, hd, name):
    """ca_attn_fwd / ca_attn_bwd with row_off per utterance against the fp32 statement; no workgroup writes a row of
    another utterance (each utterance alone == the joint launch, bit for bit) nor a row at or past Mp."""
    lens = LEN_SETS[name]
    H = 2
    d = H * hd
    row_off = [0] + list(np.cumsum(lens))
    Mp, Tmax = int(row_off[-1]), max(lens)
    rows = Mp + SLACK
    g = torch.Generator().manual_seed(hd + Mp)
    qkv = bf(torch.randn(rows, 3 * d, generator=g))
    dO = bf(torch.randn(rows, d, generator=g))
    qkv_d, dO_d = qkv.to(DEV), dO.to(DEV)
    O, lse, dqkv = _launch(ops, qkv_d, dO_d, row_off, Tmax, H, hd, rows)
    # (b) nothing at or past Mp
    assert bool((O[Mp:] == SENT).all()) and bool((dqkv[Mp:] == SENT).all())
    assert bool((O[:Mp] != SENT).any(-1).all()) and bool((dqkv[:Mp] != SENT).any(-1).all())  # every valid row written
    Oc, lsec, dc = O.float().cpu(), lse.cpu(), dqkv.float().cpu()
    figures = []
    for b, n in enumerate(lens):
        r0 = row_off[b]
        o_ref, lse_ref, dq, dk, dv = _attn_ref(qkv[r0:r0 + n], dO[r0:r0 + n], H, hd)
        e_o = (Oc[r0:r0 + n] - o_ref).abs().max().item()
        e_l = (lsec[b, :, :n] - lse_ref).abs().max().item()
        figures.append((n, e_o, e_l))
        assert e_o < 2e-2 and e_l < 2e-2, (b, n, e_o, e_l)
        for i, want in enumerate((dq, dk, dv)):
            err = (dc[r0:r0 + n, i * d:(i + 1) * d] - want).abs().max().item()
            assert err < 3e-2 * max(1.0, want.abs().max().item()), (b, n, i, err, want.abs().max().item())
    print("varlen", hd, name, figures)
    # (a) utterance b alone (same launch maxima, hence the same kernels): its rows bit for bit, every other row untouched
    for b, n in enumerate(lens):
        r0 = int(row_off[b])
        O1, lse1, d1 = _launch(ops, qkv_d, dO_d, [r0, r0 + n], Tmax, H, hd, rows)
        assert torch.equal(O1[r0:r0 + n].view(torch.int16), O[r0:r0 + n].view(torch.int16)), b
        assert torch.equal(d1[r0:r0 + n].view(torch.int16), dqkv[r0:r0 + n].view(torch.int16)), b
        assert torch.equal(lse1[0, :, :n], lse[b, :, :n]), b
        assert bool((O1[:r0] == SENT).all()) and bool((O1[r0 + n:] == SENT).all()), b
        assert bool((d1[:r0] == SENT).all()) and bool((d1[r0 + n:] == SENT).all()), b


@pytest.mark.parametrize("hd,T", [(64, 70), (64, 130), (120, 130), (80, 33)])
def test_equal_lengths_equal_the_padded_launch(ops, hd, T):
    """row_off built from equal lengths T == the launch without row_off on the same data, bit for bit."""
    B, H = 3, 2
    d = H * hd
    g = torch.Generator().manual_seed(T + hd)
    rows = B * T + SLACK
    qkv = bf(torch.randn(rows, 3 * d, generator=g)).to(DEV)
    dO = bf(torch.randn(rows, d, generator=g)).to(DEV)
    O, lse, dqkv = _launch(ops, qkv, dO, [0, T, 2 * T, 3 * T], T, H, hd, rows)
    Tqp = (T + 31) // 32 * 32
    O2 = torch.full((rows, d), SENT, dtype=torch.bfloat16, device=DEV)
    d2 = torch.full((rows, 3 * d), SENT, dtype=torch.bfloat16, device=DEV)
    lse2, Dq2 = torch.zeros(B, H, Tqp, device=DEV), torch.zeros(B, H, Tqp, device=DEV)
    common = dict(B=B, H=H, Tq=T, Tk=T, hd=hd, Tqp=Tqp, scale=hd ** -0.5, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d,
                  sqb=T * 3 * d, skb=T * 3 * d, svb=T * 3 * d, sob=T * d, q_off=0, k_off=d, v_off=2 * d)
    ops.attn_fwd(qkv, qkv, qkv, O2, lse2, **common)
    ops.attn_bwd(qkv, qkv, qkv, O2, lse2, dO, Dq2, d2, d2, d2, lddo=d, sdob=T * d, lddq=3 * d, lddk=3 * d, lddv=3 * d,
                 sdqb=T * 3 * d, sdkb=T * 3 * d, sdvb=T * 3 * d, dq_off=0, dk_off=d, dv_off=2 * d, **common)
    torch.cuda.synchronize()
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16))
    assert torch.equal(dqkv.view(torch.int16), d2.view(torch.int16))
    assert torch.equal(lse[:, :, :T], lse2[:, :, :T])


def test_row_off_refuses_what_it_does_not_cover(ops):
    from coral_amd.ops import CoralAmdError

    H, hd, T = 2, 64, 40
    d = H * hd
    qkv = torch.zeros(2 * T + SLACK, 3 * d, dtype=torch.bfloat16, device=DEV)
    O = torch.zeros(2 * T + SLACK, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(2, H, 64, device=DEV)
    ro = torch.tensor([0, T, 2 * T], dtype=torch.int32, device=DEV)
    kw = dict(B=2, H=H, Tq=T, Tk=T, hd=hd, Tqp=64, scale=1.0, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, sqb=0, skb=0,
              svb=0, sob=0, k_off=d, v_off=2 * d, row_off=ro)
    for bad in (dict(causal=True), dict(klen=torch.tensor([T, T], dtype=torch.int32, device=DEV)), dict(Tk=T + 8)):
        with pytest.raises(CoralAmdError, match="row_off"):
            ops.attn_fwd(qkv, qkv, qkv, O, lse, **{**kw, **bad})


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("C", [48, 128, 1920])
def test_pack_unpack_round_trip(ops, dt, C):
    """pack_rows -> unpack_rows: valid rows identical, padded rows exactly zero, nothing written at or past Mp."""
    B, T = 4, 37
    lens = [37, 1, 20, 36]
    row_off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    Mp = sum(lens)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, T, C, generator=g).to(dt).to(DEV)
    y = torch.full((B * T, C), SENT, dtype=dt, device=DEV)
    z = torch.full((B, T, C), SENT, dtype=dt, device=DEV)
    ops.pack_rows(x, y, row_off, B, T, C)
    ops.unpack_rows(y, z, row_off, B, T, C)
    torch.cuda.synchronize()
    assert bool((y[Mp:] == SENT).all())
    r = 0
    for b, n in enumerate(lens):
        assert torch.equal(y[r:r + n], x[b, :n]) and torch.equal(z[b, :n], x[b, :n])
        assert bool((z[b, n:] == 0).all())
        r += n


# ---- engine vs oracle ------------------------------------------------------------------------------------------------
def _oracle_case(cfg_kw, lens, lab_lens, pack, mask_time=None, layer_keep=None):
    """The body of tests/test_w2v2_gpu.py::_run_case on a training-mode engine (all dropouts 0) with pack_frames = pack."""
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    cfg = ref.W2V2Config(**cfg_kw)
    P = ref.synth_params(cfg)
    iv, am, labels = _batch(lens, lab_lens)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    kw = {} if mask_time is None else {"mask_time": mask_time}
    if layer_keep is None:
        loss_ref, logits_ref, _ = ref.forward_loss(iv, am, labels, Pr, cfg, **kw)
    else:  # (the restatement with LayerDrop; without masks it is the oracle's arithmetic)
        loss_ref, logits_ref, _ = dref.forward_loss(iv, am, labels, Pr, cfg, layer_keep=layer_keep, **kw)
    loss_ref.backward()
    logits_ref = logits_ref.detach()

    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**cfg_kw, activation_dropout=0.0), DEV)
    eng.pack_frames = pack
    eng.train()
    eng.load_state_dict(P)
    eng.zero_grad()
    out = eng(iv, am, labels, layer_keep=layer_keep, **kw)
    eng.backward()
    torch.cuda.synchronize()
    B, T = out.logits.shape[:2]
    flen = eng.feat_lengths(am.sum(-1)).tolist()
    if pack:
        assert eng.last_rows == sum(flen) < B * T, (eng.last_rows, flen, B * T)
    else:
        assert eng.last_rows == B * T
    logits = out.logits.float().cpu()
    assert torch.isfinite(logits).all()
    valid = torch.arange(T)[None, :] < torch.tensor(flen)[:, None]
    if pack:
        assert float(logits[~valid].abs().max()) == 0.0
    err = (logits[valid] - logits_ref[valid]).abs().max().item()
    cos = _cos(logits[valid], logits_ref[valid])
    rel = abs(float(out.loss) - float(loss_ref)) / abs(float(loss_ref))
    print("oracle case", cfg_kw["hidden_size"], "pack" if pack else "padded", "logits", err, cos, "loss rel", rel)
    assert err <= 6e-2 and cos >= 0.999, (err, cos)
    assert rel <= 1e-2, (float(out.loss), float(loss_ref))
    bad = []
    for name, g in eng.grad_dict().items():
        gr = Pr[name].grad
        if gr is None or (layer_keep is not None and float(gr.abs().sum()) == 0.0):  # unused here / a dropped layer
            assert float(g.abs().sum()) == 0.0, name
            continue
        if name.endswith("k_proj.bias"):  # d/d(b_k) == 0 exactly (tests/test_w2v2_gpu.py)
            gq = Pr[name.replace("k_proj", "q_proj")].grad.norm()
            assert float(gr.norm()) <= 1e-3 * float(gq)
            assert float(g.norm()) <= 3e-2 * float(gq), (name, float(g.norm()), float(gq))
            continue
        c = _cos(g.cpu(), gr)
        ratio = float(g.norm().cpu() / (gr.norm() + 1e-30))
        if not (c >= 0.99 and 0.95 <= ratio <= 1.05):
            bad.append((name, round(c, 4), round(ratio, 4)))
    assert not bad, bad
    return eng


def _mask_time():
    mt = torch.zeros(3, 12, dtype=torch.bool)
    mt[0, 2:5] = True
    mt[1, 0:2] = True
    mt[2, 7] = True
    return mt


CASES = {
    "tiny": (TINY, [4000, 3400, 2800], [5, 3, 4], {}),
    "d1920": (dict(hidden_size=1920, num_hidden_layers=1, num_attention_heads=16, intermediate_size=512),
              [16000, 12000], [12, 7], {}),
    "d1280": (dict(hidden_size=1280, num_hidden_layers=1, num_attention_heads=16, intermediate_size=512),
              [9000, 16000], [4, 10], {}),
    "specaugment": (TINY, [4000, 3400, 2800], [5, 3, 4], dict(mask_time=_mask_time())),
    "layerdrop": ({**TINY, "num_hidden_layers": 3}, [4000, 3400, 2800], [5, 3, 4], dict(layer_keep=[False, True, False])),
}


@pytest.mark.parametrize("case", list(CASES))
def test_engine_packed_matches_oracle(case):
    cfg_kw, lens, lab_lens, kw = CASES[case]
    _oracle_case(cfg_kw, lens, lab_lens, True, **kw)
    _oracle_case(cfg_kw, lens, lab_lens, False, **kw)


# ---- dropouts --------------------------------------------------------------------------------------------------------
def _packed_hidden_mask(eng, site, l, flen, T):
    """The mask of a site inside the packed region: drawn over Mp * d ones, scattered to [B, T, d] (padded frames 0)."""
    from coral_amd import ops

    d, Mp = eng.s.hidden_size, sum(flen)
    p, seed = eng.dropout_site(site, l)
    ones = torch.ones(Mp * d, dtype=torch.bfloat16, device=DEV)
    out = torch.empty_like(ones)
    ops.dropout(ones, out, Mp * d, p, seed)
    m = (out.float().cpu() != 0).float().view(Mp, d) * (1.0 / (1.0 - p))
    full, r = torch.zeros(len(flen), T, d), 0
    for b, n in enumerate(flen):
        full[b, :n] = m[r:r + n]
        r += n
    return full


def test_dropouts_packed_match_restatement():
    """tests/test_w2v2_dropout_gpu.py::_run with every dropout at 0.2 on a packed step: the sites inside the packed
    region hash the packed flat index, feat_proj / pos_conv the [B, T, d] one, the probability masks are unchanged."""
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    cfg = ref.W2V2Config(**TINY)
    P = ref.synth_params(cfg)
    iv, am, labels = _batch([4000, 3100], [4, 3])
    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**TINY, **{k: 0.2 for k in KEYS}), DEV).train()
    eng.pack_frames = True
    eng.load_state_dict(P)
    eng.step_seed = 3
    eng.zero_grad()
    out = eng(iv, am, labels)
    eng.backward()
    torch.cuda.synchronize()
    B, T = out.logits.shape[:2]
    flen = eng.feat_lengths(am.sum(-1)).tolist()
    assert eng.last_rows == sum(flen) < B * T
    masks = dict(feat_proj=_hidden_mask(eng, "feat_proj", 0, B, T), pos_conv=_hidden_mask(eng, "pos_conv", 0, B, T),
                 final=_packed_hidden_mask(eng, "final", 0, flen, T))
    for l in range(2):
        masks[f"layer{l}.attn_probs"] = _probs_mask(eng, l, B, T)
        masks[f"layer{l}.attn_out"] = _packed_hidden_mask(eng, "attn_out", l, flen, T)
        masks[f"layer{l}.ffn_out"] = _packed_hidden_mask(eng, "ffn_out", l, flen, T)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref, _ = dref.forward_loss(iv, am, labels, Pr, cfg, masks=masks)
    loss_ref.backward()
    loss_eval, _, _ = dref.forward_loss(iv, am, labels, P, cfg)
    loss_ref = float(loss_ref.detach())
    assert abs(loss_ref - float(loss_eval)) > 1e-3 * abs(float(loss_eval))
    assert abs(float(out.loss) - loss_ref) <= 1e-2 * abs(loss_ref), (float(out.loss), loss_ref)
    valid = torch.arange(T)[None, :] < torch.tensor(flen)[:, None]
    logits = out.logits.float().cpu()
    assert (logits[valid] - logits_ref.detach()[valid]).abs().max() <= 6e-2
    assert float(logits[~valid].abs().max()) == 0.0
    bad = []
    for name, g in eng.grad_dict().items():
        gr = Pr[name].grad
        if gr is None:
            assert float(g.abs().sum()) == 0.0, name
            continue
        if name.endswith("k_proj.bias"):
            gq = Pr[name.replace("k_proj", "q_proj")].grad.norm()
            assert float(g.norm()) <= 3e-2 * float(gq), name
            continue
        c = _cos(g.cpu(), gr)
        ratio = float(g.norm().cpu() / (gr.norm() + 1e-30))
        if not (c >= 0.99 and 0.94 <= ratio <= 1.06):
            bad.append((name, round(c, 4), round(ratio, 4)))
    assert not bad, bad


# ---- trainer / evaluation --------------------------------------------------------------------------------------------
def _trainer_losses(pack, lens, steps):
    from coral_amd.trainer import DataParallelTrainer
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    P = ref.synth_params(ref.W2V2Config(**TINY))
    iv, am, labels = _batch(lens, [5, 3, 4])
    eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**TINY), DEV)
    eng.pack_frames = pack
    eng.load_state_dict(P)
    tr = DataParallelTrainer(eng, learning_rate=1e-3, warmup_steps=0, max_steps=100, max_grad_norm=1.0)
    batch = dict(input_values=iv, attention_mask=am, labels=labels)
    losses, first, rows = [], None, []
    for i in range(steps):
        losses.append(float(tr.train_step([batch])))
        rows.append(eng.last_rows)
        if i == 0:
            first = eng._saved["w"]["logits"].clone()
    tr.finish()
    torch.cuda.synchronize()
    return losses, first, rows, eng


@pytest.mark.parametrize("side_stream", ["1", "0"])
def test_trainer_packed_tracks_the_padded_run(side_stream, monkeypatch):
    """Six optimiser steps on a ragged batch, pack_frames on and off from the same weights: per-step losses within the
    whole-model bound of tests/test_w2v2_gpu.py (1e-2 rel) of each other, with and without the weight-gradient stream."""
    monkeypatch.setenv("CA_WGRAD_STREAM", side_stream)
    lens = [4000, 3400, 2800]
    on, _, rows_on, eng = _trainer_losses(True, lens, 6)
    off, _, rows_off, _ = _trainer_losses(False, lens, 6)
    print("trainer losses packed", on, "padded", off)
    assert rows_on == [30] * 6 and rows_off == [36] * 6, (rows_on, rows_off)
    assert np.isfinite(on).all() and on[-1] < on[0]
    for a, b in zip(on, off):
        assert abs(a - b) <= 1e-2 * abs(b), (on, off)


def test_full_batch_with_the_switch_on_takes_the_unpacked_launches():
    lens = [4000, 4000, 4000]
    on, lg_on, rows_on, _ = _trainer_losses(True, lens, 1)
    off, lg_off, rows_off, _ = _trainer_losses(False, lens, 1)
    assert rows_on == rows_off == [36]
    assert on == off and torch.equal(lg_on, lg_off)


def test_eval_forward_stays_padded():
    from coral_amd.wav2vec2 import Wav2Vec2CTCEngine, Wav2Vec2Shape
    from oracle import wav2vec2_ref as ref

    P = ref.synth_params(ref.W2V2Config(**TINY))
    iv, am, labels = _batch([4000, 3400, 2800], [5, 3, 4])
    outs = []
    for pack in (True, False):
        eng = Wav2Vec2CTCEngine(Wav2Vec2Shape(**TINY), DEV)
        eng.pack_frames = pack
        eng.load_state_dict(P)
        eng.eval()
        o = eng(iv, am, labels)
        assert eng.last_rows == 36
        first = (o.logits.clone(), float(o.loss))  # (out.logits is a view of the workspace: the next forward rewrites it)
        o2 = eng.train()(iv, am)  # (no labels: nothing to train on, the padded layout)
        assert eng.last_rows == 36
        torch.cuda.synchronize()
        outs.append((*first, o2.logits.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
