"""Whisper path on a real MI355X against the oracle (oracle/whisper_ref.py, pinned to HF) and the HF
fixtures: GPU log-mel (<= 1e-4 abs), encoder states, teacher-forced logits, CE loss,
and greedy generation under an explicit tie-margin policy (bf16 logits can flip near-ties)."""
import numpy as np
import pytest
import torch

from greedy_check import check_greedy_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tiny():
    from oracle import whisper_ref as w

    kw = dict(d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4,
              encoder_ffn_dim=128, decoder_ffn_dim=128, num_mel_bins=80, vocab_size=200, max_target_positions=64,
              pad_token_id=150, decoder_start_token_id=151, eos_token_id=150)
    return kw, w.WhisperConfig(**kw)


def test_logmel_kernel_matches_hf_and_oracle(golden_dir):
    from coral_amd.whisper import WhisperEngine, WhisperShape, mel_filter_bank
    from oracle import whisper_ref as w

    z = np.load(golden_dir / "logmel.npz")
    rng = np.random.RandomState(5)
    t = np.arange(59_200) / 16000.0
    clips = [(0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(len(t))).astype(np.float32),
             (0.1 * rng.randn(480_000)).astype(np.float32)]
    waves = torch.from_numpy(np.stack([w.pad_or_trim(c) for c in clips]))
    for mels in (80, 128):
        np.testing.assert_allclose(mel_filter_bank(mels), z[f"filters{mels}"], atol=1e-7)
        eng = WhisperEngine(WhisperShape(d_model=64, encoder_layers=1, decoder_layers=1, encoder_attention_heads=4,
                                         decoder_attention_heads=4, encoder_ffn_dim=64, decoder_ffn_dim=64,
                                         num_mel_bins=mels, vocab_size=64, max_target_positions=16), DEV)
        feats = eng.log_mel(waves).cpu().numpy()
        assert feats.shape == (2, mels, 3000)
        np.testing.assert_allclose(feats[:, :, ::25], z[f"feat{mels}_sub"], atol=1e-4)
        np.testing.assert_allclose(feats[:, :, :40], z[f"feat{mels}_head"], atol=1e-4)
        ref = np.stack([w.log_mel(x.numpy(), mels) for x in waves])
        assert np.abs(feats - ref).max() <= 1e-4


def test_whisper_forward_loss_and_greedy_vs_oracle(golden_dir):
    from coral_amd.whisper import WhisperEngine, WhisperShape
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    z = np.load(golden_dir / "whisper_tiny.npz")
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    labels = torch.from_numpy(z["labels"])
    eng = WhisperEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(P)
    out = eng.forward(feats, labels=labels)
    enc = out["encoder_last_hidden_state"].float().cpu()
    enc_ref = w.encoder(feats, P, c)
    assert (enc - enc_ref).abs().max() <= 8e-2
    cos = torch.nn.functional.cosine_similarity(enc.flatten(), enc_ref.flatten(), dim=0)
    assert cos >= 0.999
    np.testing.assert_allclose(enc[:, ::100].numpy(), z["enc_slice"], atol=8e-2)     # HF fixture directly
    logits = out["logits"].float().cpu()
    assert (logits - torch.from_numpy(z["logits"])).abs().max() <= 5e-2
    assert abs(float(out["loss"]) - float(z["loss"])) <= 1e-2 * float(z["loss"])
    # greedy: the GPU sequence must be a valid greedy path of the fp32 oracle up to a tie margin
    prefix = [151, 160, 161, 162]
    ids = eng.generate(feats, prefix, 24, suppress_tokens=[170, 171], begin_suppress_tokens=[20, 150])
    want = z["greedy_ids"].tolist()
    enc_o = w.encoder(feats, P, c)
    for seq in ids:
        assert seq[:4] == prefix and len(seq) <= 24

    def rows(b, seq):
        lg = w.decoder(torch.tensor([seq[:-1]]), enc_o[b:b + 1], P, c)[0].clone()
        lg[:, [170, 171]] = float("-inf")
        lg[len(prefix) - 1, [20, 150]] = float("-inf")
        return lg

    # every row: a valid greedy path within 2e-2, forced (bit-exact) outside 5e-2, and a divergence from the HF fixture's
    # ids may only start at a position whose fp32 top-2 margin is inside that tie margin (tests/greedy_check.py)
    check_greedy_rows(rows, ids, want, len(prefix), accept=2e-2, forced=5e-2, label="whisper_tiny")


def test_whisper_inference_forward_is_the_training_forward_bit_for_bit():
    """encode() / decode() run the pre-LN blocks on inference workspaces (no saved states; at M <= 128 rows the FFN's
    LayerNorm inside fc1's prologue), forward_train() on training ones: with every dropout at 0 they give the same
    encoder states and logits bit for bit.  The two fp8 switches stay apart: enable_fp8_encoder() leaves forward_train()
    as it is, enable_fp8_forward() leaves encode() as it is."""
    from coral_amd.whisper import WhisperShape, shift_tokens_right
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV).eval()
    eng.load_state_dict(w.synth_params(c))
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 150, (2, 9), generator=g)
    labels[1, 6:] = -100

    def train_forward():
        out = eng.forward_train(feats, labels)
        return eng._saved["w"]["enc_out"].view(2, -1, kw["d_model"]).clone(), out["logits"].clone()

    enc_t, logits_t = train_forward()
    enc = eng.encode(feats)
    assert torch.equal(enc, enc_t)
    assert torch.equal(eng.decode(shift_tokens_right(labels, c.pad_token_id, c.decoder_start_token_id), enc), logits_t)
    bf16 = enc.clone()
    eng.enable_fp8_encoder()
    enc8 = eng.encode(feats).clone()
    assert not torch.equal(enc8, bf16)  # (the fp8 encoder really ran)
    enc_t2, logits_t2 = train_forward()
    assert torch.equal(enc_t2, enc_t) and torch.equal(logits_t2, logits_t)
    eng.enable_fp8_encoder(False)
    eng.enable_fp8_forward()
    assert torch.equal(eng.encode(feats), bf16)


def test_whisper_medium_shape_smoke():
    """Real head count / dims of whisper-medium on one clip, two layers each (shape plumbing)."""
    from coral_amd.whisper import CORAL_WHISPER_SHAPES, WhisperEngine, WhisperShape

    kw = dict(CORAL_WHISPER_SHAPES["whisper-medium"])
    kw.update(encoder_layers=2, decoder_layers=2)
    eng = WhisperEngine(WhisperShape(**kw), DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    for n in eng.exported_names():
        v = eng.store.view(n)
        if n.endswith("layer_norm.weight"):
            v.fill_(1.0)
        elif n.endswith(".bias"):
            v.zero_()
        else:
            v.normal_(0.0, 0.02, generator=g)
    eng.refresh_compute_weights()
    feats = torch.randn(1, 80, 3000) * 0.3
    out = eng.forward(feats, labels=torch.randint(0, 50000, (1, 12)))
    assert torch.isfinite(out["logits"]).all() and out["logits"].shape == (1, 12, 51865)
    assert np.isfinite(float(out["loss"]))
    ids = eng.generate(feats, [50258, 50285, 50359, 50363], 10)
    assert len(ids[0]) <= 10 and ids[0][:4] == [50258, 50285, 50359, 50363]
    with pytest.raises(ValueError):
        eng.encode(torch.zeros(1, 80, 2000))


def test_whisper_training_step_gradients_vs_oracle():
    """forward_train + backward of the Whisper engine against autograd on the oracle: every parameter
    gradient (tied embedding/LM head, cross-attention K|V projections, conv stem, LayerNorms) with
    cosine >= 0.99 and norm within 6 %; with SpecAugment masks injected on the input features."""
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 150, (2, 11), generator=g)
    labels[1, 7:] = -100
    mt = torch.zeros(2, 3000, dtype=torch.bool)
    mt[0, 100:140] = True
    mt[1, 2000:2100] = True
    mf = torch.zeros(2, 80, dtype=torch.bool)
    mf[0, 10:14] = True
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    fm = feats.clone()
    fm = fm.masked_fill(mt[:, None, :], 0.0).masked_fill(mf[:, :, None], 0.0)
    loss_ref, logits_ref = w.forward_loss(fm, labels, Pr, c)
    loss_ref.backward()

    eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(P)
    eng.zero_grad()
    out = eng.forward_train(feats, labels, mask_time=mt, mask_feature=mf)
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss_ref)) <= 1e-2 * float(loss_ref)
    assert (out["logits"].float().cpu() - logits_ref.detach()).abs().max() <= 5e-2
    bad = []
    for name, gq in eng.grad_dict().items():
        gr = Pr[name].grad
        if name == "model.encoder.embed_positions.weight":
            assert float(gq.abs().sum()) == 0.0  # constant sinusoids (requires_grad False in the reference)
            continue
        if name.endswith("k_proj.bias"):
            continue
        a, b = gq.double().cpu().flatten(), gr.double().flatten()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
        ratio = float(a.norm() / (b.norm() + 1e-30))
        if not (cos >= 0.99 and 0.94 <= ratio <= 1.06):
            bad.append((name, round(cos, 4), round(ratio, 4)))
    assert not bad, bad
    for n in eng.store.names():
        if n.endswith("__zero"):
            assert float(eng.store.view(n, "g32").abs().sum()) == 0.0


def test_whisper_trainer_reduces_loss():
    """The same DataParallelTrainer drives the Whisper engine (clip + AdamW + derived-weight refresh)."""
    from coral_amd.trainer import DataParallelTrainer
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(w.synth_params(c))
    g = torch.Generator().manual_seed(5)
    batch = dict(input_features=torch.randn(2, 80, 3000, generator=g) * 0.5, labels=torch.randint(0, 150, (2, 10), generator=g))
    tr = DataParallelTrainer(eng, learning_rate=3e-3, warmup_steps=2, max_steps=30)
    losses = [float(tr.train_step([batch])) for _ in range(14)]
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[1], losses
    # the internal zero-bias slots never move
    for n in eng.store.names():
        if n.endswith("__zero"):
            assert float(eng.store.view(n).abs().sum()) == 0.0


def test_whisper_single_micro_batch_steps_keep_the_encoder_matrix_gradients_in_bf16(monkeypatch):
    """One micro-batch per optimiser step: the encoder layers' weight-matrix gradients go to AdamW as bf16 (the dtype
    the reference's autocast computes them in; tests/test_finetune_gpu.py has the wav2vec2 form).  Against the fp32 route
    (CA_WGRAD_BF16=0): same first loss, first norm within bf16 rounding of those matrices, the runs stay together."""
    from coral_amd.trainer import DataParallelTrainer
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    g = torch.Generator().manual_seed(5)
    batch = dict(input_features=torch.randn(2, 80, 3000, generator=g) * 0.5, labels=torch.randint(0, 150, (2, 10), generator=g))
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CA_WGRAD_BF16", mode)
        eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
        eng.load_state_dict(w.synth_params(c))
        tr = DataParallelTrainer(eng, learning_rate=1e-3, warmup_steps=1, max_steps=30, max_grad_norm=0.05)
        losses, norms = [], []
        for _ in range(4):
            losses.append(float(tr.train_step([batch])))
            norms.append(tr.grad_norm())
            assert eng.matrix_grads_bf16 == (mode == "1")
        tr.finish()
        torch.cuda.synchronize()
        out[mode] = (losses, norms, eng.store.p32.clone())
    (l0, n0, p0), (l1, n1, p1) = out["0"], out["1"]
    # (the cross-entropy sum is an atomic accumulation: the same parameters give the loss to ~1e-7, not to the bit)
    assert abs(l0[0] - l1[0]) <= 1e-6 * l0[0] and abs(n0[0] - n1[0]) <= 2e-3 * n0[0], (l0, l1, n0, n1)
    assert all(a > 0.05 for a in n0), n0  # the clip is active
    assert np.allclose(l0, l1, rtol=2e-3) and np.allclose(n0, n1, rtol=2e-2), (l0, l1, n0, n1)
    assert float((p0 - p1).abs().max()) <= 4.5e-3


def test_whisper_gradient_norm_without_a_pass_over_the_encoder_matrices(monkeypatch):
    """The trainer's clip norm for the Whisper engine: encoder weight matrices are overwritten by the first
    micro-batch (not cleared, not read back) and contribute through the weight-gradient GEMMs' per-tile sums of squares;
    everything else is normed by a pass over its chunks.  Equal to the norm of the gradient buffer at every step, with
    accumulation micro-batches; and to the run that clears and re-reads everything (CA_FUSED_NORM=0) at the first step."""
    from coral_amd.trainer import DataParallelTrainer
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    g = torch.Generator().manual_seed(5)
    mbs = [dict(input_features=torch.randn(2, 80, 3000, generator=g) * 0.5, labels=torch.randint(0, 150, (2, 10), generator=g))
           for _ in range(2)]
    norms = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("CA_FUSED_NORM", fused)
        eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
        eng.load_state_dict(w.synth_params(c))
        tr = DataParallelTrainer(eng, learning_rate=1e-3, warmup_steps=1, max_steps=30, max_grad_norm=0.05, grad_accum=2,
                                 overlap_optimizer=False)
        assert (tr._norm_plan() is not None) == (fused == "1")
        out = []
        Le = kw["encoder_layers"]
        for step in range(3):
            # in step 1 the second micro-batch drops encoder layer 1, in step 2 the first one does
            keeps = [[not (step == 2 and l == 1) for l in range(Le)], [not (step == 1 and l == 1) for l in range(Le)]]
            tr.train_step([dict(mb, enc_keep=k) for mb, k in zip(mbs, keeps)])
            out.append(tr.grad_norm())
            torch.cuda.synchronize()
            direct = float(eng.store.g32.double().pow(2).sum().sqrt())
            assert abs(out[-1] - direct) <= 1e-5 * direct, (fused, out[-1], direct)
        norms[fused] = out
    assert abs(norms["1"][0] - norms["0"][0]) <= 1e-5 * norms["0"][0], norms
    for n in eng.store.names():
        if n.endswith("__zero"):
            assert float(eng.store.view(n, "g32").abs().sum()) == 0.0


def test_whisper_layerdrop_matches_oracle():
    """LayerDrop decisions are host-drawn; a dropped layer is the identity in forward and backward and
    its parameters get no gradient."""
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 150, (2, 9), generator=g)
    ek = [l != 0 for l in range(c.encoder_layers)]
    dk = [l != c.decoder_layers - 1 for l in range(c.decoder_layers)]
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref = w.forward_loss(feats, labels, Pr, c, ek, dk)
    loss_ref.backward()
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(P)
    eng.zero_grad()
    out = eng.forward_train(feats, labels, enc_keep=ek, dec_keep=dk)
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss_ref)) <= 1e-2 * float(loss_ref)
    assert (out["logits"].float().cpu() - logits_ref.detach()).abs().max() <= 5e-2
    gd = eng.grad_dict()
    for name, gq in gd.items():
        dropped = name.startswith("model.encoder.layers.0.") or name.startswith(f"model.decoder.layers.{c.decoder_layers - 1}.")
        if dropped:
            assert float(gq.abs().sum()) == 0.0, name
    for name in ["model.encoder.conv1.weight", "model.decoder.embed_tokens.weight", "model.decoder.layers.0.fc1.weight",
                 f"model.encoder.layers.{c.encoder_layers - 1}.self_attn.v_proj.weight"]:
        a, b = gd[name].double().cpu().flatten(), Pr[name].grad.double().flatten()
        assert float(a @ b / (a.norm() * b.norm())) >= 0.99, name


def test_whisper_finetune_entry_point(tmp_path):
    """`finetune(config)` with `model=test-whisper` (R/tests/test_finetune.py:8-10 runs exactly this key):
    SpecAugment + LayerDrop drawn on the host, frozen base = only the tied proj_out/embed_tokens matrix
    moves (R/src/coral/whisper.py:88-92), predict-with-generate evaluation, HF-layout save and reload."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "scripts"))
    import finetune_asr_model

    from coral_amd.whisper_setup import WhisperForConditionalGeneration

    res = finetune_asr_model.main(["model=test-whisper", "datasets=synthetic", f"models_dir={tmp_path}", "model_id=wsmoke",
                                   "max_steps=2", "total_batch_size=2", "per_device_batch_size=2",
                                   "max_seconds_per_example=2.0", "min_seconds_per_example=1.0", "logging_steps=1",
                                   "eval_steps=2", "model.max_length=12"])
    hist = res["history"]
    assert any("loss" in h for h in hist) and any("val_wer" in h for h in hist)
    mdir = tmp_path / "wsmoke"
    assert (mdir / "model.safetensors").exists() and (mdir / "config.json").exists()
    assert (mdir / "preprocessor_config.json").exists()
    trained = res["model"].engine.state_dict()
    fresh = WhisperForConditionalGeneration.from_pretrained("openai/whisper-tiny", seed=4242).engine.state_dict()
    moved = [n for n in trained if not torch.equal(trained[n], fresh[n])]
    assert moved == ["model.decoder.embed_tokens.weight"], moved
    again = WhisperForConditionalGeneration.from_pretrained(str(mdir)).engine.state_dict()
    assert all(torch.equal(again[n], trained[n]) for n in trained)


def test_whisper_cached_decode_matches_full_recompute(golden_dir):
    """Incremental decoding with the self-attention K|V cache gives the logits of the teacher-forced
    decoder at every position, and `generate` returns the same ids with and without the cache."""
    from coral_amd.whisper import WhisperEngine, WhisperShape
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    eng = WhisperEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(P)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(3, 80, 3000, generator=g) * 0.5
    ids = torch.randint(0, 150, (3, 9), generator=g)
    enc = eng.encode(feats)
    kv = eng.cross_kv(enc)
    full = eng.decode(ids, enc, kv).float().cpu()  # [B, L, V]
    cache = eng.new_decode_cache(3, 16)
    got = [eng.decode_step(ids[:, :4], kv, cache).float().cpu()]
    for t_ in range(4, 9):
        got.append(eng.decode_step(ids[:, t_:t_ + 1], kv, cache).float().cpu())
    torch.cuda.synchronize()
    assert cache["pos"] == 9
    for j, t_ in enumerate(range(3, 9)):
        assert (got[j] - full[:, t_, :]).abs().max() <= 3e-2, t_
    a = eng.generate(feats, [151, 3, 4, 5], 14, use_cache=True, use_graph=False)
    b = eng.generate(feats, [151, 3, 4, 5], 14, use_cache=False)
    assert a == b
    # the per-token step replayed from a HIP graph (device-side position / length / token state)
    c2 = eng.generate(feats, [151, 3, 4, 5], 14, use_cache=True, use_graph=True)
    assert c2 == a
    long_a = eng.generate(feats, [151, 3, 4, 5], 40, use_graph=False)
    long_g = eng.generate(feats, [151, 3, 4, 5], 40, use_graph=True)
    assert long_g == long_a


@pytest.mark.parametrize("d,H,Tk,B", [(1024, 16, 1500, 8), (1280, 20, 1500, 3), (384, 6, 200, 2), (512, 8, 77, 5)])
def test_decode_attention_with_the_query_projection_inside_is_bit_identical(d, H, Tk, B):
    """ca_decode_attn_qproj (greedy decoding: LayerNorm + q projection + single-query attention over the cached
    encoder K|V in one launch) against the three launches it replaces, on the same inputs: every output bit."""
    from coral_amd import ops

    hd = d // H
    g = torch.Generator(device=DEV).manual_seed(d + Tk)
    x = torch.randn(B, d, device=DEV, generator=g).to(torch.bfloat16)
    gamma = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g)
    beta = 0.1 * torch.randn(d, device=DEV, generator=g)
    W = (0.05 * torch.randn(d, d, device=DEV, generator=g)).to(torch.bfloat16)
    bias = 0.1 * torch.randn(d, device=DEV, generator=g)
    kv = torch.randn(B, Tk, 2 * d, device=DEV, generator=g).to(torch.bfloat16)
    klen = torch.tensor([Tk, max(1, Tk - 37), 1, Tk // 2, Tk, 64, 65, Tk][:B], dtype=torch.int32, device=DEV)
    akw = dict(B=B, H=H, Tk=Tk, hd=hd, scale=hd ** -0.5, ldk=2 * d, ldv=2 * d, ldo=d, skb=Tk * 2 * d, svb=Tk * 2 * d,
               sob=d, k_off=0, v_off=d)
    for kl in (None, klen):
        xn, q = torch.empty_like(x), torch.empty_like(x)
        want, got = torch.zeros(B, d, dtype=torch.bfloat16, device=DEV), torch.ones(B, d, dtype=torch.bfloat16, device=DEV)
        ops.layernorm_fwd(x, gamma, beta, xn, None, B, d, 1e-5)
        ops.gemm(xn, W, q, M=B, N=d, K=d, lda=d, ldb=d, ldc=d, bias=bias)
        ops.attn_fwd(q, kv, kv, want, torch.empty(B * H * 32, device=DEV), Tq=1, Tqp=32, ldq=d, sqb=d, klen=kl, **akw)
        ops.decode_attn_qproj(x, gamma, beta, W, bias, kv, kv, got, d_model=d, eps=1e-5, ldx=d, ldw=d, klen=kl, **akw)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all() and float(want.float().abs().sum()) > 0
        assert torch.equal(got, want), (d, H, Tk, float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("d,H,Tk,B,Tq", [(1024, 16, 1500, 8, 1), (1024, 16, 1500, 2, 1), (1280, 20, 1500, 3, 1), (512, 8, 1100, 5, 7),
                                         (1024, 16, 1500, 16, 1), (1280, 20, 1500, 16, 1), (1024, 16, 1500, 24, 1),
                                         (1024, 16, 1500, 32, 1)])
def test_decode_attention_with_the_keys_dealt_to_several_workgroups(d, H, Tk, B, Tq):
    """CaAttnDesc.split_ws: the keys of one (clip, head) dealt to 2-4 workgroups whose partials the last one to finish
    merges - against fp32 torch and against the one-workgroup launch (same values up to the merge order), the fused
    q-projection form bit-identical to the unfused one under the same split, the counters back at zero after every
    launch (the same workspace serves 30 launches in a row), and no split where B x H already fills the chip.  Between
    one and two rounds of items (320 = 16 clips x 20 heads, 384 = 24 x 16) only the second round's items are split, 4 or
    2 ways (CaKeySplit.tail_start); from two rounds on (512) nothing is."""
    from coral_amd import ops

    hd = d // H
    g = torch.Generator(device=DEV).manual_seed(d + Tk + B)
    x = torch.randn(B, d, device=DEV, generator=g).to(torch.bfloat16)
    gamma, beta = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g), 0.1 * torch.randn(d, device=DEV, generator=g)
    W = (0.05 * torch.randn(d, d, device=DEV, generator=g)).to(torch.bfloat16)
    bias = 0.1 * torch.randn(d, device=DEV, generator=g)
    kv = torch.randn(B, Tk, 2 * d, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(B, Tq, d, device=DEV, generator=g).to(torch.bfloat16)
    klen = torch.tensor([Tk, max(1, Tk - 37), 1, Tk // 2, Tk, 64, 65, Tk] * 4, dtype=torch.int32, device=DEV)[:B]
    ws = ops.attn_split_workspace(B, H, DEV)
    akw = dict(B=B, H=H, Tk=Tk, hd=hd, scale=hd ** -0.5, ldk=2 * d, ldv=2 * d, ldo=d, skb=Tk * 2 * d, svb=Tk * 2 * d, k_off=0, v_off=d)
    nb = (B * H * 4 + 255) // 256 * 256 // 4  # the counters' words
    for kl in (None, klen):
        one, many = (torch.zeros(B, Tq, d, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        lse1, lse2 = torch.zeros(B * H * 32, device=DEV), torch.zeros(B * H * 32, device=DEV)
        common = dict(Tq=Tq, Tqp=32, ldq=d, sqb=Tq * d, sob=Tq * d, klen=kl, **akw)
        ops.attn_fwd(q, kv, kv, one, lse1, **common)
        for _ in range(30):
            ops.attn_fwd(q, kv, kv, many, lse2, split_ws=ws, **common)
        torch.cuda.synchronize()
        assert int(ws[:nb].view(torch.int32).abs().sum()) == 0
        K, V = kv[..., :d].float().view(B, Tk, H, hd).transpose(1, 2), kv[..., d:].float().view(B, Tk, H, hd).transpose(1, 2)
        sc = (q.float().view(B, Tq, H, hd).transpose(1, 2) @ K.transpose(-1, -2)) * hd ** -0.5
        if kl is not None:
            sc = sc.masked_fill(torch.arange(Tk, device=DEV)[None, None, None, :] >= kl[:, None, None, None], float("-inf"))
        ref = (torch.softmax(sc, -1) @ V).transpose(1, 2).reshape(B, Tq, d)
        assert (many.float() - ref).abs().max() < 2e-2
        assert (many.float() - one.float()).abs().max() <= 4e-3  # (bf16 outputs of the same fp32 sums in another order)
        assert (lse2 - lse1).abs().max() < 1e-4
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        if B * H == ncu or B * H >= 2 * ncu:  # nothing to deal: the very same launch
            assert torch.equal(many, one)
        elif B * H > ncu:  # the whole items of the first round are the same launch's, the split ones differ in the last bits
            assert torch.equal(many.view(B * H, -1)[:ncu], one.view(B * H, -1)[:ncu]) if Tq == 1 else True
            assert not torch.equal(many, one)
        if Tq == 1:
            xn, qp = torch.empty_like(x), torch.empty_like(x)
            want, got = torch.zeros(B, d, dtype=torch.bfloat16, device=DEV), torch.ones(B, d, dtype=torch.bfloat16, device=DEV)
            ops.layernorm_fwd(x, gamma, beta, xn, None, B, d, 1e-5)
            ops.gemm(xn, W, qp, M=B, N=d, K=d, lda=d, ldb=d, ldc=d, bias=bias)
            ops.attn_fwd(qp, kv, kv, want, lse1, Tq=1, Tqp=32, ldq=d, sqb=d, sob=d, klen=kl, split_ws=ws, **akw)
            ops.decode_attn_qproj(x, gamma, beta, W, bias, kv, kv, got, d_model=d, eps=1e-5, ldx=d, ldw=d, sob=d, klen=kl,
                                  split_ws=ws, **akw)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
            assert int(ws[:nb].view(torch.int32).abs().sum()) == 0
    if B * H * 2 <= 256:
        with pytest.raises(Exception, match="split_ws"):
            ops.attn_fwd(q, kv, kv, many, lse2, split_ws=ws[:64], **common)


def test_whisper_generate_is_the_same_with_and_without_the_fused_decode_launches(monkeypatch):
    """The graph-replayed token step with ca_decode_attn_qproj (default) and with the three launches it replaces
    (CA_DECODE_FUSED=0): the same ids, token for token."""
    from coral_amd.whisper import WhisperEngine, WhisperShape
    from oracle import whisper_ref as w

    kw, c = _tiny()
    eng = WhisperEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(w.synth_params(c))
    feats = torch.randn(3, 80, 3000, generator=torch.Generator().manual_seed(12)) * 0.5
    monkeypatch.setenv("CA_DECODE_FUSED", "1")
    a = eng.generate(feats, [151, 3, 4, 5], 40, use_graph=True)
    monkeypatch.setenv("CA_DECODE_FUSED", "0")
    b = eng.generate(feats, [151, 3, 4, 5], 40, use_graph=True)
    assert a == b


def test_whisper_large_turbo_shape_training_step_vs_oracle():
    """BASELINE configs[4]'s architecture (whisper-large-v3-turbo: d 1280, 20 heads, 128 mel bins, 51866 tokens)
    at reduced depth (2 + 2 layers), bf16: teacher-forced loss and a few gradients against autograd on the oracle.
    The full 32 + 4-layer shape, bf16 vs the oracle and the fp8 forward vs bf16, is tests/test_fulldepth_gpu.py."""
    from coral_amd.whisper import CORAL_WHISPER_SHAPES, WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw = dict(CORAL_WHISPER_SHAPES["whisper-large-turbo"])
    kw.update(encoder_layers=2, decoder_layers=2)
    c = w.WhisperConfig(**{k: v for k, v in kw.items()})
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(1, 128, 3000, generator=g) * 0.5
    labels = torch.randint(0, 51000, (1, 10), generator=g)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref = w.forward_loss(feats, labels, Pr, c)
    loss_ref.backward()
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
    eng.load_state_dict(P)
    eng.zero_grad()
    out = eng.forward_train(feats, labels)
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss_ref.detach())) <= 1e-2 * float(loss_ref.detach())
    assert (out["logits"].float().cpu() - logits_ref.detach()).abs().max() <= 6e-2
    gd = eng.grad_dict()
    for name in ["model.encoder.conv1.weight", "model.encoder.layers.1.fc1.weight", "model.decoder.embed_tokens.weight",
                 "model.decoder.layers.0.encoder_attn.v_proj.weight", "model.decoder.layers.1.self_attn.q_proj.weight"]:
        a, b = gd[name].double().cpu().flatten(), Pr[name].grad.double().flatten()
        assert float(a @ b / (a.norm() * b.norm())) >= 0.99, name


def test_whisper_hidden_dropout_matches_oracle_with_the_same_masks():
    """WhisperConfig.dropout (R/config/model/whisper-large-turbo.yaml:12 sets 0.1): dropout on the embedded inputs and on
    every sub-layer output in front of its residual add ($TF/models/whisper/modeling_whisper.py:398,406,479,493,502,625,
    763).  The engine's masks are a hash of (step seed, site, element); extracted with `ops.dropout` on a matrix of ones
    and injected into the oracle they must give the same loss, logits and gradients - forward placement, the
    1 / (1 - p) scale and the backward's regenerated masks all checked at once."""
    from coral_amd import ops
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(21)
    B, L, T, d, p = 2, 10, 1500, c.d_model, 0.25
    feats = torch.randn(B, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 150, (B, L), generator=g)
    labels[1, 7:] = -100
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV, dropout=p)
    eng.load_state_dict(P)
    eng.step_seed = 3
    base = eng.step_seed * 4096

    def mask(rows, site):
        ones = torch.ones(rows * d, dtype=torch.bfloat16, device=DEV)
        out = torch.empty_like(ones)
        ops.dropout(ones, out, rows * d, p, base + site)
        m = out.float().cpu().view(rows, d)
        assert set(m.unique().tolist()) <= {0.0, float(torch.tensor(1 / (1 - p)).bfloat16())}
        return m

    masks = {"enc_embed": mask(B * T, 1000), "dec_embed": mask(B * L, 3000)}
    for l in range(c.encoder_layers):
        masks[f"enc{l}.attn"], masks[f"enc{l}.ffn"] = mask(B * T, 256 + l), mask(B * T, 512 + l)
    for l in range(c.decoder_layers):
        masks[f"dec{l}.self"], masks[f"dec{l}.cross"], masks[f"dec{l}.ffn"] = (
            mask(B * L, 2304 + l), mask(B * L, 2560 + l), mask(B * L, 2816 + l))
    keep = float(masks["enc_embed"].ne(0).float().mean())
    assert abs(keep - (1 - p)) < 0.01, keep
    assert not torch.equal(masks["enc0.attn"], masks["enc0.ffn"])  # sites draw different masks
    # bf16(1 / (1 - p)) is what the kernel multiplies by in fp32?  No: it scales in fp32 and rounds the product; on a
    # matrix of ones the product IS the rounded scale, so give the oracle the exact fp32 scale instead
    scale = 1.0 / (1.0 - p)
    masks = {k: (v != 0).float() * scale for k, v in masks.items()}

    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref = w.forward_loss(feats, labels, Pr, c, masks=masks)
    loss_ref.backward()
    eng.zero_grad()
    out = eng.forward_train(feats, labels)
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss_ref)) <= 1e-2 * float(loss_ref), (float(out["loss"]), float(loss_ref))
    assert (out["logits"].float().cpu() - logits_ref.detach()).abs().max() <= 6e-2
    loss_eval, _ = w.forward_loss(feats, labels, P, c)
    assert abs(float(loss_eval) - float(loss_ref)) > 1e-3      # the masks really change the forward
    bad = []
    for name, gq in eng.grad_dict().items():
        gr = Pr[name].grad
        if name == "model.encoder.embed_positions.weight" or name.endswith("k_proj.bias"):
            continue
        a, b = gq.double().cpu().flatten(), gr.double().flatten()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
        ratio = float(a.norm() / (b.norm() + 1e-30))
        if not (cos >= 0.99 and 0.94 <= ratio <= 1.06):
            bad.append((name, round(cos, 4), round(ratio, 4)))
    assert not bad, bad
    # evaluation mode: no dropout
    eng.training = False
    out_eval = eng.forward_train(feats, labels)
    assert abs(float(out_eval["loss"]) - float(loss_eval)) <= 1e-2 * float(loss_eval)


def _keep_mask_np(seed: int, n_rows: int, Tk: int, p: float) -> np.ndarray:
    """NumPy restatement of the kernels' keep decision (common.h: ca_mix32 / ca_dropout_words / ca_dropout_keep) for the
    attention-probability index space: row = (b * H + h) * Tq + q, flat index = row * round_up(Tk, 4) + key.
    -> bool [n_rows, Tk]."""
    M = np.uint64(0xFFFFFFFF)
    tkp = (Tk + 3) & ~3
    idx = (np.arange(n_rows, dtype=np.uint64)[:, None] * np.uint64(tkp) + np.arange(Tk, dtype=np.uint64)[None, :])
    group = idx >> np.uint64(2)
    s = (np.uint64(seed & 0xFFFFFFFF) * np.uint64(0x9E3779B9) + np.uint64(seed >> 32)) & M

    def mix32(x):
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7FEB352D)) & M
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(0x846CA68B)) & M
        return x ^ (x >> np.uint64(16))

    w0 = mix32(((group & M) ^ s ^ (((group >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & M)) & M)
    w1 = (w0 * np.uint64(0xC2B2AE35)) & M
    w1 = w1 ^ (w1 >> np.uint64(15))
    w = np.where((idx & np.uint64(2)) != 0, w1, w0)
    half = (w >> (np.uint64(16) * (idx & np.uint64(1)))) & np.uint64(0xFFFF)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    return half >= thr


def test_whisper_attention_dropout_matches_oracle_with_the_same_masks():
    """Dropout on the attention probabilities ($TF/models/whisper/modeling_whisper.py:234; the reference's smoke config
    test-whisper sets attention_dropout 0.1): applied inside the fused attention kernels after the softmax normaliser,
    regenerated in both backward kernels.  The keep decisions are restated in NumPy from the hash in common.h and
    injected into the oracle: loss, logits and every gradient must agree (forward scale, the dV / dP paths of the
    backward, and the three index conventions - queries in the forward and dQ kernels, keys in the dK/dV kernel)."""
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(22)
    B, L, T, H, p = 2, 10, 1500, c.encoder_attention_heads, 0.2
    feats = torch.randn(B, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 150, (B, L), generator=g)
    labels[0, 8:] = -100
    eng = WhisperTrainEngine(WhisperShape(**kw), DEV, attention_dropout=p)
    eng.load_state_dict(P)
    eng.step_seed = 5
    base = eng.step_seed * 4096
    scale = 1.0 / (1.0 - p)

    def pm(site, Tq, Tk):
        keep = _keep_mask_np(base + site, B * H * Tq, Tk, p)
        return torch.from_numpy(keep.reshape(B, H, Tq, Tk).astype(np.float32)) * scale

    masks = {}
    for l in range(c.encoder_layers):
        masks[f"enc{l}.probs"] = pm(768 + l, T, T)
    for l in range(c.decoder_layers):
        masks[f"dec{l}.self_probs"] = pm(3072 + l, L, L)
        masks[f"dec{l}.cross_probs"] = pm(3328 + l, L, T)
    assert abs(float((masks["enc0.probs"] != 0).float().mean()) - (1 - p)) < 2e-3
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss_ref, logits_ref = w.forward_loss(feats, labels, Pr, c, masks=masks)
    loss_ref.backward()
    eng.zero_grad()
    out = eng.forward_train(feats, labels)
    eng.backward()
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss_ref)) <= 1e-2 * float(loss_ref), (float(out["loss"]), float(loss_ref))
    assert (out["logits"].float().cpu() - logits_ref.detach()).abs().max() <= 6e-2
    loss_eval, _ = w.forward_loss(feats, labels, P, c)
    assert abs(float(loss_eval) - float(loss_ref)) > 1e-4      # the masks change the forward
    bad = []
    for name, gq in eng.grad_dict().items():
        gr = Pr[name].grad
        if name == "model.encoder.embed_positions.weight" or name.endswith("k_proj.bias"):
            continue
        a, b = gq.double().cpu().flatten(), gr.double().flatten()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
        ratio = float(a.norm() / (b.norm() + 1e-30))
        if not (cos >= 0.99 and 0.94 <= ratio <= 1.06):
            bad.append((name, round(cos, 4), round(ratio, 4)))
    assert not bad, bad


def test_whisper_first_micro_batch_overwrites_every_layer_matrix_gradient():
    """Trainer's contract (zero_grad(matrices=False) + backward(overwrite_matrices=True) for a step's first micro-batch):
    the encoder AND decoder layers' weight matrices are neither cleared nor read back - their weight-gradient GEMMs
    overwrite - and the result equals zero-everything-then-accumulate bit for bit, also with a dropped encoder layer and a
    dropped decoder layer (their stale slots are cleared) and when a second micro-batch then accumulates."""
    from coral_amd.whisper import WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine
    from oracle import whisper_ref as w

    kw, c = _tiny()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    labels = torch.randint(0, 200, (2, 6), generator=g)
    nl_e, nl_d = kw["encoder_layers"], kw["decoder_layers"]
    keep = dict(enc_keep=[True] * (nl_e - 1) + [False], dec_keep=[False] + [True] * (nl_d - 1))
    grads = {}
    for mode in ("accumulate", "overwrite"):
        eng = WhisperTrainEngine(WhisperShape(**kw), DEV)
        eng.load_state_dict(w.synth_params(c))
        for step, kws in enumerate((dict(), keep)):
            if mode == "accumulate":
                eng.zero_grad()
            else:
                lo_hi = [eng._enc_matrix_range(l) for l in range(eng.s.encoder_layers)] + [eng._dec_matrix_range(l) for l in range(eng.s.decoder_layers)]
                for lo, hi in lo_hi:  # stale values where nothing is cleared: an overwrite must not see them
                    eng.store.g32[lo:hi].fill_(1e3 * (step + 1))
                eng.zero_grad(matrices=False)
            eng.forward_train(feats, labels, **kws)
            eng.backward(loss_scale=0.5, overwrite_matrices=(mode == "overwrite"))
            eng.forward_train(feats.flip(0), labels.flip(0), **kws)  # second micro-batch: accumulates in both modes
            eng.backward(loss_scale=0.5, overwrite_matrices=False)
            torch.cuda.synchronize()
            grads[(mode, step)] = eng.store.g32.clone()
    for step in (0, 1):
        a, b = grads[("accumulate", step)], grads[("overwrite", step)]
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and float(a.abs().max()) < 1e2
        assert torch.equal(a, b), float((a - b).abs().max())
