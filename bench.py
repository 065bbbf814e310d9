#!/usr/bin/env python3
"""Headline benchmark: audio-seconds/sec of CTC finetuning steps (fwd + bwd + gradient all-reduce +
clip + AdamW) for CoRal's `model=wav2vec2-large` (XLS-R-2B shape) on synthetic 16 kHz audio,
8 x 10 s utterances per GPU, bf16 MFMA compute / fp32 master weights.  BASELINE.json configs[1]
(N=1) and configs[2] (N=8, weak scaling).

    python bench.py --gpus 1 --steps 8 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0: metric/value/unit/ms_per_step/... of the headline.  A plain run does only that: set-up,
`--warmup` untimed and `--steps` timed steps, the line.  `--full` adds everything else, each measured after the headline:
  roofline     — dominant GEMM template, live hipEvent timing through ca_prof_begin/end (two extra profiled steps)
  config.fwd_bwd / config.fp32_matrix_gradients — the same step without the optimiser / on the fp32 gradient route
  config.also* — the secondary workloads (N=1, wav2vec2-large); config.also_zero2 — the sharded optimiser (N>1)
  cpu_baseline — the oracle (oracle/wav2vec2_ref.py) timed on the host cores (N=1 only)
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (float32 / float64, 64 MB at most).
`--model whisper-* --decode` keeps its per-token time (config.ms_per_token, two more timed generation lengths) without
`--full`: it is that workload's headline figure (BASELINE.json configs[3]).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # before the HIP runtime initialises (see coral_amd/__init__.py)

import torch  # noqa: E402

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

MFMA_BF16_DENSE_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md: ~2.5 PF dense (spec)
DUMP_PARAM_SAMPLE = 1 << 22   # --dump-outputs: fp32 master weights sampled (16 MB per array)
DUMP_SAMPLE_SEED = 4243
DUMP_MAX_BYTES = 64 << 20


def param_sample_index(trainer, device):
    """--dump-outputs: a fixed, seeded sample of the trainable fp32 master weights (sorted flat offsets, the same for
    every run of one model); None where the master is sharded over the ranks (zero_stage 2: a rank keeps only its
    own slice up to date)."""
    if trainer is None or getattr(trainer, "zero", False):
        return None
    lo, hi = trainer.train_range
    g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
    idx = torch.randint(lo, hi, (min(DUMP_PARAM_SAMPLE, hi - lo),), generator=g, dtype=torch.int64)
    return idx.sort().values.to(device)


def write_outputs(out_dir, arrays):
    """--dump-outputs: every array as <out_dir>/<name>.npy - floating point as float32 (float64 stays float64), integers
    as float64 (exact) - at most DUMP_MAX_BYTES in all."""
    import numpy as np

    conv = {}
    for name, a in arrays.items():
        t = torch.as_tensor(a).detach().cpu()
        conv[name] = t.to(torch.float32 if t.is_floating_point() and t.dtype != torch.float64 else torch.float64).numpy()
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_MAX_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes, more than {DUMP_MAX_BYTES}")
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in conv.items():
        np.save(d / f"{name}.npy", a)


def fwd_gflop_per_utt(shape, T: int, conv_lens) -> float:
    """cnn + featproj + posconv + L*T*(8 d^2 + 4 d ffn) + L*4 T^2 d + 2 d V T."""
    d, f, L, V = shape.hidden_size, shape.intermediate_size, shape.num_hidden_layers, shape.vocab_size
    cnn, cin = 0.0, 1
    for co, k, n in zip(shape.conv_dim, shape.conv_kernel, conv_lens):
        cnn += 2.0 * n * co * cin * k
        cin = co
    featproj = 2.0 * T * cin * d
    K, G = shape.num_conv_pos_embeddings, shape.num_conv_pos_embedding_groups
    posconv = 2.0 * T * d * (d // G) * K
    enc = L * T * (8.0 * d * d + 4.0 * d * f) + L * 4.0 * T * T * d
    head = 2.0 * d * V * T
    return (cnn + featproj + posconv + enc + head) / 1e9


def init_random_(engine, seed: int):
    """Seeded random-init weights generated on the device (no checkpoints exist offline)."""
    g = torch.Generator(device=engine.device).manual_seed(seed)
    st = engine.store
    for name, (off, shape) in st.index.items():
        v = st.view(name)
        if name.endswith("layer_norm.weight"):
            v.normal_(1.0, 0.05, generator=g)
        elif name.endswith("original0"):
            v.uniform_(1.0, 1.25, generator=g)
        elif name.endswith(".bias") or name.endswith("masked_spec_embed"):
            v.normal_(0.0, 0.02, generator=g)
        else:
            fan_in = 1
            for s_ in shape[1:]:
                fan_in *= s_
            v.normal_(0.0, fan_in ** -0.5, generator=g)
    engine.refresh_compute_weights()


def synth_batch(B, seconds, rank, device, ragged=False):
    """0.1*randn clipped, peak-normalised, then the feature extractor's zero-mean /
    unit-variance (done on the GPU by ca_wave_normalize); labels U{0..41}, length U{20..120}."""
    from coral_amd import ops

    N = int(16000 * seconds)
    g = torch.Generator().manual_seed(4242 + rank)
    x = (0.1 * torch.randn(B, N, generator=g)).clamp_(-1, 1)
    x = x / x.abs().amax(dim=1, keepdim=True)
    lens = torch.full((B,), N, dtype=torch.int32)
    if ragged:
        lens = torch.randint(16000, N + 1, (B,), generator=g, dtype=torch.int32)
    am = (torch.arange(N)[None, :] < lens[:, None]).to(torch.int32)
    xd, y = x.to(device), torch.empty(B, N, device=device)
    ops.wave_normalize(xd, lens.to(device), y, B, N)
    tl = torch.randint(20, 121, (B,), generator=g)
    labels = torch.full((B, int(tl.max())), -100, dtype=torch.int32)
    for b in range(B):
        labels[b, :tl[b]] = torch.randint(0, 42, (int(tl[b]),), generator=g, dtype=torch.int32)
    return dict(input_values=y, attention_mask=am.to(device), labels=labels.to(device)), lens


def cpu_model_name() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def cpu_baseline(max_threads: int = 32, budget_s: float = 75.0):
    """the oracle (fp32 torch CPU restatement of the HF path, oracle/wav2vec2_ref.py) timed on this
    box's host cores on BASELINE configs[0] — XLS-R-300M shape, 4 x 5 s utterances, forward + backward incl. CTC —
    3 warm-up + 5 timed iterations, median (fewer if the wall budget runs out first; the counts are in `sample`).
    Threads are capped at 32: torch's CPU GEMMs get slower, not faster, when oversubscribed on the 256-thread GPU
    host (a 10 s utterance at the 2B shape took 647 s there with all threads)."""
    import statistics

    import numpy as np

    from oracle import wav2vec2_ref as ref

    cores = min(os.cpu_count() or 1, max_threads)
    torch.set_num_threads(cores)
    cfg = ref.W2V2Config(**ref.CORAL_SHAPES["wav2vec2-small"])
    g = torch.Generator().manual_seed(4242)
    P = {}
    for name, shape in ref.param_shapes(cfg).items():
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
        if name.endswith("layer_norm.weight") or name.endswith("original0"):
            t = torch.ones(shape)
        elif name.endswith(".bias") or name.endswith("masked_spec_embed"):
            t = torch.zeros(shape)
        else:
            t = torch.empty(shape).normal_(0.0, fan_in ** -0.5, generator=g)
        P[name] = t.requires_grad_(True)
    B, seconds = 4, 5.0
    N = int(16000 * seconds)
    x = 0.1 * torch.randn(B, N, generator=g)
    x = (x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True)
    labels = torch.randint(0, 42, (B, 40), generator=g)

    def once():
        for t in P.values():
            t.grad = None
        t0 = time.perf_counter()
        loss, _, _ = ref.forward_loss(x, None, labels, P, cfg)
        loss.backward()
        return time.perf_counter() - t0

    t_begin = time.perf_counter()
    warm, times = 0, []
    while warm < 3 and (warm == 0 or time.perf_counter() - t_begin < 0.3 * budget_s):
        once()
        warm += 1
    while len(times) < 5 and (len(times) < 2 or time.perf_counter() - t_begin < budget_s):
        times.append(once())
    med = statistics.median(times)
    return {"value": round(B * seconds / med, 3), "unit": "audio-seconds/sec", "cores": cores, "kind": "port",
            "cpu": cpu_model_name(),
            "sample": f"BASELINE configs[0]: {B} x {seconds:g} s utterances, wav2vec2-small (XLS-R-300M) shape, "
                      f"fwd+bwd+CTC fp32; {warm} warm-up + {len(times)} timed iterations, median {med:.2f} s "
                      f"(min {min(times):.2f}, max {max(times):.2f}); oracle/wav2vec2_ref.py, torch {torch.__version__} "
                      f"CPU, {cores} threads (capped: oversubscribed CPU GEMMs get slower on the {os.cpu_count()}-thread host)"}


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks (one per GPU) through torch.distributed.run as a
    child process and return its exit code."""
    import subprocess

    ndev = torch.cuda.device_count()  # counts devices without initialising the GPU runtime
    # CA_BENCH_SHARE_GPU=1 (tests on a single-GPU box): the ranks share the visible devices round-robin; only
    # meaningful with --backend gloo, never for a reported number
    if ndev < n and not (os.environ.get("CA_BENCH_SHARE_GPU") == "1" and ndev >= 1):
        print(f"bench.py: --gpus {n} but only {ndev} GPU(s) are visible", file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1", f"--nproc-per-node={n}",
           "--local-addr", "127.0.0.1", str(Path(__file__).resolve())] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def whisper_setup_engine(model, device, rank, B):
    """Random-init Whisper training engine of a CoRal model key + one synthetic batch (0.1*randn clips of
    7..30 s zero-padded to 30 s, labels U{0..50256} of length U{20..120})."""
    import numpy as np
    import yaml

    from coral_amd.whisper import CORAL_WHISPER_SHAPES, N_SAMPLES, WhisperShape
    from coral_amd.whisper_train import WhisperTrainEngine

    shape = WhisperShape(**CORAL_WHISPER_SHAPES[model])
    # dropouts of the CoRal model key (config/model/<key>.yaml = R/config/model/<key>.yaml): whisper-medium trains with
    # activation_dropout 0.1, whisper-large-turbo with hidden-state dropout 0.1
    mcfg = yaml.safe_load((ROOT / "config" / "model" / f"{model}.yaml").read_text())
    eng = WhisperTrainEngine(shape, device, activation_dropout=float(mcfg.get("activation_dropout", 0.0)),
                             dropout=float(mcfg.get("dropout", 0.0)))
    g = torch.Generator(device=device).manual_seed(4242)
    for n in eng.exported_names():
        v = eng.store.view(n)
        if n.endswith("layer_norm.weight"):
            v.fill_(1.0)
        elif n.endswith(".bias"):
            v.zero_()
        elif n == "model.encoder.embed_positions.weight":
            T, d = shape.max_source_positions, shape.d_model
            inc = np.log(10000.0) / (d // 2 - 1)
            inv = torch.exp(-inc * torch.arange(d // 2, device=device))
            t = torch.arange(T, device=device)[:, None] * inv[None, :]
            v.copy_(torch.cat([t.sin(), t.cos()], 1))
        else:
            v.normal_(0.0, 0.02, generator=g)
    eng.refresh_compute_weights()
    gen = torch.Generator().manual_seed(4242 + rank)
    waves = torch.zeros(B, N_SAMPLES)
    for b in range(B):
        n = int(torch.randint(112_000, N_SAMPLES + 1, (1,), generator=gen))
        waves[b, :n] = 0.1 * torch.randn(n, generator=gen)
    tl = torch.randint(20, 121, (B,), generator=gen)
    labels = torch.full((B, int(tl.max())), -100, dtype=torch.int64)
    for b in range(B):
        labels[b, :tl[b]] = torch.randint(0, 50257, (int(tl[b]),), generator=gen)
    return eng, shape, waves.to(device), labels


def whisper_decode_bytes_per_token(eng, shape, B) -> float:
    """Algorithmic HBM bytes of ONE greedy step: every bf16 decoder weight once (the tied
    proj_out = embed_tokens matrix included) + the cross-attention K|V cache of every decoder layer for every clip."""
    w = sum(int(torch.tensor(shp).prod()) for n, (_, shp) in eng.store.index.items()
            if n.startswith("model.decoder.") and not n.endswith("__zero")) * 2
    kv = shape.decoder_layers * B * shape.max_source_positions * shape.d_model * 2 * 2
    return float(w + kv)


def check_replicas(eng, trainer, rank, extra=None):
    """DDP invariant after the run: every rank holds identical parameters AND identical optimiser state.  With the
    sharded optimiser the fp32 master and the moments of a slice live on the owning rank between steps, so they are
    gathered first (`consolidate()`, a collective); the bf16 compute copy - what the forward reads, all-gathered every
    step - must agree as it stands, and must be the bf16 rounding of the gathered master."""
    torch.cuda.synchronize()
    st = eng.store
    m, v = trainer.consolidate() if trainer is not None else (None, None)
    spreads = {}
    for name, t in (("p32", st.p32), ("p16", st.p16.float()), ("m", m), ("v", v)):
        if t is None:
            continue
        lo, hi = t.clone(), t.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        spreads[name] = float((hi - lo).abs().max())
        del lo, hi
    if trainer is not None and getattr(trainer, "zero", False):
        # the sharded ranges of the compute copy against the gathered master (catches a stale or misplaced slice)
        worst = 0.0
        for name, (mlo, bhi) in trainer.sync.shard.items():
            worst = max(worst, float((st.p32[mlo:bhi].to(torch.bfloat16).float() - st.p16[mlo:bhi].float()).abs().max()))
        spreads["p16_vs_master"] = worst
    if rank == 0:
        print(json.dumps({"replica_param_spread": spreads["p32"], "replica_spreads": spreads, **(extra or {})}), flush=True)
    assert all(x == 0.0 for x in spreads.values()), f"replicas diverged: {spreads}"


def whisper_measure(model, args, world, rank, device, decode=False, fp8=False, B=None, steps=None, warmup=None,
                    dump_dir=None):
    """One Whisper workload: teacher-forced finetune step on 30 s clips (log-mel on the GPU inside the step) or greedy
    decoding (`decode`).  -> dict(ms_per_step, value, ...) on every rank.  `dump_dir`: rank 0 writes what the last
    timed step returned (loss | generated ids) and, for training, a sample of the updated weights (write_outputs)."""
    from coral_amd.trainer import DataParallelTrainer

    B = B or args.batch
    steps = steps or args.steps
    warmup = args.warmup if warmup is None else warmup
    eng, shape, waves, labels = whisper_setup_engine(model, device, rank, B)
    trainer = None if decode else DataParallelTrainer(eng, learning_rate=6e-6, betas=(0.9, 0.98), warmup_steps=1000,
                                                      max_steps=100_000, compress_grads=(args.grad_wire == "bf16"),
                                                      zero_stage=args.zero_stage or 0)
    if decode and fp8:
        eng.enable_fp8_encoder()
    if fp8 and not decode:
        eng.enable_fp8_forward()
    prefix = [50258, 50285, 50359, 50363]

    def step(new_tokens=args.decode_tokens):
        feats = eng.log_mel(waves)  # front end on the GPU, inside the step
        if decode:
            return eng.generate(feats, prefix, 4 + new_tokens)
        return trainer.train_step([dict(input_features=feats, labels=labels)])

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    last = [None]

    def timed(n, **kw):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            last[0] = step(**kw)
        sync()
        return (time.perf_counter() - t0) / n

    for _ in range(warmup):
        step()
    idx = before = None
    if dump_dir is not None:  # (outside the timed region: the weights before the timed steps, at the sampled offsets)
        idx = param_sample_index(trainer, device)
        if idx is not None:
            trainer.finish()
            before = eng.store.p32[idx].clone()
    dt = timed(steps)
    if dump_dir is not None and rank == 0:
        if decode:
            outs = {"generated_ids": torch.tensor(last[0])}
        else:
            outs = {"loss": last[0]}
            if idx is not None:
                trainer.finish()
                after = eng.store.p32[idx]
                outs.update(grad_norm=torch.tensor([trainer.grad_norm()], dtype=torch.float64),
                            params_sample=after, params_update_sample=after - before)
        write_outputs(dump_dir, outs)
    res = dict(ms_per_step=dt * 1e3, value=world * B * 30.0 / dt, B=B, label_len=int(labels.shape[1]),
               dropout=eng.dropout, activation_dropout=eng.activation_dropout, engine=eng, shape=shape, trainer=trainer)
    if decode:
        # the per-token time without the log-mel + encoder part: (T(n2 new tokens) - T(n1 new tokens)) / (n2 - n1)
        n1, n2 = 8, 8 + args.decode_tokens
        step(new_tokens=n1)
        t1, t2 = timed(max(2, steps // 2), new_tokens=n1), timed(max(2, steps // 2), new_tokens=n2)
        per_tok = (t2 - t1) / (n2 - n1)
        byt = whisper_decode_bytes_per_token(eng, shape, B)
        res.update(ms_per_token=per_tok * 1e3, bytes_per_token=byt, hbm_frac=byt / per_tok / 8.0e12)
    if trainer is not None:
        trainer.finish()
        torch.cuda.synchronize()
        if world == 1:
            trainer.close()
    return res


def whisper_bench(args, world, rank, device):
    """Secondary workload (BASELINE.json configs[3]/[4] shapes): `--model whisper-*` [--decode] [--fp8-forward]."""
    fp8 = (args.decode and args.fp8_encoder) or (args.fp8_forward and not args.decode)
    r = whisper_measure(args.model, args, world, rank, device, decode=args.decode, fp8=fp8, dump_dir=args.dump_outputs)
    eng, B = r["engine"], r["B"]
    if rank == 0:
        mode = f"greedy decode, {args.decode_tokens} new tokens" if args.decode else "finetune step fwd+bwd+clip+AdamW, teacher-forced"
        cfg = {"workload": f"{args.model} {mode}, {B} x 30 s per GPU, log-mel on GPU, dropout {r['dropout']:g} / "
                           f"activation_dropout {r['activation_dropout']:g}"
                           + (f", sharded optimiser (zero_stage {args.zero_stage}) over {args.backend}" if world > 1 and args.zero_stage
                              and not args.decode else ""), "global_batch": world * B,
               "label_len": r["label_len"], "parallelism": f"dp{world}"}
        if args.decode:
            cfg.update(ms_per_token=round(r["ms_per_token"], 4), bytes_per_token=int(r["bytes_per_token"]),
                       hbm_frac_of_8TBps=round(r["hbm_frac"], 4))
        print(json.dumps({
            "metric": f"audio-seconds/sec ({mode}), {args.model}, 30 s clips", "value": round(r["value"], 2),
            "unit": "audio-seconds/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(r["ms_per_step"], 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": ("bf16 + fp8 e4m3 (encoder q|k|v, fc1 forward)" if args.decode else
                                          "bf16 + fp8 e4m3 (encoder q|k|v, out, fc1, fc2 forward and the data gradients of fc2 / out / fc1: e4m3 weights and activations, delayed scaling)") if fp8 else "bf16",
            "data": "synthetic", "config": cfg}), flush=True)
    if world > 1:
        if args.check_replicas and not args.decode:
            check_replicas(eng, r["trainer"], rank)
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def run_w2v2(model_key, args, world, rank, device, roofline: bool, dump_dir=None):
    """Build the engine for one CoRal model key, run `--warmup` untimed and `--steps` timed finetune steps; with
    `roofline` (--full), the forward+backward-only and fp32-gradient timings and two more steps with every GEMM launch
    bracketed by hipEvents on its stream.  `dump_dir`: rank 0 writes what the last timed step computed, before anything
    else runs (write_outputs)."""
    import numpy as np

    from coral_amd import ops, specaugment
    from coral_amd.trainer import DataParallelTrainer
    from coral_amd.wav2vec2 import CORAL_W2V2_SHAPES, Wav2Vec2CTCEngine, Wav2Vec2Shape

    # CoRal model YAML values (R/config/model/wav2vec2-large.yaml:12-22); layerdrop is forced to 0
    # in the multi-GPU regime (R/src/scripts/finetune_asr_model.py:48-54) and kept 0 at N=1 so the
    # per-GPU work is identical at every N (weak scaling).
    shape = Wav2Vec2Shape(**CORAL_W2V2_SHAPES[model_key], activation_dropout=0.1, layerdrop=0.0)
    eng = Wav2Vec2CTCEngine(shape, device)
    init_random_(eng, 4242)
    trainer = DataParallelTrainer(eng, learning_rate=1e-4, betas=(0.9, 0.98), max_grad_norm=1.0,
                                  warmup_steps=1000, max_steps=100_000, compress_grads=(args.grad_wire == "bf16"),
                                  zero_stage=args.zero_stage)
    batch, lens = synth_batch(args.batch, args.seconds, rank, device, ragged=args.ragged)
    B, N = batch["input_values"].shape
    Ts = eng.conv_lengths(N)
    T = Ts[-1]
    frame_lens = [eng.conv_lengths(int(n))[-1] for n in lens]  # SpecAugment spans fall on valid frames only
    rng = np.random.RandomState(4242 + rank)

    pipe = None
    if args.from_host_pcm:
        from coral_amd.input_pipeline import DeviceInputPipeline

        pipe = DeviceInputPipeline(device, B, N, dtype=np.int16, padding="max_length")
        pcm = [(np.clip(0.1 * rng.randn(int(n)), -1, 1) * 32767).astype(np.int16) for n in lens]
        pipe.submit(pcm)

    def make_step_batch():
        mb = dict(batch)
        if pipe is not None:  # this step's batch was staged during the previous step; stage the next one now
            mb.update(pipe.get())
            mb.pop("sample_lengths", None)  # (a hint for the HF-shaped wrapper; the bare engine takes the masks below)
            pipe.submit(pcm)
        if not args.no_specaugment:
            mt, mf = specaugment.sample_masks(B, T, shape.hidden_size, frame_lens, 0.5, 10, 0.5, 64, rng=rng)
            mb["mask_time"] = torch.from_numpy(mt)
            mb["mask_feature"] = torch.from_numpy(mf)
        return [mb]

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        loss = trainer.train_step(make_step_batch())
    idx = before = None
    if dump_dir is not None:  # (outside the timed region: the weights before the timed steps, at the sampled offsets)
        idx = param_sample_index(trainer, device)
        if idx is not None:
            trainer.finish()
            before = eng.store.p32[idx].clone()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step(make_step_batch())
    sync()
    dt = time.perf_counter() - t0
    if dump_dir is not None and rank == 0:
        # what a caller of the step receives (the loss) and what the step computed on the way (the logits of its forward,
        # the gradient norm it clipped by) or left behind (the updated master weights and the timed steps' update)
        trainer.finish()
        # The logits of the last forward stay in the engine's workspace until the next forward: only the lm_head GEMM
        # writes w["logits"] (the backward reads it and writes w["dlogits"]), the same buffer greedy_decode() reads as
        # "the logits of the last forward" (coral_amd/wav2vec2.py)
        w = eng._saved["w"]
        outs = {"loss": loss, "logits": w["logits"].view(B, T, w["Vp"])[:, :, :shape.vocab_size],
                "grad_norm": torch.tensor([trainer.grad_norm()], dtype=torch.float64)}
        if idx is not None:
            after = eng.store.p32[idx]
            outs.update(params_sample=after, params_update_sample=after - before)
        write_outputs(dump_dir, outs)
    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax.item())
    secs = torch.tensor([float(lens.sum()) / 16000.0], dtype=torch.float64, device=device)  # real (unpadded) audio
    if world > 1:
        torch.distributed.all_reduce(secs)
    res = dict(engine=eng, trainer=trainer, shape=shape, B=B, T=T, loss=float(loss), ms_per_step=dt / args.steps * 1e3,
               value=round(float(secs.item()) * args.steps / dt, 2),
               step_tflop=3.0 * fwd_gflop_per_utt(shape, T, Ts) * B / 1e3)
    if world == 1 and roofline and not args.no_fwd_bwd:
        # BASELINE.json words its metric "fwd+bwd"; `value` above is the whole finetune step (clip + AdamW included, the
        # conservative reading).  The same steps without the optimiser, reported beside it, never instead of it.
        trainer.finish()
        torch.cuda.synchronize()
        eng.weights_ready = None

        def fwd_bwd(i):
            mb = make_step_batch()[0]
            eng.step_seed = 100000 + i
            trainer.model.train()
            trainer.model(**mb)
            eng.zero_grad(matrices=eng.freeze_base)
            eng.backward(loss_scale=1.0, overwrite_matrices=True, bucket_done=None)

        for i in range(2):
            fwd_bwd(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fwd_bwd(2 + i)
        torch.cuda.synchronize()
        fb = (time.perf_counter() - t0) / args.steps
        res["fwd_bwd"] = {"ms_per_step": round(fb * 1e3, 3), "value": round(float(lens.sum()) / 16000.0 / fb, 2),
                          "unit": "audio-seconds/sec",
                          "note": "forward + backward only (BASELINE.json's wording of the metric); `value` is the whole "
                                  "step with gradient-norm clip and AdamW"}
    if world == 1 and roofline and not args.no_fwd_bwd and os.environ.get("CA_WGRAD_BF16", "1") != "0":
        # The N = 1 line keeps the layers' weight-matrix gradients in bf16 (one micro-batch, one rank: what the reference's
        # autocast computes); N > 1 and accumulation use the fp32 buffer.  The same step on the fp32 route, so that an
        # N = 1 -> N = 8 comparison can start from like for like (`config.fp32_matrix_gradients`).
        trainer.finish()
        torch.cuda.synchronize()
        os.environ["CA_WGRAD_BF16"] = "0"
        try:
            for _ in range(2):
                trainer.train_step(make_step_batch())
            trainer.finish()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                trainer.train_step(make_step_batch())
            trainer.finish()
            torch.cuda.synchronize()
            f32 = (time.perf_counter() - t0) / args.steps
            res["fp32_matrix_gradients"] = {"ms_per_step": round(f32 * 1e3, 3), "value": round(float(lens.sum()) / 16000.0 / f32, 2),
                                            "unit": "audio-seconds/sec",
                                            "note": "the same step with CA_WGRAD_BF16=0 (the gradient route of N > 1 ranks and "
                                                    "of accumulation)"}
        finally:
            del os.environ["CA_WGRAD_BF16"]
        trainer.train_step(make_step_batch())  # (back on the default route before the profiled steps)
    if roofline:
        # Per-kernel durations are only meaningful with the kernels serialised: the timed steps above run the weight
        # gradients on their own stream beside the data-gradient chain (wav2vec2.py backward) and the HBM-bound AdamW
        # beside the next forward (trainer.py), where kernels share the chip and each one's begin-to-end time grows
        # (forward GEMMs measured 20-25 % longer under the optimiser's traffic).  The two profiled steps put everything
        # back on one stream - the regime of the committed rocprofv3 summaries (tools/profile_bench.sh).
        prev = os.environ.get("CA_WGRAD_STREAM")
        os.environ["CA_WGRAD_STREAM"] = "0"
        trainer.finish()
        torch.cuda.synchronize()
        ovl, trainer.overlap_optimizer = trainer.overlap_optimizer, False
        eng.weights_ready = None
        trainer.train_step(make_step_batch())
        ops.prof_begin()
        for _ in range(2):
            trainer.train_step(make_step_batch())
        torch.cuda.synchronize()
        prof = ops.prof_end()
        trainer.overlap_optimizer = ovl
        if prev is None:
            del os.environ["CA_WGRAD_STREAM"]
        else:
            os.environ["CA_WGRAD_STREAM"] = prev
        res["prof"], res["dom"] = prof, max(prof, key=lambda r: r["ms"])
        if rank == 0 and args.gemm_breakdown:
            for r in sorted(prof, key=lambda r: -r["ms"]):
                if r["count"]:
                    print(f"{r['kernel']:55s} {r['count'] // 2:5d} launches/step {r['ms'] / 2:8.2f} ms/step "
                          f"{r['flops'] / (r['ms'] * 1e-3) / 1e12:7.1f} TFLOP/s", file=sys.stderr)
    trainer.finish()
    torch.cuda.synchronize()
    res["bg_blocks"] = int(getattr(trainer, "bg_blocks", 0) or 0)
    res["matrix_grads"] = "bf16" if getattr(eng, "matrix_grads_bf16", False) else "fp32"
    if world == 1:
        trainer.close()  # (the C-ABI communicator of a --one-rank-exchange run goes back with it)
        res["trainer"] = None  # (N = 1: nothing to check afterwards; the moments' memory goes back before the next workload)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="wav2vec2-large", help="CoRal model key (wav2vec2-small/medium/large)")
    ap.add_argument("--batch", type=int, default=8, help="utterances per GPU")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-specaugment", action="store_true")
    ap.add_argument("--from-host-pcm", action="store_true",
                    help="feed every step from raw int16 PCM in host memory through the device input pipeline "
                         "(pinned staging + side-stream H2D + on-GPU normalisation): the PCIe-inclusive rate")
    ap.add_argument("--gemm-breakdown", action="store_true", help="print the per-kernel GEMM timing table to stderr")
    ap.add_argument("--decode", action="store_true",
                    help="whisper models: time greedy decoding instead of training; the line also carries the per-token "
                         "time (config.ms_per_token, from two more timed generation lengths), with or without --full")
    ap.add_argument("--decode-tokens", type=int, default=32)
    ap.add_argument("--fp8-forward", action="store_true",
                    help="whisper finetune step: encoder forward projections and the fc2 / out_proj data gradients in fp8 (DESIGN.md 4.4)")
    ap.add_argument("--fp8-encoder", action="store_true",
                    help="whisper --decode: encoder q|k|v and fc1 projections with fp8 weights (DESIGN.md 4.4)")
    ap.add_argument("--grad-wire", default="fp32", choices=["bf16", "fp32"],
                    help="dtype of the gradient all-reduce at N>1: fp32 = what the reference's DDP reduces (accelerate "
                         "bf16 autocast keeps fp32 gradients); bf16 = the DDP bf16_compress_hook trade, a separate "
                         "labelled measurement, never the headline")
    ap.add_argument("--zero-stage", type=int, default=None,
                    help="N>1: shard the optimiser over the ranks (reduce-scatter of the weight-matrix gradients, AdamW on "
                         "1/N, all-gather of the bf16 weights) - the reference's production launch `accelerate launch "
                         "--zero-stage 2` (R/makefile:79-84; a one-time self-check of the RCCL "
                         "in-place collectives falls back to replicated DDP if it fails); 0 = replicated DDP with gradient "
                         "all-reduce (BASELINE.json configs[2]).  Without the flag at N>1: BOTH - the headline line is stage 0, "
                         "stage 2 follows in the same process group and is reported as config.also_zero2")
    ap.add_argument("--ragged", action="store_true",
                    help="utterance lengths ~ U[1 s, --seconds] padded to --seconds (the regime of "
                         "R/config/asr_finetuning.yaml:31-32): masked attention / CTC lengths / SpecAugment on valid frames")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, measure everything else: roofline (profiled steps), config.fwd_bwd, "
                         "config.fp32_matrix_gradients, the secondary workloads (config.also*), the CPU baseline, and at "
                         "N>1 without --zero-stage the sharded optimiser (config.also_zero2); the --no-* options narrow it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64, "
                         "64 MB at most; the weights as a fixed, seeded sample)")
    ap.add_argument("--no-also", action="store_true", help="skip the secondary measurements (config.also*)")
    ap.add_argument("--no-fwd-bwd", action="store_true", help="skip the extra forward+backward-only timing (profile runs)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for 1-GPU debugging of the N>1 logic)")
    ap.add_argument("--check-replicas", action="store_true", help="after the run, verify every rank holds identical parameters")
    ap.add_argument("--one-rank-exchange", action="store_true",
                    help="N=1 diagnostic: run the N>1 exchange path (RCCL group of one rank, per-bucket all-reduce on the "
                         "communication stream, per-bucket norms and AdamW behind it) at full size; never a reported number")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # One command starts all ranks (the reference's `accelerate launch ... finetune_asr_model.py`,
        # R/src/scripts/finetune_asr_model.py:9-12): nothing in this process has touched the GPU yet, the ranks are
        # fresh child processes and this process only relays their exit code.  Never a silent 1-GPU run.
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # N > 1 without --zero-stage: the headline is BASELINE.json's configuration - replicated DDP, gradient ALL-REDUCE per
    # layer bucket (configs[2]; accelerate/accelerator.py:1892,2053) - and the sharded optimiser (the reference's
    # production launch, `accelerate launch --zero-stage 2`, R/makefile:79-84) is measured right after it in the same
    # process group and reported beside it as config.also_zero2.
    both_stages = args.full and args.zero_stage is None and world > 1 and not args.model.startswith("whisper")
    if args.zero_stage is None:
        args.zero_stage = 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    ndev = torch.cuda.device_count()
    local_rank = local_rank % max(1, ndev)  # (gloo debugging may put several ranks on one GPU)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world == 1 and args.one_rank_exchange:
        import socket

        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ["CA_DP_FORCE"] = "1"
        torch.distributed.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                             device_id=device)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=device)
        else:
            torch.distributed.init_process_group(args.backend)

    if args.model.startswith("whisper"):
        return whisper_bench(args, world, rank, device)

    res = run_w2v2(args.model, args, world, rank, device, roofline=args.full, dump_dir=args.dump_outputs)
    eng, loss_val, trainer_ = res.pop("engine"), res["loss"], res.pop("trainer")
    if rank == 0 and "prof" in res:  # (--full)
        dom, prof = res["dom"], res["prof"]
        tot_ms = sum(r["ms"] for r in prof)
        tot_fl = sum(r["flops"] for r in prof)
        ach = dom["flops"] / (dom["ms"] * 1e-3) / 1e12 if dom["ms"] > 0 else 0.0
        traffic, traffic_source = None, None
        pmc = ROOT / "profiles" / "pmc_traffic.json"
        if pmc.exists():
            try:
                traffic = json.loads(pmc.read_text()).get(dom["kernel"])
                traffic_source = "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, FETCH_SIZE x2 for gfx950; static table, not re-measured in this run)"
            except Exception:
                traffic = None
    if rank == 0:
        shape, B, T = res["shape"], res["B"], res["T"]
        step_ms = res["ms_per_step"]
        wire = f"{args.grad_wire} wire" if world > 1 else "no collective (1 rank)"
        out = {
            "metric": "audio-seconds/sec (CTC finetune step: fwd+bwd+allreduce+clip+AdamW), wav2vec2-large, 10 s utterances",
            "value": res["value"], "unit": "audio-seconds/sec", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_ms, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "rccl_ranks": torch.distributed.get_world_size() if (world > 1 and args.backend == "nccl") else 1,
            "backend": (args.backend if world > 1 else None), "ranks": world,
            "grad_wire": args.grad_wire if world > 1 else None,
            "config": {"workload": f"{args.model} (XLS-R shape d={shape.hidden_size} L={shape.num_hidden_layers} "
                                   f"ffn={shape.intermediate_size}) CTC finetune, {B} x {args.seconds:g} s per GPU"
                                   + (" (ragged: lengths U[1 s, max], padded)" if args.ragged else "") +
                                   f", SpecAugment {'off' if args.no_specaugment else 'on'}, activation_dropout 0.1, "
                                   "layerdrop 0 (multi-GPU rule), fp32 master + AdamW + clip 1.0"
                                   + (", inputs from host int16 PCM through the device input pipeline" if args.from_host_pcm else "")
                                   + (f", gradient all-reduce ({args.backend}) on {wire}, per-layer buckets overlapped with backward" if world > 1 and not args.zero_stage else "")
                                   + (f", sharded optimiser (zero_stage {args.zero_stage}): gradient reduce-scatter ({args.backend}) on {wire} per layer bucket overlapped with backward, AdamW on 1/{world}, bf16 all-gather under the next forward" if world > 1 and args.zero_stage else "")
                                   + (f" [DIAGNOSTIC: N>1 exchange path forced over an RCCL group of one rank, {args.grad_wire} wire]" if args.one_rank_exchange and world == 1 else ""),
                       "global_batch": world * B, "frames_per_utt": T, "parallelism": f"dp{world}",
                       # what the runtime was told: kernel arguments in device memory; AdamW's grid cap
                       # under the next forward (workgroups; 0 = full grid)
                       "runtime": {"HIP_FORCE_DEV_KERNARG": os.environ.get("HIP_FORCE_DEV_KERNARG"),
                                   "optimizer_background_blocks": res.get("bg_blocks"),
                                   # single-micro-batch steps on one GPU keep the layers' weight-matrix gradients in the
                                   # dtype the reference's bf16 autocast computes them in (fp32 master, fp32 moments and
                                   # every other gradient unchanged; CA_WGRAD_BF16=0 = fp32 buffer: + 0.9 ms per step)
                                   "layer_matrix_gradients": res.get("matrix_grads")},
                       "loss": round(loss_val, 3),
                       **({"fwd_bwd": dict(res["fwd_bwd"], frac_of_peak=round(
                           res["step_tflop"] / (res["fwd_bwd"]["ms_per_step"] * 1e-3) / MFMA_BF16_DENSE_PEAK_TFLOPS, 4))}
                          if "fwd_bwd" in res else {}),
                       **({"fp32_matrix_gradients": res["fp32_matrix_gradients"]} if "fp32_matrix_gradients" in res else {})},
        }
        if "prof" in res:  # (--full)
            out["roofline"] = {"bound": "mfma", "kernel": dom["kernel"], "achieved": round(ach, 1),
                               "timing": "hipEvents around every launch of two extra steps run with all kernels on one stream "
                                         "(the timed steps overlap the optimiser and the weight gradients on side streams)",
                               "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "traffic": traffic,
                               "traffic_source": traffic_source,
                               "launches": dom["count"] // 2, "avg_us": round(dom["ms"] * 1e3 / max(1, dom["count"]), 2),
                               "all_gemm_tflops": round(tot_fl / (tot_ms * 1e-3) / 1e12, 1) if tot_ms else 0.0,
                               "gemm_ms_per_step": round(tot_ms / 2, 2),
                               "step_algorithmic_tflop": round(res["step_tflop"], 2),
                               "step_frac_of_peak": round(res["step_tflop"] / (step_ms * 1e-3) / MFMA_BF16_DENSE_PEAK_TFLOPS, 4)}
    if args.full and world == 1 and not args.no_also and args.model == "wav2vec2-large":
        # SURVEY.md §0 decision 2: CoRal's `wav2vec2-large` key is the XLS-R-2B shape; the architecture most readers
        # call "wav2vec2-large" (24 L / 1024 / 4096) is CoRal's `wav2vec2-small` key: report it beside the headline.
        del res, eng
        torch.cuda.empty_cache()
        r2 = run_w2v2("wav2vec2-small", args, world, rank, device, roofline=False)
        del r2["engine"]
        out["config"]["also"] = {"workload": "wav2vec2-small (XLS-R-300M = classic wav2vec2-large shape 24L/1024/4096), same step",
                                 "value": r2["value"], "unit": "audio-seconds/sec", "ms_per_step": round(r2["ms_per_step"], 3),
                                 "step_frac_of_peak": round(r2["step_tflop"] / (r2["ms_per_step"] * 1e-3) / MFMA_BF16_DENSE_PEAK_TFLOPS, 4)}
        eng = None
        # The secondary workloads the round-2 review asked to be driver-visible, each run AFTER (outside) the headline's
        # timed region, with their own short warm-up: R/makefile:90's production batch (wav2vec2-small, 64 per device),
        # BASELINE configs[3] (whisper-medium greedy decode: ms per token against its HBM floor) and configs[4]'s
        # architecture (whisper-large-turbo finetune step, bf16 and with the fp8 forward projections).
        import copy

        a2 = copy.copy(args)
        a2.batch, a2.steps, a2.warmup = 64, max(3, args.steps // 2), 2
        r3 = run_w2v2("wav2vec2-small", a2, world, rank, device, roofline=False)
        del r3["engine"]
        out["config"]["also_b64"] = {"workload": "wav2vec2-small (XLS-R-300M), 64 x 10 s per GPU = the reference's production "
                                                 "per_device_batch_size (R/makefile:90), same step",
                                     "value": r3["value"], "unit": "audio-seconds/sec", "ms_per_step": round(r3["ms_per_step"], 3),
                                     "step_frac_of_peak": round(r3["step_tflop"] / (r3["ms_per_step"] * 1e-3) / MFMA_BF16_DENSE_PEAK_TFLOPS, 4)}
        del r3
        torch.cuda.empty_cache()
        dec = {}
        for Bd in (8, 16, 32, 64):  # (the K|V-cached greedy step runs on the weight-streaming kernel: M = batch <= 128)
            r4 = whisper_measure("whisper-medium", args, world, rank, device, decode=True, B=Bd, steps=3, warmup=1)
            from coral_amd import ops as _ops

            one = Bd <= 16 and os.environ.get("CA_DECODE_PERSISTENT", "1") != "0" and _ops.whisper_decode_token_supported(
                Bd, r4["shape"].d_model, r4["shape"].decoder_ffn_dim, r4["shape"].decoder_attention_heads, r4["shape"].vocab_size)
            dec[f"B{Bd}"] = {"ms_per_token": round(r4["ms_per_token"], 4), "bytes_per_token": int(r4["bytes_per_token"]),
                             "frac_of_8TBps": round(r4["hbm_frac"], 4),
                             "audio_s_per_s_incl_logmel_encoder": round(r4["value"], 1),
                             "step": "one persistent launch per token (ca_whisper_decode_token)" if one
                             else "launch sequence, ~7 launches per layer"}
            del r4
            torch.cuda.empty_cache()
        # the reference's DEFAULT model key at its evaluation batch (whisper-large = large-v3, R/config/evaluation.yaml:20):
        # 16 clips x 20 heads = 320 (clip, head) items on 256 CUs - the second round's items are key-split (attention.hip)
        r4 = whisper_measure("whisper-large", args, world, rank, device, decode=True, B=16, steps=3, warmup=1)
        dec["large_B16"] = {"workload": "whisper-large (32 + 32 layers, d 1280, 20 heads), 16 clips",
                            "ms_per_token": round(r4["ms_per_token"], 4), "bytes_per_token": int(r4["bytes_per_token"]),
                            "frac_of_8TBps": round(r4["hbm_frac"], 4),
                            "audio_s_per_s_incl_logmel_encoder": round(r4["value"], 1)}
        del r4
        torch.cuda.empty_cache()
        out["config"]["also_decode"] = dict(workload=f"whisper-medium greedy decode (log-mel + encoder + {args.decode_tokens} "
                                                     "K|V-cached, graph-replayed decoder steps), 30 s clips; per-token time = "
                                                     "difference of two generation lengths; bytes = bf16 decoder weights + "
                                                     "cross K|V cache per step", **dec)
        tb = {}
        for fp8 in (False, True):
            r5 = whisper_measure("whisper-large-turbo", args, world, rank, device, decode=False, fp8=fp8, B=8, steps=4, warmup=2)
            tb["fp8_forward" if fp8 else "bf16"] = {"ms_per_step": round(r5["ms_per_step"], 3), "value": round(r5["value"], 1)}
            del r5
            torch.cuda.empty_cache()
        out["config"]["also_turbo"] = dict(workload="whisper-large-turbo finetune step (teacher-forced, dropout 0.1), 8 x 30 s, "
                                                    "log-mel on GPU; fp8_forward = all encoder forward projections + the data gradients of fc2 / out_proj / fc1 with "
                                                    "e4m3 weights and activations (DESIGN.md 4.4)",
                                           unit="audio-seconds/sec", **tb)
        # the reference's DEFAULT model key (R/config/asr_finetuning.yaml:1-11: model=whisper-large = large-v3, 32 + 32 layers)
        r6 = whisper_measure("whisper-large", args, world, rank, device, decode=False, fp8=False, B=8, steps=4, warmup=2)
        out["config"]["also_large"] = dict(workload="whisper-large (the reference's default model key: large-v3, 32 + 32 layers, 128 mels) "
                                                    "finetune step (teacher-forced, activation_dropout 0.1), 8 x 30 s, log-mel on GPU",
                                           unit="audio-seconds/sec", ms_per_step=round(r6["ms_per_step"], 3), value=round(r6["value"], 1))
        del r6
        torch.cuda.empty_cache()
    if world > 1 and args.check_replicas:
        # DDP invariant: identical parameters on every rank after identical (averaged) updates
        # (parameters, bf16 compute copy and AdamW moments; the sharded optimiser's slices are gathered first)
        check_replicas(eng, trainer_, rank, extra={"loss_rank0": loss_val})
    if both_stages:
        import copy
        import threading

        # The headline (BASELINE's all-reduce configuration) is measured: the secondary run must not be able to lose it.
        # An exception in it becomes an `error` field; if it hangs (a rank-local failure inside a collective), rank 0
        # prints the line it has after CA_BENCH_ZERO2_TIMEOUT seconds (default 300) and leaves.
        emit_lock = threading.Lock()  # the headline line goes out ONCE: from the watchdog or from the main thread
        emitted = [False]

        def _emit_without_zero2():
            with emit_lock:
                if emitted[0]:
                    return
                emitted[0] = True
                out["config"]["also_zero2"] = {"error": "the zero_stage 2 run did not finish in time; headline unaffected"}
                print(json.dumps(out), flush=True)
            # The peers are blocked inside a collective: nothing orderly is left to do in this process.  Exit code 0 - the
            # measured headline is valid and the line says what did not finish (`also_zero2.error`); the launcher tears
            # the other ranks down when rank 0 leaves.
            os._exit(0)

        watchdog = None
        if rank == 0:
            watchdog = threading.Timer(float(os.environ.get("CA_BENCH_ZERO2_TIMEOUT", "300")), _emit_without_zero2)
            watchdog.daemon = True
            watchdog.start()
        try:
            trainer_.close()
            del trainer_, eng
            torch.cuda.empty_cache()
            a2 = copy.copy(args)
            a2.zero_stage = 2
            rz = run_w2v2(args.model, a2, world, rank, device, roofline=False)
            ez, tz = rz.pop("engine"), rz.pop("trainer")
            if rank == 0:
                out["config"]["also_zero2"] = {
                    "workload": "the same step with the sharded optimiser (zero_stage 2): gradient reduce-scatter per layer bucket, "
                                f"AdamW on 1/{world} of the state, bf16 all-gather under the next forward - the reference's production "
                                "launch mode (R/makefile:79-84)",
                    "value": rz["value"], "unit": "audio-seconds/sec", "ms_per_step": round(rz["ms_per_step"], 3),
                    "zero_stage_in_effect": 2 if getattr(tz, "zero", False) else 0}
            if args.check_replicas:
                check_replicas(ez, tz, rank, extra={"loss_rank0": rz["loss"], "zero_stage": 2})
            tz.close()
            del ez, tz
        except Exception as e:  # noqa: BLE001 - reported, the headline line still goes out
            if rank == 0:
                out["config"]["also_zero2"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        finally:
            if watchdog is not None:
                watchdog.cancel()
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        lock = locals().get("emit_lock")
        if lock is None:
            print(json.dumps(out), flush=True)
        else:
            with lock:
                if not emitted[0]:
                    emitted[0] = True
                    print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    elif torch.distributed.is_initialized():  # --one-rank-exchange
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
