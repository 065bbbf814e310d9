"""Data-parallel CTC finetuning step: the MI355X replacement for the inner loop CoRal gets from
`transformers.Trainer` + accelerate/DDP ($TF/trainer.py:1678-1800 `_run_epoch`, :1892-1963
`training_step`, :1778-1796 clip + optimizer step; launched by R/src/coral/finetune.py:60-79).

One process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI).  Utterances are
sharded across ranks; the only exchange is the gradient all-reduce (coral_amd/exchange.py), issued per parameter bucket
(head, layer L-1 ... layer 0, front — contiguous slices of the flat fp32 gradient buffer) on a
dedicated HIP stream from the engine's backward hooks, so communication of layer l overlaps the
backward of layers < l.  DDP semantics are kept: gradients are averaged over ranks
(sum all-reduce, then 1/world folded into the fused AdamW kernel), the global-norm clip and the
AdamW update (beta=(0.9, 0.98), cosine schedule with warm-up; R/src/coral/wav2vec2.py:216-240,
R/config/asr_finetuning.yaml:64-75) run replicated on every rank.

What the trainer uses of an engine is declared by `coral_amd.engine.Engine`.
"""

from __future__ import annotations

import logging
import math
import os
import warnings

import torch

from . import ops
from .exchange import GradSync, collectives_selfcheck


def cosine_lr(step: int, base_lr: float, warmup_steps: int, max_steps: int) -> float:
    """transformers.get_cosine_schedule_with_warmup (SchedulerType.COSINE,
    R/src/coral/wav2vec2.py:217): `step` = number of optimiser steps already taken."""
    if step < warmup_steps:
        return base_lr * step / max(1, warmup_steps)
    progress = (step - warmup_steps) / max(1, max_steps - warmup_steps)
    return base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def grad_accumulation_steps(total_batch_size: int, num_devices: int, per_device_batch_size: int) -> int:
    """R/src/coral/wav2vec2.py:159-181: total // devices // per-device, at least 1."""
    return max(1, total_batch_size // max(1, num_devices) // per_device_batch_size)


def shard_indices(n_items: int, rank: int, world: int) -> list[int]:
    """Utterance indices of `rank` for one global batch: contiguous equal shards (the per-device
    batches accelerate hands each DDP rank); n_items must be divisible by world."""
    if n_items % world:
        raise ValueError(f"global batch {n_items} is not divisible by world size {world}")
    per = n_items // world
    return list(range(rank * per, (rank + 1) * per))


# ---- where a rank keeps its AdamW moments ------------------------------------------------------------------------
def state_layout(buckets: dict, shard: dict, rank: int, world: int) -> dict:
    """{bucket: [(param_lo, param_hi, state_off), ...]}: the parameter ranges whose AdamW moments this rank keeps, in
    order, and where each sits in its `m` / `v`.  Without `shard` the moments have the parameters' own layout
    (state_off == param_lo).  With it ({bucket: (mlo, hi)}, GradSync's) they are compact: bucket by bucket, the
    replicated head [lo, mlo) and then this rank's 1/world slice of [mlo, hi) - the same on every rank but for the slice."""
    out, n = {}, 0
    for name, (lo, hi) in buckets.items():
        mlo = shard[name][0] if name in shard else hi
        per = (hi - mlo) // world
        segs = [(lo, mlo, n), (mlo + rank * per, mlo + (rank + 1) * per, n + mlo - lo)]
        out[name] = [(a, b, so if shard else a) for a, b, so in segs if b > a]
        n += mlo - lo + per
    return out


def state_size(layout: dict) -> int:
    return max((so + b - a for segs in layout.values() for a, b, so in segs), default=0)


def split_bf16(layout: dict, ranges: dict) -> dict:
    """`layout` with every segment cut at the bucket's bf16-gradient range ({bucket: (lo, hi)}, Engine.bf16_grad_ranges):
    {bucket: [(param_lo, param_hi, state_off, inside), ...]}; without ranges, `layout` itself with inside = False."""
    out = {}
    for name, segs in layout.items():
        lo, hi = ranges.get(name, (0, 0))
        out[name] = [(x, y, so + x - a, inside) for a, b, so in segs
                     for x, y, inside in ((a, min(b, lo), False), (max(a, lo), min(b, hi), True), (max(a, hi), b, False))
                     if y > x]
    return out


def copy_state(layout: dict, compact: torch.Tensor, full: torch.Tensor, to_full: bool):
    """This rank's moments -> their places in a full-size buffer (the other ranks' slices stay as they are), or back."""
    for segs in layout.values():
        for a, b, so in segs:
            if to_full:
                full[a:b] = compact[so:so + b - a]
            else:
                compact[so:so + b - a] = full[a:b]


# How a step gets its squared gradient norm (DataParallelTrainer._norm_route)
FUSED = "fused"                # per-tile sums out of the weight-gradient GEMMs + one pass over the rest
BUCKETS = "buckets"            # per bucket, behind each bucket's reduction on the communication stream
BUCKETS_LATE = "buckets-late"  # per bucket (sharded gradients: there is no whole buffer to pass over), behind the exchange
EARLY = "early"                # the gradients' tail on the side stream during the backward, the head behind it
SINGLE = "single"              # one pass behind the backward


class DataParallelTrainer:
    """Owns optimiser state (flat fp32 m, v) and the communication stream for one engine."""

    def __init__(self, engine, learning_rate=1e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=1.0, warmup_steps=1000, max_steps=100_000, grad_accum=1,
                 process_group=None, overlap=True, compress_grads=False, overlap_optimizer=True, zero_stage=0,
                 accum_loss: str = "mean"):
        """zero_stage > 0 (N > 1): the reference's production launch mode (`accelerate launch --use-deepspeed
        --zero-stage 2`, R/makefile:79-84,94-99,109-114) in this engine's terms - the weight-matrix part of every layer
        bucket (> 99 % of the parameters) is REDUCE-SCATTERED instead of all-reduced, each rank keeps AdamW moments for
        and updates only its 1/N slice, and the bf16 compute copy of the slices is all-gathered bucket by bucket under
        the next forward.  Per step and rank at XLS-R-2B, N = 8: AdamW traffic 64.8 -> 8.1 GB, wire 2 x 7/8 x 8.64 GB
        (all-reduce) -> 7/8 x 8.64 GB (reduce-scatter, fp32) + 7/8 x 4.32 GB (all-gather, bf16).  The small tensors of
        a layer, the front and the head bucket stay replicated.  The update is the same arithmetic on the same sums:
        parameters equal the replicated trainer's (tests/test_dp_gloo.py, tests/test_dp_gpu.py)."""
        self.model = engine                          # HF-shaped wrapper or the bare engine
        engine = getattr(engine, "engine", engine)  # the kernel-sequencing engine underneath (coral_amd.engine.Engine)
        self.engine = engine
        self.lr, self.betas, self.eps, self.wd = learning_rate, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.warmup_steps, self.max_steps = warmup_steps, max_steps
        self.grad_accum = grad_accum
        # How the micro-batches of one optimiser step combine.  "mean": loss and gradients of each micro-batch scaled by
        # 1 / grad_accum (Trainer.training_step for a model WITHOUT **kwargs in its forward, $TF/trainer.py:1952-1954).
        # "sum": no scaling - what transformers >= 4.46 (the reference pins 5.5.0) does for Wav2Vec2ForCTC and
        # WhisperForConditionalGeneration, whose forwards take **kwargs (`model_accepts_loss_kwargs`) while their own
        # losses ignore `num_items_in_batch`: the logged loss is the SUM over the micro-batches and so is the gradient
        # the clip sees (tools/gen_goldens.py trainer_traj pins it; CoralTrainer's default).
        if accum_loss not in ("mean", "sum"):
            raise ValueError(f"accum_loss must be 'mean' or 'sum', not {accum_loss!r}")
        self.accum_loss = accum_loss
        self.opt_step = 0
        st = engine.store
        lo, hi = self.train_range = tuple(engine.trainable_range())
        whole = (lo, hi) == (0, st.numel)
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(process_group)
        zero_stage = int(os.environ.get("CA_ZERO_STAGE", zero_stage) or 0)
        shard = {}
        if zero_stage and (world > 1 or os.environ.get("CA_DP_FORCE", "0") == "1") and whole:
            shard = {n: r for n, r in engine.shard_ranges().items() if (r[1] - r[0]) % (8 * world) == 0 and r[1] > r[0]}
        self.sync = GradSync(st.g32, st.buckets, process_group, compress=compress_grads, shard=shard)
        self.zero = bool(shard) and self.sync.active
        if self.zero and world > 1 and st.p32.is_cuda and not collectives_selfcheck(st.device, process_group, self.sync.capi):
            # (never silently wrong: a backend whose in-place reduce-scatter / all-gather does not behave as RCCL
            # documents falls back to the replicated path, and says so)
            logging.getLogger(__package__).warning("sharded optimiser: the collective self-check failed; using replicated DDP")
            self.sync.close(abort=True)  # (a rank that could not enqueue leaves its peers' kernels spinning)
            self.sync = GradSync(st.g32, st.buckets, process_group, compress=compress_grads)
            self.zero = False
        self.world = self.sync.world
        self.dist = self.sync.active  # gradients are exchanged (world > 1, or a forced one-rank group)
        self._set_compute_cus = False
        if self.dist and st.p32.is_cuda:
            # A collective's kernel holds CUs for most of the backward: the persistent GEMM launches hand out every tile
            # dynamically (a workgroup that only starts once others have exited finds nothing left and exits) and, with
            # CA_COMPUTE_CUS=<n>, size themselves and the tile-shape rule to n CUs (include/coral_amd.h:
            # ca_gemm_set_compute_cus; measured beside an emulated ring kernel: tools/r05_hog_gemm.py)
            ncu = torch.cuda.get_device_properties(st.device).multi_processor_count
            ops.lib().ca_gemm_set_compute_cus(int(os.environ.get("CA_COMPUTE_CUS", ncu)))
            self._set_compute_cus = True  # (process-global library state: close() puts the default back)
        self.overlap = overlap and self.dist
        # AdamW moments.  Replicated: the parameters' own offsets.  Sharded: a compact buffer holding, bucket by bucket,
        # the replicated part [lo, mlo) and this rank's slice of the sharded part - 1/N of the state (state_layout).
        self._layout = state_layout(st.buckets, self.sync.shard if self.zero else {}, self.sync.rank, self.world)
        # ... as AdamW launches (a, b, state_off, gradients in the bf16 buffer): [0] for a step whose gradients are all
        # fp32, [1] for one whose weight-matrix gradients sit in the bf16 buffer (train_step; never when sharded)
        self._launches = [split_bf16(self._layout, r) for r in ({}, {} if self.zero else engine.bf16_grad_ranges())]
        self._forward_order = sorted(st.buckets, key=lambda name: st.buckets[name][0])
        self.m = torch.zeros(state_size(self._layout), dtype=torch.float32, device=st.device)
        self.v = torch.zeros_like(self.m)
        # Sharded: the updated bf16 slices are gathered on a stream of their own.  C ABI: the exchange context's - ONE
        # communicator per rank, so no two collectives of this trainer are ever in flight in an order that could differ
        # between ranks (by the time the optimiser runs, the step's reduce-scatters have been waited for: nothing
        # queues in front)
        self._ag_comm = self.sync.capi if self.zero else None
        self._ag_stream = None
        if self.zero and st.p32.is_cuda:
            self._ag_stream = self._ag_comm.stream if self._ag_comm is not None else ops.side_stream(st.device, "gather")
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=st.device)
        self.partial = torch.zeros(4096, dtype=torch.float32, device=st.device)
        # AdamW is HBM-bound, the next forward MFMA-bound: run the update bucket by bucket on a side stream
        # and let the next forward wait per bucket (engine._await) instead of for the whole optimiser.
        # (CA_OPT_OVERLAP=0: everything on one stream - the regime the per-kernel profiles are taken in)
        self.overlap_optimizer = (overlap_optimizer and os.environ.get("CA_OPT_OVERLAP", "1") != "0"
                                  and st.p32.is_cuda and whole)
        self.opt_stream = None
        if self.overlap_optimizer:
            # the HBM-bound update only fills what the MFMA-bound forward leaves free: lowest queue priority
            prio = int(os.environ.get("CA_OPT_PRIO", "0"))
            self.opt_stream = ops.side_stream(st.device, "optimizer", prio)
        self.opt_done = None
        # ... and as a BACKGROUND kernel: one workgroup per CU, whose waves fit beside the forward GEMMs' in the register
        # file, so the two really run at the same time (ca_adamw_step_ex; CA_OPT_BG_BLOCKS=0: full grid - the A/B switch)
        self.bg_blocks = 0
        if self.overlap_optimizer:
            bg = os.environ.get("CA_OPT_BG_BLOCKS")
            self.bg_blocks = int(bg) if bg is not None else torch.cuda.get_device_properties(st.device).multi_processor_count
            if bg is None:
                # ... which holds only while the loaded kernels' register counts say so (a compiler that gives the forward
                # kernel 8 registers more turns the capped update into a 19 ms stall, tests/test_build.py): asked of the
                # code object itself; otherwise the full-grid update, which alternates with the GEMMs
                fits, rx, ru = ops.background_update_fits()
                if not fits:
                    warnings.warn(f"coral_amd: the forward GEMM kernel holds {rx} registers per lane and the update "
                                  f"kernel {ru}: the update cannot run beside it; using the full-grid update")
                    self.bg_blocks = 0
        # per-bucket squared gradient norms, computed on the side stream as the buckets complete
        self.bucket_index = {name: i for i, name in enumerate(st.buckets)}
        self.bucket_sq = torch.zeros(len(st.buckets), dtype=torch.float32, device=st.device)
        self.shard_norm = os.environ.get("CA_SHARD_NORM", "1") != "0"
        self._route = None  # the last backward's norm route; None: no train_step since the last optimizer_step
        # N = 1: the squared norm of the gradients that are final early in the backward is taken on the side stream
        # while the rest of the backward runs (one HBM-bound pass beside MFMA-bound GEMMs), see _early_norm
        self.partial_early = torch.zeros(4096, dtype=torch.float32, device=st.device)
        self.early_fraction = float(os.environ.get("CA_EARLY_NORM", "0.8"))
        self._early_lo = None   # [self._early_lo, hi) is already inside gnorm_sq
        self._done = {}

    # ---- one optimiser step ----------------------------------------------------------------------
    def train_step(self, micro_batches) -> float | torch.Tensor:
        """micro_batches: list (len = grad_accum) of dicts with input_values / attention_mask /
        labels (+ optional mask_time / mask_feature / layer_keep).  Returns the loss tensor (device) of this rank
        over the micro-batches, combined as `accum_loss` says (see __init__)."""
        eng = self.engine
        self.model.train()
        total = None
        n = len(micro_batches)
        rank = int(os.environ.get("RANK", "0")) % 64
        # One micro-batch per optimiser step on one GPU: the layers' weight-matrix gradients stay bf16 - the dtype the
        # reference's autocast computes them in ($TF/trainer.py training_step under torch.autocast: a Linear's weight
        # gradient is the bf16 output of a bf16 matmul, cast to fp32 only when it is accumulated into .grad) - from the
        # weight-gradient GEMM's epilogue to AdamW.  With accumulation or several ranks the fp32 buffer is what is
        # accumulated into / reduced, as in the reference.  CA_WGRAD_BF16=0: fp32 always.
        eng.wgrad_bf16 = (n == 1 and not self.dist and not self.zero and not eng.freeze_base
                          and os.environ.get("CA_WGRAD_BF16", "1") != "0" and self._norm_plan() is not None)
        for i, mb in enumerate(micro_batches):
            # fresh activation-dropout masks per micro-batch and rank (HF draws new masks in every forward); the
            # backward of micro-batch i runs before the next forward and regenerates the masks from the same seed
            eng.step_seed = (self.opt_step * n + i) * 64 + rank
            out = self.model(**mb)
            if i == 0:  # the previous optimiser step may still be reading the gradients
                self.finish()
                eng.zero_grad(matrices=eng.freeze_base)
            self._route, hook = self._norm_route(last=i == n - 1)
            scale = 1.0 / n if self.accum_loss == "mean" else 1.0
            eng.backward(loss_scale=scale, overwrite_matrices=(i == 0), bucket_done=hook)
            loss = out.loss.detach()  # (the autograd route of coral_amd/autograd.py is not used here)
            total = loss * scale if total is None else total + loss * scale
        if self.dist and not self.overlap:
            self.sync.start_all()
        self.sync.finish()
        self.optimizer_step()
        # the choice belongs to THIS step: a later direct engine.backward(overwrite_matrices=True) (the autograd
        # route, tests reading store.g32) must find fp32 matrix gradients, not stale ones beside a bf16 buffer
        eng.wgrad_bf16 = False
        return total

    def _norm_plan(self):
        """The engine's plan for a gradient norm without a pass over the weight matrices (whole model trainable,
        CA_FUSED_NORM != 0), else None."""
        if os.environ.get("CA_FUSED_NORM", "1") == "0" or self.train_range != (0, self.engine.store.numel):
            return None
        return self.engine.norm_plan()

    def _norm_route(self, last: bool):
        """(route, backward hook) of a micro-batch's backward - `last`: the step's final one, whose hooks see final
        gradients; last=False is also what holds when no backward of train_step ran.  The route says where the step's
        squared gradient norm comes from and so what optimizer_step still has to add (_finish_norm)."""
        if self.dist:
            # Per-bucket norms during the backward pay off where the buckets are being all-reduced anyway (N > 1: the
            # squared norm rides behind each bucket's reduction on the communication stream).  At N = 1 the side-stream
            # kernels only contend with the backward GEMMs for HBM (+20 % on the weight-gradient kernel for 0.2 ms).
            if last and self.overlap and (self.overlap_optimizer or self.zero):
                # (all gradients of a bucket are enqueued: reduce it on the communication stream, its squared norm behind)
                return BUCKETS, lambda name: self.sync.start(name, post=self._bucket_sumsq)
            return (BUCKETS_LATE if self.zero else SINGLE), (self.sync.start if last and self.overlap else None)
        if self._norm_plan() is not None:
            return FUSED, None  # the squared norm comes out of the weight-gradient GEMMs
        if last and self.overlap_optimizer and self.early_fraction > 0:
            self._done, self._early_lo = {}, None
            return EARLY, self._early_norm
        return SINGLE, None

    def _bucket_sumsq(self, name: str):
        """Squared norm of a bucket's (reduced) gradients.  With several ranks every rank holds the same reduced
        gradients, so each takes the squared norm of its 1/world slice of the bucket only and the slices' sums are
        added over ranks in _finish_norm (one scalar all-reduce, identical on every rank): 1/world of the bytes."""
        g = self.engine.store.g32
        lo, hi = self.engine.store.buckets[name]
        i = self.bucket_index[name]

        def piece(lo, hi):  # this rank's 1/world of [lo, hi); the pieces start 32-byte aligned
            per = (-(-(hi - lo) // self.world) + 7) // 8 * 8
            a = min(hi, lo + self.sync.rank * per)
            return a, min(hi, a + per)

        if self.zero and name in self.sync.shard:
            # sharded bucket: this rank's slice of the matrices + its 1/world piece of the replicated small tensors
            a, b = self.sync.slice_of(name)
            ops.sumsq(g[a:b], b - a, self.bucket_sq[i:i + 1], self.partial)
            a, b = piece(lo, self.sync.shard[name][0])
            if b > a:
                ops.sumsq(g[a:b], b - a, self.bucket_sq[i:i + 1], self.partial, accumulate=True)
            return
        if self.world > 1 and (self.shard_norm or self.zero):
            a, b = piece(lo, hi)
            if b > a:
                ops.sumsq(g[a:b], b - a, self.bucket_sq[i:i + 1], self.partial)
            else:
                ops.clear_f32(self.bucket_sq, 1, off=i)
            return
        ops.sumsq(g[lo:hi], hi - lo, self.bucket_sq[i:i + 1], self.partial)

    def _early_norm(self, name: str):
        """Backward hook (N = 1).  Buckets complete roughly from the end of the flat gradient buffer towards its start;
        once the completed tail [x, hi) covers `early_fraction` of the gradients its squared norm is started on the
        side stream (the split depends only on the bucket layout: deterministic) and only the head of the buffer is
        left for the pass behind the backward."""
        if self._early_lo is not None:
            return
        a, b = self.engine.store.buckets[name]
        lo, hi = self.train_range
        self._done[b] = a  # completed interval, keyed by its end
        x = hi
        while x in self._done:
            x = self._done[x]
        if hi - x < self.early_fraction * (hi - lo) or x <= lo:
            return
        self._early_lo = x
        self.opt_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.opt_stream):
            ops.sumsq(self.engine.store.g32[x:hi], hi - x, self.gnorm_sq, self.partial_early)

    def _finish_norm(self, route: str):
        """Behind the backward and the exchange: whatever `route` left undone of the squared norm, into gnorm_sq."""
        st = self.engine.store
        lo, hi = self.train_range
        if route == BUCKETS_LATE:  # (no per-bucket hooks ran: take the sharded norms here)
            for name in st.buckets:
                self._bucket_sumsq(name)
        if route == FUSED:
            # N = 1: per-tile sums of squares from the weight-gradient GEMMs' epilogues + one pass over the < 1 % of the
            # buffer that is not a layer weight matrix (instead of reading all 8.6 GB of gradients again: 1.5 ms of
            # HBM traffic beside the backward at XLS-R-2B)
            plan = self._norm_plan()
            ops.sumsq_ranges(st.g32, plan["chunks"], plan["nchunks"], self.gnorm_sq, plan["partial"])
            ops.sum_f32(plan["slots"], plan["nslots"], self.gnorm_sq, self.partial, accumulate=True)
        elif route in (BUCKETS, BUCKETS_LATE):
            self.gnorm_sq.copy_(self.bucket_sq.sum().reshape(1))
            if self.world > 1 and (self.shard_norm or self.zero):  # add the ranks' slices (the same result on every rank)
                if self.sync.capi is not None:
                    self.sync.capi.after_current()
                    self.sync.capi.all_reduce(self.gnorm_sq)
                    self.sync.capi.before_current()
                else:
                    torch.distributed.all_reduce(self.gnorm_sq, op=torch.distributed.ReduceOp.SUM, group=self.sync.pg)
        elif route == EARLY and self._early_lo is not None:  # the tail's squared norm is already in gnorm_sq (side stream)
            torch.cuda.current_stream().wait_stream(self.opt_stream)
            ops.sumsq(st.g32[lo:self._early_lo], self._early_lo - lo, self.gnorm_sq, self.partial, accumulate=True)
            self._early_lo = None
        else:  # (EARLY whose tail never reached early_fraction included)
            ops.sumsq(st.g32[lo:hi], hi - lo, self.gnorm_sq, self.partial)

    def finish(self):
        """Make the current stream wait for an optimiser step that is still running on the side stream."""
        if self.opt_done is not None:
            torch.cuda.current_stream().wait_event(self.opt_done)
            self.opt_done = None

    def close(self):
        """Teardown: wait for the optimiser, give the C-ABI communicator and its stream back (one RCCL communicator per
        trainer otherwise stays behind - bench workloads and tests build several per process)."""
        self.finish()
        if torch.cuda.is_available() and self.engine.store.p32.is_cuda:
            torch.cuda.synchronize()
        self._ag_comm = None
        self.sync.close()
        if self._set_compute_cus:
            ops.lib().ca_gemm_set_compute_cus(0)  # later single-GPU trainers of this process launch as a fresh process would
            self._set_compute_cus = False

    def optimizer_step(self):
        eng, st = self.engine, self.engine.store
        lo, hi = self.train_range
        lr = cosine_lr(self.opt_step, self.lr, self.warmup_steps, self.max_steps)
        self.last_lr = lr  # the rate THIS update uses (what Trainer logs as `learning_rate` for the step)
        self.opt_step += 1
        route, self._route = self._route or self._norm_route(last=False)[0], None
        self._finish_norm(route)
        max_blocks = self.bg_blocks if eng.background_optimizer else 0

        def adam(a, b, so, g):
            ops.adamw_step(st.p32[a:b], self.m[so:so + b - a], self.v[so:so + b - a], g[a:b], st.p16[a:b], b - a,
                           lr, self.betas[0], self.betas[1], self.eps, self.wd, self.opt_step,
                           grad_scale=1.0 / self.world, max_norm=self.max_grad_norm, gnorm_sq=self.gnorm_sq,
                           max_blocks=max_blocks)

        # this step's weight-matrix gradients are in the bf16 buffer (train_step), inside the layers' buckets
        bf16 = bool(eng.matrix_grads_bf16 and eng.wgrad_bf16)

        def update(name):
            """AdamW over what this rank keeps of bucket `name`.  Returns the stream the bucket's bf16 slices are being
            gathered on (sharded bucket), else None."""
            for a, b, so, half in self._launches[bf16][name]:  # sharded: the replicated small tensors, this rank's slice
                adam(a, b, so, st.g16 if half else st.g32)
            if not self.zero or name not in self.sync.shard:
                return None
            # the bf16 slices travel on a stream of their own: the AdamW of the next bucket does not wait for this
            # bucket's all-gather, only the forward's per-bucket wait does (the event below is recorded behind it)
            self._ag_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._ag_stream):
                self._allgather_bf16(*self.sync.shard[name], *self.sync.slice_of(name))
            return self._ag_stream

        if not self.overlap_optimizer:
            if self.zero or bf16:
                for name in st.buckets:
                    update(name)
                if self.zero:
                    torch.cuda.current_stream().wait_stream(self._ag_stream)
            else:
                adam(lo, hi, lo, st.g32)  # (one launch over the trainable range: the moments sit at the parameters' offsets)
            if not eng.freeze_base:
                eng.refresh_derived()
            if eng.bucket_copies:
                for name in st.buckets:
                    eng.refresh_bucket(name)
            return
        # buckets in the order the next forward consumes them; one event per bucket
        self.opt_stream.wait_stream(torch.cuda.current_stream())
        events = {}
        with torch.cuda.stream(self.opt_stream):
            for name in self._forward_order:
                gathered_on = update(name)
                if eng.bucket_copies:
                    if gathered_on is not None:
                        self.opt_stream.wait_stream(gathered_on)  # (derived per-bucket copies read the gathered weights)
                    eng.refresh_bucket(name)
                parts = eng.derived_parts if name == "front" else ()
                if name == "front":
                    eng.refresh_derived(parts[0] if parts else None)
                ev = torch.cuda.Event()
                ev.record(gathered_on if (gathered_on is not None and not eng.bucket_copies) else self.opt_stream)
                events[name] = ev
                for part in parts[1:]:  # later parts of the derived weights get events of their own
                    eng.refresh_derived(part)
                    ev = torch.cuda.Event()
                    ev.record(self.opt_stream)
                    events[f"front_{part}"] = ev
            if "front" not in events:
                eng.refresh_derived()
            if eng.preclear_small_grads and not eng.freeze_base:
                # the gradients are consumed: clear what the next backward accumulates into (front / head buckets and
                # the layers' small tensors) here, under the next forward
                eng.clear_small_grads()
                eng.pre_zeroed = True
            if self.zero:
                self.opt_stream.wait_stream(self._ag_stream)  # `finish()` = every gather has landed too
            self.opt_done = torch.cuda.Event()
            self.opt_done.record(self.opt_stream)
        eng.weights_ready = events

    def _allgather_bf16(self, mlo, hi, a, b):
        """Every rank's freshly updated bf16 slice -> the whole [mlo, hi) of the compute copy, on the current stream."""
        p16, pg = self.engine.store.p16, self.sync.pg
        if self._ag_comm is not None:  # C ABI (ca_allgather_bucket, in place, on the gather context's stream)
            self._ag_comm.all_gather(p16[mlo:hi])
            return
        if self.sync._has_rs:  # RCCL: in place (the input slice sits at output + rank * count)
            torch.distributed.all_gather_into_tensor(p16[mlo:hi], p16[a:b], group=pg)
            return
        per = b - a
        outs = [p16[mlo + r * per: mlo + (r + 1) * per] for r in range(self.world)]
        mine = p16[a:b].clone()
        torch.distributed.all_gather(outs, mine, group=pg)

    def consolidate(self):
        """Sharded optimiser: bring the fp32 master parameters of the other ranks' slices up to date on this rank
        (checkpoints and `save_pretrained` read the master buffer; between steps only the bf16 copy is complete) and
        return full-size (m, v) moment buffers in the parameters' layout.  A collective: every rank calls it."""
        st = self.engine.store
        if not self.zero:
            return self.m, self.v
        self.finish()
        m = torch.zeros_like(st.p32)
        v = torch.zeros_like(st.p32)
        copy_state(self._layout, self.m, m, to_full=True)
        copy_state(self._layout, self.v, v, to_full=True)
        for name in (n for n in st.buckets if n in self.sync.shard):  # the other ranks' slices
            mlo = self.sync.shard[name][0]
            a, b = self.sync.slice_of(name)
            per = b - a
            for buf in (st.p32, m, v):
                outs = [buf[mlo + r * per: mlo + (r + 1) * per] for r in range(self.world)]
                torch.distributed.all_gather(outs, buf[a:b].clone(), group=self.sync.pg)
        return m, v

    def load_moments(self, m_full, v_full):
        """Inverse of `consolidate` for resuming: take this rank's part of full-size moment buffers."""
        copy_state(self._layout, self.m, m_full, to_full=False)
        copy_state(self._layout, self.v, v_full, to_full=False)

    def grad_norm(self) -> float:
        """Global gradient norm of the last step (after the DDP mean), host scalar."""
        return float(self.gnorm_sq.sqrt().item()) / self.world
