"""What `DataParallelTrainer` (coral_amd/trainer.py) uses of an engine, written down once: `Engine` declares every
attribute and method the trainer reads, writes or calls, with the default an engine gets without doing anything.
`Wav2Vec2CTCEngine` and the Whisper engines inherit it and override what differs; the trainer never probes."""

from __future__ import annotations

import torch

from .blocks import norm_plan


class Engine:
    """An engine owns `store` (ParamStore: p32 / g32 / p16 and the bucket table) and `device`, and provides
    `__call__(**micro_batch)`, `backward(loss_scale=, overwrite_matrices=, bucket_done=)` and `zero_grad(matrices=)`."""

    # ---- state the trainer sets
    training = False
    step_seed = 0              # of the current micro-batch: the dropout masks derive from it
    freeze_base = False        # only `trainable_range()` is trained
    wgrad_bf16 = False         # this step may keep the layers' weight-matrix gradients in bf16 ...
    matrix_grads_bf16 = False  # ... and the last backward did: they are in store.g16, inside bf16_grad_ranges()
    # {bucket: event}: the trainer may still be updating parameter buckets on its optimiser stream when the next forward
    # starts (the HBM-bound AdamW overlaps the MFMA-bound forward); a forward waits for a bucket's event right before the
    # first kernel that reads its weights
    weights_ready: dict | None = None
    pre_zeroed = False         # the small gradients are already cleared, behind AdamW (preclear_small_grads)
    # ---- capabilities
    background_optimizer = True   # AdamW may run capped to one workgroup per CU beside this engine's forward
    preclear_small_grads = False  # the trainer calls `clear_small_grads()` behind AdamW, under the next forward
    derived_parts = ()            # `refresh_derived(part)` in the order the forward needs them: one event each
    bucket_copies = False         # derived per-bucket weight copies: `refresh_bucket` reads a bucket's final weights
    # ---- caches
    _norm_plan = None
    _small_ranges = None  # the range table of the gradients a step clears
    _wstream = None       # blocks.wgrad_stream

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def _await(self, bucket: str):
        ev = self.weights_ready.get(bucket) if self.weights_ready else None
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def _await_all(self):
        for ev in (self.weights_ready or {}).values():
            torch.cuda.current_stream().wait_event(ev)

    def trainable_range(self) -> tuple:
        """[lo, hi) of the flat parameter buffer the optimiser updates."""
        return tuple(self.store.buckets["head"]) if self.freeze_base else (0, self.store.numel)

    def shard_ranges(self) -> dict:
        """{bucket: (mlo, bucket end)}: what a sharded optimiser may split over the ranks."""
        return {}

    def bf16_grad_ranges(self) -> dict:
        """{bucket: (lo, hi)}: the weight matrices whose gradients a single-micro-batch step may keep in bf16."""
        return {}

    def norm_matrices(self) -> list:
        """(layer, key, first parameter name, rows, cols) of the matrices whose weight-gradient GEMMs leave per-tile
        sums of squares."""
        return []

    def norm_plan(self):
        """Squared gradient norm without a pass over `norm_matrices()` (blocks.norm_plan).  None when the model is frozen
        up to `trainable_range()` (the norm then covers that range only), or without such matrices."""
        if self.freeze_base:
            return None
        if self._norm_plan is None:
            self._norm_plan = norm_plan(self.store, self.norm_matrices(), self.device)
        return self._norm_plan

    def refresh_derived(self, part: str | None = None):
        """Rebuild the weights whose compute copy is not a plain cast.  part: None = all, or one of `derived_parts`."""

    def refresh_bucket(self, name: str):
        """Bucket `name` has just been updated, on the trainer's optimiser stream (`bucket_copies`)."""
