"""The gradient exchange of the data-parallel trainer (coral_amd/trainer.py): one RCCL communicator behind the C ABI
(`CommContext`), the bucketed all-reduce / reduce-scatter over the flat gradient buffer (`GradSync`), and the two
start-up self-checks of the collectives they rely on (`make_comm_context`, `collectives_selfcheck`).  Nothing here
knows about engines or the optimiser; `GradSync` is device-agnostic, so the N > 1 logic runs under gloo on the CPU
(tests/test_dp_gloo.py)."""

from __future__ import annotations

import ctypes as C
import logging
import os

import torch

from . import ops

log = logging.getLogger(__package__)


class _Handles:
    """Several asynchronous collectives waited for as one."""

    def __init__(self, hs):
        self.hs = hs

    def wait(self):
        for h in self.hs:
            h.wait()


class _Done:
    """Handle of a collective that is ordered by the communication stream itself (the C-ABI path)."""

    def wait(self):
        pass


class CommContext:
    """One RCCL communicator + its communication stream behind the C ABI (include/coral_amd.h: ca_comm_*).  The
    rendezvous - handing rank 0's 128-byte unique id to every rank - rides on the torch.distributed group that launched
    the ranks; every collective afterwards is a ca_* call enqueued on the context's own HIP stream."""

    def __init__(self, device, ident: bytes, rank: int, world: int):
        """`ident`: rank 0's 128-byte unique id (`new_unique_id()`), handed to every rank by the caller."""
        lib = ops.lib()
        self.rank, self.world = rank, world
        self.ctx = None
        with torch.cuda.device(device):
            ctx = C.c_void_p()
            ops.check(lib.ca_comm_init(C.byref(ctx), ident, rank, world), "ca_comm_init")
        self.ctx = ctx
        self.lib = lib
        self.stream = torch.cuda.ExternalStream(lib.ca_comm_stream(ctx), device=device)

    @staticmethod
    def new_unique_id() -> bytes:
        """Binds RCCL through the C ABI (ca_comm_unique_id) and returns a fresh id; raises where it cannot."""
        buf = C.create_string_buffer(128)
        ops.check(ops.lib().ca_comm_unique_id(buf), "ca_comm_unique_id")
        return bytes(buf.raw)

    def close(self, abort: bool = False):
        """Give the communicator and its stream back (ca_comm_destroy: waits for the stream first; `abort`:
        ca_comm_abort, for a context whose peers never joined a collective)."""
        ctx, self.ctx = self.ctx, None
        if ctx is not None:
            (self.lib.ca_comm_abort if abort else self.lib.ca_comm_destroy)(ctx)

    def __del__(self):
        # Not `close()`: ca_comm_destroy waits for the context's stream, and a garbage-collected context (or one collected
        # at interpreter shutdown) may still have a collective in flight whose peers are gone - that wait would never end.
        # An owner that is done with a context calls close(); a context that is merely dropped is left to the process's end.
        self.ctx = None

    @staticmethod
    def _dt(t):
        return {torch.float32: 0, torch.bfloat16: 1}[t.dtype]

    def after_current(self):
        """The communication stream waits for what is enqueued on torch's current stream."""
        ops.check(self.lib.ca_comm_after(self.ctx, torch.cuda.current_stream().cuda_stream), "ca_comm_after")

    def before_current(self):
        """torch's current stream waits for the collectives enqueued so far."""
        ops.check(self.lib.ca_comm_before(self.ctx, torch.cuda.current_stream().cuda_stream), "ca_comm_before")

    def all_reduce(self, t):
        ops.check(self.lib.ca_allreduce_bucket(self.ctx, t.data_ptr(), t.numel(), self._dt(t)), "ca_allreduce_bucket")

    def reduce_scatter(self, t):
        """In place over t (world equal slices): this rank's slice ends with the sum over ranks."""
        ops.check(self.lib.ca_reduce_scatter_bucket(self.ctx, t.data_ptr(), t.numel() // self.world, self._dt(t)),
                  "ca_reduce_scatter_bucket")

    def all_gather(self, t):
        """In place over t: every rank's slice -> all of t on every rank."""
        ops.check(self.lib.ca_allgather_bucket(self.ctx, t.data_ptr(), t.numel() // self.world, self._dt(t)),
                  "ca_allgather_bucket")


# ---- start-up self-checks -----------------------------------------------------------------------------------------
def agree(ok: bool, device, pg) -> bool:
    """True only if EVERY rank of `pg` says so - exchanged over torch.distributed's own communicator on the current
    stream, never over a context under test (one rank: its own verdict, nothing to exchange)."""
    dist = torch.distributed
    if dist.get_world_size(pg) == 1:
        return ok
    flag = torch.tensor([1.0 if ok else 0.0], device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=pg)
    return bool(flag.item() > 0.5)


def _all_enqueued(ctx: CommContext, enqueue, what: str, device, pg) -> bool:
    """Run `enqueue()` (ca_* collectives of `ctx`) behind the current stream's work, under a guard, and return whether
    EVERY rank enqueued.  Only after a True may anything wait for the context's stream: a rank whose call raised has
    enqueued nothing, so its peers' kernels spin - they are aborted, not waited for, and a verdict exchanged behind them
    would never arrive."""
    ok = True
    try:
        ctx.after_current()
        enqueue()
    except Exception as e:  # noqa: BLE001
        log.warning("C-ABI %s not enqueued (%s)", what, e)
        ok = False
    return agree(ok, device, pg)


def make_comm_context(device, pg):
    """A CommContext all ranks agree on, or None (every rank then uses torch.distributed's collectives).  The context
    is created and, with more than one rank, checked once against torch.distributed on a small buffer; the ranks
    exchange their verdicts, so that one rank's failure moves ALL of them to the fallback - never a mixed group."""
    dist = torch.distributed
    world, rank = dist.get_world_size(pg), dist.get_rank(pg)

    def fallback(ctx=None, abort=False):
        if ctx is not None:
            ctx.close(abort=abort)
        log.warning("gradient exchange falls back to torch.distributed's RCCL collectives")
        return None

    # 1. every rank binds RCCL through the C ABI (its own throw-away id proves it); rank 0's id is the one used.
    #    The broadcast happens WHATEVER rank 0 found - its id or a None sentinel - so no rank is left waiting in it.
    ident, ok = None, True
    try:
        ident = CommContext.new_unique_id()
    except Exception as e:  # noqa: BLE001
        log.warning("C-ABI collectives unavailable (%s)", e)
        ok = False
    box = [ident]
    if world > 1:
        src = dist.get_global_rank(pg, 0) if pg is not None else 0
        dist.broadcast_object_list(box, src=src, group=pg)
    if not agree(ok and box[0] is not None, device, pg):
        return fallback()
    # 2. the communicator (collective: every rank passed step 1, so every rank calls it)
    ctx = None
    try:
        ctx = CommContext(device, box[0], rank, world)
    except Exception as e:  # noqa: BLE001
        log.warning("C-ABI communicator not created (%s)", e)
        ok = False
    if not agree(ok, device, pg):
        return fallback(ctx, abort=True)
    # 3. one all-reduce against torch.distributed's
    if world > 1:
        x = (torch.arange(4096, dtype=torch.float32, device=device) % 61) * (rank + 1)
        want = x.clone()
        dist.all_reduce(want, group=pg)
        if not _all_enqueued(ctx, lambda: ctx.all_reduce(x), "all-reduce", device, pg):
            return fallback(ctx, abort=True)
        ctx.before_current()
        if not agree(bool(torch.equal(x, want)), device, pg):
            return fallback(ctx)
    return ctx


def collectives_selfcheck(device, pg, capi: CommContext | None = None) -> bool:
    """One-time check, on the real process group, of the two in-place forms the sharded optimiser relies on:
    reduce-scatter with the output slice inside the input buffer (at input + rank x count) and all-gather with the
    input slice inside the output buffer, against their defining sums - through the C ABI's ca_* collectives when
    `capi` is given, else torch.distributed's.  False on any rank is False on all (the caller rebuilds GradSync without
    the sharded path; a context that failed to enqueue is left to abort)."""
    dist = torch.distributed
    world, rank = dist.get_world_size(pg), dist.get_rank(pg)
    if capi is None and dist.get_backend(pg) != "nccl":
        return True  # (gloo: GradSync cuts the slices out of all-reduces, nothing in place to check)
    n = 4096
    mine = slice(rank * n, (rank + 1) * n)
    base = torch.arange(world * n, dtype=torch.float32, device=device) % 257
    want = base * (world * (world + 1) // 2)
    rs = base * (rank + 1)                                                       # reduce-scattered in place
    ag = torch.zeros(world * n, dtype=torch.bfloat16, device=device)             # all-gathered in place
    ag[mine] = base[mine].to(torch.bfloat16)

    def rs_good():
        return bool(torch.equal(rs[mine], want[mine]))

    def ag_good():
        return bool(torch.equal(ag, base.to(torch.bfloat16)))

    if capi is not None:
        for what, collective, buf, good in (("reduce_scatter", capi.reduce_scatter, rs, rs_good),
                                            ("all_gather", capi.all_gather, ag, ag_good)):
            if not _all_enqueued(capi, lambda: collective(buf), what, device, pg):
                return False
            capi.before_current()
            if not agree(good(), device, pg):
                return False
        return True
    try:
        dist.reduce_scatter_tensor(rs[mine], rs, group=pg)
        dist.all_gather_into_tensor(ag, ag[mine], group=pg)
        ok = rs_good() and ag_good()
    except Exception:  # noqa: BLE001
        ok = False
    try:
        return agree(ok, device, pg)
    except Exception:  # noqa: BLE001
        return False


class GradSync:
    """Bucketed gradient all-reduce over a flat fp32 buffer (device-agnostic, so the N>1 logic is
    testable with gloo on CPU).  `start(name)` launches the asynchronous SUM all-reduce of one
    contiguous bucket — on a side HIP stream when the buffer lives on a GPU — and `finish()` waits
    for all of them.  The 1/world averaging is NOT applied here (it is folded into the fused AdamW
    kernel / `scale_`), so the wire carries plain sums like DDP's buckets.

    compress=True sends bf16 on the wire (the DDP `bf16_compress_hook` trade: half the xGMI bytes —
    4.3 GB instead of 8.6 GB per step for XLS-R-2B — for one bf16 rounding of each rank's gradient);
    the fp32 buffer is refilled from the reduced bf16 values."""

    def __init__(self, flat_grad: torch.Tensor, buckets: dict, process_group=None, compress: bool = False,
                 force: bool = False, shard: dict | None = None):
        """shard: {bucket name: (mlo, hi)} - the part of a bucket that is REDUCE-SCATTERED instead of all-reduced
        (sharded optimiser, see DataParallelTrainer zero_stage): rank r ends up with the sum over ranks of its slice
        [mlo + r * per, mlo + (r + 1) * per), per = (hi - mlo) / world, and nothing defined elsewhere in [mlo, hi); the
        rest of the bucket [lo, mlo) is all-reduced as before."""
        self.g = flat_grad
        self.buckets = buckets
        self.pg = process_group
        self.world = 1
        self.rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        self.shard = dict(shard or {})
        for name, (mlo, hi) in self.shard.items():
            lo, bhi = buckets[name]
            if not (lo <= mlo <= hi == bhi) or (hi - mlo) % (8 * max(1, self.world)):
                raise ValueError(f"shard range of bucket {name!r} must end the bucket and divide into 32-byte aligned slices")
        # reduce_scatter_tensor exists on RCCL; the CPU test backend (gloo) has none: there the slice is cut out of an
        # all-reduce (the same sums; at two ranks the same bits)
        self._has_rs = (torch.distributed.is_available() and torch.distributed.is_initialized()
                        and torch.distributed.get_backend(process_group) == "nccl")
        # force (or CA_DP_FORCE=1): run the whole exchange path with a process group of one rank - how the RCCL
        # plumbing (communication stream, asynchronous handles, per-bucket callbacks) is exercised on a 1-GPU box
        force = force or os.environ.get("CA_DP_FORCE", "0") == "1"
        self.active = self.world > 1 or (force and torch.distributed.is_available() and torch.distributed.is_initialized())
        self.on_gpu = flat_grad.is_cuda
        # RCCL ranks exchange through the C ABI (ca_allreduce_bucket / ca_reduce_scatter_bucket on the context's own
        # stream: include/coral_amd.h); torch.distributed collectives remain for the gloo CPU tests (CA_COMM_CAPI=0
        # forces them on RCCL too: the A/B switch)
        self.capi = None
        if self.active and self.on_gpu and self._has_rs and os.environ.get("CA_COMM_CAPI", "1") != "0":
            self.capi = make_comm_context(flat_grad.device, process_group)
        if self.capi is not None:
            self.comm_stream = self.capi.stream
        else:
            self.comm_stream = ops.side_stream(flat_grad.device, "exchange") if (self.on_gpu and self.active) else None
        self.compress = compress and self.active
        self.g16 = torch.empty_like(flat_grad, dtype=torch.bfloat16) if self.compress else None
        self._pending = []
        self.launched: list[str] = []

    def _to_wire(self, lo, hi):
        if self.on_gpu:
            ops.cast_f32_bf16(self.g[lo:hi], self.g16[lo:hi], hi - lo)  # enqueued on the current (= comm) stream
        else:
            self.g16[lo:hi].copy_(self.g[lo:hi])

    def _from_wire(self, lo, hi):
        if self.on_gpu:
            ops.cast_bf16_f32(self.g16[lo:hi], self.g[lo:hi], hi - lo)
        else:
            self.g[lo:hi].copy_(self.g16[lo:hi])

    def slice_of(self, name: str):
        """This rank's slice (a, b) of bucket `name`'s sharded part."""
        mlo, hi = self.shard[name]
        per = (hi - mlo) // self.world
        return mlo + self.rank * per, mlo + (self.rank + 1) * per

    def _launch(self, lo, hi, name=None):
        buf = self.g
        if self.compress:
            self._to_wire(lo, hi)
            buf = self.g16
        SUM = torch.distributed.ReduceOp.SUM
        if self.capi is not None:  # (called with the communication stream current: ordered by the stream itself)
            if name is None or name not in self.shard:
                self.capi.all_reduce(buf[lo:hi])
            else:
                mlo, _ = self.shard[name]
                if mlo > lo:
                    self.capi.all_reduce(buf[lo:mlo])
                self.capi.reduce_scatter(buf[mlo:hi])
            return _Done()
        if name is None or name not in self.shard:
            return torch.distributed.all_reduce(buf[lo:hi], op=SUM, group=self.pg, async_op=True)
        mlo, _ = self.shard[name]
        hs = []
        if mlo > lo:
            hs.append(torch.distributed.all_reduce(buf[lo:mlo], op=SUM, group=self.pg, async_op=True))
        a, b = self.slice_of(name)
        if self._has_rs:  # in place: the output slice sits at input + rank * count, RCCL's in-place form
            hs.append(torch.distributed.reduce_scatter_tensor(buf[a:b], buf[mlo:hi], op=SUM, group=self.pg, async_op=True))
        else:
            hs.append(torch.distributed.all_reduce(buf[mlo:hi], op=SUM, group=self.pg, async_op=True))
        return _Handles(hs)

    def start(self, name: str, post=None):
        """post(name): run on the communication stream as soon as the bucket's reduced gradients are in
        the fp32 buffer (the trainer computes the bucket's squared norm there, off the critical path)."""
        if not self.active:
            return
        lo, hi = self.buckets[name]
        self.launched.append(name)

        def go():
            h = self._launch(lo, hi, name)
            if post is None:
                return h
            h.wait()  # stream-level wait on a GPU, blocking on the CPU backends
            if self.compress:
                self._from_wire(lo, hi)
            post(name)
            return None

        if self.comm_stream is not None:
            if self.capi is not None:
                self.capi.after_current()  # (ca_comm_after: the bucket's grads are enqueued)
            else:
                self.comm_stream.wait_stream(torch.cuda.current_stream())  # the bucket's grads are enqueued
            with torch.cuda.stream(self.comm_stream):
                h = go()
        else:
            h = go()
        self._pending.append((h, lo, hi))

    def start_all(self):
        for name in self.buckets:
            self.start(name)

    def finish(self):
        def drain():
            for h, lo, hi in self._pending:
                if h is None:
                    continue  # completed on the communication stream in start()
                h.wait()
                if self.compress:
                    self._from_wire(lo, hi)

        if self.comm_stream is not None:
            with torch.cuda.stream(self.comm_stream):
                drain()
            if self.capi is not None:
                self.capi.before_current()
            else:
                torch.cuda.current_stream().wait_stream(self.comm_stream)
        else:
            drain()
        self._pending.clear()
        self.launched.clear()

    def close(self, abort: bool = False):
        """Give the C-ABI communicator (and its stream) back; `abort`: without waiting for its stream."""
        if self.capi is not None:
            self.capi.close(abort=abort)
            self.capi = None
            self.comm_stream = None  # (it wrapped the communicator's HIP stream, gone with it)

    def scale_(self):
        """DDP-mean semantics for host-side consumers: g /= world."""
        if self.world > 1:
            self.g.mul_(1.0 / self.world)
