"""The kernels that end every training step, each called directly on a real MI355X and held to the float64 restatements
of tests/step_ref.py (proved on the CPU in tests/test_step_ref_cpu.py): the cross-entropy forward and backward, the
embedding gather and its scatter-add, the fp32 <-> bf16 casts, ca_clear_ranges, the squared norm and the fused AdamW.

Inputs come from seeded CPU generators.  Every output buffer is pre-filled with a sentinel before the launch (NaN for
floats, the byte 0xA5 for integers) and sits between sentinel guards, so an element that was not written, and one that
was written but should not have been, both show.

Tolerances.  Where the result is a function of the bits alone (casts, gathers, sums of small integers, clears) the
comparison is exact.  Cross-entropy and AdamW are held to 16x the error that a plain fp32 evaluation of the same formula
on the CPU (step_ref.ce_f32, step_ref.adamw_f32) has against float64 on the same inputs: the device pre-scales into
hardware exp2 / log2 and sums in another order, a small multiple of one fp32 rounding, whereas a wrong mask, maximum,
label or coefficient is wrong at 1e-3 or worse.  Sums are held to the textbook bound (additions on the longest path)
x 2^-24 x sum |terms|.  The measured error / yardstick ratios are printed (run with -s): on an MI355X the cross-entropy
gradient reaches at most 8.1x the restatement's error (the shifted row at V = 7; 5.6x on the sharp rows) and AdamW at
most 2.4x (v under a bf16 gradient), against the 16x allowed.
"""
import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")
U = R.U


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sentinel(n, dtype):
    """n device elements of sentinel: NaN (floats) or bytes of 0xA5 (integers)."""
    if dtype.is_floating_point:
        return torch.full((n,), NAN, dtype=dtype, device=DEV)
    t = torch.empty(n, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t


def is_sentinel(t):
    t = t.cpu()
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t.contiguous().view(torch.uint8) == 0xA5).all())


def guarded(n, dtype, guard=8, init=None):
    """-> (whole buffer, view of its n payload elements): `guard` sentinel elements on each side; the payload holds
    `init` (a CPU tensor) or sentinel."""
    buf = sentinel(n + 2 * guard, dtype)
    view = buf[guard:guard + n]
    if init is not None:
        view.copy_(init.to(dtype).reshape(-1))
    return buf, view


def guards_intact(buf, n, guard=8):
    return is_sentinel(buf[:guard]) and is_sentinel(buf[guard + n:])


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- cross-entropy ----------------------------------------------------------------------------------------------------
CE_CASES = [(5, 7, 8), (4, 1003, 1008), (3, 4100, 4100), (2, 51865, 51872)]
REGIMES = ("N(0,1)", "N(0,1)*30", "N(0,1)+1e4", "all equal", "-inf in a tenth")


@functools.lru_cache(maxsize=None)
def ce_problem(rows, V, ldv):
    """Every logit regime with every kept label (column 0, column V - 1, 3, the middle), then the skipped labels (-100,
    -1, V, ldv - 1: the last is a valid label where ldv == V), laid out as launches of `rows` rows each.  Columns V..ldv
    hold NaN in even rows and +inf in odd rows.  The references for ignore_index -100 and 3 are computed once."""
    combos = [(reg, lab) for reg in range(5) for lab in (0, V - 1, 3, V // 2)]
    combos += [(i, lab) for i, lab in enumerate((-100, -1, V, ldv - 1))]
    while len(combos) % rows:
        combos.append((len(combos) % 5, 1))
    g = gen(1000 + V)
    x = torch.randn(len(combos), ldv, generator=g)
    for r, (reg, lab) in enumerate(combos):
        if reg == 1:
            x[r] *= 30.0
        elif reg == 2:
            x[r] += 1e4
        elif reg == 3:
            x[r] = -2.71875
        elif reg == 4:
            k = max(1, V // 10)
            cols = [c for c in torch.randperm(V, generator=g)[:k + 1].tolist() if c != lab][:k]
            x[r, cols] = -INF
        x[r, V:] = NAN if r % 2 == 0 else INF
    labels = torch.tensor([lab for _, lab in combos], dtype=torch.int32)
    refs = {}
    for ignore in (-100, 3):
        loss64, kept, grad64 = R.ce_rows_ref(x, labels, V, ignore)
        loss32, grad32 = R.ce_f32(x, labels, V, ignore)
        e_row = (grad32.double() - grad64).abs().amax(dim=1)
        refs[ignore] = (loss64, kept, grad64, loss32, e_row)
    assert bool(refs[-100][1][:20].all()) and int(refs[3][1].sum()) < int(refs[-100][1].sum())
    return x, labels, [reg for reg, _ in combos], refs


def ce_launch(ops, rows, V, ldv, ignore, with_grad, loss0, cnt0):
    x, labels, _, _ = ce_problem(rows, V, ldv)
    total = x.shape[0]
    nl = total // rows
    lg, lab = x.to(DEV), labels.to(DEV)
    loss = sentinel(nl + 2, torch.float32)
    loss[1:-1] = loss0
    cnt = sentinel(nl + 2, torch.int32)
    cnt[1:-1] = cnt0
    gbuf = g = None
    if with_grad:
        gbuf, g = guarded(total * ldv, torch.float32)
    for i in range(nl):
        r0, r1 = i * rows, (i + 1) * rows
        ops.cross_entropy_fwd_bwd(lg[r0:r1], lab[r0:r1], loss[i + 1:i + 2], cnt[i + 1:i + 2],
                                  g[r0 * ldv:r1 * ldv] if with_grad else None, rows, V, ldv, ignore)
    torch.cuda.synchronize()
    assert is_sentinel(loss[:1]) and is_sentinel(loss[-1:]) and is_sentinel(cnt[:1]) and is_sentinel(cnt[-1:])
    grad = None
    if with_grad:
        assert guards_intact(gbuf, total * ldv)
        grad = g.cpu().view(total, ldv)
    return loss[1:-1].cpu().double(), cnt[1:-1].cpu(), grad


def ce_check_loss(rows, V, ldv, ignore, loss, cnt, loss0, cnt0):
    """Per launch: count exact; loss_sum within 16x the fp32 restatement's error on the same sum + rows 2^-23 max
    |loss_row| for the order of the atomic additions.  Onto a non-zero accumulator every one of the `rows` additions
    also rounds at the accumulator's magnitude: + rows 2^-24 (|loss0| + sum |loss_row|), zero when loss0 is."""
    loss64, kept, _, loss32, _ = ce_problem(rows, V, ldv)[3][ignore]
    worst = 0.0
    for i in range(loss.numel()):
        s = slice(i * rows, (i + 1) * rows)
        ref = float(loss64[s].sum())
        e_sum = abs(float(loss32[s].sum()) - ref)
        tol = 16.0 * e_sum + rows * 2.0 ** -23 * float(loss64[s].abs().max())
        if loss0 != 0.0:
            tol += rows * U * (abs(loss0) + float(loss64[s].abs().sum()))
        assert int(cnt[i]) == cnt0 + int(kept[s].sum()), (i, int(cnt[i]))
        got = float(loss[i])
        assert got == got and abs(got) != INF, (i, got)
        err = abs(got - (loss0 + ref))
        assert err <= tol, (i, got, loss0 + ref, err, tol)
        worst = max(worst, err / tol if tol > 0 else 0.0)
    return worst


def ce_check_grad(rows, V, ldv, ignore, grad):
    _, labels, regs, refs = ce_problem(rows, V, ldv)
    _, kept, grad64, _, e_row = refs[ignore]
    assert bool((grad[:, V:] == 0.0).all()), "pad gradient must be written as exactly 0.0"
    ratio = {}
    for r in range(grad.shape[0]):
        if not kept[r]:
            assert bool((grad[r] == 0.0).all()), (r, int(labels[r]))
            continue
        err = float((grad[r].double() - grad64[r]).abs().max())
        e = float(e_row[r])
        q = err / e if e > 0 else (0.0 if err == 0 else INF)
        ratio[regs[r]] = max(ratio.get(regs[r], 0.0), q)
        assert err <= 16.0 * e, (r, REGIMES[regs[r]], int(labels[r]), err, e)
    return ratio


@pytest.mark.parametrize("ignore", [-100, 3])
@pytest.mark.parametrize("rows,V,ldv", CE_CASES)
def test_cross_entropy_matches_float64(ops, rows, V, ldv, ignore):
    loss, cnt, grad = ce_launch(ops, rows, V, ldv, ignore, True, 0.0, 0)
    ratio = ce_check_grad(rows, V, ldv, ignore, grad)
    worst = ce_check_loss(rows, V, ldv, ignore, loss, cnt, 0.0, 0)
    print(f"\nce ({rows}, {V}, {ldv}) ignore {ignore}: grad error / e_row "
          + ", ".join(f"{REGIMES[k]}: {v:.2f}" for k, v in sorted(ratio.items()))
          + f" (allowed 16); loss error / tolerance {worst:.3f}")


@pytest.mark.parametrize("rows,V,ldv", CE_CASES)
def test_cross_entropy_accumulates_and_needs_no_grad_buffer(ops, rows, V, ldv):
    """loss_sum and count are added to (2.5 + sum, 7 + kept), with grad=None, and give what the run with a gradient
    buffer gives (up to the order of the atomic additions)."""
    loss, cnt, _ = ce_launch(ops, rows, V, ldv, -100, False, 2.5, 7)
    ce_check_loss(rows, V, ldv, -100, loss, cnt, 2.5, 7)
    loss_g, cnt_g, _ = ce_launch(ops, rows, V, ldv, -100, True, 0.0, 0)
    loss64 = ce_problem(rows, V, ldv)[3][-100][0]
    assert torch.equal(cnt, cnt_g + 7)
    for i in range(loss.numel()):
        s = slice(i * rows, (i + 1) * rows)
        tol = rows * 2.0 ** -23 * float(loss64[s].abs().max()) + rows * U * (2.5 + float(loss64[s].abs().sum()))
        assert abs(float(loss[i]) - 2.5 - float(loss_g[i])) <= tol


# ---- embedding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 8), (77, 264), (4100, 4096)])
@pytest.mark.parametrize("with_pos", [True, False])
def test_embed_tokens_is_bit_exact(ops, rows, C, with_pos):
    vocab, npos = 11, 13
    g = gen(rows + C)
    table = torch.randn(vocab, C, generator=g).bfloat16()
    pos = (torch.randn(npos, C, generator=g) * 0.5).bfloat16()
    id_sets = []
    if rows == 1:  # one row cannot hit both ends of the table: two launches
        id_sets = [torch.tensor([0], dtype=torch.int32), torch.tensor([vocab - 1], dtype=torch.int32)]
    else:
        ids = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
        ids[0], ids[1], ids[2], ids[-1] = 0, vocab - 1, 0, vocab - 1
        id_sets = [ids]
    td, pd = table.to(DEV), pos.to(DEV)
    for ids in id_sets:
        pos_ids = torch.randint(0, npos, (rows,), generator=g, dtype=torch.int32)
        pos_ids[0], pos_ids[-1] = npos - 1, 0
        ybuf, y = guarded(rows * C, torch.bfloat16)
        ops.embed_tokens(td, pd if with_pos else None, ids.to(DEV), pos_ids.to(DEV) if with_pos else None, y, rows, C)
        torch.cuda.synchronize()
        want = table[ids.long()]
        if with_pos:
            want = (want.float() + pos[pos_ids.long()].float()).bfloat16()
        assert guards_intact(ybuf, rows * C)
        assert torch.equal(bits(y).view(rows, C), bits(want))


def embed_bwd_problem(rows, C, same_id, exact, seed):
    vocab, npos = 13, 16  # (npos >= vocab: a kernel that mixed the two index arrays up would still write inside dpos)
    g = gen(seed)
    if same_id:
        ids = torch.full((rows,), 5, dtype=torch.int32)
        pos_ids = torch.full((rows,), 2, dtype=torch.int32)
    else:  # 11 of the 13 tokens and 7 of the 16 positions: rows 4 and 12 of dtable, 0 and 8.. of dpos are named by no id
        ids = torch.tensor([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11], dtype=torch.int32)[
            torch.randint(0, 11, (rows,), generator=g)]
        pos_ids = torch.randint(1, 8, (rows,), generator=g, dtype=torch.int32)
    if exact:
        dy = torch.randint(-8, 9, (rows, C), generator=g).bfloat16()
        dt0 = torch.randint(-50, 51, (vocab, C), generator=g).float()
        dp0 = torch.randint(-50, 51, (npos, C), generator=g).float()
    else:
        dy = torch.randn(rows, C, generator=g).bfloat16()
        dt0, dp0 = torch.randn(vocab, C, generator=g), torch.randn(npos, C, generator=g)
    return ids, pos_ids, dy, dt0, dp0


@pytest.mark.parametrize("mode", ["both", "dtable_only", "dpos_only", "flat"])
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("rows,same_id", [(64, True), (300, False)])
def test_embed_tokens_bwd_exact_sums(ops, rows, same_id, C, mode):
    """Integer-valued dy on integer-valued accumulators: every fp32 sum is exact, so the result equals the float64
    scatter-add bit for bit whatever the order of the atomics, and rows that no id names keep their bits."""
    ids, pos_ids, dy, dt0, dp0 = embed_bwd_problem(rows, C, same_id, True, 7 * rows + C)
    nt, npz = dt0.numel(), dp0.numel()
    dyd, idd, pid = dy.to(DEV), ids.to(DEV), pos_ids.to(DEV)
    want_t, want_p = R.embed_bwd_ref(dy, ids, pos_ids, dt0, dp0)
    if mode == "flat":  # as the engine: two offsets into one flat fp32 buffer, a sentinel gap between them
        flat = sentinel(8 + nt + 8 + npz + 8, torch.float32)
        t_off, p_off = 8, 8 + nt + 8
        flat[t_off:t_off + nt] = dt0.reshape(-1).to(DEV)
        flat[p_off:p_off + npz] = dp0.reshape(-1).to(DEV)
        ops.embed_tokens_bwd(dyd, idd, pid, flat, flat, rows, C, dtable_off=t_off, dpos_off=p_off)
        torch.cuda.synchronize()
        assert is_sentinel(flat[:8]) and is_sentinel(flat[t_off + nt:p_off]) and is_sentinel(flat[p_off + npz:])
        got_t, got_p = flat[t_off:t_off + nt].cpu(), flat[p_off:p_off + npz].cpu()
    else:
        tbuf, t = guarded(nt, torch.float32, init=dt0)
        pbuf, p = guarded(npz, torch.float32, init=dp0)
        ops.embed_tokens_bwd(dyd, idd, pid, None if mode == "dpos_only" else t, None if mode == "dtable_only" else p,
                             rows, C)
        torch.cuda.synchronize()
        assert guards_intact(tbuf, nt) and guards_intact(pbuf, npz)
        got_t, got_p = t.cpu(), p.cpu()
        if mode == "dpos_only":
            want_t = dt0.double()
        if mode == "dtable_only":
            want_p = dp0.double()
    assert torch.equal(got_t.view_as(dt0).double(), want_t)
    assert torch.equal(got_p.view_as(dp0).double(), want_p)
    if mode in ("both", "flat"):
        assert not torch.equal(want_t, dt0.double()) and not torch.equal(want_p, dp0.double())


@pytest.mark.parametrize("C", [8, 264])
def test_embed_tokens_bwd_random_values_within_summation_bound(ops, C):
    """N(0, 1) gradients, 64 rows on one token: n terms (the accumulator's value and the element's fan-in) added in any
    order differ from the exact sum by at most (n - 1) 2^-24 sum |terms|.  An element with no fan-in keeps its bits."""
    rows = 300
    ids, pos_ids, dy, dt0, dp0 = embed_bwd_problem(rows, C, False, False, 99 + C)
    ids[:64] = 5
    pos_ids[:64] = 2
    tbuf, t = guarded(dt0.numel(), torch.float32, init=dt0)
    pbuf, p = guarded(dp0.numel(), torch.float32, init=dp0)
    ops.embed_tokens_bwd(dy.to(DEV), ids.to(DEV), pos_ids.to(DEV), t, p, rows, C)
    torch.cuda.synchronize()
    assert guards_intact(tbuf, dt0.numel()) and guards_intact(pbuf, dp0.numel())
    want_t, want_p = R.embed_bwd_ref(dy, ids, pos_ids, dt0, dp0)
    abs_t, abs_p = R.embed_bwd_ref(dy.abs(), ids, pos_ids, dt0.abs(), dp0.abs())
    for got, want, mag, index, n0 in ((t, want_t, abs_t, ids, dt0), (p, want_p, abs_p, pos_ids, dp0)):
        fan = torch.bincount(index.long(), minlength=n0.shape[0]).double()[:, None]
        assert int(fan.max()) >= 64
        err = (got.cpu().view_as(n0).double() - want).abs()
        assert bool((err <= fan * U * mag).all()), float((err / (fan * U * mag).clamp_min(1e-300)).max())
        assert torch.equal(got.cpu().view_as(n0)[fan[:, 0] == 0], n0[fan[:, 0] == 0])


# ---- casts ------------------------------------------------------------------------------------------------------------
CAST_SPECIAL = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: kept mantissa even (down) and odd (up)
    0x3F807FFF, 0x3F808001, 0xBF817FFF, 0xBF818001,  # just under and just over the tie
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
    0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x80008001, 0x007F8000,  # fp32 subnormals (the last rounds to normal)
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,  # the largest finite fp32 rounds to inf
    0x7FC00000, 0x7F800001, 0xFFC00001, 0x7F80FFFF, 0xFFFFFFFF,  # NaN (two of them inf-like once truncated)
]


def cast_pool():
    special = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in CAST_SPECIAL], dtype=torch.int32)
    return torch.cat([special.view(torch.float32), torch.randn(101, generator=gen(5)) * 3.0])


def cast_input(n):
    pool = cast_pool()
    reps = (n + pool.numel() - 1) // pool.numel()
    return pool.repeat(reps)[:n].clone()


def assert_bf16_cast(x, y):
    """y (bf16, CPU) is x.to(bfloat16) bit for bit; where x is NaN only NaN is asked."""
    want = x.to(torch.bfloat16)
    nan = torch.isnan(x)
    assert bool(torch.isnan(y[nan]).all())
    assert torch.equal(bits(y)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099, 8 * 2 ** 20 + 1, 8 * 2 ** 20 + 7])
def test_cast_f32_bf16_is_bit_exact(ops, n):
    """(8 * 2^20 floats fill the 8192 x 256 grid of four-float threads exactly: + 1 is the full grid and the tail, + 7 a
    second grid-stride trip and the tail.)"""
    x = cast_input(n)
    ybuf, y = guarded(n, torch.bfloat16)
    ops.cast_f32_bf16(x.to(DEV), y, n)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, n)
    assert_bf16_cast(x, y.cpu())


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_cast_f32_bf16_every_special_value_through_the_tail(ops, n):
    """Windows of n elements over the special patterns, each at x_off = y_off = 8 w: every pattern goes through the
    scalar tail (and through the vector body at n = 5), and the rest of each 8-element slot of y keeps its sentinel."""
    pool = cast_pool()[:len(CAST_SPECIAL) + 5]
    nw = (len(CAST_SPECIAL) + n - 1) // n
    x = torch.zeros(8 * nw)
    for w in range(nw):
        x[8 * w:8 * w + n] = pool[w * n:w * n + n]
    xd = x.to(DEV)
    y = sentinel(8 * nw, torch.bfloat16)
    for w in range(nw):
        ops.cast_f32_bf16(xd, y, n, x_off=8 * w, y_off=8 * w)
    torch.cuda.synchronize()
    yc = y.cpu().view(nw, 8)
    assert bool(torch.isnan(yc[:, n:]).all())
    assert_bf16_cast(x.view(nw, 8)[:, :n].contiguous(), yc[:, :n].contiguous())


def test_cast_f32_bf16_offsets_and_alignment_guard(ops):
    n = 4099
    x = cast_input(n + 4)
    ybuf, y = guarded(n + 4, torch.bfloat16)
    xd = x.to(DEV)
    ops.cast_f32_bf16(xd, y, n, x_off=4, y_off=4)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, n + 4) and is_sentinel(y[:4])
    assert_bf16_cast(x[4:], y[4:].cpu())
    with pytest.raises(ops.CoralAmdError):
        ops.cast_f32_bf16(xd, y, n, x_off=1, y_off=4)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [65536, 2 ** 21 + 5])
def test_cast_bf16_f32_is_exact_for_every_pattern(ops, n):
    pat = (torch.arange(n, dtype=torch.int64) * (1 if n == 65536 else 40503)) % 65536
    assert n != 65536 or pat.unique().numel() == 65536
    x = (pat - (pat >= 32768) * 65536).to(torch.int16).view(torch.bfloat16)
    ybuf, y = guarded(n, torch.float32)
    ops.cast_bf16_f32(x.to(DEV), y, n)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, n)
    want, got = x.float(), y.cpu()
    nan = torch.isnan(want)
    assert bool(torch.isnan(got[nan]).all()) and torch.equal(bits(got)[~nan], bits(want)[~nan])


# ---- clear_ranges -----------------------------------------------------------------------------------------------------
def clear_case(ops, dtype, nelem, ranges, view_start=0, calls=1, one_by_one=False, fn=None):
    """Fill a buffer of `nelem` elements (16 spare on each side) with 0xA5, clear `ranges` (element units, relative to
    the view that starts `view_start` elements in), and compare every byte: exactly the union of the ranges is zero."""
    elt = torch.empty(0, dtype=dtype).element_size()
    base = sentinel(nelem + 32, dtype)
    x = base[16 + view_start:]
    want = torch.full(((nelem + 32) * elt,), 0xA5, dtype=torch.uint8)
    for a, n in ranges:
        lo = (16 + view_start + a) * elt
        want[lo:lo + n * elt] = 0
    for _ in range(calls):
        base.view(torch.uint8).fill_(0xA5)
        if fn is not None:
            fn(x)
        elif one_by_one:
            for r in ranges:
                ops.clear_ranges(x, (r,))
        else:
            ops.clear_ranges(x, ranges)
        torch.cuda.synchronize()
        got = base.view(torch.uint8).cpu()
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, f"{bad.numel()} wrong bytes, first at byte {int(bad[0]) - (16 + view_start) * elt} of the view"


def fp32_edge_ranges():
    """Every start (0, 4, 8, 12 mod 16 bytes) with every length (4 .. 36 and 4100 bytes), 5 to 8 words apart.  (Start 4
    mod 16 with 8 bytes is the range shorter than its own 12-byte head.)"""
    ranges, cur = [], 0
    for nbytes in (4, 8, 12, 16, 20, 28, 32, 36, 4100):
        for start in (0, 1, 2, 3):
            cur = (cur + 3) // 4 * 4 + start
            ranges.append((cur, nbytes // 4))
            cur += nbytes // 4 + 5
    return tuple(ranges), cur


@pytest.mark.parametrize("one_by_one", [False, True])
@pytest.mark.parametrize("view_start", [0, 3])  # 3: the buffer itself is a misaligned view, buf[3:]
def test_clear_ranges_heads_bodies_tails(ops, view_start, one_by_one):
    ranges, n = fp32_edge_ranges()
    clear_case(ops, torch.float32, n + view_start + 8, ranges, view_start=view_start, one_by_one=one_by_one)


def test_clear_ranges_loss_cnt_pattern(ops):
    clear_case(ops, torch.float32, 8, ((0, 2),))
    clear_case(ops, torch.int32, 8, ((0, 2),), view_start=1)


def test_clear_ranges_more_ranges_than_grid_rows(ops):
    ranges = tuple((3 * i + 1, 1) for i in range(1500))  # starts walk 4, 0, 12, 8 mod 16
    clear_case(ops, torch.float32, 4600, ranges)


def test_clear_ranges_long_and_short_ranges_make_two_launches(ops):
    big = (2 ** 20 + 4) // 4
    ranges = [(1, big)]
    cur = 1 + big + 3
    for i in range(20):
        ranges.append((cur, 1 + (i % 9)))
        cur += 1 + (i % 9) + 1 + (i % 3)
    clear_case(ops, torch.float32, cur + 8, tuple(ranges))


def test_clear_ranges_empty_and_adjacent_ranges(ops):
    clear_case(ops, torch.float32, 64, ((5, 0), (9, 3), (12, 6), (40, 0), (41, 2)))
    clear_case(ops, torch.float32, 64, ((7, 0),))  # (nothing to clear: no launch, nothing written)


def test_clear_ranges_bf16_buffer(ops):
    clear_case(ops, torch.bfloat16, 4300, ((2, 2), (6, 10), (30, 4098), (4200, 8)))
    clear_case(ops, torch.bfloat16, 64, ((10, 6),), view_start=2)
    x = sentinel(64, torch.bfloat16)
    with pytest.raises(ops.CoralAmdError):
        ops.clear_ranges(x, ((4, 3),))
    with pytest.raises(ops.CoralAmdError):
        ops.clear_ranges(x, ((3, 4),))
    torch.cuda.synchronize()
    assert is_sentinel(x)


def test_clear_f32(ops):
    clear_case(ops, torch.float32, 5000, ((0, 4099),), fn=lambda x: ops.clear_f32(x, 4099))
    clear_case(ops, torch.float32, 5000, ((7, 4099),), fn=lambda x: ops.clear_f32(x, 4099, off=7))
    clear_case(ops, torch.float32, 16, ((5, 1),), fn=lambda x: ops.clear_f32(x, 1, off=5))


def test_clear_ranges_cached_table_is_reused(ops):
    ranges, n = fp32_edge_ranges()
    ranges += ((n + 2, 3),)  # (a tuple no other test passes: its table is built here)
    before = len(ops._CLEAR_TABLES)
    clear_case(ops, torch.float32, n + 16, ranges, calls=2)  # the same tuple twice, a refill between
    assert len(ops._CLEAR_TABLES) == before + 1


# ---- squared norm -----------------------------------------------------------------------------------------------------
def sumsq_path(n, accumulate):
    """Additions on the longest path from a product to out[0], read off sumsq_kernel and sumsq_finish_kernel:
    per grid-stride trip of a thread 3 (inside v0^2 + v1^2 + v2^2 + v3^2) + 1 (a +=), with 1024 x 256 threads of four
    floats; 1 for the n & 3 tail; 6 (wave butterfly) + 3 (four waves); the finish kernel: 1024 partials / 256 threads =
    4, again 6 + 3, and 1 more when it accumulates onto out[0]."""
    trips = ((n >> 2) + 1024 * 256 - 1) // (1024 * 256)
    return 4 * trips + (1 if n & 3 else 0) + 6 + 3 + 4 + 6 + 3 + (1 if accumulate else 0)


@pytest.mark.parametrize("regime", ["N(0,1)", "1e-20", "1e15", "accumulate"])
@pytest.mark.parametrize("n", [1, 3, 5, 100003, 2 ** 20 + 2])
def test_sumsq_within_summation_bound(ops, n, regime):
    """All terms are non-negative, so the relative error is at most 2^-24 x (additions on the longest path + 1 for the
    rounding of the product).  At 1e-20 the squares are subnormal (their sum is normal again): each product then rounds
    to the 2^-149 grid instead, n 2^-150 in all; 1e15 squares to 1e30, 2^20 of them stay finite."""
    g = gen(n)
    x = torch.randn(n, generator=g)
    if regime in ("1e-20", "1e15"):
        x = torch.sign(x) * (1.0 + 0.25 * torch.rand(n, generator=g)) * float(regime)
    acc = regime == "accumulate"
    buf = sentinel(n + 8, torch.float32)
    buf[4:4 + n] = x.to(DEV)  # the input is a slice at a 16-byte-aligned non-zero offset, NaN on both sides
    out = sentinel(3, torch.float32)
    out0 = 3.25 if acc else None
    if acc:
        out[1] = out0
    partial = sentinel(1024 + 2, torch.float32)
    ops.sumsq(buf[4:4 + n], n, out[1:2], partial[1:1025], accumulate=acc)
    torch.cuda.synchronize()
    assert is_sentinel(out[:1]) and is_sentinel(out[2:]) and is_sentinel(partial[:1]) and is_sentinel(partial[1025:])
    ref = float((x.double() ** 2).sum()) + (out0 if acc else 0.0)
    bound = (sumsq_path(n, acc) + 1) * U * ref + n * 2.0 ** -150
    got = float(out[1])
    assert abs(got - ref) <= bound, (got, ref, abs(got - ref) / bound)


# ---- AdamW ------------------------------------------------------------------------------------------------------------
HYPER = tuple(R.f32r(h) for h in (1e-3, 0.9, 0.98, 1e-8))  # lr, beta1, beta2, eps as the kernel's floats hold them
WD = R.f32r(0.1)
BIG = 8192 * 256 * 4  # the full grid of four-float threads, once


@functools.lru_cache(maxsize=3)
def adamw_inputs(n, gscale, g16, seed=0):
    g = gen(17 * seed + n % 1000 + 1)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    gr = torch.randn(n, generator=g) * gscale
    return p, m, v, gr.bfloat16() if g16 else gr


def norm_sq(g):
    return R.f32r(float((g.double() ** 2).sum()))


def adamw_launch(ops, state, g, wd, step, grad_scale, max_norm, nsq, with_p16=True, max_blocks=0, misalign=False):
    """One ca_adamw_step on guarded device copies.  misalign: the views [1:] of buffers one element longer, so p, m, v
    and an fp32 g are 4-byte aligned only and p16 (and a bf16 g) 2-byte aligned: the kernel's scalar path.  Element 0
    and the element past n keep their sentinels in all five arrays either way.  -> (p, m, v, p16) on the CPU."""
    n = g.numel()
    guard = 1 if misalign else 8
    bufs = [guarded(n, t.dtype, guard, init=t) for t in (*state, g)]
    b16 = guarded(n, torch.bfloat16, guard) if with_p16 else (None, None)
    assert all((b[1].data_ptr() % 16 != 0) == misalign for b in bufs)
    nsq_d = None if nsq is None else torch.tensor([nsq], dtype=torch.float32, device=DEV)
    ops.adamw_step(bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], b16[1], n, *HYPER, wd, step, grad_scale, max_norm,
                   nsq_d, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert all(guards_intact(b[0], n, guard) for b in bufs) and (not with_p16 or guards_intact(b16[0], n, guard))
    assert torch.equal(bits(bufs[3][1]), bits(g)), "the gradient is read only"
    return tuple(b[1].cpu() for b in bufs[:3]) + ((b16[1].cpu(),) if with_p16 else (None,))


def adamw_check(got, state, g, wd, step, grad_scale, max_norm, nsq, ref=None, rest=None):
    """p, m, v: within 16x the fp32 restatement's largest error on the array + 2^-22 |value|; p16 = bf16(p) exactly.
    -> the measured error / restatement error per array."""
    ref = ref or R.adamw_ref(*state, g, *HYPER, wd, step, grad_scale, max_norm, nsq)
    rest = rest or R.adamw_f32(*state, g, *HYPER, wd, step, grad_scale, max_norm, nsq)
    ratios = []
    for name, a, r64, r32 in zip("pmv", got, ref, rest):
        e = float((r32.double() - r64).abs().max())
        err = (a.double() - r64).abs()
        tol = 16.0 * e + 2.0 ** -22 * r64.abs()
        assert bool((err <= tol).all()), (name, float(err.max()), e, float((err / tol.clamp_min(1e-300)).max()))
        ratios.append(float(err.max()) / e if e > 0 else 0.0)
    if got[3] is not None:
        assert torch.equal(bits(got[3]), bits(got[0].to(torch.bfloat16))), "p16 must be bf16(p) of the stored p"
    return ratios


ADAMW_REGIMES = {  # name -> (grad_scale, max_norm, gradient scale, norm given)
    "clip active": (0.25, 1.0, 1.0, True),       # ||g|| grad_scale = 16 at n = 4099
    "clip inactive": (0.25, 1.0, 1e-2, True),    # 0.16: under max_norm, the coefficient is exactly grad_scale
    "max_norm 0": (1.0, 0.0, 1.0, True),
    "no norm": (0.25, 1.0, 1.0, False),
}


@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, WD], ids=["wd0", "wd0.1"])
@pytest.mark.parametrize("regime", list(ADAMW_REGIMES))
def test_adamw_matches_float64(ops, regime, wd, step, g16):
    grad_scale, max_norm, gscale, given = ADAMW_REGIMES[regime]
    n = 4099
    *state, g = adamw_inputs(n, gscale, g16)
    nsq = norm_sq(g) if given else None
    if regime == "clip active":
        assert nsq ** 0.5 * grad_scale > 4 * max_norm
    got = adamw_launch(ops, state, g, wd, step, grad_scale, max_norm, nsq)
    ratios = adamw_check(got, state, g, wd, step, grad_scale, max_norm, nsq)
    print(f"\nadamw {regime}, wd {wd:.1f}, step {step}, {'bf16' if g16 else 'fp32'} g: error / fp32 restatement error "
          f"p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f} (allowed 16 + floor)")
    if regime == "clip inactive":  # the coefficient is exactly grad_scale: the bits of the run without a norm
        assert nsq ** 0.5 * grad_scale < 0.5 * max_norm
        plain = adamw_launch(ops, state, g, wd, step, grad_scale, max_norm, None)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, plain))


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("n,max_blocks", [(1, 0), (3, 0), (7, 0), (4099, 0), (4099, 37)])
def test_adamw_lengths_on_both_paths(ops, n, max_blocks, g16, misalign):
    """The vector path (aligned buffers: quads, then the n & 3 tail) and the scalar path (misaligned views) against the
    same reference at the same tolerance."""
    *state, g = adamw_inputs(n, 3.0, g16, seed=1)
    nsq = norm_sq(g)
    got = adamw_launch(ops, state, g, WD, 2, 0.25, 1.0, nsq, max_blocks=max_blocks, misalign=misalign)
    adamw_check(got, state, g, WD, 2, 0.25, 1.0, nsq)
    none16 = adamw_launch(ops, state, g, WD, 2, 0.25, 1.0, nsq, with_p16=False, max_blocks=max_blocks, misalign=misalign)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got[:3], none16[:3]))  # p16=None changes nothing else


@pytest.mark.parametrize("n,max_blocks,misalign", [(BIG + 3, 0, False), (BIG + 3, 37, False), (BIG + 7, 0, False),
                                                   (BIG + 3, 0, True)])
def test_adamw_full_grid(ops, n, max_blocks, misalign):
    """BIG + 3: every thread of the full grid has one quad, and the tail; + 7: a second grid-stride trip as well; 37
    blocks: many trips per thread; misaligned: the scalar path's grid-stride loop."""
    *state, g = adamw_inputs(n, 1.0, False, seed=2)
    nsq = norm_sq(g)
    got = adamw_launch(ops, state, g, WD, 3, 0.25, 1.0, nsq, max_blocks=max_blocks, misalign=misalign)
    adamw_check(got, state, g, WD, 3, 0.25, 1.0, nsq)


@pytest.mark.parametrize("wd", [0.0, WD], ids=["wd0", "wd0.1"])
def test_adamw_zero_gradient_is_pure_decay(ops, wd):
    n = 4099
    p, _, _, g = adamw_inputs(n, 1.0, False, seed=3)
    g = g.clone()
    zero = torch.arange(n) % 3 == 0
    g[zero] = 0.0
    state = (p, torch.zeros(n), torch.zeros(n))
    nsq = norm_sq(g)
    for misalign in (False, True):
        got = adamw_launch(ops, state, g, wd, 1, 0.25, 1.0, nsq, misalign=misalign)
        adamw_check(got, state, g, wd, 1, 0.25, 1.0, nsq)
        assert bool((got[1][zero] == 0).all()) and bool((got[2][zero] == 0).all())
        decayed = p.double()[zero] * (1.0 - HYPER[0] * wd)
        assert bool(((got[0][zero].double() - decayed).abs() <= 2.0 ** -22 * decayed.abs()).all())
        if wd == 0.0:
            assert torch.equal(bits(got[0][zero]), bits(p[zero]))
        assert not bool((got[1][~zero] == 0).any())


def test_adamw_trajectory_with_device_norm(ops):
    """20 steps with fresh gradients, the norm taken by ops.sumsq each step, above max_norm on even steps and under it
    on odd ones; the float64 and the fp32 restatement trajectories are carried on their own from the same gradients and
    norms."""
    n, grad_scale, max_norm = 4099, 0.25, 1.0
    p, m, v, _ = adamw_inputs(n, 1.0, False, seed=4)
    bufs = [guarded(n, torch.float32, init=t) for t in (p, m, v)]
    gbuf, gd = guarded(n, torch.float32)
    b16, p16 = guarded(n, torch.bfloat16)
    nsq_d = sentinel(1, torch.float32)
    partial = sentinel(1024, torch.float32)
    ref = (p.double(), m.double(), v.double())
    rest = (p, m, v)
    gg = gen(44)
    active = 0
    for step in range(1, 21):
        g = torch.randn(n, generator=gg) * (1.0 if step % 2 == 0 else 1e-2)
        gd.copy_(g)
        ops.sumsq(gd, n, nsq_d, partial)
        ops.adamw_step(bufs[0][1], bufs[1][1], bufs[2][1], gd, p16, n, *HYPER, WD, step, grad_scale, max_norm, nsq_d)
        nsq = float(nsq_d.item())
        assert abs(nsq - float((g.double() ** 2).sum())) <= (sumsq_path(n, False) + 1) * U * nsq
        active += nsq ** 0.5 * grad_scale > max_norm
        ref = R.adamw_ref(*ref, g, *HYPER, WD, step, grad_scale, max_norm, nsq)
        rest = R.adamw_f32(*rest, g, *HYPER, WD, step, grad_scale, max_norm, nsq)
    torch.cuda.synchronize()
    assert active == 10
    assert all(guards_intact(b[0], n) for b in bufs) and guards_intact(gbuf, n) and guards_intact(b16, n)
    got = tuple(b[1].cpu() for b in bufs) + (p16.cpu(),)
    ratios = adamw_check(got, None, None, WD, 20, grad_scale, max_norm, None, ref=ref, rest=rest)
    print(f"\nadamw 20-step trajectory: error / fp32 restatement error p {ratios[0]:.2f} m {ratios[1]:.2f} v {ratios[2]:.2f}")


KNOB_ARGS = (WD, 2, 0.25, 1.0)  # wd, step, grad_scale, max_norm of the tuning-knob children


def knob_child(out_path):
    """Runs in a fresh process (CA_ADAMW_VEC / CA_ADAMW_NT are read once per process): the n = 4099 case, saved."""
    from coral_amd import ops as o

    o.lib()
    *state, g = adamw_inputs(4099, 3.0, False, seed=1)
    got = adamw_launch(o, state, g, *KNOB_ARGS, norm_sq(g))
    torch.save(got, out_path)


@pytest.mark.parametrize("knob", ["CA_ADAMW_VEC", "CA_ADAMW_NT"])
def test_adamw_tuning_knobs(knob, tmp_path):
    out = tmp_path / "adamw.pt"
    here = Path(__file__).resolve().parent
    code = (f"import sys; sys.path[:0] = [{str(here)!r}, {str(here.parent)!r}]; "
            f"import test_step_kernels_gpu as t; t.knob_child({str(out)!r})")
    res = subprocess.run([sys.executable, "-c", code], timeout=120, env={**os.environ, knob: "0"}, capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    got = torch.load(out)
    *state, g = adamw_inputs(4099, 3.0, False, seed=1)
    adamw_check(got, state, g, *KNOB_ARGS, norm_sq(g))
