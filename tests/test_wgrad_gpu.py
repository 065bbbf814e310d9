"""Every route behind ops.wgrad_gemm and ops.wgrad_gemm_group on a real MI355X, each with two kinds of input
(tests/test_wgrad_plan_cpu.py makes them and checks on the CPU that they meet the conditions assumed here):

  exact  dY and X hold -1 / 0 / +1 with density 1 / sqrt(K): every element, column sum and sum of squares is a small
         integer, exact in fp32 (and in bf16) under ANY summation order, so the asserts are torch.equal against the
         float64 reference - a dropped or doubled K-step, a stale slot, a slice accumulated instead of overwritten, a
         wrong tile-to-problem mapping or offset changes bits.  No tolerance.
  real   randn * 0.5 in bf16 against the float64 product, within the derived bound
         2 (K + splits + 2) 2^-24 (|dY|^T |X|) per element (test_wgrad_plan_cpu.g_bound; + 2^-8 |want| for a bf16 G):
         what small integers hide, such as an intermediate rounded to bf16.  max(err / bound) is printed per case.

Operands sit in wider, offset buffers with a large finite value everywhere else; outputs are slices of larger buffers
with sentinels on both sides, pre-filled with NaN when they are to be overwritten.  `-m gpu` only."""
import pytest
import torch

import test_wgrad_plan_cpu as W
from test_wgrad_plan_cpu import EXACT, REAL, U8, U24

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -640.0    # around every output slice (exact in bf16 too)
SLOT = 5.0       # the norm slots before a call (inside and around the matrix's range)
POISON = 1000.0  # operand buffers outside the [K, M] / [K, N] matrices
GAP = 40         # sentinel words between output slices (a multiple of 8)


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return o


def r8(x):
    return (x + 7) // 8 * 8


def embed(t, ld, off):
    """t [K, cols] bf16 -> flat device buffer with t[k, c] at off + k * ld + c and POISON everywhere else."""
    K, cols = t.shape
    assert ld >= r8(cols) and ld % 8 == 0 and off % 8 == 0
    buf = torch.full((off + K * ld + 512,), POISON, dtype=torch.bfloat16)
    buf[off:off + K * ld].view(K, ld)[:, :cols] = t
    return buf.to(DEV)


def dev64(t):
    return t.to(DEV).double()


def report(label, ratio):
    print(f"[wgrad] {label}: max(err / bound) = {ratio:.4f}")


def check_values(kind, got, want, bound, label):
    """got (any dtype) against the float64 `want`: bits in the exact pass, err <= bound in the real pass."""
    assert bool(torch.isfinite(got.float()).all()), label
    if kind == EXACT:
        W.assert_exact_totals(want)
        assert torch.equal(got, want.to(got.dtype)), label
        return
    ratio = float(((got.double() - want).abs() / bound).max())
    report(label, ratio)
    assert ratio <= 1.0, (label, ratio)


def check_matrix(kind, got, want, bound, label):
    if got.dtype == torch.bfloat16:
        if kind == EXACT:
            assert float(want.abs().max()) <= 256
        bound = bound + U8 * want.abs()  # the one rounding
    check_values(kind, got, want, bound, label)


def check_sumsq(kind, inside, stored, split_k, label):
    """The sum over the matrix's slots `inside` against the float64 sum of squares of `stored`: the REFERENCE of what
    the call leaves in the slice (not the result), rounded to bf16 for a bf16 gradient."""
    want = float(stored.double().pow(2).sum())
    got = float(inside.double().sum())
    if kind == EXACT:
        W.assert_exact_sumsq(stored, split_k)
        assert got == want, (label, got, want)
        return
    M, N = stored.shape
    bound = (M * N + 1) * U24 * want  # all terms positive: any fp32 order of M * N + 1 adds is inside
    report(label + " sumsq", abs(got - want) / bound)
    assert abs(got - want) <= bound, (label, got, want)


class Out:
    """A flat gradient buffer: [c_off SENT | M * N slice | GAP SENT | M bias | GAP SENT]; with a bf16 gradient the bias
    part lives in the fp32 buffer Gb as [8 SENT | M bias | 8 SENT]."""

    def __init__(self, kind, M, N, c_off, g16, acc, seed=0):
        dt = torch.bfloat16 if g16 else torch.float32
        self.M, self.N, self.c_off, self.g16 = M, N, c_off, g16
        self.old = W.make_old(kind, M * N, seed).to(DEV) if acc else None
        self.old_b = W.make_old(kind, M, seed + 1).to(DEV)
        self.G = torch.full((c_off + M * N + 2 * GAP + M,), SENT, dtype=dt, device=DEV)
        self.G[c_off:c_off + M * N] = self.old.to(dt) if acc else float("nan")
        if g16:
            self.Gb = torch.full((M + 16,), SENT, dtype=torch.float32, device=DEV)
            self.bias_off = 8
        else:
            self.Gb = None
            self.bias_off = c_off + M * N + GAP
        self.bias_buf()[self.bias_off:self.bias_off + M] = self.old_b

    def bias_buf(self):
        return self.Gb if self.g16 else self.G

    def matrix(self):
        return self.G[self.c_off:self.c_off + self.M * self.N].view(self.M, self.N)

    def bias(self):
        return self.bias_buf()[self.bias_off:self.bias_off + self.M]

    def check_sentinels(self, label, bias_written):
        G, c, n = self.G, self.c_off, self.M * self.N
        assert bool((G[:c] == SENT).all()) and bool((G[c + n:c + n + GAP] == SENT).all()), label
        b, o = self.bias_buf(), self.bias_off
        if self.g16:
            assert bool((G[c + n:] == SENT).all()), label
            assert bool((b[:o] == SENT).all()), label
        assert bool((b[o + self.M:] == SENT).all()), label
        if not bias_written:
            assert torch.equal(self.bias(), self.old_b), label


MODES = ["f32", "f32acc", "bf16"]


def run_wgrad(ops, kind, mode, M, N, K, lda, ldb, *, splits, cs_rows=None, extras=True, label=""):
    """One ops.wgrad_gemm call with everything checked; -> (Out, the operand buffers, their offsets)."""
    g16, acc = mode == "bf16", mode == "f32acc"
    dY, X = W.make_inputs(kind, K, M, N)
    a_off, b_off, c_off = 16, 40, 24
    A, B = embed(dY, lda, a_off), embed(X, ldb, b_off)
    out = Out(kind, M, N, c_off, g16, acc)
    want = W.product64(dev64(dY), dev64(X))
    bound = W.g_bound(dev64(dY), dev64(X), K, splits, out.old)
    if acc:
        want = want + out.old.double().view(M, N)
    ns = ops.sumsq_slots(M, N)
    slots = torch.full((3 + ns + 5,), SLOT, dtype=torch.float32, device=DEV)
    kw = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, c_off=c_off, accumulate=acc, a_off=a_off, b_off=b_off, Gb=out.Gb)
    fused = cs_rows is not None
    if fused:
        cs_off, ld = 24, 24 + M + 40
        ws = torch.full((ops.COLSUM_PARTS, ld), SENT, dtype=torch.float32, device=DEV)
        kw["cs"] = (ws, cs_off, ld)
    elif extras:
        part = torch.zeros(max(ops.colsum_partial_floats(K, M), 4096), dtype=torch.float32, device=DEV)
        kw.update(bias_off=out.bias_off, part=part)
    if extras:
        kw["sq"] = (slots, 3)
    if g16:
        with pytest.raises(ops.CoralAmdError):
            ops.wgrad_gemm(A, B, out.G, **{**kw, "accumulate": True})
    ops.wgrad_gemm(A, B, out.G, **kw)
    torch.cuda.synchronize()
    out.check_sentinels(label, bias_written=extras and not fused)
    check_matrix(kind, out.matrix(), want, bound, label)
    if extras:
        stored = want.to(torch.bfloat16) if g16 else want
        check_sumsq(kind, slots[3:3 + ns], stored, splits > 1, label)
        assert bool((slots[:3] == SLOT).all()) and bool((slots[3 + ns:] == SLOT).all()), label
    else:
        assert bool((slots == SLOT).all())
    colsum = dev64(dY).sum(0)
    if fused:
        got = ws[:cs_rows, cs_off:cs_off + M]
        assert bool(torch.isfinite(got).all()), label
        if kind == EXACT:
            W.assert_exact_totals(got.double(), colsum)  # (each partial row is a small integer too)
        check_values(kind, got.double().sum(0), colsum, W.colsum_bound(dev64(dY), K), label + " colsum")
        rest = ws.clone()
        rest[:cs_rows, cs_off:cs_off + M] = SENT
        assert bool((rest == SENT).all()), label  # both sides of the slice and the rows below
    elif extras:
        check_values(kind, out.bias(), colsum + out.old_b.double(), W.colsum_bound(dev64(dY), K, out.old_b),
                     label + " colsum")
    return out, (A, B), (a_off, b_off)


# ---- 1. wgrad_gemm: every route x both gradient dtypes --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", [EXACT, REAL])
@pytest.mark.parametrize("case", range(len(W.SOLO_CASES)), ids=["%dx%dx%d" % c for c in W.SOLO_CASES])
def test_wgrad_gemm_direct_and_split_k_routes(ops, case, kind, mode):
    """Direct (splits 1) and split-K (2 / 4 / 8) with fp32 overwrite, fp32 accumulate and bf16 overwrite: the matrix,
    the sentinels around it, the norm slots (against the reference, not the result) and the separate column-sum pass
    that accumulates into G[bias_off:] (Gb[bias_off:] with a bf16 G); once bare, once with sq and bias_off."""
    M, N, K = W.SOLO_CASES[case]
    splits = ops._wgrad_splits(M, N, K)
    assert splits == W.SOLO_SPLITS[case]
    lda, ldb = 3 * M, N + 64
    for extras in (False, True):
        label = f"solo {M}x{N}x{K} splits={splits} {kind} {mode}" + (" +sq+bias" if extras else "")
        out, (A, B), (a_off, b_off) = run_wgrad(ops, kind, mode, M, N, K, lda, ldb, splits=splits, extras=extras, label=label)
    if kind == EXACT and K == 1024:
        # the split-K result equals the direct one bit for bit: a plain GEMM with the direct branch's arguments
        assert splits > 1
        acc, g16 = mode == "f32acc", mode == "bf16"
        direct = Out(kind, M, N, out.c_off, g16, acc)
        ops.gemm(A, B, direct.G, M=M, N=N, K=K, a_layout=ops.MNMAJOR, lda=lda, b_layout=ops.MNMAJOR, ldb=ldb, ldc=N,
                 c_off=out.c_off, a_off=a_off, b_off=b_off, out_f32=not g16, accumulate=acc, stream_out=ops.STREAM_WGRAD)
        torch.cuda.synchronize()
        n = out.c_off + M * N + GAP
        assert torch.equal(direct.G[:n], out.G[:n])


# ---- 2. fused bias partials from kernel X ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", [EXACT, REAL])
@pytest.mark.parametrize("M,N,K,rows", W.COLSUM_CASES)
def test_wgrad_gemm_fused_bias_partials(ops, M, N, K, rows, kind, mode):
    """cs=(ws, off, ld): the first min(ceil(N / 256), 8) rows of columns [off, off + M) are overwritten and add up to
    dY.sum(0) - also the rows of parts that own no K-step - and every other word of ws keeps its sentinel."""
    assert rows == min((N + 255) // 256, ops.COLSUM_PARTS)
    run_wgrad(ops, kind, mode, M, N, K, r8(M) + 64, r8(N) + 64, splits=1, cs_rows=rows,
              label=f"cs {M}x{N}x{K} rows={rows} {kind} {mode}")


# ---- 3. ca_gemm_bf16_group on small ragged problems ----------------------------------------------------------------------------
def launch_group(ops, descs):
    from coral_amd._lib import CaGemmDesc, check

    arr = (CaGemmDesc * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = d
    check(ops.lib().ca_gemm_bf16_group(arr, len(descs), ops._stream()), "ca_gemm_bf16_group")


@pytest.mark.parametrize("g16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", [EXACT, REAL])
@pytest.mark.parametrize("K", W.GROUP_KS)
@pytest.mark.parametrize("count", sorted(W.GROUP_ORDERS))
def test_grouped_launch_on_small_ragged_problems(ops, count, K, kind, g16):
    """1, 2, 5 and 8 problems sharing one tile list, each with its own slice of one flat buffer; every second one
    accumulates (fp32), the others get c_sumsq.  Exact pass: a problem gives the same bits alone and in the group."""
    shapes = [W.GROUP_SHAPES[i] for i in W.GROUP_ORDERS[count]]
    dt = torch.bfloat16 if g16 else torch.float32
    probs, c_off, s_off = [], GAP, 3
    for i, (M, N) in enumerate(shapes):
        dY, X = W.make_inputs(kind, K, M, N, seed=i)
        p = dict(M=M, N=N, dY=dY, X=X, lda=r8(M) + 8 * (i % 3), ldb=r8(N) + 16, a_off=8 * i, b_off=16, c_off=c_off,
                 acc=(i % 2 == 1) and not g16, sq=s_off if i % 2 == 0 else None, ns=ops.sumsq_slots(M, N))
        p["A"], p["B"] = embed(dY, p["lda"], p["a_off"]), embed(X, p["ldb"], p["b_off"])
        p["old"] = W.make_old(kind, M * N, seed=i).to(DEV) if p["acc"] else None
        probs.append(p)
        c_off += r8(M * N) + GAP
        s_off += p["ns"] + 3

    def fresh():
        flat = torch.full((c_off,), SENT, dtype=dt, device=DEV)
        for p in probs:
            flat[p["c_off"]:p["c_off"] + p["M"] * p["N"]] = p["old"].to(dt) if p["acc"] else float("nan")
        return flat, torch.full((s_off,), SLOT, dtype=torch.float32, device=DEV)

    def desc(p, flat, slots):
        kw = dict(c_sumsq=slots, c_sumsq_off=p["sq"]) if p["sq"] is not None else {}
        return ops._gemm_desc(p["A"], p["B"], flat, M=p["M"], N=p["N"], K=K, a_layout=ops.MNMAJOR, lda=p["lda"],
                              b_layout=ops.MNMAJOR, ldb=p["ldb"], ldc=p["N"], c_off=p["c_off"], a_off=p["a_off"],
                              b_off=p["b_off"], out_f32=not g16, accumulate=p["acc"], stream_out=ops.STREAM_WGRAD, **kw)

    flat, slots = fresh()
    launch_group(ops, [desc(p, flat, slots) for p in probs])
    torch.cuda.synchronize()
    covered = torch.zeros(c_off, dtype=torch.bool, device=DEV)
    slot_used = torch.zeros(s_off, dtype=torch.bool, device=DEV)
    for i, p in enumerate(probs):
        M, N = p["M"], p["N"]
        label = f"group of {count} K={K} #{i} {M}x{N} {kind} {'bf16' if g16 else 'f32'}" + (" acc" if p["acc"] else "")
        want = W.product64(dev64(p["dY"]), dev64(p["X"]))
        bound = W.g_bound(dev64(p["dY"]), dev64(p["X"]), K, 1, p["old"])
        if p["acc"]:
            want = want + p["old"].double().view(M, N)
        check_matrix(kind, flat[p["c_off"]:p["c_off"] + M * N].view(M, N), want, bound, label)
        covered[p["c_off"]:p["c_off"] + M * N] = True
        if p["sq"] is not None:
            check_sumsq(kind, slots[p["sq"]:p["sq"] + p["ns"]], want.to(torch.bfloat16) if g16 else want, False, label)
            slot_used[p["sq"]:p["sq"] + p["ns"]] = True
    assert bool((flat[~covered] == SENT).all()) and bool((slots[~slot_used] == SLOT).all())
    if kind == EXACT:
        alone, slots1 = fresh()
        for p in probs:
            launch_group(ops, [desc(p, alone, slots1)])
        torch.cuda.synchronize()
        assert torch.equal(alone, flat) and torch.equal(slots1, slots)


# ---- 4. wgrad_gemm_group across plans on one workspace -------------------------------------------------------------------------
@pytest.mark.parametrize("g16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", [EXACT, REAL])
def test_wgrad_gemm_group_across_plans_on_one_workspace(ops, monkeypatch, kind, g16):
    """Step A (one solo launch + one group of four, all fused) and step B (solo + split-K fallback, with new dY) on the
    same bias workspace: after each step the reduced COLSUM_PARTS rows are that step's dY.sum(0) alone, so the partial
    rows that step A's grouped launch left in the fallback problem's slice are gone."""
    K = W.PLAN_K
    monkeypatch.setattr(ops, "FUSE_BIAS_PARTIAL_MIN_K", 512)
    dt = torch.bfloat16 if g16 else torch.float32
    shapes = W.PLAN_STEP_A
    offs, cs_offs, sq_offs = [0], [0], [2]
    for M, N in shapes:
        offs.append(offs[-1] + M * N + GAP)
        cs_offs.append(cs_offs[-1] + M)
        sq_offs.append(sq_offs[-1] + ops.sumsq_slots(M, N) + 2)
    nb = cs_offs[-1]
    ws = torch.zeros(ops.COLSUM_PARTS * nb, dtype=torch.float32, device=DEV)  # (fresh per test: its own _CS_DIRTY entry)
    ops._CS_DIRTY.pop(ws.data_ptr(), None)
    part = torch.zeros(max(ops.colsum_partial_floats(K, 3840), 4096), dtype=torch.float32, device=DEV)
    for step, members in (("A", [0, 1, 2, 3, 4]), ("B", [0, 4])):
        plan = ops._wgrad_plan_idx(tuple((*shapes[i], K) for i in members))
        assert plan == (([0], [[1, 2, 3, 4]], []) if step == "A" else ([0], [], [1]))
        G = torch.full((offs[-1] + (0 if g16 else nb + GAP),), SENT, dtype=dt, device=DEV)
        Gb = torch.full((nb + GAP,), SENT, dtype=torch.float32, device=DEV) if g16 else G
        b0 = 0 if g16 else offs[-1]
        slots = torch.full((sq_offs[-1],), SLOT, dtype=torch.float32, device=DEV)
        probs = []
        for j, i in enumerate(members):
            M, N = shapes[i]
            dY, X = W.make_inputs(kind, K, M, N, seed=ord(step))
            acc = (j % 2 == 1) and not g16
            old = W.make_old(kind, M * N, seed=i).to(DEV) if acc else None
            old_b = W.make_old(kind, M, seed=100 + i).to(DEV)
            G[offs[i]:offs[i] + M * N] = old.to(dt) if acc else float("nan")
            Gb[b0 + cs_offs[i]:b0 + cs_offs[i] + M] = old_b
            # (wgrad_gemm_group passes no operand offsets; the leading dimensions must be multiples of 8: N = 1500)
            probs.append(dict(dY=embed(dY, r8(M), 0), X=embed(X, r8(N), 0), M=M, N=N, K=K, lda=r8(M), ldb=r8(N),
                              c_off=offs[i], accumulate=acc, bias_off=b0 + cs_offs[i], part=part, cs_off=cs_offs[i],
                              sq=(slots, sq_offs[i]), old=old, old_b=old_b, i=i, dY64=dev64(dY), X64=dev64(X)))
        fused = ops.wgrad_gemm_group(probs, G, colsum_ws=ws, colsum_ld=nb, Gb=Gb if g16 else None)
        assert fused == ops.FUSE_BIAS_GRAD  # (CA_FUSE_BIAS=0: separate column-sum passes into the bias slices)
        if fused:
            ops.reduce_rows(ws, ops.COLSUM_PARTS, nb, nb, Gb[b0:], accumulate=True)  # as the engines do
        torch.cuda.synchronize()
        print(f"[wgrad] plan step {step} {kind} {'bf16' if g16 else 'f32'}: plan={plan} fused={fused}")
        covered = torch.zeros(G.numel(), dtype=torch.bool, device=DEV)
        for p in probs:
            M, N, i = p["M"], p["N"], p["i"]
            fallback = step == "B" and i == 4
            splits = ops._wgrad_splits(M, N, K) if fallback else 1
            label = f"plan step {step} {M}x{N}x{K} splits={splits} {kind} {'bf16' if g16 else 'f32'}" + (" acc" if p["accumulate"] else "")
            dY64, X64 = p["dY64"], p["X64"]
            want = W.product64(dY64, X64)
            bound = W.g_bound(dY64, X64, K, splits, p["old"])
            if p["accumulate"]:
                want = want + p["old"].double().view(M, N)
            check_matrix(kind, G[p["c_off"]:p["c_off"] + M * N].view(M, N), want, bound, label)
            covered[p["c_off"]:p["c_off"] + M * N] = True
            ns, so = ops.sumsq_slots(M, N), sq_offs[i]
            check_sumsq(kind, slots[so:so + ns], want.to(torch.bfloat16) if g16 else want, splits > 1, label)
            assert bool((slots[so - 2:so] == SLOT).all()) and bool((slots[so + ns:so + ns + 2] == SLOT).all()), label
            # the bias gradient: this step's column sums alone, on top of what the slice held
            gb = Gb[p["bias_off"]:p["bias_off"] + M]
            check_values(kind, gb, dY64.sum(0) + p["old_b"].double(), W.colsum_bound(dY64, K, p["old_b"]), label + " colsum")
        if not g16:
            covered[offs[-1]:offs[-1] + nb] = True  # (the bias part: slices of problems outside step B hold stale sums)
        assert bool((G[~covered] == SENT).all())
        assert bool((Gb[b0 + nb:] == SENT).all())
    ops._CS_DIRTY.pop(ws.data_ptr(), None)
