"""Weight-gradient routes, host side (no GPU): the invariants of the split-K rule, the workspace wgrad_gemm asks for, the
launch plans tests/test_wgrad_gpu.py relies on, and the test inputs themselves - the exact inputs must give totals
that fp32 holds exactly under any summation order, and a plain fp32 matmul of the real inputs must pass the derived
bound, before either is used to judge a kernel.

The input makers, the bounds and the case lists live here and tests/test_wgrad_gpu.py imports them."""
import re
from pathlib import Path

import pytest
import torch

U24 = 2.0 ** -24  # unit roundoff of fp32
U8 = 2.0 ** -8    # ... of bf16
EXACT, REAL = "exact", "real"

# ---- the cases (M, N, K) of tests/test_wgrad_gpu.py ------------------------------------------------------------------
SOLO_CASES = [(192, 192, 1001), (192, 192, 520), (192, 192, 1024), (192, 192, 2048), (200, 136, 600), (200, 136, 1024)]
SOLO_SPLITS = [1, 2, 4, 8, 2, 4]  # what _wgrad_splits gives for them
COLSUM_CASES = [(40, 72, 130, 1), (300, 520, 130, 3), (1000, 2100, 130, 8), (1000, 2100, 601, 8)]  # (.., rows written)
GROUP_SHAPES = [(300, 264), (40, 520), (257, 257), (512, 256), (64, 1030)]
GROUP_ORDERS = {1: [2], 2: [4, 0], 5: [3, 1, 4, 0, 2], 8: [1, 2, 0, 4, 3, 2, 0, 1]}  # indices into GROUP_SHAPES
GROUP_KS = [64, 200, 576]
PLAN_K = 576
PLAN_STEP_A = [(3840, 3600), (2048, 2048), (2048, 2304), (1000, 1500), (520, 264)]
PLAN_STEP_B = [(3840, 3600), (520, 264)]


def _gen(*key):
    seed = 0
    for k in key:  # (a fixed mix of the case's integers: the same inputs in every process)
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def make_inputs(kind, K, M, N, seed=0):
    """-> dY [K, M], X [K, N] in bf16 (on the CPU).  EXACT: -1 / 0 / +1 with density 1 / sqrt(K), so that every product
    sum, column sum and sum of squares is a small integer; REAL: randn * 0.5 rounded to bf16."""
    g = _gen(K, M, N, seed, kind == EXACT)
    if kind == EXACT:
        p = K ** -0.5

        def one(cols):
            keep = torch.rand(K, cols, generator=g) < p
            sign = torch.randint(0, 2, (K, cols), generator=g) * 2 - 1
            return (keep * sign).to(torch.bfloat16)
    else:
        def one(cols):
            return (torch.randn(K, cols, generator=g) * 0.5).to(torch.bfloat16)
    return one(M), one(N)


def make_old(kind, n, seed=0):
    """What a gradient slice (or a bias slice) holds before an accumulating call: integers in -3..3, or randn."""
    g = _gen(n, seed, 77, kind == EXACT)
    if kind == EXACT:
        return torch.randint(-3, 4, (n,), generator=g).float()
    return torch.randn(n, generator=g)


def product64(dY, X):
    return dY.double().t() @ X.double()


def g_bound(dY, X, K, splits, old=None):
    """Per element: products of two bf16 numbers are exact in fp32, so ANY fp32 summation of n terms is within
    n * 2^-24 * sum |a_k b_k| of the truth; n = K terms + the splits' partial sums + the add of the old value, and the
    factor 2 covers the MFMA's internal adds (which need not round like IEEE).  Accumulating adds the same expression
    on the old value."""
    f = 2.0 * (K + splits + 2) * U24
    b = f * (dY.double().abs().t() @ X.double().abs())
    if old is not None:
        b = b + f * old.double().abs().view_as(b)
    return b


def colsum_bound(dY, K, old=None):
    f = 2.0 * (K + 8) * U24
    b = f * dY.double().abs().sum(0)
    if old is not None:
        b = b + f * old.double().abs()
    return b


def assert_exact_totals(*tensors):
    """The exact pass compares bits: every total it compares must be an integer that fp32 holds under any summation
    order (|t| < 2^24), judged on the float64 reference."""
    for t in tensors:
        t = torch.as_tensor(t, dtype=torch.float64)
        assert bool((t == t.round()).all()) and float(t.abs().max()) < 2.0 ** 24


def slot_sumsq64(G):
    """Sums of squares of the 64 x 64 tiles of G [M, N] (float64), row-major over tiles: what CaGemmDesc.c_sumsq puts
    into the matrix's sumsq_slots(M, N) slots on the direct route."""
    M, N = G.shape
    P = torch.zeros((M + 63) // 64 * 64, (N + 63) // 64 * 64, dtype=torch.float64, device=G.device)
    P[:M, :N] = G.double().pow(2)
    return P.view(P.shape[0] // 64, 64, P.shape[1] // 64, 64).sum((1, 3)).flatten()


def assert_exact_sumsq(G, split_k):
    """Each fp32 total of the norm must be exact: one per 64 x 64 tile on the direct route (the test adds the slots in
    float64), the whole matrix's on the split-K route."""
    s = slot_sumsq64(G)
    assert_exact_totals(s.sum() if split_k else s)


def _all_input_cases():
    for M, N, K in SOLO_CASES:
        yield M, N, K
    for M, N, K, _ in COLSUM_CASES:
        yield M, N, K
    for M, N in GROUP_SHAPES:
        for K in GROUP_KS:
            yield M, N, K
    for M, N in PLAN_STEP_A[2:]:  # (the two largest: the same densities and K, only more of them)
        yield M, N, PLAN_K


# ---- the inputs alone stay inside both conditions ----------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", sorted(set(_all_input_cases())))
def test_inputs_meet_the_conditions_the_gpu_tests_assume(M, N, K):
    dY, X = make_inputs(EXACT, K, M, N)
    assert set(dY.float().unique().tolist()) == {-1.0, 0.0, 1.0} and set(X.float().unique().tolist()) == {-1.0, 0.0, 1.0}
    old = make_old(EXACT, M * N).view(M, N)
    G = product64(dY, X)
    assert float(G.abs().max()) > 0  # (not an empty product)
    assert_exact_totals(G, G + old, dY.double().abs().t() @ X.double().abs(), dY.double().sum(0),
                        dY.double().sum(0) + make_old(EXACT, M, 1))
    from coral_amd import ops

    for t in (G, G + old):
        assert_exact_sumsq(t, ops._wgrad_splits(M, N, K) > 1)
    assert slot_sumsq64(G).numel() == ops.sumsq_slots(M, N)
    assert float((G + old).abs().max()) <= 256  # then bf16 holds every element exactly too
    assert torch.equal((G + old).to(torch.bfloat16).double(), G + old)
    # a plain fp32 product of the real inputs passes the bound of the direct route (and so of every other: it is the
    # smallest), also when it accumulates, and so do fp32 column sums
    dY, X = make_inputs(REAL, K, M, N)
    want = product64(dY, X)
    got = dY.float().t() @ X.float()
    assert bool(((got.double() - want).abs() <= g_bound(dY, X, K, 1)).all())
    old = make_old(REAL, M * N).view(M, N)
    assert bool((((got + old).double() - (want + old.double())).abs() <= g_bound(dY, X, K, 1, old)).all())
    assert bool(((dY.float().sum(0).double() - dY.double().sum(0)).abs() <= colsum_bound(dY, K)).all())
    ss = float(want.pow(2).sum())
    assert abs(float(got.pow(2).sum()) - ss) <= (M * N + 1) * U24 * ss  # (all terms positive: provable)
    if (M, N, K) in SOLO_CASES:
        assert M * N <= 2 ** 16 and (M * N + 1) * U24 < 0.004


# ---- the split rule ----------------------------------------------------------------------------------------------------
SPLIT_KS = sorted(set(list(range(1, 64, 7)) + list(range(250, 530)) + list(range(1000, 1050)) + list(range(2040, 2056))
                      + [576, 600, 601, 904, 3992, 4096, 8192, 12000, 16384, 65536]))


@pytest.mark.parametrize("lo,hi", [(64, 1984), (1984, 3904), (3904, 5824), (5824, 7744)])
def test_split_rule_invariants(lo, hi):
    from coral_amd import ops

    assert len(SPLIT_KS) > 300 and any(k % 2 for k in SPLIT_KS)
    seen = set()
    for M in range(lo, min(hi, 7681), 64):
        tm = (M + 127) // 128
        for N in range(64, 7681, 64):
            tiles = tm * ((N + 127) // 128)
            for K in SPLIT_KS:
                s = ops._wgrad_splits(M, N, K)
                if s == 1:
                    continue
                seen.add(s)
                assert s in (2, 4, 8) and K % s == 0 and K // s >= 256 and tiles * s <= 512, (M, N, K, s)
    assert lo > 64 or seen == {2, 4, 8}


def test_split_rule_on_the_shapes_of_the_gpu_tests():
    from coral_amd import ops

    assert [ops._wgrad_splits(*c) for c in SOLO_CASES] == SOLO_SPLITS
    assert ops._wgrad_splits(520, 264, PLAN_K) == 2   # the fallback problem of step B runs split-K
    assert ops.COLSUM_PARTS == 8 and ops.GROUP_MAX == 8
    for M, N, _, rows in COLSUM_CASES:
        assert min((N + 255) // 256, ops.COLSUM_PARTS) == rows


def test_launch_plans_of_the_gpu_tests():
    """Step A: one solo launch and one group of four, no fallback; step B: solo plus fallback."""
    from coral_amd import ops

    assert ops._wgrad_plan_idx(tuple((m, n, PLAN_K) for m, n in PLAN_STEP_A)) == ([0], [[1, 2, 3, 4]], [])
    assert ops._wgrad_plan_idx(tuple((m, n, PLAN_K) for m, n in PLAN_STEP_B)) == ([0], [], [1])
    assert PLAN_K >= 512 and ops.FUSE_BIAS_PARTIAL_MIN_K > PLAN_K  # (the GPU test lowers it to 512 for step B)


# ---- the workspace of the split-K route ---------------------------------------------------------------------------------
def _sumsq_blocks():
    src = (Path(__file__).resolve().parents[1] / "coral_amd" / "csrc" / "misc.hip").read_text()
    return int(re.search(r"#define\s+SUMSQ_BLOCKS\s+(\d+)", src).group(1))


@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("M,N,K", [(16, 16, 512), (8, 64, 2048), (64, 64, 512), (192, 192, 520), (192, 192, 2048), (200, 136, 1024), (520, 264, 576),
                                   (1280, 1280, 904)])
def test_split_k_workspace_leaves_room_for_the_norm_partials(monkeypatch, M, N, K, g16):
    """wgrad_gemm's split-K branch with the kernels replaced by recorders (CPU tensors, nothing is launched): the
    workspace holds `splits` slices, and ca_sumsq_f32's SUMSQ_BLOCKS partials fit where the branch puts them - behind
    the M * N values whose norm is taken when the gradient is bf16, at the start of the free workspace otherwise."""
    from coral_amd import ops

    blocks = _sumsq_blocks()
    assert blocks == 1024
    s = ops._wgrad_splits(M, N, K)
    assert s > 1
    calls = []
    for name in ("gemm", "reduce_rows", "cast_f32_bf16", "cast_bf16_f32", "sumsq", "clear_f32"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)))
    monkeypatch.setattr(ops, "_SPLITK_WS", {})
    G = torch.zeros(M * N + 8, dtype=torch.bfloat16 if g16 else torch.float32)
    slots = torch.zeros(ops.sumsq_slots(M, N) + 2)
    dY, X = torch.zeros(K, M, dtype=torch.bfloat16), torch.zeros(K, N, dtype=torch.bfloat16)
    ops.wgrad_gemm(dY, X, G, M=M, N=N, K=K, lda=M, ldb=N, c_off=8, accumulate=False, sq=(slots, 1))
    ws = ops._SPLITK_WS[G.device]
    assert ws.numel() >= max(s * M * N, M * N + 4096) and ws.dtype == torch.float32
    by = {n: (a, kw) for n, a, kw in calls}
    ga, gk = by["gemm"]
    assert ga[2] is ws and gk["batch2"] == s and gk["K"] * s == K and gk["sC"] == (0, M * N)
    assert gk["sA"] == (0, gk["K"] * M) and gk["sB"] == (0, gk["K"] * N)
    (src, n, out, partial), _ = by["sumsq"]
    assert n == M * N and out.data_ptr() == slots[1:].data_ptr()
    assert partial.numel() >= blocks
    if g16:
        assert src.data_ptr() == ws.data_ptr() and partial.data_ptr() == ws.data_ptr() + 4 * M * N
        assert by["cast_f32_bf16"][1]["y_off"] == 8
    else:
        assert src.data_ptr() == G[8:].data_ptr() and partial.data_ptr() == ws.data_ptr()
    if ops.sumsq_slots(M, N) > 1:
        (_, n_clear), kw = by["clear_f32"]
        assert n_clear == ops.sumsq_slots(M, N) - 1 and kw["off"] == 2
