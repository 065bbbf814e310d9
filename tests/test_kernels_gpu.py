"""Per-kernel parity on a real MI355X: every C-ABI entry point against a plain torch fp32
statement of the same op (floating point) or bit-exact (integer outputs).  `-m gpu` only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return o


def bf(x):
    return x.to(torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (499, 120, 504), (1000, 1920, 328), (46, 1024, 3992), (100, 72, 40),
                                   (260, 264, 136)])
def test_gemm_layouts(ops, al, bl, M, N, K):
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(N, K, seed=2, scale=0.5))
    ref = A.float() @ B.float().t()
    Mp, Np = (M + 7) // 8 * 8, (N + 7) // 8 * 8
    if al:  # [K][Mp] zero padded rows
        Ad = torch.zeros(K, Mp, dtype=torch.bfloat16)
        Ad[:, :M] = A.t()
    else:
        Ad = A
    if bl:
        Bd = torch.zeros(K, Np, dtype=torch.bfloat16)
        Bd[:, :N] = B.t()
    else:
        Bd = B
    Ad, Bd = Ad.contiguous().to(DEV), Bd.contiguous().to(DEV)
    C = torch.zeros(M, Np, dtype=torch.float32, device=DEV)
    ops.gemm(Ad, Bd, C, M=M, N=N, K=K, lda=(Mp if al else K), ldb=(Np if bl else K), ldc=Np,
             a_layout=al, b_layout=bl)
    torch.cuda.synchronize()
    err = (C[:, :N].cpu() - ref).abs().max().item()
    assert err <= 1e-3 * (K ** 0.5), err  # fp32 accumulate of exact bf16 products


@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(1000, 520, 328), (3992, 1920, 704), (300, 136, 64)])
def test_gemm_pipelined_256x128_kernel(ops, al, bl, M, N, K):
    """Same parity check with the 256x128 3-stage kernel forced (it is normally picked only for
    large problems), including ragged M/N tails, odd K-step counts and a single K-step."""
    ops.lib().ca_gemm_force_kernel(2)
    try:
        test_gemm_layouts(ops, al, bl, M, N, K)
    finally:
        ops.lib().ca_gemm_force_kernel(0)


@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(1000, 520, 328), (3992, 768, 704), (300, 264, 64)])
def test_gemm_256x256_kernel(ops, al, bl, M, N, K):
    """Parity of the 256x256 kernel (forced), ragged tails in both dimensions."""
    ops.lib().ca_gemm_force_kernel(3)
    try:
        test_gemm_layouts(ops, al, bl, M, N, K)
    finally:
        ops.lib().ca_gemm_force_kernel(0)


@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(1000, 520, 328), (904, 1024, 1024), (300, 264, 64), (130, 40, 200), (700, 300, 136)])
def test_gemm_128x128_two_waves_per_simd_kernel(ops, al, bl, M, N, K):
    """Parity of kernel M (128x128 tile shared by 8 waves of 64x32, four-stage ring, forced): ragged tails, a single
    K-step, fewer K-steps than ring stages, a partial last K-step."""
    ops.lib().ca_gemm_force_kernel(5)
    try:
        test_gemm_layouts(ops, al, bl, M, N, K)
    finally:
        ops.lib().ca_gemm_force_kernel(0)


@pytest.mark.parametrize("force", [1, 3])
@pytest.mark.parametrize("al,bl", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("kseg", [24, 100])
def test_gemm_segmented_k(ops, kseg, al, bl, force):
    """Segmented K (a_kseg / b_kseg: row(k) = (k / kseg) * kseg_stride + (k % kseg) * ld of an MN-major operand) on the
    two kernels that have it, S and X, forced.  The source is [nseg][kseg + 5][ld]: five gap rows of 1e4 behind every
    segment, so a wrong hop misses every bound by orders of magnitude.  M, N ragged for both tile sizes, K = 200 with a
    partial last K-step; kseg = 24: two or three hops inside one 64-row K-step and a partial last segment, kseg = 100:
    K-steps with no hop and with one.  A K-major operand keeps kseg = 0.
    (a) every bit of the fp32 output equals the same kernel's on a contiguous copy of the gathered operand (kseg = 0):
    both instantiations feed the same values to the same MFMA chain in the same order, only the addresses differ;
    (b) test_gemm_layouts' bound against the fp32 torch product; (c) the profiler's variant is kind * 8 + 4 + lay."""
    M, N, K = 136, 264, 200
    nseg, rps = -(-K // kseg), kseg + 5
    krow = torch.arange(K)
    src_row = (krow // kseg) * rps + krow % kseg  # row of k in the [nseg * rps][ld] source

    def operand(rows, layout, seed):
        """(device operand as passed, its contiguous twin, [rows][K] fp32 values, ld, kseg arguments)"""
        x = bf(rnd(rows, K, seed=seed, scale=0.5))
        if layout == 0:
            return x.to(DEV), x.to(DEV), x.float(), K, (0, 0)
        seg = torch.full((nseg * rps, rows), 1e4, dtype=torch.bfloat16)
        seg[src_row] = x.t()
        return seg.to(DEV), x.t().contiguous().to(DEV), x.float(), rows, (kseg, rps * rows)

    Ad, Ac, Af, lda, (ak, aks) = operand(M, al, 1)
    Bd, Bc, Bf, ldb, (bk, bks) = operand(N, bl, 2)
    ref = Af @ Bf.t()
    kw = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=N, a_layout=al, b_layout=bl)
    C = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    Cc = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    ops.lib().ca_gemm_force_kernel(force)
    try:
        ops.prof_begin()
        try:
            ops.gemm(Ad, Bd, C, a_kseg=ak, a_kseg_stride=aks, b_kseg=bk, b_kseg_stride=bks, **kw)
        finally:
            fired = [i for i, p in enumerate(ops.prof_end()) if p["count"]]
        ops.gemm(Ac, Bc, Cc, **kw)
        torch.cuda.synchronize()
    finally:
        ops.lib().ca_gemm_force_kernel(0)
    err = (C.cpu() - ref).abs().max().item()
    print(f"segmented K: kseg {kseg} lay {al}{bl} force {force}: variant {fired}, max |err| {err:.3e}, "
          f"bits differing from the contiguous run {int((C != Cc).sum())}")
    assert torch.equal(C, Cc)
    assert err <= 1e-3 * (K ** 0.5), err
    assert fired == [(0 if force == 1 else 2) * 8 + 4 + al * 2 + bl], fired


def test_gemm_epilogues_and_batch(ops):
    M, N, K, Bt = 300, 256, 192, 3
    A, W = bf(rnd(Bt, M, K, seed=3, scale=0.5)), bf(rnd(N, K, seed=4, scale=0.2))
    bias = rnd(N, seed=5)
    R = bf(rnd(Bt, M, N, seed=6))
    Ad, Wd, Rd, bd = A.to(DEV), W.to(DEV), R.to(DEV), bias.to(DEV)
    v = A.float() @ W.float().t() + bias
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, batch2=Bt, sA=(0, M * K), sC=(0, M * N), bias=bd)
    C = torch.zeros(Bt, M, N, dtype=torch.bfloat16, device=DEV)
    C2 = torch.zeros_like(C)
    ops.gemm(Ad, Wd, C, C2=C2, epilogue=ops.EPI_GELU, **kw)
    assert (C.float().cpu() - v).abs().max() < 0.05
    assert (C2.float().cpu() - torch.nn.functional.gelu(v)).abs().max() < 0.05
    ops.gemm(Ad, Wd, C, epilogue=ops.EPI_RESIDUAL, R=Rd, ldr=N, sR=(0, M * N), **kw)
    assert (C.float().cpu() - (v + R.float())).abs().max() < 0.06
    ops.gemm(Ad, Wd, None, C2=C2, epilogue=ops.EPI_GELU_RESIDUAL, R=Rd, ldr=N, sR=(0, M * N), **kw)
    assert (C2.float().cpu() - (torch.nn.functional.gelu(v) + R.float())).abs().max() < 0.06
    u = R.float().requires_grad_(True)
    torch.nn.functional.gelu(u).sum().backward()
    ops.gemm(Ad, Wd, C, epilogue=ops.EPI_DGELU, R=Rd, ldr=N, sR=(0, M * N), **kw)
    assert (C.float().cpu() - v * u.grad).abs().max() < 0.06
    # fp32 accumulate
    Cf = torch.full((Bt, M, N), 2.0, dtype=torch.float32, device=DEV)
    ops.gemm(Ad, Wd, Cf, accumulate=True, **kw)
    assert (Cf.cpu() - (v + 2.0)).abs().max() < 1e-2
    # dropout: same mask in GELU forward and DGELU backward, keep-rate ~ 1-p
    ops.gemm(Ad, Wd, None, C2=C2, epilogue=ops.EPI_GELU, dropout_p=0.25, dropout_seed=7, **kw)
    g = torch.nn.functional.gelu(v)
    kept = (C2.float().cpu() != 0) | (g.abs() < 1e-3)
    rate = kept.float().mean().item()
    assert 0.72 < rate < 0.78, rate
    sel = C2.float().cpu() != 0
    assert ((C2.float().cpu() - g / 0.75)[sel].abs().max()) < 0.08
    ops.gemm(Ad, Wd, C, epilogue=ops.EPI_DGELU, R=Rd, ldr=N, sR=(0, M * N), dropout_p=0.25,
             dropout_seed=7, **kw)
    # the DGELU mask is keyed on (m, n) exactly like the GELU one
    ops.gemm(Ad, Wd, None, C2=C2, epilogue=ops.EPI_GELU, dropout_p=0.25, dropout_seed=7, **kw)
    z1 = (C.float().cpu() == 0) & (v.abs() > 1e-2) & (u.grad.abs() > 1e-2)
    z2 = (C2.float().cpu() == 0) & (g.abs() > 1e-3)
    assert (z1 & ~z2 & (g.abs() > 1e-3)).sum() == 0


@pytest.mark.parametrize("C,act", [(512, 1), (1024, 0), (1920, 0), (128, 0)])
def test_layernorm_fwd_bwd(ops, C, act):
    rows = 777
    x = bf(rnd(rows, C, seed=1, scale=2.0))
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    dy = bf(rnd(rows, C, seed=4))
    dres = bf(rnd(rows, C, seed=5))
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    if act:
        y = torch.nn.functional.gelu(y)
    y.backward(dy.float())
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    yd = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    st = torch.empty(rows, 2, dtype=torch.float32, device=DEV)
    ops.layernorm_fwd(xd, gd, bd, yd, st, rows, C, 1e-5, act)
    assert (yd.float().cpu() - y.detach()).abs().max() < 0.04
    dx = torch.empty_like(yd)
    dg = torch.ones(C, dtype=torch.float32, device=DEV)
    db = torch.ones(C, dtype=torch.float32, device=DEV)
    part = torch.empty(ops.layernorm_bwd_partial_floats(rows, C), dtype=torch.float32, device=DEV)
    ops.layernorm_bwd(dy.to(DEV), xd, gd, bd, st, dres.to(DEV), dx, dg, db, part, rows, C, act)
    want = xr.grad + dres.float()
    assert (dx.float().cpu() - want).abs().max() < 0.05 * max(1.0, want.abs().max().item() / 4)
    assert (dg.cpu() - 1 - gr.grad).abs().max() < 2e-3 * gr.grad.abs().max() + 1e-2
    assert (db.cpu() - 1 - br.grad).abs().max() < 2e-3 * br.grad.abs().max() + 1e-2


@pytest.mark.parametrize("C,act,y32", [(512, 1, False), (512, 1, True), (512, 0, False), (1024, 0, True), (264, 1, False)])
def test_layernorm_fp32_rows_fwd_bwd(ops, C, act, y32):
    """ca_layernorm_fwd_ex / ca_layernorm_bwd_ex: the conv stack's fp32 pre-norm rows (and the fp32 output of its last
    block).  With fp32 on both sides nothing is rounded to bf16: the forward is compared at fp32 tolerance."""
    rows = 1031
    x = rnd(rows, C, seed=1, scale=2.0) + 0.5
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    dy = bf(rnd(rows, C, seed=4))
    dres = bf(rnd(rows, C, seed=5))
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    if act:
        y = torch.nn.functional.gelu(y)
    y.backward(dy.float())
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    yd = torch.empty(rows, C, dtype=torch.float32 if y32 else torch.bfloat16, device=DEV)
    st = torch.empty(rows, 2, dtype=torch.float32, device=DEV)
    ops.layernorm_fwd(xd, gd, bd, yd, st, rows, C, 1e-5, act)
    err = (yd.float().cpu() - y.detach()).abs().max()
    assert err < (2e-5 if y32 else 0.04), err
    # the same row through the bf16 form differs by the rounding of its input: the fp32 form must be the closer one
    if not y32:
        yb = torch.empty_like(yd)
        ops.layernorm_fwd(bf(x).to(DEV), gd, bd, yb, None, rows, C, 1e-5, act)
        assert (yd.float().cpu() - y.detach()).pow(2).mean() <= (yb.float().cpu() - y.detach()).pow(2).mean()
    dx = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    dg = torch.ones(C, dtype=torch.float32, device=DEV)
    db = torch.ones(C, dtype=torch.float32, device=DEV)
    part = torch.empty(ops.layernorm_bwd_partial_floats(rows, C), dtype=torch.float32, device=DEV)
    ops.layernorm_bwd(dy.to(DEV), xd, gd, bd, st, dres.to(DEV), dx, dg, db, part, rows, C, act)
    want = xr.grad + dres.float()
    assert (dx.float().cpu() - want).abs().max() < 0.05 * max(1.0, want.abs().max().item() / 4)
    assert (dg.cpu() - 1 - gr.grad).abs().max() < 2e-3 * gr.grad.abs().max() + 1e-2
    assert (db.cpu() - 1 - br.grad).abs().max() < 2e-3 * br.grad.abs().max() + 1e-2


def test_colsum_and_dgelu(ops):
    rows, N = 3992, 1920
    x = bf(rnd(rows, N, seed=1))
    mask = (torch.arange(rows) % 3 == 0).to(torch.uint8)
    out = torch.zeros(N, dtype=torch.float32, device=DEV)
    part = torch.empty(ops.colsum_partial_floats(rows, N), dtype=torch.float32, device=DEV)
    ops.colsum(x.to(DEV), N, rows, N, out, part, accumulate=False)
    assert (out.cpu() - x.float().sum(0)).abs().max() < 1e-2
    ops.colsum(x.to(DEV), N, rows, N, out, part, accumulate=True, rowmask=mask.to(DEV))
    want = x.float().sum(0) + x.float()[mask.bool()].sum(0)
    assert (out.cpu() - want).abs().max() < 1e-2
    u = bf(rnd(rows, N, seed=2))
    o = torch.empty_like(x, device=DEV)
    ops.dgelu_mul(x.to(DEV), u.to(DEV), o, rows * N)
    ur = u.float().requires_grad_(True)
    torch.nn.functional.gelu(ur).backward(x.float())
    assert (o.float().cpu() - ur.grad).abs().max() < 0.03


def test_wave_normalize_and_conv0(ops):
    B, N = 3, 4000
    x = rnd(B, N, seed=1, scale=0.1) + 0.01
    lens = torch.tensor([4000, 3333, 800], dtype=torch.int32)
    y = torch.empty(B, N, device=DEV)
    ops.wave_normalize(x.to(DEV), lens.to(DEV), y, B, N)
    for b in range(B):
        n = int(lens[b])
        a = x[b, :n]
        want = (a - a.mean()) / torch.sqrt(a.var(unbiased=False) + 1e-7)
        assert (y[b, :n].cpu() - want).abs().max() < 2e-5
        assert (y[b, n:] == 0).all()
    # fused layer 0
    C, k, s = 512, 10, 5
    w, bias = rnd(C, 1, k, seed=2, scale=0.3), 0.05 * rnd(C, seed=3)
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    xin = y.cpu()
    wr, br, gr, ber = [t.clone().requires_grad_(True) for t in (w, bias, gamma, beta)]
    h = torch.nn.functional.conv1d(xin[:, None, :], wr, br, stride=s).transpose(1, 2)
    h = torch.nn.functional.gelu(torch.nn.functional.layer_norm(h, (C,), gr, ber, 1e-5))
    T0 = h.shape[1]
    out = torch.empty(B, T0, C, dtype=torch.bfloat16, device=DEV)
    args = [t.to(DEV).contiguous() for t in (w.view(C, k), bias, gamma, beta)]
    ops.conv0_fwd(y, *args, out, B, N, C, k, s)
    assert (out.float().cpu() - h.detach()).abs().max() < 0.03
    dy = bf(rnd(B, T0, C, seed=6))
    h.backward(dy.float())
    dw = torch.zeros(C, k, device=DEV)
    dbs, dg, dbt = (torch.zeros(C, device=DEV) for _ in range(3))
    part = torch.empty(ops.conv0_bwd_partial_floats(B, N, C, k, s), device=DEV)
    ops.conv0_bwd(y, *args, dy.to(DEV), dw, dbs, dg, dbt, part, B, N, C, k, s)
    for got, want in ((dw.cpu().view(C, 1, k), wr.grad), (dbs.cpu(), br.grad), (dg.cpu(), gr.grad),
                      (dbt.cpu(), ber.grad)):
        assert (got - want).abs().max() < 2e-3 * want.abs().max() + 1e-3


def test_col2im(ops):
    B, L, C, k, s = 2, 41, 16, 3, 2
    T = (L - k) // s + 1
    dcol = bf(rnd(B, T, k * C, seed=1))
    want = torch.zeros(B, L, C)
    dc = dcol.float().view(B, T, k, C)
    for t in range(T):
        for j in range(k):
            want[:, t * s + j] += dc[:, t, j]
    dx = torch.empty(B, L, C, dtype=torch.bfloat16, device=DEV)
    ops.col2im_1d(dcol.to(DEV), dx, B, T, L, C, k, s)
    assert (dx.float().cpu() - want).abs().max() < 0.02


def test_ctc_matches_golden_and_torch(ops, golden_dir):
    z = np.load(golden_dir / "ctc_cases.npz")
    for i in range(int(z["n_cases"])):
        lg = torch.tensor(z[f"c{i}_logits"])
        T, V = lg.shape
        tg = torch.tensor(z[f"c{i}_targets"], dtype=torch.int32)
        L = max(1, len(tg))
        labels = torch.full((1, L + 2), -100, dtype=torch.int32)
        labels[0, :len(tg)] = tg
        Vp = (V + 7) // 8 * 8
        lgd = torch.zeros(1, T, Vp, device=DEV)
        lgd[0, :, :V] = lg.to(DEV)
        nll = torch.zeros(1, device=DEV)
        grad = torch.full((1, T, Vp), 7.0, device=DEV)
        ws = torch.zeros(ops.ctc_workspace_bytes(1, T, L + 2), dtype=torch.uint8, device=DEV)
        tin = torch.tensor([int(z[f"c{i}_tin"])], dtype=torch.int32, device=DEV)
        ops.ctc_loss_fwd_bwd(lgd, labels.to(DEV), tin, nll, grad, None, ws, 1, T, V, Vp, L + 2, V - 1)
        want = float(z[f"c{i}_loss"])
        assert abs(nll.item() - want) <= 1e-4 * max(1.0, abs(want)), (i, nll.item(), want)  # << 1e-3 rel
        np.testing.assert_allclose(grad[0, :, :V].cpu().numpy(), z[f"c{i}_grad"], atol=3e-5, rtol=1e-3)
        assert (grad[0, :, V:] == 0).all()
    # BASELINE-sized batch vs torch on the same seeded inputs
    B, T, V, Vp, Lmax = 8, 499, 46, 48, 120
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(B, T, V, generator=g)
    labels = torch.full((B, Lmax), -100, dtype=torch.long)
    tl = torch.randint(20, Lmax + 1, (B,), generator=g)
    for b in range(B):
        labels[b, :tl[b]] = torch.randint(0, 42, (int(tl[b]),), generator=g)
    tin = torch.tensor([499, 499, 400, 300, 499, 250, 499, 130])
    lgr = lg.clone().requires_grad_(True)
    lp = torch.log_softmax(lgr, -1).transpose(0, 1)
    ref = torch.nn.functional.ctc_loss(lp, labels[labels >= 0], tin, tl, blank=45, reduction="none",
                                       zero_infinity=True)
    ref.sum().backward()
    lgd = torch.zeros(B, T, Vp, device=DEV)
    lgd[..., :V] = lg.to(DEV)
    nll = torch.zeros(B, device=DEV)
    grad = torch.zeros(B, T, Vp, device=DEV)
    ws = torch.zeros(ops.ctc_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    ops.ctc_loss_fwd_bwd(lgd, labels.to(torch.int32).to(DEV), tin.to(torch.int32).to(DEV), nll, grad, None,
                         ws, B, T, V, Vp, Lmax, 45)
    assert (nll.cpu() - ref.detach()).abs().max() <= 1e-4 * ref.abs().max()
    # alpha+beta+nll-lp has magnitude ~1.5e3 here: a few fp32 ulps (1.2e-4) of it move exp() by ~1e-3 rel
    assert (grad[..., :V].cpu() - lgr.grad).abs().max() < 2e-3


def test_greedy_decode_bit_exact(ops, golden_dir):
    import json

    from oracle import wav2vec2_ref as ref

    z = json.loads((golden_dir / "tokenizer_collapse.json").read_text())
    T = max(len(r) for r in z["rows"])
    B, V, Vp = len(z["rows"]), 46, 48
    lg = torch.full((B, T, Vp), -3.0)
    lens = []
    for b, row in enumerate(z["rows"]):
        lg[b, torch.arange(len(row)), torch.tensor(row)] = 4.0
        lg[b, len(row):, 45] = 4.0
        lens.append(len(row))
    g = torch.Generator().manual_seed(3)
    lg[..., :V] += 0.5 * torch.rand(B, T, V, generator=g)
    raw = torch.empty(B, T, dtype=torch.int32, device=DEV)
    ids = torch.empty(B, T, dtype=torch.int32, device=DEV)
    olen = torch.empty(B, dtype=torch.int32, device=DEV)
    ops.ctc_greedy_decode(lg.to(DEV), None, raw, ids, olen, B, T, V, Vp, 45)
    want = ref.greedy_ctc_ids(lg[..., :V].numpy(), 45)
    assert (raw.cpu().numpy() == lg[..., :V].numpy().argmax(-1)).all()
    for b in range(B):
        got = ids[b, :int(olen[b])].cpu().tolist()
        assert got == want[b]
        assert ref.ids_to_text(got, z["vocab"]) == z["texts"][b]
    # ties: first maximum wins (np.argmax semantics)
    tie = torch.zeros(1, 4, Vp)
    tie[0, :, 5] = 1.0
    tie[0, :, 9] = 1.0
    traw, tids = raw[:1, :4].contiguous(), ids[:1, :4].contiguous()
    ops.ctc_greedy_decode(tie.to(DEV), None, traw, tids, olen[:1], 1, 4, V, Vp, 45)
    assert (traw == 5).all()
    assert int(tids[0, 0]) == 5 and int(olen[0]) == 1 and (tids[0, 1:] == -1).all()


def test_posconv_weight_fwd_bwd(ops):
    d, G, K = 128, 16, 128
    Cg = d // G
    v, g = rnd(d, Cg, K, seed=1, scale=0.1), 1 + 0.2 * torch.rand(1, 1, K)
    vr, gr = v.clone().requires_grad_(True), g.clone().requires_grad_(True)
    w = gr * vr / vr.norm(p=2, dim=(0, 1), keepdim=True)
    wf = torch.empty(d * K * Cg, dtype=torch.bfloat16, device=DEV)
    wb = torch.empty_like(wf)
    norm = torch.empty(K, device=DEV)
    part = torch.empty(ops.posconv_partial_floats(K), device=DEV)
    vd, gd = v.to(DEV), g.to(DEV)
    ops.posconv_weight(vd, gd, wf, wb, norm, part, d, Cg, K)
    want_f = w.detach().view(G, Cg, Cg, K).permute(0, 1, 3, 2)          # [g][co][j][ci]
    want_b = w.detach().flip(-1).view(G, Cg, Cg, K).permute(0, 2, 3, 1)  # [g][ci][j'][co]
    assert (wf.float().cpu().view(G, Cg, K, Cg) - want_f).abs().max() < 2e-3
    assert (wb.float().cpu().view(G, Cg, K, Cg) - want_b).abs().max() < 2e-3
    dw = rnd(d, Cg, K, seed=2)
    w.backward(dw)
    dwf = dw.view(G, Cg, Cg, K).permute(0, 1, 3, 2).contiguous().to(DEV)
    dv = torch.zeros(d, Cg, K, device=DEV)
    dg = torch.zeros(K, device=DEV)
    ops.posconv_weight_bwd(dwf, vd, gd, norm, dv, dg, part, d, Cg, K)
    assert (dv.cpu() - vr.grad).abs().max() < 1e-3 * vr.grad.abs().max() + 1e-5
    assert (dg.cpu() - gr.grad.view(K)).abs().max() < 1e-3 * gr.grad.abs().max() + 1e-5


def test_optimizer_kernels(ops):
    n = 100_003
    p, g = rnd(n, seed=1), rnd(n, seed=2, scale=0.1)
    pad = (n + 7) // 8 * 8
    pd = torch.zeros(pad, device=DEV)
    pd[:n] = p.to(DEV)
    gd = torch.zeros(pad, device=DEV)
    gd[:n] = g.to(DEV)
    m, v = torch.zeros(pad, device=DEV), torch.zeros(pad, device=DEV)
    p16 = torch.zeros(pad, dtype=torch.bfloat16, device=DEV)
    nsq = torch.zeros(1, device=DEV)
    part = torch.zeros(4096, device=DEV)
    ops.sumsq(gd, pad, nsq, part)
    assert abs(nsq.item() - (g.double() ** 2).sum().item()) < 1e-3 * (g ** 2).sum().item()
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
    for step in (1, 2, 3):
        pr.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([pr], 1.0)
        opt.step()
        ops.sumsq(gd, pad, nsq, part)
        ops.adamw_step(pd, m, v, gd, p16, pad, 1e-3, 0.9, 0.98, 1e-8, 0.01, step, 1.0, 1.0, nsq)
    assert (pd[:n].cpu() - pr.detach()).abs().max() < 2e-6
    assert (p16[:n].float().cpu() - pr.detach()).abs().max() < 2e-2
    # the grid cap of ca_adamw_step_ex (the background form the trainer runs under the next forward): the same bits
    outs = []
    for blocks in (0, 1, 37, 256):
        q, qm, qv, q16 = pd.clone(), m.clone(), v.clone(), p16.clone()
        ops.adamw_step(q, qm, qv, gd, q16, pad, 1e-3, 0.9, 0.98, 1e-8, 0.01, 4, 1.0, 1.0, nsq, max_blocks=blocks)
        outs.append((q, qm, qv, q16))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    assert not torch.equal(outs[0][0], pd)
    # a bf16 gradient (ca_adamw_step_g16: weight-matrix gradients kept as the reference's autocast produces them) gives
    # the bits of the fp32 kernel on the same, rounded values - full grid, capped grid, odd length (scalar tail)
    g16 = gd.to(torch.bfloat16)
    gr = g16.float()
    for length, blocks in ((pad, 0), (pad, 37), (pad - 3, 0)):
        a = [t.clone() for t in (pd, m, v, p16)]
        b = [t.clone() for t in (pd, m, v, p16)]
        ops.adamw_step(a[0], a[1], a[2], gr, a[3], length, 1e-3, 0.9, 0.98, 1e-8, 0.01, 4, 1.0, 1.0, nsq, max_blocks=blocks)
        ops.adamw_step(b[0], b[1], b[2], g16, b[3], length, 1e-3, 0.9, 0.98, 1e-8, 0.01, 4, 1.0, 1.0, nsq, max_blocks=blocks)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], pd)


def test_misc_reorders(ops):
    Co, Ci, k = 8, 16, 3
    w = rnd(Co, Ci, k, seed=1)
    wr = torch.empty(Co * k * Ci, dtype=torch.bfloat16, device=DEV)
    ops.conv_weight_reorder(w.to(DEV), wr, Co, Ci, k)
    assert (wr.float().cpu().view(Co, k, Ci) - w.permute(0, 2, 1)).abs().max() < 1e-2
    dwr = rnd(Co, k, Ci, seed=2)
    dw = torch.ones(Co, Ci, k, device=DEV)
    ops.conv_weight_grad_reorder(dwr.to(DEV), dw, Co, Ci, k)
    assert (dw.cpu() - 1 - dwr.permute(0, 2, 1)).abs().max() < 1e-6
    x = rnd(37, 53, seed=3)
    y = torch.empty(53, 37, dtype=torch.bfloat16, device=DEV)
    ops.transpose_f32_bf16(x.to(DEV), y, 37, 53)
    assert (y.float().cpu() - x.t()).abs().max() < 2e-2
    # regroup_pad + mask_frames
    B, T, G, Cg, pad = 2, 9, 4, 8, 3
    h = bf(rnd(B, T, G * Cg, seed=4))
    xg = torch.empty(B, G, T + 2 * pad, Cg, dtype=torch.bfloat16, device=DEV)
    ops.regroup_pad(h.to(DEV), xg, B, T, G, Cg, pad)
    want = torch.zeros(B, G, T + 2 * pad, Cg)
    want[:, :, pad:pad + T] = h.float().view(B, T, G, Cg).permute(0, 2, 1, 3)
    assert (xg.float().cpu() - want).abs().max() == 0
    tm = torch.zeros(B, T, dtype=torch.uint8)
    tm[0, 2] = 1
    fm = torch.zeros(B, G * Cg, dtype=torch.uint8)
    fm[1, 5] = 1
    emb = bf(rnd(G * Cg, seed=5))
    flen = torch.tensor([9, 6], dtype=torch.int32)
    hd = h.clone().to(DEV)
    ops.mask_frames(hd, tm.to(DEV), fm.to(DEV), emb.to(DEV), flen.to(DEV), B, T, G * Cg)
    want = h.clone()
    want[0, 2] = emb
    want[1, :, 5] = 0
    want[1, 6:] = 0
    assert (hd.cpu().float() - want.float()).abs().max() == 0


@pytest.mark.parametrize("hd,H,Tq,Tk,causal,pad", [(64, 2, 499, 499, False, True), (120, 2, 499, 499, False, True),
                                                    (80, 3, 130, 130, False, False), (32, 4, 12, 12, False, True),
                                                    (64, 2, 77, 77, True, False), (64, 2, 40, 300, False, False),
                                                    (64, 4, 1, 1500, False, False), (64, 3, 5, 333, False, True),
                                                    (128, 1, 200, 200, True, True), (64, 3, 130, 333, False, True),
                                                    (64, 2, 300, 300, True, False), (120, 2, 257, 129, False, False)])
def test_fused_attention_fwd_bwd(ops, hd, H, Tq, Tk, causal, pad):
    _check_attention_fwd_bwd(ops, 2, hd, H, Tq, Tk, causal, pad)


def _check_attention_fwd_bwd(ops, B, hd, H, Tq, Tk, causal, pad, dropout_p=0.0, dropout_seed=0):
    """ca_attn_fwd / ca_attn_bwd against an fp32 torch statement of softmax(scale QK^T + masks) V and
    its autograd gradients; q,k,v live in one fused [B*T, 3d] buffer like the engine's (self-attention)
    or in separate buffers (cross-attention shapes).  With dropout the kernels' keep decisions, restated in NumPy
    (_keep_mask_np), scale the reference's probabilities."""
    d = H * hd
    g = torch.Generator().manual_seed(hd + Tq + Tk)
    scale = hd ** -0.5
    fused = Tq == Tk
    if fused:
        qkv = bf(torch.randn(B, Tq, 3 * d, generator=g))
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    else:
        q, k, v = bf(torch.randn(B, Tq, d, generator=g)), bf(torch.randn(B, Tk, d, generator=g)), bf(torch.randn(B, Tk, d, generator=g))
    klen = torch.tensor(([Tk, max(1, Tk * 3 // 5)] * B)[:B], dtype=torch.int32) if pad else None
    dO = bf(torch.randn(B, Tq, d, generator=g))

    def heads(x, T):
        return x.float().view(B, T, H, hd).transpose(1, 2)

    qr, kr, vr = [heads(t, T).clone().requires_grad_(True) for t, T in ((q, Tq), (k, Tk), (v, Tk))]
    s = qr @ kr.transpose(-1, -2) * scale
    mask = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if klen is not None:
        mask = mask & (torch.arange(Tk)[None, None, None, :] < klen[:, None, None, None])
    if causal:
        mask = mask & (torch.arange(Tk)[None, None, None, :] <= torch.arange(Tq)[None, None, :, None])
    s = s.masked_fill(~mask, float("-inf"))
    probs = torch.softmax(s, -1)
    if dropout_p:
        from test_whisper_gpu import _keep_mask_np

        keep = _keep_mask_np(dropout_seed, B * H * Tq, Tk, dropout_p).reshape(B, H, Tq, Tk)
        probs = probs * (torch.from_numpy(keep.astype("float32")) / (1.0 - dropout_p))
    o_ref = probs @ vr
    o_ref.backward(heads(dO, Tq))
    o_ref = o_ref.detach().transpose(1, 2).reshape(B, Tq, d)

    Tqp = (Tq + 31) // 32 * 32
    lse = torch.zeros(B, H, Tqp, device=DEV)
    Dq = torch.zeros(B, H, Tqp, device=DEV)
    O = torch.zeros(B, Tq, d, dtype=torch.bfloat16, device=DEV)
    kd = klen.to(DEV) if klen is not None else None
    if fused:
        buf = qkv.to(DEV).contiguous()
        Qd = Kd = Vd = buf
        offs = dict(q_off=0, k_off=d, v_off=2 * d)
        lds = dict(ldq=3 * d, ldk=3 * d, ldv=3 * d, sqb=Tq * 3 * d, skb=Tk * 3 * d, svb=Tk * 3 * d)
        dbuf = torch.zeros(B, Tq, 3 * d, dtype=torch.bfloat16, device=DEV)
        dQd = dKd = dVd = dbuf
        doffs = dict(dq_off=0, dk_off=d, dv_off=2 * d)
        dlds = dict(lddq=3 * d, lddk=3 * d, lddv=3 * d, sdqb=Tq * 3 * d, sdkb=Tk * 3 * d, sdvb=Tk * 3 * d)
    else:
        Qd, Kd, Vd = q.to(DEV).contiguous(), k.to(DEV).contiguous(), v.to(DEV).contiguous()
        offs = {}
        lds = dict(ldq=d, ldk=d, ldv=d, sqb=Tq * d, skb=Tk * d, svb=Tk * d)
        dQd = torch.zeros(B, Tq, d, dtype=torch.bfloat16, device=DEV)
        dKd, dVd = torch.zeros(B, Tk, d, dtype=torch.bfloat16, device=DEV), torch.zeros(B, Tk, d, dtype=torch.bfloat16, device=DEV)
        doffs = {}
        dlds = dict(lddq=d, lddk=d, lddv=d, sdqb=Tq * d, sdkb=Tk * d, sdvb=Tk * d)
    common = dict(B=B, H=H, Tq=Tq, Tk=Tk, hd=hd, Tqp=Tqp, scale=scale, ldo=d, sob=Tq * d, klen=kd, causal=causal,
                  dropout_p=dropout_p, dropout_seed=dropout_seed, **lds, **offs)
    ops.attn_fwd(Qd, Kd, Vd, O, lse, **common)
    torch.cuda.synchronize()
    assert (O.float().cpu() - o_ref).abs().max() < 2e-2
    lse_ref = torch.logsumexp(s.detach(), -1)
    assert (lse[:, :, :Tq].cpu() - lse_ref).abs().max() < 2e-2
    ops.attn_bwd(Qd, Kd, Vd, O, lse, dO.to(DEV).contiguous(), Dq, dQd, dKd, dVd, lddo=d, sdob=Tq * d, **dlds, **doffs,
                 **common)
    torch.cuda.synchronize()

    def unheads(x, T):
        return x.transpose(1, 2).reshape(B, T, d)

    if fused:
        dq, dk, dv = dbuf[..., :d], dbuf[..., d:2 * d], dbuf[..., 2 * d:]
    else:
        dq, dk, dv = dQd, dKd, dVd
    for got, want, T in ((dq, qr.grad, Tq), (dk, kr.grad, Tk), (dv, vr.grad, Tk)):
        want = unheads(want, T)
        err = (got.float().cpu() - want).abs().max().item()
        assert err < 3e-2 * max(1.0, want.abs().max().item()), (err, want.abs().max().item())


@pytest.mark.parametrize("M,N,K", [(8, 1024, 1024), (3, 1000, 4096), (16, 51865, 384), (1, 72, 40), (32, 1024, 1024), (17, 520, 264),
                                   (29, 51865, 128), (64, 1024, 1024), (48, 520, 264), (128, 1024, 1280), (100, 4096, 1024),
                                   (64, 51865, 128), (33, 72, 40)])
def test_skinny_gemm_matches_torch(ops, M, N, K):
    """M <= 32 (one decoded token per clip; 17..32 rows take a second row block against the same weight fragment) takes
    the weight-streaming kernel, and so do 33 .. 128 rows (round 5: four / eight row blocks - evaluation batches of 64 and
    128 clips): bias, GELU (second output),
    residual, fp32 output with a padded leading dimension (the LM head)."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    A = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g).to(torch.bfloat16)
    ref = A.float() @ W.float().t() + bias
    Ad, Wd, bd, Rd = A.to(DEV), W.to(DEV), bias.to(DEV), R.to(DEV)
    Np = (N + 7) // 8 * 8
    out32 = torch.zeros(M, Np, dtype=torch.float32, device=DEV)
    ops.gemm(Ad, Wd, out32, M=M, N=N, K=K, lda=K, ldb=K, ldc=Np, bias=bd)
    assert (out32[:, :N].cpu() - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max()))
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(Ad, Wd, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bd, epilogue=ops.EPI_RESIDUAL, R=Rd, ldr=N)
    want = ref + R.float()
    assert (out.float().cpu() - want).abs().max() <= 2e-2 * max(1.0, float(want.abs().max()))
    g2 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(Ad, Wd, None, C2=g2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bd, epilogue=ops.EPI_GELU)
    want = torch.nn.functional.gelu(ref)
    assert (g2.float().cpu() - want).abs().max() <= 2e-2 * max(1.0, float(want.abs().max()))
    if M > 32:
        # how the rows are dealt to workgroups (32-row blocks, or 16-row blocks where the launch would leave CUs idle)
        # never changes a value: the first 32 rows on their own (one workgroup per column block) give the same bits
        part = torch.zeros(32, N, dtype=torch.bfloat16, device=DEV)
        ops.gemm(Ad[:32].contiguous(), Wd, part, M=32, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bd, epilogue=ops.EPI_RESIDUAL,
                 R=Rd[:32].contiguous(), ldr=N)
        assert torch.equal(part, out[:32])


def test_weight_gradient_with_fused_bias_gradient_and_grouped_launch(ops):
    """ops.wgrad_gemm_group: grouped / solo launches of the 256x256 kernel with the bias gradients taken from the
    kernel's A stream as partial column sums (CaGemmDesc.a_colsum), and the unfused fallback, against torch."""
    g = torch.Generator().manual_seed(21)
    K = 1000
    for specs, expect_fused in ([(5760, 1920), (1920, 1920), (1920, 7680), (7680, 1920)], True), \
                               ([(2304, 768), (768, 768), (768, 3072), (3072, 768)], False):
        dYs = [(torch.randn(K, m, generator=g) * 0.5).to(torch.bfloat16) for m, _ in specs]
        Xs = [(torch.randn(K, n, generator=g) * 0.5).to(torch.bfloat16) for _, n in specs]
        offs = np.concatenate([[0], np.cumsum([m * n for m, n in specs])]).tolist()
        nb = sum(m for m, _ in specs)
        cs_offs = np.concatenate([[0], np.cumsum([m for m, _ in specs])]).tolist()
        G = torch.full((offs[-1] + nb,), 0.25, dtype=torch.float32, device=DEV)
        ws = torch.zeros(ops.COLSUM_PARTS * nb, dtype=torch.float32, device=DEV)
        part = torch.zeros(max(ops.colsum_partial_floats(K, 7680), 4096), dtype=torch.float32, device=DEV)
        probs = [dict(dY=dYs[i].to(DEV), X=Xs[i].to(DEV), M=specs[i][0], N=specs[i][1], K=K, lda=specs[i][0],
                      ldb=specs[i][1], c_off=offs[i], accumulate=True, bias_off=offs[-1] + cs_offs[i], part=part,
                      cs_off=cs_offs[i]) for i in range(4)]
        fused = ops.wgrad_gemm_group(probs, G, colsum_ws=ws, colsum_ld=nb)
        assert fused == (expect_fused and ops.FUSE_BIAS_GRAD)  # (CA_FUSE_BIAS=0 takes the unfused route everywhere)
        if fused:
            ops.reduce_rows(ws, ops.COLSUM_PARTS, nb, nb, G[offs[-1]:], accumulate=True)
        torch.cuda.synchronize()
        Gc = G.cpu()
        for i, (m, n) in enumerate(specs):
            want = dYs[i].float().t() @ Xs[i].float() + 0.25
            got = Gc[offs[i]:offs[i] + m * n].view(m, n)
            assert (got - want).abs().max() <= 2e-3 * float(want.abs().max()), i
            wb = dYs[i].float().sum(0) + 0.25
            gb = Gc[offs[-1] + cs_offs[i]:offs[-1] + cs_offs[i] + m]
            assert (gb - wb).abs().max() <= 2e-3 * max(1.0, float(wb.abs().max())), ("bias", i, fused)


@pytest.mark.parametrize("M,N,K", [(8, 1024, 1024), (5, 1000, 1280), (16, 264, 384), (32, 1024, 512), (21, 264, 384),
                                   (64, 1024, 512), (100, 264, 384), (128, 1024, 1024)])
def test_gemm_skinny_row_index(ops, M, N, K):
    """CaGemmDesc.c_row_index (one decoded token per clip): the output rows land at device-side positions of a
    [M, L, N] cache, bit-identical to the plain GEMM's rows; the tiled kernels refuse the option."""
    x = bf(rnd(M, K, seed=21, scale=0.5)).to(DEV)
    W = bf(rnd(N, K, seed=22, scale=0.1)).to(DEV)
    bias = rnd(N, seed=25).to(DEV)
    Np = (N + 7) // 8 * 8
    ref = torch.zeros(M, Np, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x, W, ref, M=M, N=N, K=K, lda=K, ldb=K, ldc=Np, bias=bias)
    want = x.float() @ W.float().t() + bias
    assert (ref[:, :N].float() - want).abs().max().item() <= 2e-2 * max(1.0, want.abs().max().item())
    L = 7
    pos = torch.tensor([(3 * m + 1) % L for m in range(M)], dtype=torch.int32, device=DEV)
    cache = torch.zeros(M, L, Np, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x, W, cache, M=M, N=N, K=K, lda=K, ldb=K, ldc=Np, bias=bias, c_row_index=pos, c_row_mul=L)
    torch.cuda.synchronize()
    want_cache = torch.zeros_like(cache)
    want_cache[torch.arange(M, device=DEV), pos.long()] = ref
    assert torch.equal(cache, want_cache)
    with pytest.raises(Exception):
        big = torch.zeros(160 * L, Np, dtype=torch.bfloat16, device=DEV)
        ops.gemm(torch.zeros(160, K, dtype=torch.bfloat16, device=DEV), W, big, M=160, N=N, K=K, lda=K, ldb=K, ldc=Np,
                 c_row_index=torch.zeros(160, dtype=torch.int32, device=DEV), c_row_mul=L)


def test_frame_lengths(ops):
    """ca_frame_lengths against `_get_feat_extract_output_lengths` arithmetic on ragged masks (one shorter than the
    first kernel)."""
    B, N = 5, 16000
    lens = torch.tensor([16000, 12345, 400, 7, 9999])
    mask = (torch.arange(N)[None, :] < lens[:, None]).to(torch.int32).to(DEV)
    kernels, strides = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
    out = torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.frame_lengths(mask, kernels, strides, out)
    n = lens.clone()
    for k, s in zip(kernels, strides):
        n = torch.div(n - k, s, rounding_mode="floor") + 1
    assert out.cpu().tolist() == n.tolist()


def test_gemm_random_shapes_all_kernels(ops):
    """Seeded sweep of ragged shapes (M, N not multiples of the tiles, K with and without a partial K-step) through the
    128 x 128 and the 256 x 256 kernel in all four operand forms."""
    rng = np.random.RandomState(1234)
    for _ in range(10):
        M = int(rng.randint(1, 700))
        N = int(rng.randint(1, 90)) * 8
        K = int(rng.randint(1, 60)) * 8
        al, bl = int(rng.randint(0, 2)), int(rng.randint(0, 2))
        for force in (1, 3, 5):
            ops.lib().ca_gemm_force_kernel(force)
            try:
                test_gemm_layouts(ops, al, bl, M, N, K)
            finally:
                ops.lib().ca_gemm_force_kernel(0)


@pytest.mark.parametrize("V,Vp", [(51865, 51872), (200, 200), (1003, 1008)])
def test_argmax_masked_first_maximum_and_suppression(ops, V, Vp):
    """ca_argmax_masked = np.argmax over the non-suppressed tokens (first maximum wins), on the vector path (row
    pitch multiple of 4) with planted ties across the 4-wide groups and in the scalar tail."""
    B = 8
    lg = rnd(B, Vp, seed=31)
    sup = np.zeros(V, dtype=np.uint8)
    rng = np.random.RandomState(3)
    sup[rng.choice(V, V // 50, replace=False)] = 1
    top = float(lg.max()) + 1.0
    for b in range(B):  # ties at the maximum: some suppressed, the first unsuppressed one must win
        idx = np.sort(rng.choice(V, 6, replace=False))
        lg[b, idx] = top
        sup[idx[0]] = 1 if b % 2 == 0 else sup[idx[0]]
    lg[3, V - 1] = top + 1.0  # the last valid token (scalar tail when V % 4 != 0)
    sup[V - 1] = 0
    out = torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.argmax_masked(lg.to(DEV), torch.from_numpy(sup).to(DEV), out, B, V, Vp)
    torch.cuda.synchronize()
    ref = np.where(sup[None, :] == 1, -np.inf, lg[:, :V].numpy()).argmax(-1)
    assert out.cpu().numpy().tolist() == ref.tolist()


@pytest.mark.parametrize("M", [8, 24, 64, 100])
def test_gemm_skinny_split_output(ops, M):
    """CaGemmDesc.c_split_n: columns [0, d) to one buffer in place, columns [d, 3d) to the rows of a cache at
    device-side positions - the q projection and the new K|V rows of a decoded token from one launch."""
    d, K, L = 128, 256, 5
    x = bf(rnd(M, K, seed=41, scale=0.5)).to(DEV)
    W = bf(rnd(3 * d, K, seed=42, scale=0.1)).to(DEV)
    bias = rnd(3 * d, seed=43).to(DEV)
    ref = torch.zeros(M, 3 * d, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x, W, ref, M=M, N=3 * d, K=K, lda=K, ldb=K, ldc=3 * d, bias=bias)
    pos = torch.tensor([(2 * m + 1) % L for m in range(M)], dtype=torch.int32, device=DEV)
    q = torch.zeros(M, d, dtype=torch.bfloat16, device=DEV)
    cache = torch.zeros(M, L, 2 * d, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x, W, q, M=M, N=3 * d, K=K, lda=K, ldb=K, ldc=d, bias=bias, c_split_n=d, C_hi=cache, ldc_hi=2 * d,
             c_row_index=pos, c_row_mul=L)
    torch.cuda.synchronize()
    assert torch.equal(q, ref[:, :d])
    want = torch.zeros_like(cache)
    want[torch.arange(M, device=DEV), pos.long()] = ref[:, d:]
    assert torch.equal(cache, want)


@pytest.mark.parametrize("M,N,K,force", [(7680, 1920, 512, 0), (1920, 1920, 512, 0), (296, 200, 256, 0), (520, 392, 192, 1),
                                         (520, 392, 192, 2), (1000, 1496, 320, 3), (520, 392, 192, 5)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_gemm_sum_of_squares_partials(ops, M, N, K, force, accumulate):
    """CaGemmDesc.c_sumsq: the weight-gradient form (both operands MN-major, fp32 output) leaves, per 64 x 64 block of
    the output, the sum of squares of what it stored - every kernel (S / L / X forced), ragged edges, with accumulate."""
    g = torch.Generator().manual_seed(M + N + K)
    dY = bf(torch.randn(K, M, generator=g)).to(DEV)
    X = bf(torch.randn(K, N, generator=g)).to(DEV)
    G0 = torch.randn(M * N, generator=g).to(DEV)
    G = G0.clone()
    nbm, nbn = (M + 63) // 64, (N + 63) // 64
    slots = torch.full((nbm * nbn + 8,), -1.0, device=DEV)
    ops.lib().ca_gemm_force_kernel(force)
    try:
        ops.gemm(dY, X, G, M=M, N=N, K=K, a_layout=1, lda=M, b_layout=1, ldb=N, ldc=N, out_f32=True, accumulate=accumulate,
                 c_sumsq=slots, c_sumsq_off=0)
    finally:
        ops.lib().ca_gemm_force_kernel(0)
    torch.cuda.synchronize()
    want = dY.float().t() @ X.float() + (G0.view(M, N) if accumulate else 0)
    got = G.view(M, N)
    assert (got - want).abs().max() <= 2e-3 * want.abs().max()
    sq = torch.zeros(nbm * 64, nbn * 64, dtype=torch.float64, device=DEV)
    sq[:M, :N] = got.double() ** 2
    blocks = sq.view(nbm, 64, nbn, 64).sum(dim=(1, 3)).reshape(-1)
    assert torch.all(slots[nbm * nbn:] == -1.0)  # nothing written past the last block
    rel = (slots[:nbm * nbn].double() - blocks).abs() / blocks.clamp_min(1e-30)
    assert float(rel.max()) <= 1e-5, float(rel.max())


@pytest.mark.parametrize("M,N,K,force", [(7680, 1920, 512, 0), (296, 200, 256, 0), (520, 392, 192, 1), (520, 392, 192, 2),
                                         (1000, 1496, 320, 3), (520, 392, 192, 5)])
def test_gemm_sum_of_squares_partials_of_a_bf16_output(ops, M, N, K, force):
    """c_sumsq with a bf16 output (weight-matrix gradients kept in bf16): the partials are the sums of squares of the
    ROUNDED values that were stored; the stored values are the fp32 launch's, rounded."""
    g = torch.Generator().manual_seed(M + N + K + 1)
    dY = bf(torch.randn(K, M, generator=g)).to(DEV)
    X = bf(torch.randn(K, N, generator=g)).to(DEV)
    G32 = torch.zeros(M * N, device=DEV)
    G16 = torch.zeros(M * N, dtype=torch.bfloat16, device=DEV)
    nbm, nbn = (M + 63) // 64, (N + 63) // 64
    slots = torch.full((nbm * nbn + 8,), -1.0, device=DEV)
    ops.lib().ca_gemm_force_kernel(force)
    try:
        ops.gemm(dY, X, G32, M=M, N=N, K=K, a_layout=1, lda=M, b_layout=1, ldb=N, ldc=N, out_f32=True)
        ops.gemm(dY, X, G16, M=M, N=N, K=K, a_layout=1, lda=M, b_layout=1, ldb=N, ldc=N, out_f32=False, stream_out=True,
                 c_sumsq=slots, c_sumsq_off=0)
    finally:
        ops.lib().ca_gemm_force_kernel(0)
    torch.cuda.synchronize()
    assert torch.equal(G16, G32.to(torch.bfloat16))
    sq = torch.zeros(nbm * 64, nbn * 64, dtype=torch.float64, device=DEV)
    sq[:M, :N] = G16.view(M, N).double() ** 2
    blocks = sq.view(nbm, 64, nbn, 64).sum(dim=(1, 3)).reshape(-1)
    assert torch.all(slots[nbm * nbn:] == -1.0)
    rel = (slots[:nbm * nbn].double() - blocks).abs() / blocks.clamp_min(1e-30)
    assert float(rel.max()) <= 1e-5, float(rel.max())


def test_sumsq_ranges_and_plain_sum(ops):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1_000_003, generator=g).to(DEV)
    chunks = torch.tensor([[0, 65536], [65536, 1234], [200000, 3], [400004, 70001], [999996, 7]], dtype=torch.int64, device=DEV)
    out = torch.full((1,), 5.0, device=DEV)
    part = torch.zeros(4096, device=DEV)
    ops.sumsq_ranges(x, chunks, 5, out, part)
    want = sum(float(x[a:a + n].double().pow(2).sum()) for a, n in chunks.tolist())
    assert abs(float(out) - want) <= 1e-5 * want
    ops.sumsq_ranges(x, chunks, 5, out, part, accumulate=True)
    assert abs(float(out) - 2 * want) <= 1e-5 * want
    ops.sum_f32(x, 1_000_003, out, part)
    assert abs(float(out) - float(x.double().sum())) <= 1e-3 * float(x.double().abs().sum()) ** 0.5 + 1e-2
    ops.sum_f32(x[:10], 10, out, part, accumulate=True)
    assert abs(float(out) - float(x.double().sum()) - float(x[:10].double().sum())) <= 0.1


@pytest.mark.parametrize("force", [1, 2, 3, 5])
def test_gemm_interior_tile_epilogue_is_bit_identical_to_the_general_walk(ops, force):
    """Interior 64 x 64 wave tiles take a specialised, predicate-free epilogue (gemm_common.h, gemm_epilogue_fast); ragged
    ones the general walk.  Same arithmetic in the same order: with the specialised form switched off
    (ca_gemm_debug_general_epilogue) every output bit is the same - plain bf16 / bias, bias + GELU + dropout with both
    outputs, residual (+ dropout), GELU'(R) + dropout, fp32 output written and accumulated with the per-tile sums of
    squares - on each of the four kernels, at a shape with interior and ragged tiles in both dimensions."""
    lib = ops.lib()
    M, N, K = 840, 712, 200
    g = torch.Generator(device=DEV).manual_seed(5)
    A = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    B = torch.randn(N, K, device=DEV, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=g)
    R = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
    cases = {
        "plain": dict(),
        "bias": dict(bias=bias),
        "gelu2": dict(bias=bias, epilogue=ops.EPI_GELU, two=True),
        "gelu2_drop": dict(bias=bias, epilogue=ops.EPI_GELU, two=True, dropout_p=0.1, dropout_seed=11),
        "residual": dict(bias=bias, epilogue=ops.EPI_RESIDUAL, R=R, ldr=N),
        "residual_drop": dict(bias=bias, epilogue=ops.EPI_RESIDUAL, R=R, ldr=N, dropout_p=0.2, dropout_seed=3),
        "dgelu_drop": dict(epilogue=ops.EPI_DGELU, R=R, ldr=N, dropout_p=0.1, dropout_seed=11),
        "f32": dict(f32=True),
        "f32_acc": dict(f32=True, accumulate=True),
    }

    def run(case):
        c = dict(cases[case])
        two, f32 = c.pop("two", False), c.pop("f32", False)
        out = torch.full((M, N), 0.5, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
        out2 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        slots = torch.zeros(ops.sumsq_slots(M, N), dtype=torch.float32, device=DEV)
        extra = dict(C2=out2, c2_off=0) if two else {}
        if f32:
            extra.update(c_sumsq=slots, c_sumsq_off=0)
        ops.gemm(A, B, out, **kw, **c, **extra)
        torch.cuda.synchronize()
        return out.clone(), out2.clone(), slots.clone()

    lib.ca_gemm_force_kernel(force)
    try:
        for case in cases:
            lib.ca_gemm_debug_general_epilogue(1)
            want = run(case)
            lib.ca_gemm_debug_general_epilogue(0)
            got = run(case)
            for a, b in zip(got, want):
                assert torch.equal(a, b), (force, case)
            assert float(got[0].float().abs().sum()) > 0
    finally:
        lib.ca_gemm_debug_general_epilogue(0)
        lib.ca_gemm_force_kernel(0)


@pytest.mark.parametrize("force", [1, 3])
def test_gemm_fp8_interior_tile_epilogue_is_bit_identical_to_the_general_walk(ops, force):
    """The same for the fp8 kernels (128 x 128 and 256 x 256, forced), whose file has its own copy of the switch
    ca_gemm_debug_general_epilogue sets: plain and bias + GELU with both outputs, at a shape with interior and ragged
    wave tiles for both tile sizes.  (Random e4m3 bytes below 2 in magnitude, unit scales.)"""
    lib = ops.lib()
    M, N, K = 300, 264, 256
    g = torch.Generator(device=DEV).manual_seed(6)
    sign = torch.randint(0, 2, (M + N, K), device=DEV, generator=g) * 0x80
    AB = (torch.randint(0, 0x40, (M + N, K), device=DEV, generator=g) + sign).to(torch.uint8)
    A8, B8 = AB[:M], AB[M:]
    bias = torch.randn(N, device=DEV, generator=g)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=1.0 / 16)

    def run(gelu):
        out = torch.full((M, N), 0.5, dtype=torch.bfloat16, device=DEV)
        out2 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        extra = dict(bias=bias, epilogue=ops.EPI_GELU, C2=out2, c2_off=0) if gelu else {}
        ops.gemm_fp8(A8, B8, out, **kw, **extra)
        torch.cuda.synchronize()
        return out.clone(), out2.clone()

    lib.ca_gemm_force_kernel(force)
    try:
        for gelu in (False, True):
            lib.ca_gemm_debug_general_epilogue(1)
            want = run(gelu)
            lib.ca_gemm_debug_general_epilogue(0)
            got = run(gelu)
            for a, b in zip(got, want):
                assert torch.equal(a, b), (force, gelu)
            assert float(got[0].float().abs().sum()) > 0 and not bool(torch.isnan(got[0].float()).any())
    finally:
        lib.ca_gemm_debug_general_epilogue(0)
        lib.ca_gemm_force_kernel(0)


def test_grouped_second_stage_reductions_are_bit_identical(ops):
    """ca_reduce_rows_multi: a layer's second-stage reductions (different partial counts, strides, widths, accumulate
    or overwrite) in one launch, against ca_reduce_rows_f32 one by one: every bit."""
    g = torch.Generator(device=DEV).manual_seed(77)
    specs = [(512, 3840, 3840, True), (8, 17280, 17280, True), (500, 2048 + 64, 2048, False), (3, 40, 33, True)]
    parts = [torch.randn(np_, stride, device=DEV, generator=g) for np_, stride, _, _ in specs]
    base = [torch.randn(n, device=DEV, generator=g) for _, _, n, _ in specs]
    want = [b.clone() for b in base]
    got = [b.clone() for b in base]
    for (np_, stride, n, acc), p, o in zip(specs, parts, want):
        ops.reduce_rows(p, np_, stride, n, o, accumulate=acc)
    ops.reduce_rows_multi([(p, np_, stride, n, o, acc) for (np_, stride, n, acc), p, o in zip(specs, parts, got)])
    torch.cuda.synchronize()
    for a, b, (np_, stride, n, acc), p, b0 in zip(got, want, specs, parts, base):
        assert torch.equal(a, b)
        ref = p[:, :n].double().sum(0) + (b0.double() if acc else 0)
        assert (a.double() - ref).abs().max() <= 1e-3
    ops.reduce_rows_multi([(parts[3], 3, 40, 33, got[3], False)])
    torch.cuda.synchronize()
    assert (got[3].double() - parts[3][:, :33].double().sum(0)).abs().max() <= 1e-5


def test_side_streams_are_one_per_role_and_process(ops, monkeypatch):
    """Every engine of a process gets the SAME weight-gradient / optimiser stream (the stream -> hardware-queue assignment,
    hence the overlap, must not depend on how many engines were built before); CA_SHARED_STREAMS=0 is the A/B switch."""
    a, b = ops.side_stream("cuda:0", "wgrad"), ops.side_stream(torch.device("cuda", 0), "wgrad")
    assert a is b and a.cuda_stream != torch.cuda.default_stream().cuda_stream
    assert ops.side_stream("cuda:0", "optimizer") is not a
    assert ops.side_stream("cuda:0", "wgrad", -1) is not a
    monkeypatch.setenv("CA_SHARED_STREAMS", "0")
    assert ops.side_stream("cuda:0", "wgrad") is not a


@pytest.mark.parametrize("M,N,K", [(8, 3072, 1024), (16, 4096, 1024), (1, 72, 40), (5, 1000, 384), (24, 1280, 1280), (32, 5120, 1280),
                                   (16, 136, 2048), (64, 3072, 1024), (100, 1280, 1280), (128, 4096, 1024), (64, 1024, 1024),
                                   (48, 1280, 1280)])
def test_skinny_gemm_with_layernorm_prologue_is_bit_identical_to_two_launches(ops, M, N, K):
    """CaGemmDesc.a_ln_gamma: LayerNorm(A rows) inside the weight-streaming kernel's prologue = ca_layernorm_fwd followed by
    the same GEMM, bit for bit (plain, GELU second output, the q | K|V split with device-side row positions); rows of A
    may be further apart than K (lda)."""
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    lda = K + 16
    A = (torch.randn(M, lda, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    bias, gamma, beta = torch.randn(N, generator=g).to(DEV), (torch.rand(K, generator=g) + 0.5).to(DEV), torch.randn(K, generator=g).to(DEV)
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    Ac = A[:, :K].contiguous()
    ops.layernorm_fwd(Ac, gamma, beta, x, None, M, K, 1e-5)
    ref = torch.nn.functional.layer_norm(Ac.float(), (K,), gamma, beta, 1e-5)
    assert (x.float() - ref).abs().max() <= 2e-2 * max(1.0, float(ref.abs().max()))
    ln = (gamma, beta, 1e-5)
    for kw in (dict(), dict(epilogue=ops.EPI_GELU)):
        outs = []
        for fused in (False, True):
            c = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            dst = dict(Cout=None, C2=c) if kw else dict(Cout=c)
            ops.gemm(A if fused else x, W, dst.pop("Cout"), M=M, N=N, K=K, lda=lda if fused else K, ldb=K, ldc=N, bias=bias,
                     a_ln=ln if fused else None, **dst, **kw)
            outs.append(c)
        assert torch.equal(outs[0], outs[1]) and float(outs[0].float().abs().max()) > 0
    if N % 48 == 0:  # q | K|V: columns [N/3, N) go to a cache row picked on the device
        d3, Lmax = N // 3, 7
        pos = torch.arange(M, dtype=torch.int32, device=DEV) % Lmax
        outs = []
        for fused in (False, True):
            q = torch.zeros(M, d3, dtype=torch.bfloat16, device=DEV)
            kv = torch.zeros(M * Lmax, 2 * d3, dtype=torch.bfloat16, device=DEV)
            ops.gemm(A if fused else x, W, q, M=M, N=N, K=K, lda=lda if fused else K, ldb=K, ldc=d3, bias=bias, c_split_n=d3,
                     C_hi=kv, ldc_hi=2 * d3, c_row_index=pos, c_row_mul=Lmax, a_ln=ln if fused else None)
            outs.append((q, kv))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    if M == 16:  # the prologue exists in the skinny form only (up to 128 rows)
        big = torch.zeros(160, N, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(Exception, match="skinny form only"):
            ops.gemm(torch.zeros(160, K, dtype=torch.bfloat16, device=DEV), W, big, M=160, N=N, K=K, lda=K, ldb=K, ldc=N, a_ln=ln)


@pytest.mark.parametrize("M,N,K,al,bl,kind", [(3992, 7680, 1920, 0, 0, "gelu"), (3992, 1920, 1920, 0, 0, "res"),
                                              (3992, 1920, 5760, 0, 1, "plain"), (7680, 1920, 3992, 1, 1, "wgrad"),
                                              (2000, 5760, 1024, 0, 0, "bias")])
def test_gemm_results_do_not_depend_on_the_compute_cu_setting(ops, M, N, K, al, bl, kind):
    """ca_gemm_set_compute_cus (round 5: the chip shared with a resident collective): every tile of a persistent launch
    through the counter, launches sized to n CUs, every XCD given the same number of tiles, the tile shape chosen by
    counting rounds on n CUs - none of it may change a bit of the result (the per-tile sums of squares included, where the
    tile shape stays the same), also with idle workgroups (ca_debug_cu_hog) holding CUs meanwhile."""
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    A = (A.t().contiguous() if al else A).to(DEV)
    B = (B.t().contiguous() if bl else B).to(DEV)
    kw = dict(M=M, N=N, K=K, a_layout=al, b_layout=bl, lda=(M if al else K), ldb=(N if bl else K), ldc=N)
    bias = torch.randn(N, generator=g).to(DEV)
    R = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    lib = ops.lib()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    side = torch.cuda.Stream()

    def run():
        if kind == "wgrad":
            G = torch.zeros(M * N, dtype=torch.float32, device=DEV)
            ops.gemm(A, B, G, out_f32=True, accumulate=False, **kw)
            return (G,)
        C1 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        if kind == "plain":
            ops.gemm(A, B, C1, **kw)
        elif kind == "bias":
            ops.gemm(A, B, C1, bias=bias, **kw)
        elif kind == "res":
            ops.gemm(A, B, C1, bias=bias, R=R, ldr=N, epilogue=ops.EPI_RESIDUAL, **kw)
        else:
            C2 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            ops.gemm(A, B, C1, bias=bias, C2=C2, c2_off=0, epilogue=ops.EPI_GELU, dropout_p=0.1, dropout_seed=11, **kw)
            return C1, C2
        return (C1,)

    try:
        lib.ca_gemm_set_compute_cus(0)
        want = run()
        torch.cuda.synchronize()
        for cus, hog in ((ncu, 0), (ncu - 32, 0), (ncu - 16, 16), (ncu, 32)):
            lib.ca_gemm_set_compute_cus(cus)
            if hog:
                with torch.cuda.stream(side):
                    ops.check(lib.ca_debug_cu_hog(hog, 256, 96 * 1024, 20.0, side.cuda_stream), "ca_debug_cu_hog")
            got = run()
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a, b), (cus, hog)
    finally:
        lib.ca_gemm_set_compute_cus(0)
        torch.cuda.synchronize()


def _plan_rows_one_per_kernel():
    """From tests/golden/gemm_plan.json: for every kernel family, and for every skinny variant (row blocks, LayerNorm
    prologue or not, k-steps in flight, columns per workgroup), the smallest plain ca_gemm_bf16 problem that the
    automatic choice - default knobs, the whole 256-CU chip - sends there.  The 256x256 row is the smallest product
    M N (at K = 512, weight-gradient form) its fill rule accepts."""
    import json
    from pathlib import Path

    t = json.loads((Path(__file__).parent / "golden" / "gemm_plan.json").read_text())
    c = {k: i for i, k in enumerate(t["columns"])}
    default = dict(x_persist=1, skinny_mb1=4, skinny_mb1_rows=16, skinny_nt=0, skinny_u=0, prefer_l=3, l_over_x=0, l_min=100,
                   m_max=256, force_kernel=0, compute_cus=0, device_cus=256, api=0, batch1=1, batch2=1)
    plain = ("a_kseg", "b_kseg", "epilogue", "dropout", "a_colsum", "c_row_index", "c_split_n", "C8", "c_sumsq", "error")
    best = {}
    for r in t["rows"]:
        if any(r[c[k]] != v for k, v in default.items()) or any(r[c[k]] for k in plain):
            continue
        key = (r[c["family"]], r[c["mb"]], min(r[c["nch"]], 1), r[c["u"]], r[c["nt"]])
        if key not in best or r[c["M"]] * r[c["N"]] * r[c["K"]] < best[key]["M"] * best[key]["N"] * best[key]["K"]:
            best[key] = {k: r[i] for k, i in c.items()}
    assert {k[0] for k in best} == {0, 1, 2, 3, 4} and 10 <= len(best) <= 16, sorted(best)
    return [best[k] for k in sorted(best)]


@pytest.mark.parametrize("row", _plan_rows_one_per_kernel(),
                         ids=lambda r: "fam{family}_mb{mb}_nch{nch}_u{u}_nt{nt}".format(**r))
def test_gemm_automatic_choice_fires_the_planned_kernel(ops, row):
    """One launch per kernel family and skinny variant with automatic choice: the profiler's variant index that fired is
    the table's (kind * 8 + segmented * 4 + layout), and the result is torch.matmul's within test_gemm_layouts' bound
    (tiled kernels) / test_skinny_gemm_matches_torch's bound (skinny form; with the LayerNorm prologue the reference
    operand is ca_layernorm_fwd's output, which the prologue reproduces bit for bit)."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the table's default rows are for a 256-CU device"
    M, N, K, al, bl = row["M"], row["N"], row["K"], row["a_layout"], row["b_layout"]
    skinny = row["family"] == 0
    g = torch.Generator(device=DEV).manual_seed(M * 1000 + N)
    Mp, Np, Kp = (M + 7) // 8 * 8, (N + 7) // 8 * 8, (K + 7) // 8 * 8
    A = torch.zeros(Mp, Kp, dtype=torch.bfloat16, device=DEV)  # (zero padding: rows / k beyond the problem are readable)
    B = torch.zeros(Np, Kp, dtype=torch.bfloat16, device=DEV)
    A[:M, :K] = bf(torch.randn(M, K, generator=g, device=DEV) * 0.5)
    B[:N, :K] = bf(torch.randn(N, K, generator=g, device=DEV) * (0.05 if skinny else 0.5))
    Ad = A.t().contiguous() if al else A
    Bd = B.t().contiguous() if bl else B
    kw = {}
    Aref = A[:M, :K]
    if row["a_ln"]:
        gamma, beta = torch.rand(K, generator=g, device=DEV) + 0.5, torch.randn(K, generator=g, device=DEV)
        Aref = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        ops.layernorm_fwd(A[:M, :K].contiguous(), gamma, beta, Aref, None, M, K, 1e-5)
        kw["a_ln"] = (gamma, beta, 1e-5)
    ref = torch.matmul(Aref.float(), B[:N, :K].float().t())
    C = torch.zeros(M, Np, dtype=torch.float32, device=DEV)
    ops.prof_begin()
    try:
        ops.gemm(Ad, Bd, C, M=M, N=N, K=K, lda=(Mp if al else Kp), ldb=(Np if bl else Kp), ldc=Np, a_layout=al, b_layout=bl, **kw)
    finally:
        fired = [i for i, p in enumerate(ops.prof_end()) if p["count"]]
    assert fired == [row["kind"] * 8 + row["ks"] * 4 + row["lay"]], (fired, row)
    err = (C[:, :N] - ref).abs().max().item()
    bound = 2e-3 * max(1.0, float(ref.abs().max())) if skinny else 1e-3 * (K ** 0.5)
    print(f"plan row M {M} N {N} K {K} family {row['family']}: variant {fired}, max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


_ATTN_INST = ("kernel", "hdpv", "drop", "wpe", "dt", "qp", "ks")


def _attn_plan_rows_one_per_instantiation():
    """From tests/golden/attn_plan.json: for every attention instantiation that default knobs on the whole 256-CU chip
    reach (kernel, head-dim image, dropout, workgroups per CU; the single-query kernel's ring depth, query projection
    and key_slot table), the smallest problem (B H Tq Tk) that the rule sends there - without packed rows, O8 or a split
    workspace, which no instantiation depends on; two clips and at least 40 queries for the tiled kernels."""
    import json
    from pathlib import Path

    t = json.loads((Path(__file__).parent / "golden" / "attn_plan.json").read_text())
    c = {k: i for i, k in enumerate(t["columns"])}
    default = dict(wide=1, wpe3=1, dq_wpe3=1, dkv_wide=1, dkv_wpe3=0, smallq_2percu=-1, split=4, split_tail=1, device_cus=256,
                   row_off=0, O8=0, ws=0, error=0)
    best = {}
    for r in t["rows"]:
        if any(r[c[k]] != v for k, v in default.items()):
            continue
        row = {k: r[i] for k, i in c.items()}
        if row["kernel0"] != 3 and (row["B"] != 2 or row["Tq"] < 40):  # (the table also holds one-element problems)
            continue
        size = row["B"] * row["H"] * row["Tq"] * row["Tk"]
        for slot in range(3):
            inst = tuple(row[f"{k}{slot}"] for k in _ATTN_INST)
            if inst[0] and (inst not in best or size < best[inst][0]):
                best[inst] = (size, dict(row, inst=inst))
    # 4 + 4 forward, 6 single-query, prep, 4 + 2 dK|dV, 4 + 4 dQ (the two- / three-per-CU twins behind knobs are not default)
    assert len(best) == 29 and {k[0] for k in best} == set(range(1, 9)), sorted(best)
    return [best[k][1] for k in sorted(best)]


@pytest.mark.parametrize("row", _attn_plan_rows_one_per_instantiation(),
                         ids=lambda r: "k{}_hdpv{}_drop{}_wpe{}_dt{}_qp{}_ks{}".format(*r["inst"]))
def test_attention_every_planned_instantiation_computes_attention(ops, row):
    """One launch per attention instantiation at the smallest shape of the plan table that reaches it.  Forward,
    dQ and dK|dV kernels: ca_attn_fwd + ca_attn_bwd at that shape against the fp32 torch statement with
    test_fused_attention_fwd_bwd's bounds, dropout through the restated keep mask.  Single-query kernels: against fp32
    torch as test_decode_attention_with_the_keys_dealt_to_several_workgroups does (2e-2), the key_slot form with the
    keys gathered by the table, the query-projection form bit-identical to LayerNorm + GEMM + ca_attn_fwd."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the table's default rows are for a 256-CU device"
    B, H, Tq, Tk, hd = (row[k] for k in ("B", "H", "Tq", "Tk", "hd"))
    if row["inst"][0] != 3:
        _check_attention_fwd_bwd(ops, B, hd, H, Tq, Tk, bool(row["causal"]), bool(row["klen"]),
                                 dropout_p=0.1 if row["drop"] else 0.0, dropout_seed=0x1234567 + Tq)
        return
    d = H * hd
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + Tk)
    kv = torch.randn(B, Tk, 2 * d, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(B, Tq, d, device=DEV, generator=g).to(torch.bfloat16)
    kl = torch.tensor(([Tk, max(1, Tk - 37), 1, Tk // 2] * B)[:B], dtype=torch.int32, device=DEV) if row["klen"] else None
    slot = torch.randint(0, B, (B, Tk), device=DEV, generator=g).to(torch.int32) if row["key_slot"] else None
    akw = dict(B=B, H=H, Tk=Tk, hd=hd, scale=hd ** -0.5, ldk=2 * d, ldv=2 * d, ldo=d, skb=Tk * 2 * d, svb=Tk * 2 * d, k_off=0,
               v_off=d, klen=kl)
    Tqp = 32
    lse = torch.zeros(B * H * Tqp, device=DEV)
    if row["api"] == 1:  # ca_decode_attn_qproj: the query is LayerNorm(x) Wq^T + bq
        x = torch.randn(B, d, device=DEV, generator=g).to(torch.bfloat16)
        gamma, beta = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g), 0.1 * torch.randn(d, device=DEV, generator=g)
        W = (0.05 * torch.randn(d, d, device=DEV, generator=g)).to(torch.bfloat16)
        bias = 0.1 * torch.randn(d, device=DEV, generator=g)
        xn, q = torch.empty_like(x), torch.empty_like(x)
        ops.layernorm_fwd(x, gamma, beta, xn, None, B, d, 1e-5)
        ops.gemm(xn, W, q, M=B, N=d, K=d, lda=d, ldb=d, ldc=d, bias=bias)
        q = q.view(B, 1, d)
    got = torch.zeros(B, Tq, d, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd(q, kv, kv, got, lse, Tq=Tq, Tqp=Tqp, ldq=d, sqb=Tq * d, sob=Tq * d, key_slot=slot, **akw)
    if row["api"] == 1:
        fused = torch.ones(B, Tq, d, dtype=torch.bfloat16, device=DEV)
        ops.decode_attn_qproj(x, gamma, beta, W, bias, kv, kv, fused, d_model=d, eps=1e-5, ldx=d, ldw=d, sob=d, **akw)
        torch.cuda.synchronize()
        assert torch.equal(fused, got)
    kve = kv if slot is None else kv[slot.long(), torch.arange(Tk, device=DEV)[None, :]]  # key t of clip b from row slot[b, t]
    K, V = kve[..., :d].float().view(B, Tk, H, hd).transpose(1, 2), kve[..., d:].float().view(B, Tk, H, hd).transpose(1, 2)
    sc = (q.float().view(B, Tq, H, hd).transpose(1, 2) @ K.transpose(-1, -2)) * hd ** -0.5
    if kl is not None:
        sc = sc.masked_fill(torch.arange(Tk, device=DEV)[None, None, None, :] >= kl[:, None, None, None], float("-inf"))
    ref = (torch.softmax(sc, -1) @ V).transpose(1, 2).reshape(B, Tq, d)
    err = float((got.float() - ref).abs().max())
    print(f"single-query instantiation {row['inst']} B {B} H {H} Tq {Tq} Tk {Tk} hd {hd}: max |err| {err:.3e}")
    assert torch.isfinite(got.float()).all() and float(got.float().abs().sum()) > 0 and err < 2e-2
