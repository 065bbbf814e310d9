"""tests/norm_ref.py checked without a GPU: the float64 references against autograd, the derived bounds against an fp32
emulation of the kernels' own arithmetic (they must admit it with room to spare), and against the wrong implementations
they exist to reject (they must not admit those)."""
import pytest
import torch

import norm_ref as R

EPS = 1e-5
SMALL_C = (8, 264, 512, 520, 1024, 1032)
EMU_C = (8, 264, 520, 1032, 1544, 2056)
GAMMAS = ("plain", "e")


# ---- fp32 emulation of csrc/norm.hip -------------------------------------------------------------------------------
def emu_row_sum(v):
    """Row sums of fp32 [rows, C] in the kernel's order: lane l holds chunks l, l + 64, ... of 8 elements and adds them
    one by one, then a 6-step xor butterfly over the 64 lanes.  (Chunks past the row are zeros and add nothing.)"""
    rows, C = v.shape
    nch = R.nch_of(C)
    pad = torch.zeros(rows, nch * 512, dtype=torch.float32)
    pad[:, :C] = v
    pad = pad.view(rows, nch, 64, 8)
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for c in range(nch):
        for e in range(8):
            s = s + pad[:, c, :, e]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def _half_erfc(x):
    """ca_half_erfc in fp32 (torch has no fma: each fused step rounds twice here, once on the GPU)."""
    ax = x.abs().clamp(max=14.0)
    w = ax * 0.84932180028801904272
    e = torch.exp2(-w * w)
    t = 1.0 / (ax * 0.23164189 + 1.0)
    poly = t * (0.5 * 1.061405429) + (0.5 * -1.453152027)
    poly = t * poly + 0.5 * 1.421413741
    poly = t * poly + 0.5 * -0.284496736
    poly = t * poly + 0.5 * 0.254829592
    return t * poly * e, e, ax


def emu_gelu(x):
    he, _, ax = _half_erfc(x)
    return -ax * he + x.clamp(min=0.0)


def emu_dgelu(x):
    he, e, ax = _half_erfc(x)
    cdf = torch.where(x >= 0, 1.0 - he, he)
    return torch.copysign(ax, x) * 0.39894228040143267794 * e + cdf


def emu_fwd(x, gamma, beta, act, one_pass=False):
    """(y fp32 before any output rounding, mean, rstd) the way ln_fwd_kernel computes them; one_pass: the variance as
    E[x^2] - mean^2 instead (the wrong implementation)."""
    v = x.float()
    C = v.shape[1]
    mean = emu_row_sum(v) / C
    if one_pass:
        var = emu_row_sum(v * v) / C - mean * mean
    else:
        dlt = v - mean[:, None]
        var = emu_row_sum(dlt * dlt) / C
    rstd = torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32))
    y = (v - mean[:, None]) * rstd[:, None] * gamma + beta
    return (emu_gelu(y) if act else y), mean, rstd


def emu_reduce(partial, out, accumulate):
    """reduce_partials_kernel on [nparts, n] fp32: 16 partial lanes, four accumulators in the unrolled loop."""
    nparts, n = partial.shape
    z = torch.zeros(n, dtype=torch.float32)
    red = []
    for pl in range(16):
        a, p = [z, z, z, z], pl
        while p + 48 < nparts:
            a = [a[k] + partial[p + 16 * k] for k in range(4)]
            p += 64
        while p < nparts:
            a[0] = a[0] + partial[p]
            p += 16
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    t = z
    for q in range(16):
        t = t + red[q]
    return out + t if accumulate else t


def emu_bwd(dy, x, gamma, beta, mean, rstd, dres, act, grid, init, drop_hm2=False, stale_mean=False):
    """(dx fp32 before its rounding to bf16, dgamma, dbeta) the way ln_bwd_kernel + reduce_partials_kernel compute them with `grid` blocks.
    drop_hm2 / stale_mean: the two wrong implementations (dx without its h m2 term; the previous row's mean)."""
    rows, C = x.shape
    v, dyf, mean, rstd = x.float(), dy.float(), mean.float(), rstd.float()
    if stale_mean:
        mean = torch.roll(mean, 1)
    h = (v - mean[:, None]) * rstd[:, None]
    du = dyf * emu_dgelu(h * gamma + beta) if act else dyf
    d = du * gamma
    m1, m2 = emu_row_sum(d) / C, emu_row_sum(d * h) / C
    inner = d - m1[:, None] if drop_hm2 else d - m1[:, None] - h * m2[:, None]
    dx = rstd[:, None] * inner + (dres.float() if dres is not None else 0.0)
    slots = 4 * grid
    passes = -(-rows // slots)
    outs = []
    for term in (du * h, du):
        t = torch.zeros(passes * slots, C, dtype=torch.float32)
        t[:rows] = term
        t = t.view(passes, slots, C)
        acc = torch.zeros(slots, C, dtype=torch.float32)
        for k in range(passes):
            acc = acc + t[k]
        acc = acc.view(grid, 4, C)
        part = torch.zeros(grid, C, dtype=torch.float32)
        for w in range(4):
            part = part + acc[:, w]
        outs.append(emu_reduce(part, torch.full((C,), float(init)), True))
    return dx, outs[0], outs[1]


def ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound is inside it)."""
    err = (R.f64(got) - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def _fwd_inputs(C, fam, gam, fp32=False, rows=24):
    return R.make_x(rows, C, fam, seed=1, fp32=fp32), *R.make_affine(C, gam)


# ---- the references against autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", SMALL_C)
def test_references_agree_with_float64_autograd(C, act):
    rows = 9
    x = R.f64(R.make_x(rows, C, "mixed")).requires_grad_(True)
    gamma, beta = (R.f64(t).requires_grad_(True) for t in R.make_affine(C))
    dy, dres = R.f64(R.make_dy(rows, C)), R.f64(R.make_dy(rows, C, seed=5))
    y = torch.nn.functional.layer_norm(x, (C,), gamma, beta, EPS)
    if act:
        y = torch.nn.functional.gelu(y)
    y.backward(dy)
    yr, mean, rstd = R.ln_fwd_ref(x, gamma, beta, EPS, act)
    dx, dg, db = R.ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, act)

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    assert rel(yr, y.detach()) <= 1e-12
    assert rel(dx, x.grad + dres) <= 1e-12
    assert rel(dg, gamma.grad) <= 1e-12 and rel(db, beta.grad) <= 1e-12


# ---- the bounds admit a correct fp32 implementation ----------------------------------------------------------------
FWD_FAMILIES = ("a", "b300", "b30", "c", "d", "mixed")


@pytest.mark.parametrize("fam", FWD_FAMILIES + ("b1000",))
def test_forward_bounds_admit_the_fp32_emulation(fam):
    """Largest error / bound of the emulation over C in EMU_C, act in {0, 1}, both gamma families, for
    (y rounded to bf16 against the whole bound, y before rounding against the slack alone, mean, rstd):
        a      0.995 0.151 0.005 0.136      b300   0.946 0.037 0.055 0.152      b30    0.966 0.024 0.034 0.172
        c      0.939 0.016 0.000 0.070      d      0.995 0.176 0.029 0.187      mixed  0.995 0.151 0.033 0.138
        b1000  -     0.074 0.113 0.154  (fp32 rows, C <= 1024)
    The first figure approaches 1 by construction: it is the rounding to bf16 itself, which just above a power of two is
    the whole 2^-8 |ref| the kernel is entitled to.  It must stay <= 1.  The others measure the derivation: <= 0.25."""
    fp32 = fam == "b1000"
    worst = [0.0, 0.0, 0.0, 0.0]
    for C in EMU_C:
        if fp32 and C > 1024:
            continue
        for gam in GAMMAS:
            x, gamma, beta = _fwd_inputs(C, fam, gam, fp32)
            ms, rs = R.fwd_stats_slack(x, EPS)
            for act in (0, 1):
                yr, mean, rstd = R.ln_fwd_ref(x, gamma, beta, EPS, act)
                y, m, r = emu_fwd(x, gamma, beta, act)
                got = [0.0 if fp32 else ratio(y.bfloat16(), yr, R.fwd_y_bound(x, gamma, beta, EPS, act, True)),
                       ratio(y, yr, R.fwd_y_bound(x, gamma, beta, EPS, act, False)), ratio(m, mean, ms), ratio(r, rstd, rs)]
                worst = [max(a, b) for a, b in zip(worst, got)]
    print(fam, ["%.3f" % w for w in worst])
    assert worst[0] <= 1.0 and max(worst[1:]) <= 0.25, worst


@pytest.mark.parametrize("fam", FWD_FAMILIES)
def test_backward_bounds_admit_the_fp32_emulation(fam):
    """Largest error / bound of the emulation over C in EMU_C, act in {0, 1}, both gamma families, rows in
    {5, 8, 9, 21, 26} on a grid of 2 blocks (one to four rows per wave, ragged), dres given, for (dgamma, dbeta into
    zeroed buffers | dx rounded to bf16 against the whole bound, dx before rounding against the slack alone, dgamma,
    dbeta into buffers that held 1):
        a      0.108 0.105 | 0.996 0.278 0.171 0.124      b300   0.140 0.122 | 0.996 0.244 0.392 0.128
        b30    0.139 0.093 | 0.995 0.223 0.172 0.107      c      0.000 0.198 | 0.995 0.205 0.000 0.198
        d      0.136 0.116 | 0.996 0.877 0.316 0.117      mixed  0.155 0.125 | 0.996 0.676 0.374 0.141
    The first two are sums along chains: <= 0.25.  The other four are each dominated somewhere by ONE rounding, whose own
    worst case the bound has to grant in full, so they approach 1 with a correct implementation and must stay <= 1: the
    rounding to bf16; the fp32 addition of dres where dres is most of dx (rows with an outlier have rstd ~ 0.08, and where
    gamma = 0 nothing else is left), error u |dx| against a slack of little more; the addition into a buffer that holds 1
    of a sum much smaller than 1, error u against the 2 u granted.  No constant was raised to bring these under 0.25:
    that would loosen the bound where it is tight for a reason.  (dx has no fp32 form: on the GPU its slack is four
    orders of magnitude below the bf16 term it stands next to.)  Statistics: the float64 ones rounded to fp32, as the
    GPU test feeds them."""
    grid = 2
    worst = [0.0] * 6
    for C in EMU_C:
        for rows in (5, 8, 9, 21, 26):
            x = R.make_x(rows, C, fam)
            dy, dres = R.make_dy(rows, C), R.make_dy(rows, C, seed=5)
            for gam in GAMMAS:
                gamma, beta = R.make_affine(C, gam)
                _, mean, rstd = R.ln_fwd_ref(x, gamma, beta, EPS, 0)
                mean, rstd = mean.float(), rstd.float()
                for act in (0, 1):
                    ref = R.ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, act)
                    chain = R.bwd_chain(rows, grid)
                    b0 = R.bwd_bounds(dy, x, gamma, beta, mean, rstd, dres, act, chain)
                    b1 = R.bwd_bounds(dy, x, gamma, beta, mean, rstd, dres, act, chain, init=1.0)
                    dx, dg0, db0 = emu_bwd(dy, x, gamma, beta, mean, rstd, dres, act, grid, 0.0)
                    _, dg1, db1 = emu_bwd(dy, x, gamma, beta, mean, rstd, dres, act, grid, 1.0)
                    got = [ratio(dg0, ref[1], b0["dgamma"]), ratio(db0, ref[2], b0["dbeta"]),
                           ratio(dx.bfloat16(), ref[0], b0["dx"]), ratio(dx, ref[0], b0["dx_slack"]),
                           ratio(R.f64(dg1) - 1, ref[1], b1["dgamma"]), ratio(R.f64(db1) - 1, ref[2], b1["dbeta"])]
                    worst = [max(a, c) for a, c in zip(worst, got)]
    print(fam, ["%.3f" % w for w in worst])
    assert max(worst[:2]) <= 0.25 and max(worst[2:]) <= 1.0, worst


@pytest.mark.parametrize("nparts", [1, 15, 16, 17, 63, 64, 65, 500])
def test_reduction_bound_admits_the_fp32_emulation(nparts):
    """error / bound of reduce_partials_kernel's order of additions on N(0, 1) partials plus an accumulated output:
        nparts 1: 0.315   15: 0.148   16: 0.063   17: 0.138   63: 0.009   64: 0.011   65: 0.010   500: 0.001
    With one part the whole computation is one addition, whose worst case u |sum| is a third of the (1 + 2) u sum|term|
    granted: up to 1/3 there, <= 0.25 from 15 parts on."""
    g = torch.Generator().manual_seed(nparts)
    part, out = torch.randn(nparts, 65, generator=g), torch.randn(65, generator=g)
    got = emu_reduce(part, out, True)
    ref = R.f64(part).sum(0) + R.f64(out)
    r = ratio(got, ref, R.sum_bound(R.f64(part).abs().sum(0) + R.f64(out).abs(), nparts))
    print(nparts, "%.3f" % r)
    assert r <= (0.25 if nparts >= 15 else 0.34)


# ---- the bounds reject the implementations they are meant to catch ---------------------------------------------------
@pytest.mark.parametrize("C,fam,fp32", [(264, "b300", False), (1032, "b300", False), (264, "b300", True),
                                         (264, "b1000", True), (1024, "b1000", True)])
def test_forward_bounds_reject_a_one_pass_variance(C, fam, fp32):
    x, gamma, beta = _fwd_inputs(C, fam, "plain", fp32)
    yr, _, rstd = R.ln_fwd_ref(x, gamma, beta, EPS, 0)
    y, _, r = emu_fwd(x, gamma, beta, 0, one_pass=True)
    _, rs = R.fwd_stats_slack(x, EPS)
    assert ratio(r, rstd, rs) > 10.0
    assert ratio(y, yr, R.fwd_y_bound(x, gamma, beta, EPS, 0, False)) > 10.0


@pytest.mark.parametrize("wrong", ["drop_hm2", "stale_mean"])
@pytest.mark.parametrize("fam", ["a", "mixed"])
@pytest.mark.parametrize("act", [0, 1])
def test_dx_bound_rejects_a_wrong_backward(fam, act, wrong):
    rows, C, grid = 26, 520, 2
    x, dy = R.make_x(rows, C, fam), R.make_dy(rows, C)
    gamma, beta = R.make_affine(C)
    _, mean, rstd = R.ln_fwd_ref(x, gamma, beta, EPS, 0)
    mean, rstd = mean.float(), rstd.float()
    ref = R.ln_bwd_ref(dy, x, gamma, beta, mean, rstd, None, act)
    b = R.bwd_bounds(dy, x, gamma, beta, mean, rstd, None, act, R.bwd_chain(rows, grid))
    dx, _, _ = emu_bwd(dy, x, gamma, beta, mean, rstd, None, act, grid, 0.0, **{wrong: True})
    assert ratio(dx.bfloat16(), ref[0], b["dx"]) > 2.0


# ---- the dropout mask -------------------------------------------------------------------------------------------------
def test_dropout_mask_reference_is_a_fair_coin_per_element():
    """dropout_keep follows ca_dropout_keep4's integer arithmetic; here only what can be checked without the kernel: the
    keep rate, p = 0 keeping everything, and dependence on the seed."""
    idx = torch.arange(1 << 20)
    for p in (0.1, 0.5):
        k = R.dropout_keep(1234, idx, p).double().mean().item()
        assert abs(k - (1 - int(p * 65536) / 65536)) < 4 * (p * (1 - p) / (1 << 20)) ** 0.5
    assert bool(R.dropout_keep(7, idx, 0.0).all())
    assert not torch.equal(R.dropout_keep(1, idx, 0.5), R.dropout_keep(2, idx, 0.5))
    big = torch.tensor([(1 << 34) + 5, (1 << 34) + 6])
    assert R.dropout_keep(9, big, 0.5).dtype == torch.bool
