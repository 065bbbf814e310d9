"""Test-side float64 references of the LayerNorm (+ exact GELU) forward and backward, of the partial-sum reductions and
of the element-wise kernels in csrc/norm.hip, the error bounds a correct fp32 kernel is held to, and the seeded input
families that tests/test_norm_ref_cpu.py (no GPU) and tests/test_norm_gpu.py build identically.  Plain torch on the
CPU; nothing here imports `coral_amd`.

Notation of the derivations: u = 2^-24 is the unit roundoff of fp32 (every fp32 operation returns its exact result times
(1 + d), |d| <= u), a sum of n terms added along a chain of length k has error <= k u sum|term| (first order; the
constants below carry the few roundings around the chain), and a bf16 result is the fp32 value rounded once more to 8
significant bits: half an ulp, between 2^-9 of the value (just below a power of two) and 2^-8 of it (just above),
bounded here by 2^-8 |ref|.

Margin.  Every bound below is the worst case, all roundings pushing the same way; none of its constants is fitted to a
kernel's output.  An fp32 emulation of the kernel's own order of operations (tests/test_norm_ref_cpu.py) uses at most
a quarter of each fp32 slack, usually a few percent: rounding errors of a chain of k additions grow like sqrt(k), not
k.  (The bf16 term has no margin and needs none: half an ulp is what round-to-nearest delivers, and a kernel reaches it
just above a power of two.)  That factor of four or more on the slack is the margin, and it is why
the wrong implementations the bounds are meant to reject (a one-pass variance, a missing term of dx, another row's
mean) still miss them by orders of magnitude: they are wrong by a multiple of the VALUE, not of its rounding.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff
BF16_HALF_ULP = 2.0 ** -8
ERF_APPROX = 1.5e-7     # csrc/common.h, ca_half_erfc: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 on erf
GELU_LIP = 1.13         # max |gelu'(z)|  (1.1289 at z = sqrt 2)
DGELU_LIP = 0.80        # max |gelu''(z)| (2 pdf(0) = 0.7979 at z = 0)

C_LIST = (8, 264, 512, 520, 1024, 1032, 1280, 1536, 1544, 1920, 2048, 2056, 4096)
FAMILIES = ("a", "b300", "b30", "c", "d", "mixed")


def f64(t):
    return t.detach().to("cpu", torch.float64)


def nch_of(C: int) -> int:
    """Chunks of 8 elements per lane of the kernel instantiation that serves rows of C channels."""
    n = (C // 8 + 63) // 64
    return n if n <= 4 else 8


def depth_of(C: int) -> int:
    """Longest addition chain of a row sum: 8 elements per chunk in the lane, NCH chunks, 6 butterfly steps."""
    return 8 * nch_of(C) + 6


# ---- seeded inputs -------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_x(rows: int, C: int, family: str, seed: int = 1, fp32: bool = False) -> torch.Tensor:
    """[rows, C] input rows of one family, bf16 (or fp32 with fp32=True; then 'b1000' exists too and is not rounded).
      a      N(0, 2)
      b300   300 + N(0, 1) rounded to bf16;  b30: 30 + 0.25 N(0, 1) rounded to bf16;  b1000: 1000 + 4 N(0, 1), fp32 only
      c      constant rows (a bf16 value per row)
      d      N(0, 1) with one outlier of +-200 per row
      mixed  family a with rows of b300, b30, c, d (and b1000 in fp32) at row % 97 in 1..6, and a b300 last row
    """
    g = _gen(seed)
    n = torch.randn(rows, C, generator=g)
    if family == "a":
        x = 2.0 * n
    elif family == "b300":
        x = (300.0 + n).bfloat16().float()
    elif family == "b30":
        x = (30.0 + 0.25 * n).bfloat16().float()
    elif family == "b1000":
        assert fp32
        x = 1000.0 + 4.0 * n
    elif family == "c":
        x = (3.0 * n[:, :1]).bfloat16().float().expand(rows, C).clone()
    elif family == "d":
        x = n.clone()
        col = torch.randint(0, C, (rows,), generator=g)
        sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)
        x[torch.arange(rows), col] = 200.0 * sign
    elif family == "mixed":
        x = 2.0 * n
        idx = torch.arange(rows)
        for k, fam in enumerate(("b300", "b30", "c", "d", "d", "b1000" if fp32 else "b30"), start=1):
            sel = idx % 97 == k
            if sel.any():
                x[sel] = make_x(rows, C, fam, seed + 10 * k, fp32)[sel].float()
        x[rows - 1] = make_x(1, C, "b300", seed + 100)[0].float()
    else:
        raise ValueError(family)
    return x if fp32 else x.bfloat16()


def make_affine(C: int, family: str = "plain", seed: int = 2):
    """(gamma, beta) fp32.  'plain': 1 + 0.1 N(0, 1) and 0.1 N(0, 1).  'e': gamma with exact zeros (every 5th) and
    negative entries (every 3rd), beta = 0."""
    g = _gen(seed)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    if family == "e":
        i = torch.arange(C)
        gamma = torch.where(i % 3 == 0, -gamma, gamma)
        gamma = torch.where(i % 5 == 0, torch.zeros(()), gamma)
        beta = torch.zeros(C)
    return gamma, beta


def make_dy(rows: int, C: int, seed: int = 4) -> torch.Tensor:
    return torch.randn(rows, C, generator=_gen(seed)).bfloat16()


# ---- float64 references ------------------------------------------------------------------------------------------
def gelu64(z):
    return z * 0.5 * (1.0 + torch.special.erf(z / math.sqrt(2.0)))


def dgelu64(z):
    """gelu'(z) = Phi(z) + z pdf(z); 1 and 0 at +-inf (where z pdf(z) is 0, not inf * 0)."""
    cdf = 0.5 * (1.0 + torch.special.erf(z / math.sqrt(2.0)))
    zc = z.clamp(-40.0, 40.0)
    return cdf + zc * torch.exp(-0.5 * zc * zc) / math.sqrt(2.0 * math.pi)


def ln_fwd_ref(x, gamma, beta, eps, act):
    """(y [rows, C], mean [rows], rstd [rows]) in float64 from the exact input values."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    return (gelu64(y) if act else y), mean, rstd


def _bwd_terms(dy, x, gamma, beta, mean, rstd, act):
    dy, x, gamma = f64(dy), f64(x), f64(gamma)
    mean, rstd = f64(mean)[:, None], f64(rstd)[:, None]
    h = (x - mean) * rstd
    du = dy * dgelu64(h * gamma + f64(beta)) if act else dy
    return dy, gamma, rstd, h, du


def ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, act):
    """(dx [rows, C], dgamma [C], dbeta [C]) in float64, closed form, with mean / rstd taken as given."""
    dy, gamma, rstd, h, du = _bwd_terms(dy, x, gamma, beta, mean, rstd, act)
    d = du * gamma
    dx = rstd * (d - d.mean(1, keepdim=True) - h * (d * h).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + f64(dres)
    return dx, (du * h).sum(0), du.sum(0)


# ---- bounds: forward ---------------------------------------------------------------------------------------------
def fwd_stats_slack(x, eps):
    """(mean_slack [rows], rstd_slack [rows]) for the fp32 statistics.

    mean: the row sum runs along a chain of depth = 8 NCH + 6 additions, error <= depth u sum|x|; the division by C
    adds u |mean| <= u mean|x|:  mean_slack = (depth + 1) u mean|x|.
    rstd: the kernel's variance is mean((x - mean^)^2) with its own mean^ = mean + dm.  In exact arithmetic that is
    var + dm^2 (the cross term sums to zero), the subtraction and the square put 3 u on each term, the chain another
    depth u, the division and the + eps two more: relative (depth + 5) u on var + eps, plus dm^2 / (var + eps).  rsqrt
    halves a relative error and is itself a hardware approximation good to 1 ulp = 2 u; eps arrives as an fp32
    (relative u / 2 on its part).  rstd_slack = rstd ((depth / 2 + 6) u + mean_slack^2 rstd^2 / 2).  The second term is
    what a large offset costs a two-pass variance; it is ~1e-6 at 300 + N(0, 1), where a one-pass variance
    E[x^2] - mean^2 loses depth u 300^2 ~ 1e-2 outright."""
    x = f64(x)
    depth = depth_of(x.shape[1])
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + eps)
    ms = (depth + 1) * U * x.abs().mean(1)
    rs = rstd * ((depth / 2 + 6) * U + 0.5 * (ms * rstd) ** 2)
    return ms, rs


def fwd_y_bound(x, gamma, beta, eps, act, bf16_out):
    """Bound on |y_kernel - y_ref|, shaped like y.

    z^ = ((x - mean^) rstd^ gamma + beta) in fp32 (ln_apply): the subtraction, two products and the addition round
    once each, relative to a partial result no larger than (|x| + |mean|) rstd |gamma| + |beta|: 4 u of that.  mean^ is
    off by mean_slack, which reaches z multiplied by rstd |gamma| - the factor that makes large-offset rows the hard
    case - and rstd^ is off by rstd_slack, which reaches z multiplied by |x - mean| |gamma|:
        slack_z = 4 u ((|x| + |mean|) rstd |gamma| + |beta|) + (mean_slack rstd + |x - mean| rstd_slack) |gamma|.
    With GELU the error of z passes through gelu' (at most 1.13 in magnitude), Phi(z) carries half the 1.5e-7 of the
    erf approximation plus ~8 roundings of its polynomial, exponential and reciprocal on a value <= 1/2, both
    multiplied by |z|, and the final fma rounds once: slack = 1.13 slack_z + |z| (1.5e-7 + 8 u) + u |y| (the whole
    1.5e-7 is granted, not the half: the documented figure is for erf on its argument z / sqrt 2, margin 2).
    A bf16 output adds the rounding it is entitled to, 2^-8 |ref|."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    y, mean, rstd = ln_fwd_ref(x, gamma, beta, eps, 0)
    ms, rs = fwd_stats_slack(x, eps)
    mean, rstd, ms, rs = mean[:, None], rstd[:, None], ms[:, None], rs[:, None]
    slack = 4 * U * ((x.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs())
    slack = slack + (ms * rstd + (x - mean).abs() * rs) * gamma.abs()
    if act:
        z, y = y, gelu64(y)
        slack = GELU_LIP * slack + z.abs() * (ERF_APPROX + 8 * U) + U * y.abs()
    return slack + (BF16_HALF_ULP * y.abs() if bf16_out else 0.0)


# ---- bounds: backward --------------------------------------------------------------------------------------------
def bwd_chain(rows: int, grid: int, reduced: bool = True) -> int:
    """Longest addition chain of a d gamma / d beta element: the rows a wave walks, the 4 waves of a block, and (when
    the kernel's own second stage ran) reduce_partials_kernel: ceil(grid / 64) additions per accumulator, 3 to join the
    accumulators and the partial lanes' first, 16 across the partial lanes, 1 into the output."""
    chain = -(-rows // (4 * grid)) + 4
    return chain + (-(-grid // 64) + 3 + 16 + 1 if reduced else 0)


def bwd_bounds(dy, x, gamma, beta, mean, rstd, dres, act, chain, init=None):
    """{'dx': [rows, C], 'dx_slack': the same without the bf16 rounding, 'dx_nores': the bound on dx when the kernel is
    called without dres (its reference is then dx - dres), 'dgamma': [C], 'dbeta': [C]}: bounds on
    |kernel - ln_bwd_ref| with mean / rstd given (exact fp32 inputs of both).  `chain` is bwd_chain(...); `init` the value the d gamma / d beta buffers held before (or None).

    h^ = (x - mean) rstd rounds twice: |dh| <= 2 u |h|.
    du: without GELU du = dy exactly (e_du = 0).  With it z^ = h^ gamma + beta is off by <= 4 u (|h gamma| + |beta|),
    which passes through gelu'' (at most 0.80); gelu' itself carries the erf approximation (half of 1.5e-7 on Phi, all of
    it granted) and ~8 roundings on values <= 1; the product with dy rounds once:
        e_du = |dy| (0.8 * 4 u (|h gamma| + |beta|) + 1.5e-7 + 8 u) + u |du|.
    d = du gamma: e_d = |gamma| e_du + u |d|.
    m1 = mean(d), m2 = mean(d h^): chains of depth = 8 NCH + 6, the division, and the terms' own errors:
        e_m1 = (depth + 2) u mean|d| + mean(|gamma| e_du),  e_m2 = (depth + 5) u mean|d h| + mean(|gamma| e_du |h|).
    dx = rstd (d - m1 - h^ m2) + dres: the inputs' errors e_d + e_m1 + |h| e_m2, then a product, two subtractions, the
    product with rstd and the last addition, each relative to at most |d| + |m1| + |h m2| (6 u of it covers them and the
    2 u of dh), and u |dx| for the addition of dres:
        slack_dx = rstd (|gamma| e_du + e_m1 + |h| e_m2 + 6 u (|d| + |m1| + |h m2|)) + u |dx|;  bound = 2^-8 |dx| + slack_dx.
    dgamma = sum_rows du h^: each term is off by |h| e_du + 3 u |du h| and the sum runs along `chain` additions:
        slack = (chain + 4) u sum|du h| + sum(|h| e_du) + u (|init| + |dgamma + init|)
    and dbeta likewise with sum|du| and sum e_du."""
    rows, C = x.shape
    depth = depth_of(C)
    dy, gamma, rstd, h, du = _bwd_terms(dy, x, gamma, beta, mean, rstd, act)
    if act:
        e_du = dy.abs() * (DGELU_LIP * 4 * U * ((h * gamma).abs() + f64(beta).abs()) + ERF_APPROX + 8 * U) + U * du.abs()
    else:
        e_du = torch.zeros_like(du)
    d = du * gamma
    m1, m2 = d.mean(1, keepdim=True), (d * h).mean(1, keepdim=True)
    ge = gamma.abs() * e_du
    e_m1 = (depth + 2) * U * d.abs().mean(1, keepdim=True) + ge.mean(1, keepdim=True)
    e_m2 = (depth + 5) * U * (d * h).abs().mean(1, keepdim=True) + (ge * h.abs()).mean(1, keepdim=True)
    dx = rstd * (d - m1 - h * m2) + (f64(dres) if dres is not None else 0.0)
    slack_in = rstd * (ge + e_m1 + h.abs() * e_m2 + 6 * U * (d.abs() + m1.abs() + (h * m2).abs()))
    slack_dx = slack_in + U * dx.abs()
    dx_nores = (rstd * (d - m1 - h * m2)).abs()
    out = {"dx": BF16_HALF_ULP * dx.abs() + slack_dx, "dx_slack": slack_dx,
           "dx_nores": (BF16_HALF_ULP + U) * dx_nores + slack_in,
           "_dgamma": ((du * h).sum(0), (du * h).abs().sum(0), (h.abs() * e_du).sum(0)),
           "_dbeta": (du.sum(0), du.abs().sum(0), e_du.sum(0))}
    out["dgamma"], out["dbeta"] = param_grad_bound(out, "dgamma", chain, init), param_grad_bound(out, "dbeta", chain, init)
    return out


def param_grad_bound(bounds, which, chain, init=None):
    """The d gamma / d beta bound of bwd_bounds for another chain length or starting value (the sums over the rows are
    kept in `bounds`, so the arrangements of one case share them)."""
    value, mass, e_terms = bounds["_" + which]
    i0 = 0.0 if init is None else abs(float(init))
    return (chain + 4) * U * mass + e_terms + U * (i0 + (value + i0).abs())


# ---- bounds: reductions, column sums, element-wise -------------------------------------------------------------------
def sum_bound(terms_abs_sum, chain: int, c: int = 2):
    """(chain + c) u sum|term|: a sum along a chain of `chain` fp32 additions; c covers the addition into the output
    and, with accumulate, the term that was there (include it in terms_abs_sum)."""
    return (chain + c) * U * terms_abs_sum


def colsum_chain(rows: int, nslab: int) -> int:
    """colsum_kernel + the reduction of its slabs: a row lane adds every 8th row of its slab (ceil(per / 8) additions, in
    row order whether four are in flight or one), 8 row lanes are added through LDS, then reduce_partials_kernel over the
    slabs (ceil(nslab / 64) + 3 + 16) and 1 into the output."""
    per = -(-rows // nslab)
    return -(-per // 8) + 8 + -(-nslab // 64) + 3 + 16 + 1


def dgelu_mul_bound(dy, u):
    """out = bf16(dy gelu'(u)) from exact bf16 inputs: the erf approximation and ~8 roundings on gelu' (absolute, it is <=
    1.13), one product, the bf16 rounding: 2^-8 |ref| + |dy| (1.5e-7 + 8 u) + u |ref|."""
    ref = dy * dgelu64(u)
    return BF16_HALF_ULP * ref.abs() + dy.abs() * (ERF_APPROX + 8 * U) + U * ref.abs()


# ---- the dropout mask of csrc/common.h (ca_dropout_keep4), as integer arithmetic on int64 tensors -----------------------
_M32 = 0xFFFFFFFF


def _mul32(x, k):
    """(x * k) mod 2^32 for 0 <= x < 2^32 held in int64 (the int64 product wraps; its low 32 bits are right)."""
    if k >= 1 << 31:
        k -= 1 << 32   # the same residue mod 2^32, and the product stays inside int64's wrap-around arithmetic
    return (x * k) & _M32


def dropout_keep(seed: int, idx: torch.Tensor, p: float) -> torch.Tensor:
    """keep[i] (bool) of flat element index idx[i] (int64 tensor, any device), bit for bit ca_dropout_keep."""
    s = ((seed & _M32) * 0x9E3779B9 + (seed >> 32)) & _M32
    group = idx >> 2
    x = ((group & _M32) ^ s ^ _mul32(group >> 32, 0x85EBCA6B)) & _M32
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    w0 = x ^ (x >> 16)
    w1 = _mul32(w0, 0xC2B2AE35)
    w1 = w1 ^ (w1 >> 15)
    w = torch.where((idx & 2) != 0, w1, w0)
    thr = int(torch.tensor(p, dtype=torch.float32).item() * 65536.0)
    return ((w >> (16 * (idx & 1))) & 0xFFFF) >= thr
