"""Test-side float64 reference of the GEMM epilogues (include/coral_amd.h: CA_EPI_*, bias, alpha, accumulate, the fused
dropout and the two batch dimensions), the inputs that make the matrix product exact, the bounds a correct epilogue is
held to, and the case table that tests/test_gemm_epi_ref_cpu.py (no GPU) and tests/test_gemm_epilogue_gpu.py iterate.
Plain torch on the CPU; nothing here imports `coral_amd`.

Exact inputs.  A and B hold integers in [-3, 3] (bf16, or e4m3 bytes for the fp8 kernels) and K <= 512, so every product
and every partial sum is an integer below 2^24: exact in fp32 in any order, on any MFMA chain.  alpha is 1 or 2^-3, the
bias (fp32), R (bf16) and the previous contents of C under `accumulate` are multiples of 2^-3 of magnitude <= 8, dropout
runs at p = 0.5 (keep_scale = 2).  Then v = alpha acc + bias, v + R, 2 v + R and C_old + v are all exactly representable
in fp32 - whether or not the compiler contracts a multiply-add - and check_exact() proves it per case.  What is left to
compare is the epilogue alone: which element it reads, which mask bit it takes, how it rounds, where it stores.

Two kinds of expected value (reference()):
  * exact: EPI_NONE, EPI_RESIDUAL (with or without dropout), accumulate, alpha, and the pre-activation C of the GELU
    epilogues.  The expected bits are the exact value (fp32 C) or its round-to-nearest-even bf16 (many are ties).
  * bounded: what passes through gelu_erf / gelu_erf' - the forms tests/norm_ref.py derives, no new constant:
      C2 of GELU            |z| (ERF_APPROX + 8 U) + U |y| + BF16_HALF_ULP |y|,   y = gelu(z) x the exact dropout factor
      C2 of GELU_RESIDUAL   the same + U |y + r| for the addition, the bf16 term taken on |y + r|
      C  of DGELU           dgelu_mul_bound(v, r) x the exact dropout factor (an fp32 C: without its 2^-8 |ref| term)

Batch.  z = z1 * batch2 + z2, pointer offsets z1 * s?1 + z2 * s?2, and the mask bit of element (z, m, n) is
dropout_keep(seed, (z * M + m) * N + n, p): the flat index of a dense [batch1 * batch2 * M, N] output.
"""
from __future__ import annotations

import functools

import torch

from norm_ref import BF16_HALF_ULP, ERF_APPROX, U, dgelu64, dgelu_mul_bound, dropout_keep, gelu64

EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_GELU_RESIDUAL = 0, 1, 2, 3, 4
SENTINEL = 0.5
DROP_P = 0.5
DROP_SEED = (5 << 32) + 0x3039  # above 2^32: both seed words matter
C_OFF, R_OFF, C2_OFF, TAIL = 8, 16, 24, 16  # base offsets (multiples of 8 elements) and sentinel elements behind a buffer

# (M, N, ldc, ldr); what each one reaches is listed in tests/test_gemm_epilogue_gpu.py
SHAPES = {
    "A": dict(M=300, N=264, ldc=264, ldr=264),
    "B": dict(M=200, N=204, ldc=208, ldr=216),
    "C": dict(M=136, N=203, ldc=203, ldr=205),
    "D": dict(M=72, N=80, ldc=240, ldr=240, batch1=2, batch2=3, sC=(72 * 240, 80), sR=(72 * 240, 80), sBias=(0, 80)),
}
SKINNY_SHAPES = {f"s{M}x{N}": dict(M=M, N=N, ldc=80 if N == 72 else N, ldr=88 if N == 72 else N + 2)
                 for M in (1, 5, 17, 32) for N in (72, 203)}

_G = 2.0 ** -3
# name -> what differs from the plain bf16 launch
VARIANTS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias_off3": dict(bias=True, bias_off=3),
    "f32": dict(bias=True, f32=True),
    "f32_acc": dict(bias=True, f32=True, accumulate=True),
    "bf16_acc": dict(bias=True, accumulate=True),
    "alpha": dict(bias=True, alpha=_G),
    "stream": dict(bias=True, stream_out=True),
    "stream_f32": dict(bias=True, f32=True, stream_out=True),
    "residual": dict(bias=True, epi=EPI_RESIDUAL),
    "residual_drop": dict(bias=True, epi=EPI_RESIDUAL, drop=True),
    "gelu2": dict(bias=True, epi=EPI_GELU, alpha=_G),
    "gelu_noC": dict(bias=True, epi=EPI_GELU, alpha=_G, noC=True),
    "gelu_drop": dict(bias=True, epi=EPI_GELU, alpha=_G, drop=True),
    "gelu_res": dict(bias=True, epi=EPI_GELU_RESIDUAL, alpha=_G),
    "gelu_res_noC": dict(bias=True, epi=EPI_GELU_RESIDUAL, alpha=_G, noC=True),
    "gelu_f32C": dict(bias=True, epi=EPI_GELU, alpha=_G, f32=True),
    "dgelu": dict(bias=True, epi=EPI_DGELU),
    "dgelu_drop": dict(bias=True, epi=EPI_DGELU, drop=True),
    "dgelu_f32": dict(bias=True, epi=EPI_DGELU, f32=True),
}
FP8_VARIANTS = ("plain", "bias", "gelu2", "residual", "f32")
_VAR_DEFAULT = dict(bias=False, bias_off=0, f32=False, accumulate=False, alpha=1.0, stream_out=False, epi=EPI_NONE,
                    drop=False, noC=False)


def cases(kind: str = "tiled"):
    """The case table.  kind 'tiled': shapes A - D x every variant, K = 72 (kernels S, L, X, M); 'skinny': M in
    {1, 5, 17, 32} x N in {72, 203}, K = 72, the variants the skinny plan rule admits (no dropout, no DGELU); 'fp8':
    shapes A and B, K = 128, plain / bias / GELU with both outputs / residual / fp32."""
    if kind == "tiled":
        shapes, names, K = SHAPES, list(VARIANTS), 72
    elif kind == "skinny":
        shapes, K = SKINNY_SHAPES, 72
        names = [n for n, v in VARIANTS.items() if not v.get("drop") and v.get("epi") != EPI_DGELU]
    elif kind == "fp8":
        shapes, names, K = {k: SHAPES[k] for k in "AB"}, list(FP8_VARIANTS), 128
    else:
        raise ValueError(kind)
    out = []
    for sname, s in shapes.items():
        for vname in names:
            c = dict(batch1=1, batch2=1, sC=(0, 0), sR=(0, 0), sBias=(0, 0))
            c.update(s)
            c.update(_VAR_DEFAULT)
            c.update(VARIANTS[vname])
            c.update(id=f"{kind}-{sname}-{vname}", shape=sname, variant=vname, kind=kind, K=K, fp8=kind == "fp8")
            out.append(c)
    return out


def case(kind, shape, variant):
    return next(c for c in cases(kind) if c["shape"] == shape and c["variant"] == variant)


# ---- seeded inputs (one set per shape: the variants share it) --------------------------------------------------------------
def _eighths(g, *shape):
    """multiples of 2^-3 in [-8, 8]"""
    return torch.randint(-64, 65, shape, generator=g).double() * _G


@functools.lru_cache(maxsize=None)
def _inputs(kind, shape, K):
    s = dict(batch1=1, batch2=1)
    s.update((SKINNY_SHAPES if kind == "skinny" else SHAPES)[shape])
    Z1, Z2, M, N = s["batch1"], s["batch2"], s["M"], s["N"]
    g = torch.Generator().manual_seed(1000 + sum(map(ord, kind + shape)))
    return dict(
        A=torch.randint(-3, 4, (Z1, Z2, M, K), generator=g).double(),  # sA = (Z2 M K, M K), lda = K
        B=torch.randint(-3, 4, (Z2, N, K), generator=g).double(),      # sB = (0, N K), ldb = K
        bias_buf=_eighths(g, 3 + Z2 * N),                              # the vector starts at bias_off (0 or 3)
        R=_eighths(g, Z1 * Z2, M, N),
        C_old=_eighths(g, Z1 * Z2, M, N),
    )


def make_inputs(c):
    """{'A' [batch1, batch2, M, K], 'B' [batch2, N, K] (integers), 'bias_buf' [3 + batch2 N], 'R' and 'C_old'
    [batch1 batch2, M, N]}, float64 holding the exact values.  Shared between the cases of a shape: do not modify."""
    return _inputs(c["kind"], c["shape"], c["K"])


def bias_of(c, inp):
    """[Z, N]: the bias row of batch z = (z1, z2) is bias[z1 sBias1 + z2 sBias2 : + N] (zeros without a bias)"""
    Z1, Z2, N = c["batch1"], c["batch2"], c["N"]
    if not c["bias"]:
        return torch.zeros(Z1 * Z2, N, dtype=torch.float64)
    vec = inp["bias_buf"][c["bias_off"]:]
    rows = [vec[z1 * c["sBias"][0] + z2 * c["sBias"][1]:][:N] for z1 in range(Z1) for z2 in range(Z2)]
    return torch.stack(rows)


def preact(c, inp):
    """(acc, v) [Z, M, N]: the integer product and v = alpha acc + bias, float64"""
    Z, M, N = c["batch1"] * c["batch2"], c["M"], c["N"]
    acc = torch.einsum("abmk,bnk->abmn", inp["A"], inp["B"]).reshape(Z, M, N)
    return acc, c["alpha"] * acc + bias_of(c, inp)[:, None, :]


def mask_index(c):
    """[Z, M, N] int64: the flat element index the header keys the dropout mask on"""
    Z, M, N = c["batch1"] * c["batch2"], c["M"], c["N"]
    z, m, n = torch.arange(Z)[:, None, None], torch.arange(M)[None, :, None], torch.arange(N)[None, None, :]
    return (z * M + m) * N + n


def drop_factor(c, idx=None):
    """[Z, M, N] float64: 1 without dropout, else 0 or 1 / (1 - p) = 2"""
    idx = mask_index(c) if idx is None else idx
    if not c["drop"]:
        return torch.ones(idx.shape, dtype=torch.float64)
    return dropout_keep(DROP_SEED, idx, DROP_P).double() / (1.0 - DROP_P)


def _is_f32(x):
    return bool(torch.equal(x.float().double(), x))


def _is_bf16(x):
    return bool(torch.equal(x.bfloat16().double(), x))


def check_exact(c):
    """The premises of the exact comparisons, asserted in float64 on this case's inputs."""
    inp = make_inputs(c)
    assert c["K"] <= 512 and c["alpha"] in (1.0, _G) and (not c["drop"] or DROP_P == 0.5)
    for k in ("A", "B"):
        assert float(inp[k].abs().max()) <= 3 and torch.equal(inp[k], inp[k].round())
    for k in ("bias_buf", "R", "C_old"):
        assert float(inp[k].abs().max()) <= 8 and torch.equal(inp[k] * 8, (inp[k] * 8).round())
    assert _is_bf16(inp["R"]) and _is_bf16(inp["C_old"]) and _is_f32(inp["bias_buf"])
    acc, v = preact(c, inp)
    assert float(acc.abs().max()) < 2 ** 24 and 9 * c["K"] < 2 ** 24
    for name, x in (("acc", acc), ("v", v), ("v + R", v + inp["R"]), ("2 v + R", 2 * v + inp["R"]),
                    ("C_old + v", inp["C_old"] + v)):
        assert _is_f32(x), (c["id"], name)


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference(c, idx=None):
    """{'C': (value, bound), 'C2': (value, bound)}: float64 [Z, M, N] each; bound None = the value is exact and the output
    must be its bits; an output the case does not have is absent.  idx: another mask index (the CPU tests' wrong ones)."""
    inp = make_inputs(c)
    _, v = preact(c, inp)
    f, r, epi = drop_factor(c, idx), inp["R"], c["epi"]
    out = {}
    if epi == EPI_NONE:
        out["C"] = (v + inp["C_old"] if c["accumulate"] else v, None)
    elif epi == EPI_RESIDUAL:
        out["C"] = (f * v + r, None)
    elif epi == EPI_DGELU:
        ref = v * dgelu64(r) * f
        bound = dgelu_mul_bound(v, r) * f
        if c["f32"]:
            bound = bound - BF16_HALF_ULP * ref.abs()
        out["C"] = (ref, bound)
    else:
        if not c["noC"]:
            out["C"] = (v, None)
        y = gelu64(v) * f
        bound = v.abs() * (ERF_APPROX + 8 * U) + U * y.abs()
        if epi == EPI_GELU_RESIDUAL:
            out["C2"] = (y + r, bound + (U + BF16_HALF_ULP) * (y + r).abs())
        else:
            out["C2"] = (y, bound + BF16_HALF_ULP * y.abs())
    return out


def out_dtype(c, which):
    return torch.float32 if (which == "C" and c["f32"]) else torch.bfloat16


# ---- where the elements live ------------------------------------------------------------------------------------------
def offsets(c, which):
    """[Z, M, N] int64 flat element offsets of output / side input `which` ('C', 'C2' or 'R') in its buffer, and the
    buffer's length: base offset + z1 s?1 + z2 s?2 + m ld + n, TAIL elements behind the last one."""
    Z1, Z2, M, N = c["batch1"], c["batch2"], c["M"], c["N"]
    ld, st, base = (c["ldr"], c["sR"], R_OFF) if which == "R" else (c["ldc"], c["sC"], C_OFF if which == "C" else C2_OFF)
    z1, z2 = torch.arange(Z1)[:, None, None, None], torch.arange(Z2)[None, :, None, None]
    m, n = torch.arange(M)[None, None, :, None], torch.arange(N)[None, None, None, :]
    off = (base + z1 * st[0] + z2 * st[1] + m * ld + n).reshape(Z1 * Z2, M, N)
    assert off.unique().numel() == off.numel()
    return off, int(off.max()) + 1 + TAIL


def pack(c, which, values=None, dtype=torch.bfloat16, fill=SENTINEL):
    """Flat CPU buffer of `which`, filled with the sentinel, `values` [Z, M, N] (if any) at their places."""
    off, size = offsets(c, which)
    buf = torch.full((size,), fill, dtype=dtype)
    if values is not None:
        buf[off.reshape(-1)] = values.reshape(-1).to(dtype)
    return buf


def unpack(c, which, buf):
    """-> ([Z, M, N] elements of `which`, True if every other element of the buffer still holds the sentinel)"""
    off, size = offsets(c, which)
    buf = buf.detach().cpu()
    assert buf.numel() == size
    other = torch.ones(size, dtype=torch.bool)
    other[off.reshape(-1)] = False
    return buf[off], bool((buf[other] == SENTINEL).all())


# ---- the comparison ---------------------------------------------------------------------------------------------------
def _where(c, bad):
    z, m, n = (int(t) for t in bad.nonzero()[0])
    interior = (m // 64) * 64 + 64 <= c["M"] and (n // 64) * 64 + 64 <= c["N"]
    return f"{int(bad.sum())} wrong elements, first at (z, m, n) = ({z}, {m}, {n}), " \
           f"{'an interior' if interior else 'a ragged'} 64 x 64 wave tile"


def compare(c, got, ref=None):
    """got: {'C': [Z, M, N] tensor of the output's dtype, 'C2': ...} - exactly the outputs the case has.  Asserts the exact
    outputs bit for bit and the bounded ones inside their bound; -> the largest error / bound of the bounded ones (0.0 if
    the case has none)."""
    ref = reference(c) if ref is None else ref
    assert set(got) == set(ref), (c["id"], sorted(got), sorted(ref))
    worst = 0.0
    for which, (value, bound) in ref.items():
        g, dt = got[which].detach().cpu(), out_dtype(c, which)
        assert g.dtype == dt and g.shape == value.shape, (c["id"], which, g.dtype, tuple(g.shape))
        if bound is None:
            # fp32: the exact value; bf16: its round-to-nearest-even.  (+ 0.0: an exact zero is +0 - sums that start from
            # +0 accumulators and a +0 bias or residual never give -0)
            want = (value + 0.0).float().to(dt)
            bits = torch.int32 if dt == torch.float32 else torch.int16
            bad = g.contiguous().view(bits) != want.contiguous().view(bits)
            assert not bool(bad.any()), f"{c['id']} {which} (exact): {_where(c, bad)}"
        else:
            err = (g.double() - value).abs()
            bad = ~(err <= bound)  # (a NaN is outside every bound)
            ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
            assert not bool(bad.any()), f"{c['id']} {which} (bounded): {_where(c, bad)}, error / bound up to {float(ratio[bad].max()):.3g}"
            worst = max(worst, float(ratio.max()))
    return worst
