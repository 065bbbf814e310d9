"""tests/gemm_epi_ref.py checked without a GPU: the premises of its exact comparisons on every case of the table, its
float64 reference against a direct torch statement (F.linear, F.gelu, autograd for GELU'), its bounds against an fp32
emulation of the epilogue's own arithmetic (admitted on every case), and its comparison against ten wrong epilogues
(each rejected wherever it differs from the right one).

Which shapes can tell a wrong epilogue from the right one is a property of the shapes, not of the inputs:
  bias one column off in the last lane group, residual from row m + 1, tanh-GELU, bf16 truncation, `accumulate` ignored,
  dropout after the residual add                                            every shape: checked on A, C and D
  residual read with ldc for ldr                                            needs ldr != ldc: B and C
  mask keyed on m N + n without z                                           needs a batch: D
  mask keyed with ldc in place of N                                         needs ldc != N: B and D
  mask from the 4-aligned group of an unaligned index                       needs N % 4 != 0: C
On the other shapes such an epilogue computes what the right one computes, which the test asserts as well (so the table
above cannot go stale)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_epi_ref as G
from test_norm_ref_cpu import emu_dgelu, emu_gelu

ALL_CASES = G.cases("tiled") + G.cases("skinny") + G.cases("fp8")


# ---- fp32 emulation of the epilogue (csrc/gemm_common.h, gemm_skinny.hip) -----------------------------------------------
def rne(x):
    return x.bfloat16()


def trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def tanh_gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


def emulate(c, *, bias=None, R=None, idx=None, gelu=emu_gelu, to_bf16=rne, accumulate=None, drop_after=False):
    """The outputs of case c the way the kernels form them, every step in fp32: v = acc alpha + bias, the mask, the
    activation, the residual, `accumulate`, one rounding to the output type.  The keyword arguments swap in what a
    wrong epilogue would use."""
    inp = G.make_inputs(c)
    acc, _ = G.preact(c, inp)
    b = (G.bias_of(c, inp) if bias is None else bias).float()
    r = (inp["R"] if R is None else R).float()
    f = G.drop_factor(c, idx).float()
    accumulate = c["accumulate"] if accumulate is None else accumulate
    scale = torch.tensor(1.0 / (1.0 - G.DROP_P) if c["drop"] else 1.0, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)

    def drop(x):
        return torch.where(f != 0, x * scale, zero) if c["drop"] else x

    v = acc.float() * torch.tensor(c["alpha"], dtype=torch.float32) + b[:, None, :]
    v2, epi = None, c["epi"]
    if epi in (G.EPI_GELU, G.EPI_GELU_RESIDUAL):
        g = gelu(v)
        if epi == G.EPI_GELU_RESIDUAL:
            v2 = drop(g + r) if drop_after else drop(g) + r
        else:
            v2 = drop(g) + zero
    elif epi == G.EPI_RESIDUAL:
        v = drop(v + r) if drop_after else drop(v) + r
    elif epi == G.EPI_DGELU:
        v = v * drop(emu_dgelu(r))
    if accumulate:
        v = v + (inp["C_old"].float() if c["f32"] else inp["C_old"].bfloat16().float())
    out = {}
    if not c["noC"]:
        out["C"] = v if c["f32"] else to_bf16(v)
    if v2 is not None:
        out["C2"] = to_bf16(v2)
    return out


# ---- the premises --------------------------------------------------------------------------------------------------------
def test_every_case_is_exact_by_construction():
    for c in ALL_CASES:
        G.check_exact(c)
    ids = [c["id"] for c in ALL_CASES]
    assert len(set(ids)) == len(ids) == 4 * 20 + 8 * 15 + 2 * 5
    big = 1 << 32
    assert G.DROP_SEED > big and G.DROP_SEED % big != 0 and G.C_OFF % 8 == G.R_OFF % 8 == G.C2_OFF % 8 == 0


def test_layout_round_trip_and_sentinel():
    """pack / unpack are inverse, and unpack reports an element written outside the case's blocks"""
    for c in (G.case("tiled", "C", "residual"), G.case("tiled", "D", "gelu2")):
        for which in ("C", "C2", "R"):
            x = G.make_inputs(c)["R"]
            buf = G.pack(c, which, x)
            y, clean = G.unpack(c, which, buf)
            assert clean and torch.equal(y.double(), x)
            off, size = G.offsets(c, which)
            hit = torch.zeros(size, dtype=torch.bool)
            hit[off.reshape(-1)] = True
            outside = (~hit).nonzero().reshape(-1)
            assert outside.numel() >= G.TAIL
            for i in (int(outside[0]), int(outside[-1]), int(outside[outside.numel() // 2])):
                buf2 = buf.clone()
                buf2[i] = 1.0
                assert not G.unpack(c, which, buf2)[1]


# ---- the reference against a direct statement ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.cases("tiled"), ids=lambda c: c["id"])
def test_reference_agrees_with_a_direct_float64_statement(c):
    """With the mask off: F.linear per batch, F.gelu, autograd for GELU'.  With it on: the same values times the
    keep bits of the flattened [batch1 batch2 M, N] index."""
    inp = G.make_inputs(c)
    Z1, Z2, M, N = c["batch1"], c["batch2"], c["M"], c["N"]
    bias = G.bias_of(c, inp)
    v = torch.stack([c["alpha"] * F.linear(inp["A"][z1, z2], inp["B"][z2]) + bias[z1 * Z2 + z2]
                     for z1 in range(Z1) for z2 in range(Z2)])
    r = inp["R"].clone().requires_grad_(True)
    F.gelu(r).sum().backward()
    flat = torch.arange(Z1 * Z2 * M * N).view(Z1 * Z2, M, N)
    f = G.dropout_keep(G.DROP_SEED, flat, G.DROP_P).double() * 2.0 if c["drop"] else torch.ones(Z1 * Z2, M, N).double()
    assert torch.equal(G.mask_index(c), flat) and torch.equal(G.drop_factor(c), f)
    want = {}
    if c["epi"] == G.EPI_NONE:
        want["C"] = v + inp["C_old"] if c["accumulate"] else v
    elif c["epi"] == G.EPI_RESIDUAL:
        want["C"] = f * v + inp["R"]
    elif c["epi"] == G.EPI_DGELU:
        want["C"] = v * r.grad * f
    else:
        want["C"] = v
        want["C2"] = F.gelu(v) * f + (inp["R"] if c["epi"] == G.EPI_GELU_RESIDUAL else 0.0)
    if c["noC"]:
        del want["C"]
    ref = G.reference(c)
    assert set(ref) == set(want)
    for k, (value, bound) in ref.items():
        assert float((value - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), (c["id"], k)
        assert (bound is None) == (k == "C" and c["epi"] != G.EPI_DGELU)
        if c["drop"] and bound is not None and c["epi"] != G.EPI_GELU:
            assert bool((bound[f == 0] == 0).all())
    if c["drop"]:
        rate = float((f != 0).double().mean())
        assert abs(rate - 0.5) < 4 * (0.25 / f.numel()) ** 0.5


# ---- the bounds admit a correct fp32 epilogue ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tiled", "skinny", "fp8"])
def test_comparison_admits_the_fp32_emulation(kind):
    """Every case of the table: the exact outputs bit for bit, the bounded ones inside their bound.  Largest error / bound
    of the bounded outputs over the table: tiled 0.996, skinny 0.990, fp8 0.840 - the rounding to bf16 itself, which just
    above a power of two is the whole 2^-8 |ref| granted, so these must stay <= 1; on the fp32 C of DGELU, where that term
    is absent and the figure measures the derivation, 0.274 (<= 0.5 asserted)."""
    worst, worst_f32 = 0.0, 0.0
    for c in G.cases(kind):
        w = G.compare(c, emulate(c))
        if c["epi"] == G.EPI_DGELU and c["f32"]:
            worst_f32 = max(worst_f32, w)
        else:
            worst = max(worst, w)
    print(f"{kind}: {len(G.cases(kind))} cases, worst error / bound {worst:.3f} (bf16 outputs), {worst_f32:.3f} (fp32 DGELU)")
    assert worst <= 1.0 and worst_f32 <= 0.5


# ---- the comparison rejects wrong epilogues ------------------------------------------------------------------------------
def _bias_shift(c):
    b = G.bias_of(c, G.make_inputs(c)).clone()
    N = c["N"]
    n = torch.arange(((N - 1) // 8) * 8, N)
    src = torch.where((n ^ 1) < N, n ^ 1, n)
    b[:, n] = b[:, src]
    return dict(bias=b)


def _res_row(c):
    return dict(R=torch.roll(G.make_inputs(c)["R"], -1, dims=1))


def _res_ldc(c):
    buf = G.pack(c, "R", G.make_inputs(c)["R"], dtype=torch.float64)
    off, _ = G.offsets(dict(c, ldr=c["ldc"]), "R")
    return dict(R=buf[off])


def _zmn(c):
    Z, M, N = c["batch1"] * c["batch2"], c["M"], c["N"]
    return torch.arange(Z)[:, None, None], torch.arange(M)[None, :, None], torch.arange(N)[None, None, :]


def _mask_noz(c):
    z, m, n = _zmn(c)
    return dict(idx=(m * c["N"] + n).expand(z.numel(), -1, -1))


def _mask_ldc(c):
    z, m, n = _zmn(c)
    return dict(idx=(z * c["M"] + m) * c["ldc"] + n)


def _mask_group(c):
    z, m, n = _zmn(c)
    idx0 = (z * c["M"] + m) * c["N"] + (n // 8) * 8  # the lane's first element
    return dict(idx=(idx0 // 4) * 4 + n % 8)


WRONG = {
    # name: (what emulate() gets, the variants it is tried on, the shapes that can tell)
    "bias_shift": (_bias_shift, ("bias", "f32"), "ABCD"),
    "res_row": (_res_row, ("residual", "gelu_res", "dgelu"), "ABCD"),
    "res_ldc": (_res_ldc, ("residual", "gelu_res", "dgelu"), "BC"),
    "mask_noz": (_mask_noz, ("residual_drop", "gelu_drop", "dgelu_drop"), "D"),
    "mask_ldc": (_mask_ldc, ("residual_drop", "gelu_drop", "dgelu_drop"), "BD"),
    "mask_group": (_mask_group, ("residual_drop", "gelu_drop", "dgelu_drop"), "C"),
    "tanh_gelu": (lambda c: dict(gelu=tanh_gelu), ("gelu2", "gelu_noC", "gelu_res", "gelu_drop"), "ABCD"),
    "trunc": (lambda c: dict(to_bf16=trunc), ("bias", "bf16_acc", "residual"), "ABCD"),
    "no_accumulate": (lambda c: dict(accumulate=False), ("f32_acc", "bf16_acc"), "ABCD"),
    "drop_after": (lambda c: dict(drop_after=True), ("residual_drop",), "ABCD"),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_comparison_rejects_a_wrong_epilogue(name):
    make, variants, shapes = WRONG[name]
    assert set(shapes) >= set("ACD") or name in ("res_ldc", "mask_noz", "mask_ldc", "mask_group")
    for shape in "ABCD":
        for variant in variants:
            c = G.case("tiled", shape, variant)
            got = emulate(c, **make(c))
            if shape in shapes:
                with pytest.raises(AssertionError, match="wrong elements"):
                    G.compare(c, got)
            else:  # this shape cannot tell: the same bits as the right epilogue
                right = emulate(c)
                assert all(torch.equal(got[k], right[k]) for k in right), (name, c["id"])


def test_a_wrong_mask_is_also_rejected_by_its_zeros():
    """A dropped element is exactly zero (plus the residual) and its bound is zero wherever the output is gated by the mask
    alone (DGELU): one flipped mask bit fails, however small the values."""
    c = G.case("tiled", "C", "dgelu_drop")
    got = emulate(c)
    f = G.drop_factor(c)
    z, m, n = (int(t) for t in (f == 0).nonzero()[7])
    got["C"][z, m, n] = 2.0 ** -20
    with pytest.raises(AssertionError, match="1 wrong elements"):
        G.compare(c, got)
