"""The GEMM epilogues on a real MI355X against the float64 reference of tests/gemm_epi_ref.py (proved on the CPU in
tests/test_gemm_epi_ref_cpu.py): gemm_epilogue's general walk and its interior-tile form (csrc/gemm_common.h) on the
kernels S, L, X and M and on the two fp8 kernels, and the skinny kernel's own epilogue (csrc/gemm_skinny.hip).

The matrix product is exact by construction (integer operands, K <= 512, power-of-two alpha, bias / R / C_old in eighths,
p = 0.5), so every assertion is about the epilogue: EPI_NONE, EPI_RESIDUAL (+ dropout), accumulate, alpha and the
pre-activation C of the GELU epilogues must come out bit for bit (fp32: the exact value; bf16: its round-to-nearest-even);
what passes through gelu_erf / gelu_erf' must lie inside the bounds derived in tests/norm_ref.py.  Every output buffer
starts as the sentinel 0.5 (or C_old under accumulate): padding columns n >= N, the elements between and behind the batch
blocks and the TAIL behind the buffer must still hold it afterwards.

On the tiled kernels every case runs twice, with ca_gemm_debug_general_epilogue(0) and (1), and BOTH runs are compared with
the reference: the interior-tile form and the general walk are each held to the mathematics, not to each other.

What each case reaches (lines of the general walk no other test runs):
  shape A (300 x 264, ldc = ldr = 264)  interior and ragged wave tiles in both dimensions, a second tile row / column for
                                        the 128-wide kernels and the 256 x 256 one; nvalid = 8 everywhere
  shape B (200 x 204, ldc 208, ldr 216) 0 < nvalid < 8 (the last lane group has 4 columns) for R, C, C2 and the bias with
                                        aligned rows; no interior tile; ldr != ldc
  shape C (136 x 203, ldc 203, ldr 205) vec_ok == false: the scalar loads and stores of R, C and C2; nvalid = 3; N odd, so
                                        every other row's dropout groups are not 4-aligned (the per-element
                                        ca_dropout_keep branch)
  shape D (2 x 3 batches of 72 x 80)    batch1 > 1 and batch2 > 1 together with different sC / sR / sBias strides, the
                                        grouped pos-conv form; the mask's flat index in batch z > 0
  variants  gelu_res, gelu_res_noC      CA_EPI_GELU_RESIDUAL at kernel level (with batch1 x batch2 and sBias on shape D)
            gelu_noC, gelu_res_noC      C == NULL with only C2
            f32 / gelu_f32C / dgelu_f32 an fp32 C, with a non-plain epilogue in the last two
            bf16_acc                    accumulate into a bf16 C
            alpha, gelu*                alpha != 1
            bias_off3                   a bias pointer that is not 16-byte aligned (epi_load_bias's scalar branch)
            stream, stream_f32          c_stream_out (the non-temporal stores of interior tiles)
            residual_drop, gelu_drop, dgelu_drop   the mask with a seed above 2^32
The skinny kernel takes the variants its plan rule admits (no dropout, no DGELU) at M in {1, 5, 17, 32} x N in {72, 203};
the fp8 kernels plain, bias, GELU with both outputs, residual and fp32 at K = 128 on shapes A and B.

Which kernel ran is read from the profiler's variant index (kind * 8 + layout: S, M and the skinny kernel 0, L 8, X 16);
the fp8 form is not profiled (its plan has kind -1), so there the index list must be empty and the force switch - which
gemm_plan_fp8 obeys unconditionally - names the kernel.  One summary line per kernel (run with -s): the number of cases
and the largest error / bound of the bounded outputs.  Measured on an MI355X: S, L, X and M 160 cases each (both walks),
0.996; the skinny kernel 120 cases, 0.990; the two fp8 kernels 20 cases each, 0.840 - in every one the rounding to bf16
just above a power of two, which is the whole 2^-8 |ref| a correct kernel is entitled to (the CPU emulation reaches the
same figures).  All seven tests together take under three seconds.
"""
import functools

import pytest
import torch

import gemm_epi_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert (o.EPI_NONE, o.EPI_GELU, o.EPI_RESIDUAL, o.EPI_DGELU, o.EPI_GELU_RESIDUAL) == \
        (G.EPI_NONE, G.EPI_GELU, G.EPI_RESIDUAL, G.EPI_DGELU, G.EPI_GELU_RESIDUAL)
    return o


@functools.lru_cache(maxsize=None)
def _device_inputs(kind, shape):
    """(A, B, bias buffer, R buffer) on the device for the cases of one shape"""
    c = next(x for x in G.cases(kind) if x["shape"] == shape)
    inp = G.make_inputs(c)
    if kind == "fp8":
        A, B = (inp[k].float().to(torch.float8_e4m3fn).view(torch.uint8) for k in ("A", "B"))
        assert torch.equal(A.view(torch.float8_e4m3fn).double(), inp["A"])
    else:
        A, B = inp["A"].bfloat16(), inp["B"].bfloat16()
    return (A.contiguous().to(DEV), B.contiguous().to(DEV), inp["bias_buf"].float().to(DEV),
            G.pack(c, "R", inp["R"]).to(DEV))


@functools.lru_cache(maxsize=None)
def _reference(case_id, kind):
    c = next(x for x in G.cases(kind) if x["id"] == case_id)
    G.check_exact(c)
    return G.reference(c)


def run_case(ops, c):
    """One launch of case c: -> the largest error / bound of its bounded outputs (asserts everything else)."""
    ref = _reference(c["id"], c["kind"])
    inp = G.make_inputs(c)
    A, B, bias_buf, Rbuf = _device_inputs(c["kind"], c["shape"])
    Z2, M, N, K = c["batch2"], c["M"], c["N"], c["K"]
    batched = c["batch1"] * c["batch2"] > 1
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=c["ldc"], batch1=c["batch1"], batch2=Z2, sC=c["sC"], sBias=c["sBias"],
              sA=(Z2 * M * K, M * K) if batched else (0, 0), sB=(0, N * K) if batched else (0, 0), c_off=G.C_OFF,
              epilogue=c["epi"], accumulate=c["accumulate"], alpha=c["alpha"], stream_out=c["stream_out"])
    if c["bias"]:
        kw.update(bias=bias_buf, bias_off=c["bias_off"])
    if c["epi"] in (G.EPI_RESIDUAL, G.EPI_DGELU, G.EPI_GELU_RESIDUAL):
        kw.update(R=Rbuf, r_off=G.R_OFF, ldr=c["ldr"], sR=c["sR"])
    if c["drop"]:
        kw.update(dropout_p=G.DROP_P, dropout_seed=G.DROP_SEED)
    bufs = {}
    if "C" in ref:
        bufs["C"] = G.pack(c, "C", inp["C_old"] if c["accumulate"] else None, G.out_dtype(c, "C")).to(DEV)
    if "C2" in ref:
        bufs["C2"] = G.pack(c, "C2").to(DEV)
        kw.update(C2=bufs["C2"], c2_off=G.C2_OFF)
    (ops.gemm_fp8 if c["fp8"] else ops.gemm)(A, B, bufs.get("C"), **kw)
    torch.cuda.synchronize()
    got = {}
    for which, buf in bufs.items():
        got[which], clean = G.unpack(c, which, buf)
        assert clean, f"{c['id']} {which}: an element outside the output's blocks was written"
    return G.compare(c, got, ref)


def run_table(ops, kind, force, both_walks, fired_want):
    lib = ops.lib()
    worst, n = 0.0, 0
    lib.ca_gemm_force_kernel(force)
    try:
        ops.prof_begin()
        try:
            for general in ((0, 1) if both_walks else (0,)):
                lib.ca_gemm_debug_general_epilogue(general)
                for c in G.cases(kind):
                    try:
                        worst = max(worst, run_case(ops, c))
                    except AssertionError as e:
                        raise AssertionError(f"force {force}, general walk {general}: {e}") from None
                    n += 1
        finally:
            fired = [i for i, p in enumerate(ops.prof_end()) if p["count"]]
    finally:
        lib.ca_gemm_debug_general_epilogue(0)
        lib.ca_gemm_force_kernel(0)
    assert fired == fired_want, (fired, fired_want)
    return n, worst


@pytest.mark.parametrize("name,force,kind", [("S", 1, 0), ("L", 2, 1), ("X", 3, 2), ("M", 5, 0)])
def test_tiled_kernel_epilogues_match_the_float64_reference(ops, name, force, kind):
    n, worst = run_table(ops, "tiled", force, True, [kind * 8])
    print(f"gemm epilogue, kernel {name}: {n} cases (both walks), worst error / bound {worst:.3f}")
    assert n == 2 * len(G.cases("tiled"))


def test_skinny_kernel_epilogue_matches_the_float64_reference(ops):
    n, worst = run_table(ops, "skinny", 0, False, [0])
    print(f"gemm epilogue, skinny kernel: {n} cases, worst error / bound {worst:.3f}")
    assert n == len(G.cases("skinny"))


@pytest.mark.parametrize("name,force", [("fp8 128x128", 1), ("fp8 256x256", 3)])
def test_fp8_kernel_epilogues_match_the_float64_reference(ops, name, force):
    n, worst = run_table(ops, "fp8", force, True, [])
    print(f"gemm epilogue, kernel {name}: {n} cases (both walks), worst error / bound {worst:.3f}")
    assert n == 2 * len(G.cases("fp8"))
