"""`ops.ctc_loss_fwd_bwd` on a real MI355X against the float64 reference of tests/ctc_ref.py, on every combination of
its recursion path (one wave per direction for S = 2L+1 <= 256, LDS rows above), its log-prob fetch (LDS copy up to
T*V*4 = 120 KiB, global gather above) and its arguments.  `-m gpu` only.

Bounds.  nll: |got - ref64| <= 1e-4 max(1, |ref64|).  Gradient: with e32 = max |grad of torch's float32 CPU loss - ref64|
on the same inputs, max |got - ref64| <= max(3e-5, 4 e32): the kernel is held to four times what a correctly-rounded
fp32 statement of the same recursion loses (hardware exp/log, unordered LDS float atomics), and to the golden file's
atol where e32 is next to nothing.  The bound is applied to every utterance with its own e32 (utterances do not share
arithmetic), which implies the same bound over the batch.  Every test prints its figures before it asserts.

Worst err_gpu / e32 measured on an MI355X, over the batch and (in brackets) over single utterances whose 4 e32 is above
the 3e-5 floor; no case family and neither recursion path stands out, the kernel loses what torch's fp32 CPU loss loses:
  (a) alternating labels  1.16 (1.09)   at L = 1 the errors are <= 4.1e-7 against e32 = 1.6e-8: 27, under the floor
      repeated label      1.34 (1.34)   the peaked slack rows: <= 8.6e-7 absolute at every L
  (b) mixed launch        1.31 (1.83)   blank = 0: 1.10 (1.39)
  (c) largest labels      1.19 (1.69)   workspace reused: 0.97 (1.29)
  (d) LDS boundary        1.06 (1.07)   T = 640 in LDS 1.06, T = 641 gathered 1.05, T = 700 0.93
  (e) vocabulary width    1.27 (1.44)   V = 2: 1.15
  (f) arguments           1.31 (1.83)   the inputs of (b); in_len = None / T / T+5: 1.00 (1.52)
"""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
FILL = 7.0


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return o


def roundup8(v):
    return (v + 7) // 8 * 8


def label_rows(targets, width):
    lab = torch.full((len(targets), max(width, 1)), -100, dtype=torch.int32)
    for b, tg in enumerate(targets):
        lab[b, :len(tg)] = torch.tensor(tg, dtype=torch.int32)
    return lab


def new_workspace(ops, B, T, Lmax):
    """Workspace plus guard, every byte 0xFF: as float that is NaN, so reading a cell the kernel did not write shows."""
    n = ops.ctc_workspace_bytes(B, T, Lmax)
    return torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV), n


def launch(ops, case, *, ldv=None, labels=None, in_len="case", gscale=None, want_grad=True, zero_infinity=True, ws=None):
    """One call under the harness: guarded workspace, nll and grad; returns (nll [B], grad [B, T, V] or None) on the CPU
    after checking the guards, the padding columns, the frames past in_len and NaN."""
    B, T, V = case.shape
    ldv = ldv or roundup8(V)
    labels = label_rows(case.targets, max(len(tg) for tg in case.targets)) if labels is None else labels
    Lmax = labels.shape[1]
    lg = torch.zeros(B, T, ldv)
    lg[..., :V] = case.logits
    ws, nws = ws or new_workspace(ops, B, T, Lmax)
    assert nws == ops.ctc_workspace_bytes(B, T, Lmax)
    nll = torch.full((B + 1,), -FILL, device=DEV)
    gbuf = torch.full((B * T * ldv + 64,), FILL, device=DEV) if want_grad else None
    if isinstance(in_len, str):
        in_len = case.in_len
    tin = None if in_len is None else torch.tensor(in_len, dtype=torch.int32, device=DEV)
    gs = None if gscale is None else torch.tensor(gscale, dtype=torch.float32, device=DEV)
    ops.ctc_loss_fwd_bwd(lg.to(DEV), labels.to(DEV), tin, nll, gbuf, gs, ws, B, T, V, ldv, Lmax, case.blank,
                         zero_infinity=zero_infinity)
    torch.cuda.synchronize()
    assert (ws[nws:] == 0xFF).all(), "workspace guard overwritten"
    assert float(nll[B]) == -FILL, "nll guard overwritten"
    nll = nll[:B].cpu()
    assert not torch.isnan(nll).any()
    if not want_grad:
        return nll, None
    assert (gbuf[B * T * ldv:] == FILL).all(), "grad guard overwritten"
    grad = gbuf[:B * T * ldv].view(B, T, ldv).cpu()
    assert not torch.isnan(grad).any()
    assert not grad[..., V:].any(), "padding columns of grad must be zero"
    for b in range(B):
        n = T if in_len is None else min(max(int(in_len[b]), 0), T)
        assert not grad[b, n:].any(), f"row {b}: frames past in_len must have a zero gradient"
    return nll, grad[..., :V]


def check(name, case, nll, grad):
    """The two bounds of the module docstring; returns err_gpu / e32."""
    nll64, g64, e32_rows = ref.reference(case)
    e32 = float(e32_rows.max())
    nerr = (nll.double() - nll64).abs()
    nbound = 1e-4 * nll64.abs().clamp(min=1.0)
    gerr = (grad.double() - g64).abs().amax(dim=(1, 2))
    bound = max(3e-5, 4 * e32)
    ratio = float(gerr.max()) / max(e32, 1e-30)
    rows = [f"{float(e):.1e}/{float(r):.1e}" for e, r in zip(gerr, e32_rows)]
    print(f"{name}: shape {case.shape} nll {nll64.min():.1f}..{nll64.max():.1f} nll_err/bound {float((nerr / nbound).max()):.3f} "
          f"grad_err {float(gerr.max()):.3e} e32 {e32:.3e} bound {bound:.3e} err/e32 {ratio:.2f} per-row err/e32 {rows}")
    assert (nerr <= nbound).all(), (name, nll.tolist(), nll64.tolist())
    assert (gerr <= (4 * e32_rows).clamp(min=3e-5)).all(), (name, gerr.tolist(), e32_rows.tolist())
    assert float(gerr.max()) <= bound, (name, gerr.tolist(), bound)
    return ratio


def check_infeasible_rows(case, nll, grad):
    for b, ok in enumerate(ref.feasible(case)):
        if not ok:
            assert float(nll[b]) == 0.0 and not grad[b].any(), f"row {b} is infeasible: nll and grad must be exactly 0"


# ---- (a) single-path and few-path inputs: every transition on the path is necessary ----------------------------------------
@pytest.mark.parametrize("family", ["alternating", "repeated"])
@pytest.mark.parametrize("L", ref.SHARP_L)
def test_single_path_and_few_path_labels(ops, family, L):
    case = ref.alternating_case(L) if family == "alternating" else ref.repeated_case(L)
    assert case.paths[0] is not None and ref.feasible(case) == [True, True, True, False]
    nll, grad = launch(ops, case)
    check(f"{family} L={L}", case, nll, grad)
    check_infeasible_rows(case, nll, grad)


# ---- (b) both recursion paths, Lmax = 190 strides and in_len = 0 in one launch ----------------------------------------------
@pytest.mark.parametrize("blank", [45, 0])
def test_fast_and_slow_path_utterances_in_one_launch(ops, blank):
    case = ref.mixed_case(blank)
    nll, grad = launch(ops, case)
    check(f"mixed blank={blank}", case, nll, grad)
    check_infeasible_rows(case, nll, grad)


# ---- (c) the largest accepted labels: S = 1025, slow path, global gather ------------------------------------------------------
def test_largest_labels_and_workspace_reuse(ops):
    case = ref.largest_case()
    B, T, V = case.shape
    assert T * V * 4 > 120 * 1024 and max(len(tg) for tg in case.targets) == 512
    ws = new_workspace(ops, B, T, 512)
    nll, grad = launch(ops, case, ws=ws)
    check("largest", case, nll, grad)
    # the same workspace again, not refilled, with shorter labels and utterances: stale alpha/beta rows must not leak
    short = ref.largest_case_short_labels()
    assert short.shape == case.shape
    nll, grad = launch(ops, short, labels=label_rows(short.targets, 512), ws=ws)
    check("largest, workspace reused", short, nll, grad)


# ---- (d) the boundary between the LDS copy of the log-probs and the global gather -----------------------------------------
@pytest.mark.parametrize("i", range(len(ref.LDS_BOUNDARY)))
def test_log_probs_in_lds_and_gathered_from_global_memory(ops, i):
    case = ref.lds_boundary_case(i)
    B, T, V = case.shape
    Ls = [len(tg) for tg in case.targets]
    assert min(Ls) <= 127 < max(Ls)   # both recursion paths meet this fetch mode
    nll, grad = launch(ops, case, ldv=48)
    check(f"lds boundary T={T} V={V} ({'LDS' if T * V * 4 <= 120 * 1024 else 'global'})", case, nll, grad)


# ---- (e) vocabulary width: lanes j >= 1 of the log-softmax, blank in the middle -------------------------------------------------
@pytest.mark.parametrize("V", ref.WIDE_V)
def test_vocabulary_widths_up_to_256(ops, V):
    case = ref.wide_case(V)
    assert case.blank == V // 2
    nll, grad = launch(ops, case, ldv=V + 8 if V == 65 else roundup8(V))
    check(f"wide V={V}", case, nll, grad)


# ---- (f) arguments, on the inputs of (b) ---------------------------------------------------------------------------------------
def test_gscale_scales_the_gradient_rows_and_not_the_loss(ops):
    case = ref.mixed_case(45)
    B = case.shape[0]
    gs = [0.5, 2.0] + [1.0 / (max(len(tg), 1) * B) for tg in case.targets[2:]]
    nll1, grad1 = launch(ops, case)
    nll, grad = launch(ops, case, gscale=gs)
    assert torch.equal(nll, nll1)
    gs32 = torch.tensor(gs, dtype=torch.float32)[:, None, None]
    check("gscale", case, nll, grad.double() / gs32.double())   # every row, whatever its factor
    assert torch.equal(grad, grad1 * gs32), "gscale must multiply each row of the unscaled gradient exactly"


def test_loss_without_gradient_has_the_same_bits(ops):
    case = ref.mixed_case(45)
    nll1, _ = launch(ops, case)
    nll, grad = launch(ops, case, want_grad=False)
    assert grad is None and torch.equal(nll, nll1)


def test_missing_and_overlong_in_len_mean_every_frame(ops):
    full = ref.mixed_case(45)
    B, T, _ = full.shape
    case = ref.Case(full.logits, full.targets, (T,) * B, full.blank)
    assert all(ref.feasible(case))
    nll1, grad1 = launch(ops, case)
    check("in_len=[T]*B", case, nll1, grad1)
    for name, in_len in (("in_len=None", None), ("in_len=T+5", (T + 5,) * B)):
        nll, grad = launch(ops, case, in_len=in_len)
        check(name, case, nll, grad)
        assert torch.equal(nll, nll1)


def test_ignored_labels_between_the_targets(ops):
    case = ref.mixed_case(45)
    nll1, _ = launch(ops, case)
    W = 2 * 190 + 5
    g = torch.Generator().manual_seed(77)
    lab = torch.full((case.shape[0], W), -100, dtype=torch.int32)
    for b, tg in enumerate(case.targets):
        pos = torch.randperm(W, generator=g)[:len(tg)].sort().values
        lab[b, pos] = torch.tensor(tg, dtype=torch.int32)
    assert (lab[:, 0] == -100).any() and (lab >= 0).sum() == sum(len(tg) for tg in case.targets)
    nll, grad = launch(ops, case, labels=lab)
    check("-100 between labels", case, nll, grad)
    check_infeasible_rows(case, nll, grad)
    assert torch.equal(nll, nll1)


def test_zero_infinity_off_reports_infinity_and_a_zero_gradient(ops):
    for case in (ref.mixed_case(45), ref.alternating_case(64), ref.repeated_case(129)):
        ok = ref.feasible(case)
        assert not all(ok)
        nll, grad = launch(ops, case, zero_infinity=False)
        for b in range(case.shape[0]):
            if not ok[b]:
                assert float(nll[b]) == float("inf") and not grad[b].any()
        nll = torch.where(torch.tensor(ok), nll, torch.zeros(()))
        check("zero_infinity=False", case, nll, grad)


# ---- (g) refusals: host argument checks, nothing is launched --------------------------------------------------------------------
@pytest.mark.parametrize("why,V,ldv,Lmax,blank", [("V=257", 257, 264, 4, 0), ("Lmax=513", 46, 48, 513, 45),
                                                  ("blank=V", 46, 48, 4, 46), ("blank=-1", 46, 48, 4, -1),
                                                  ("ldv<V", 46, 40, 4, 45)])
def test_bad_arguments_are_refused_before_any_launch(ops, why, V, ldv, Lmax, blank):
    B, T = 2, 8
    W = max(V, ldv)   # every buffer is large enough for either reading of the arguments
    lg = torch.zeros(B, T, W, device=DEV)
    labels = torch.full((B, Lmax), -100, dtype=torch.int32, device=DEV)
    labels[:, :2] = 1
    nll = torch.full((B,), -FILL, device=DEV)
    grad = torch.full((B, T, W), FILL, device=DEV)
    ws = torch.zeros(ops.ctc_workspace_bytes(B, T, Lmax) + GUARD, dtype=torch.uint8, device=DEV)
    tin = torch.full((B,), T, dtype=torch.int32, device=DEV)
    with pytest.raises(ops.CoralAmdError, match="ca_ctc_loss_fwd_bwd"):
        ops.ctc_loss_fwd_bwd(lg, labels, tin, nll, grad, None, ws, B, T, V, ldv, Lmax, blank)
    torch.cuda.synchronize()
    assert (grad == FILL).all() and (nll == -FILL).all() and not ws.any(), why
