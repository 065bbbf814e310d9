"""The CTC reference of tests/ctc_ref.py checked against three independent statements of the loss (no GPU): the golden
cases, brute force over every alignment, and the closed form of inputs with a single feasible alignment."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ctc_ref as ref  # noqa: E402


def test_ctc_ref_reproduces_the_golden_cases(golden_dir):
    z = np.load(golden_dir / "ctc_cases.npz")
    assert int(z["n_cases"]) > 0
    for i in range(int(z["n_cases"])):
        lg = torch.tensor(z[f"c{i}_logits"])
        T, V = lg.shape
        tg = [int(c) for c in z[f"c{i}_targets"]]
        nll, grad = ref.ctc_ref(lg[None], [tg], [int(z[f"c{i}_tin"])], V - 1)
        want = float(z[f"c{i}_loss"])
        assert abs(float(nll[0]) - want) <= 1e-4 * max(1.0, abs(want)), (i, float(nll[0]), want)
        np.testing.assert_allclose(grad[0].numpy(), z[f"c{i}_grad"], atol=3e-5, rtol=1e-3)


TINY = [  # (T, in_len, targets, blank)
    (1, 1, (), 0), (1, 1, (1,), 0), (3, 3, (), 2), (4, 4, (1,), 0), (5, 5, (1, 2), 0), (5, 5, (1, 1), 0),
    (5, 5, (2, 2, 1), 0), (5, 5, (0, 0), 1), (5, 5, (0, 2, 0), 1), (5, 4, (1, 1), 2), (5, 3, (0, 1, 0), 2),
    (5, 5, (1, 1, 1), 0), (5, 2, (1, 1), 0), (5, 5, (1, 2, 1, 2, 1), 0),
]


@pytest.mark.parametrize("T,in_len,tg,blank", TINY)
def test_ctc_ref_equals_brute_force_over_all_alignments(T, in_len, tg, blank):
    for seed in range(3):
        lg = torch.randn(T, 3, generator=torch.Generator().manual_seed(100 * T + seed), dtype=torch.float64) * 1.5
        nll, grad = ref.ctc_ref(lg[None], [tg], [in_len], blank)
        bnll, bgrad = ref.brute_force(lg, tg, in_len, blank)
        if in_len < ref.min_frames(tg):
            assert float(bnll) == 0.0 and float(nll[0]) == 0.0 and not grad.any()
        assert abs(float(nll[0]) - float(bnll)) <= 1e-12, (float(nll[0]), float(bnll))
        assert float((grad[0] - bgrad).abs().max()) <= 1e-12
        assert not grad[0, in_len:].any()


@pytest.mark.parametrize("family", ["alternating", "repeated"])
@pytest.mark.parametrize("L", ref.SHARP_L)
def test_ctc_ref_equals_the_closed_form_on_single_path_inputs(family, L):
    case = ref.alternating_case(L) if family == "alternating" else ref.repeated_case(L)
    nll, grad = ref.ctc_ref(case.logits, case.targets, case.in_len, case.blank)
    assert ref.feasible(case) == [True, True, True, False]
    assert case.shape[1] == max(case.in_len) + 3
    snll, sgrad = ref.single_path(case.logits[0], case.paths[0], case.in_len[0])
    assert ref.collapse(case.paths[0][:case.in_len[0]], case.blank) == list(case.targets[0])
    assert abs(float(nll[0]) - float(snll)) <= 1e-10, (float(nll[0]), float(snll))
    assert float((grad[0] - sgrad).abs().max()) <= 1e-10
    assert float(nll[3]) == 0.0 and not grad[3].any()   # one frame short: infeasible
    assert (nll[:3] > 0).all()
    for b in range(4):
        assert not grad[b, max(case.in_len[b], 0):].any()


def test_the_seeded_cases_are_what_the_gpu_tests_assume():
    for blank in (45, 0):
        case = ref.mixed_case(blank)
        assert ref.feasible(case) == [True] * 9 + [False]
        assert all(c != blank and 0 <= c < 46 for tg in case.targets for c in tg)
        nll, grad, e32 = ref.reference(case)
        assert (nll[:9] > 0).all() and float(nll[9]) == 0.0 and not grad[9].any()
        assert torch.isfinite(grad).all() and float(e32.max()) < 1e-2
    assert ref.mixed_case(45) is ref.mixed_case(45)               # built once, shared
    for V in ref.WIDE_V:
        case = ref.wide_case(V)
        assert all(ref.feasible(case)) and all(c != V // 2 and 0 <= c < V for tg in case.targets for c in tg)
    for case in [ref.largest_case(), ref.largest_case_short_labels()] + [ref.lds_boundary_case(i) for i in range(3)]:
        assert all(ref.feasible(case))
    T, V = ref.lds_boundary_case(0).shape[1:]
    assert T * V * 4 == 120 * 1024
