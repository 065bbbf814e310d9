"""ca_resample on the GPU (coral_amd/csrc/resample.hip) against the float64 restatement of tests/resample_ref.py.

The bound is derived, not measured: for any summation order of K fp32 products of fp32-rounded taps,
    |y_gpu[n] - y_ref[n]| <= (K + 2) * 2^-23 * A[n],   A[n] = sum_k |h_k x_k|
(gamma_{K+1} of the running-error bound, doubled).  Lengths are exact, routes and runs give identical bits.

Row lengths: per ratio the shortest inputs whose output lengths reach CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 3.  When
the rate goes down every output length exists and these are met exactly (with Nw * len no multiple of O: the ceil
rounds); when it goes up (8 000 and 11 025 Hz) some lengths do not exist (8 kHz gives even lengths only) and the next one
that does is taken."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0


def _chunk():
    from coral_amd import _lib

    return _lib.RESAMPLE_CHUNK


def _route1_fits(p) -> bool:
    from coral_amd import _lib

    window = 4 * (-((-_lib.RESAMPLE_CHUNK * p.O) // p.Nw) + p.K + 1)
    return window + 4 * p.Nw * (p.K | 1) <= _lib.RESAMPLE_LDS_BYTES


def _shortest_input(p, n_out: int) -> int:
    n = -((-n_out * p.O) // p.Nw)
    while n > 0 and p.out_length(n - 1) >= n_out:
        n -= 1
    return n


def _signals(lengths, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return [rng.integers(-32768, 32768, n).astype(np.int16) for n in lengths]
    return [rng.standard_normal(n).astype(np.float32) for n in lengths]


_REFS: dict = {}


def _reference(key, xs, src, L):
    """(y, bound, K) per row, computed once per key and left unchanged."""
    if key not in _REFS:
        out = []
        for x in xs:
            y, A, K = rref.resample(x, src, 16_000, L, 0.99, int16=x.dtype == np.int16)
            out.append((y, rref.bound(A, K)))
        _REFS[key] = out
    return _REFS[key]


def _run(xs, p, route, ld_in=None, ld_out=None, rows=None, batch=None, guard=0):
    """Stage `xs` as rows 0.. of a [batch, ld_in] buffer whose padding is NaN (fp32) or 32767 (int16), run ca_resample,
    -> (y [batch, ld_out] with SENTINEL where nothing was written, len_out with -7 likewise, the guard floats behind y)."""
    from coral_amd import ops

    dtype = xs[0].dtype
    B = batch or len(xs)
    ld_in = ld_in or max(len(x) for x in xs) + 37
    host = np.full((B, ld_in), 32767 if dtype == np.int16 else np.nan, dtype)
    for i, x in enumerate(xs):
        host[i, :len(x)] = x
    n_out = [p.out_length(len(x)) for x in xs]
    ld_out = ld_out or max(n_out) + 5
    src = torch.from_numpy(host).to(DEV)
    len_in = torch.tensor([len(x) for x in xs] + [0] * (B - len(xs)), dtype=torch.int32).to(DEV)
    flat = torch.full((B * ld_out + guard,), SENTINEL, dtype=torch.float32, device=DEV)
    y = flat[:B * ld_out].view(B, ld_out)
    len_out = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    taps, off = p.device_tables(DEV)
    rows_t = None if rows is None else torch.tensor(rows, dtype=torch.int32).to(DEV)
    ops.resample(src, len_in, rows_t, len(rows) if rows is not None else B, taps, off, p.O, p.Nw, p.K, y, len_out,
                 route=route)
    torch.cuda.synchronize()
    return y.cpu().numpy(), len_out.cpu().numpy(), flat[B * ld_out:].cpu().numpy()


def _check_row(y_row, n_written, ref, worst):
    y_ref, bnd = ref
    n = min(n_written, len(y_ref))
    assert np.isfinite(y_row).all()
    err = np.abs(y_row[:n].astype(np.float64) - y_ref[:n])
    assert np.all(err <= bnd[:n]), (int(np.argmax(err - bnd[:n])), float(err.max()))
    assert np.all(y_row[n:] == 0)
    used = err[bnd[:n] > 0] / bnd[:n][bnd[:n] > 0]
    return max(worst, float(used.max()) if len(used) else 0.0)


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
@pytest.mark.parametrize("L", [6, 32])
@pytest.mark.parametrize("src", [48_000, 44_100, 11_025, 8_000])
def test_against_reference_every_route(src, L, dtype):
    from coral_amd import resample as rs

    p = rs.plan(src, 16_000, L, 0.99)
    C = _chunk()
    lengths = [_shortest_input(p, n) for n in (C - 1, C, C + 1, 2 * C + 3)]
    n_out = [p.out_length(n) for n in lengths]
    if p.O > p.Nw:
        assert n_out == [C - 1, C, C + 1, 2 * C + 3]
        assert any((p.Nw * n) % p.O for n in lengths)  # the ceil rounds
    xs = _signals(lengths, dtype, seed=src + L)
    refs = _reference((src, L, np.dtype(dtype).name), xs, src, L)
    assert all(len(r[0]) == n for r, n in zip(refs, n_out))
    routes = [2, 2, 0] + ([1] if _route1_fits(p) else [])
    base, worst = None, 0.0
    for route in routes:
        y, len_out, _ = _run(xs, p, route)
        assert len_out.tolist() == n_out
        if base is None:
            base = y
            for i in range(len(xs)):
                worst = _check_row(y[i], n_out[i], refs[i], worst)
        else:  # another route, or the same again: identical bits
            assert np.array_equal(base.view(np.uint32), y.view(np.uint32)), route
    print(f"{src} Hz, L = {L}, {np.dtype(dtype).name}: K = {p.K}, routes {routes}, largest share of the bound {worst:.3f}")
    if not _route1_fits(p):
        from coral_amd import ops

        with pytest.raises(ops.CoralAmdError, match="route 1"):
            _run(xs, p, 1)


@pytest.mark.parametrize("src", [48_000, 8_000])
def test_short_rows(src):
    from coral_amd import resample as rs

    p = rs.plan(src, 16_000, 32, 0.99)
    xs = _signals([0, 1, 2, p.K - 1], np.float32, seed=5)
    refs = _reference((src, "short"), xs, src, 32)
    for route in (2, 1):
        y, len_out, _ = _run(xs, p, route)
        assert len_out.tolist() == [0] + [p.out_length(n) for n in (1, 2, p.K - 1)]
        assert np.all(y[0] == 0)
        for i in range(4):
            _check_row(y[i], int(len_out[i]), refs[i], 0.0)


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
def test_truncation_writes_nothing_past_the_rows(dtype):
    from coral_amd import resample as rs

    p = rs.plan(44_100, 16_000, 6, 0.99)
    C = _chunk()
    xs = _signals([4000, 3 * C, 10], dtype, seed=9)  # 1452, 1115 and 4 outputs
    refs = _reference(("trunc", np.dtype(dtype).name), xs, 44_100, 6)
    ld_out = C + 7
    for route in (1, 2):
        y, len_out, guard = _run(xs, p, route, ld_in=5000, ld_out=ld_out, guard=256)
        assert len_out.tolist() == [min(len(r[0]), ld_out) for r in refs] == [ld_out, ld_out, 4]
        assert np.all(guard == SENTINEL)
        for i in range(3):
            _check_row(y[i], int(len_out[i]), refs[i], 0.0)


def test_rows_leave_the_other_rows_alone():
    from coral_amd import resample as rs

    p = rs.plan(48_000, 16_000, 6, 0.99)
    xs = _signals([5000, 7000, 3333], np.float32, seed=11)
    refs = _reference("rows", xs, 48_000, 6)
    y, len_out, _ = _run(xs, p, 0, rows=[2, 0])
    assert len_out.tolist() == [p.out_length(5000), -7, p.out_length(3333)]
    assert np.all(y[1] == SENTINEL)
    for i in (0, 2):
        _check_row(y[i], int(len_out[i]), refs[i], 0.0)


def test_a_table_whose_offsets_do_not_follow_the_outputs_is_served_from_global_memory():
    """`off` reaches the C ABI from outside: with offsets that jump back and forth an output's taps leave the chunk's LDS
    window, and the kernel reads those samples (masked) from global memory - the same sums, nothing out of bounds."""
    from types import SimpleNamespace

    O, Nw, K = 2, 3, 5
    rng = np.random.default_rng(19)
    taps = rng.standard_normal((Nw, K)).astype(np.float32)
    off = np.array([7, -9, 2500], np.int32)
    tables = (torch.from_numpy(taps).to(DEV), torch.from_numpy(off).to(DEV))
    p = SimpleNamespace(O=O, Nw=Nw, K=K, out_length=lambda n: -((-Nw * n) // O), device_tables=lambda dev: tables)
    x = rng.standard_normal(3001).astype(np.float32)
    n = np.arange(p.out_length(len(x)), dtype=np.int64)
    idx = ((n // Nw) * O + off[n % Nw])[:, None] + np.arange(K)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    prod = taps[n % Nw].astype(np.float64) * np.where(ok, x[np.clip(idx, 0, len(x) - 1)], 0.0)
    ref = (prod.sum(axis=1), rref.bound(np.abs(prod).sum(axis=1), K))
    y2, len_out, _ = _run([x], p, 2)
    assert len_out.tolist() == [len(n)] == [4502]
    _check_row(y2[0], len(n), ref, 0.0)
    y1, _, _ = _run([x], p, 1)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))


def test_identity_plan_is_an_exact_copy():
    from coral_amd import resample as rs

    p = rs.plan(16_000, 16_000)
    C = _chunk()
    xs = _signals([0, 1, C + 1, 2 * C - 1], np.float32, seed=13)
    xs[2][0] = -0.0  # a negative zero keeps its sign bit too
    for route in (0, 1, 2):
        y, len_out, _ = _run(xs, p, route)
        assert len_out.tolist() == [len(x) for x in xs]
        for i, x in enumerate(xs):
            assert np.array_equal(y[i, :len(x)].view(np.uint32), x.view(np.uint32)) and np.all(y[i, len(x):] == 0)
    xi = _signals([3, C, C + 5], np.int16, seed=14)
    xi[1][:2] = (-32768, 32767)
    y, len_out, _ = _run(xi, p, 0)
    for i, x in enumerate(xi):
        assert np.array_equal(y[i, :len(x)], x.astype(np.float32) / np.float32(32768.0))


def test_rows_behind_two_to_the_31_elements():
    """64-bit indexing: row 2 of a batch whose rows are 2^30 + 3 samples apart, in and out (the input is int16, 6.4 GB of
    untouched device memory; only row 2 is served, its zero tail included)."""
    from coral_amd import ops
    from coral_amd import resample as rs

    p = rs.plan(48_000, 16_000, 6, 0.99)
    ld = (1 << 30) + 3
    x = _signals([6001], np.int16, seed=15)[0]
    ref = _reference("far", [x], 48_000, 6)[0]
    src = torch.empty(3, ld, dtype=torch.int16, device=DEV)
    src[2, :8000] = 32767
    src[2, :len(x)] = torch.from_numpy(x).to(DEV)
    len_in = torch.tensor([0, 0, len(x)], dtype=torch.int32).to(DEV)
    y = torch.empty(3, ld, dtype=torch.float32, device=DEV)
    y[2, :4096] = SENTINEL
    y[2, -4096:] = SENTINEL
    len_out = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    taps, off = p.device_tables(DEV)
    ops.resample(src, len_in, torch.tensor([2], dtype=torch.int32).to(DEV), 1, taps, off, p.O, p.Nw, p.K, y, len_out)
    torch.cuda.synchronize()
    assert len_out.tolist() == [-7, -7, 2001]
    _check_row(y[2, :4096].cpu().numpy(), 2001, ref, 0.0)
    assert bool((y[2, -4096:] == 0).all())


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "fp32"])
def test_resample_function_ragged_mixed_rates(dtype):
    from coral_amd import resample as rs

    rates = [48_000, 16_000, 44_100, 8_000]
    xs = _signals([7001, 1234, 5000, 999], dtype, seed=17)
    got = rs.resample(xs, rates, device=DEV)
    on_device = rs.resample(xs, rates, device=DEV, to_host=False)
    for x, r, y, yd in zip(xs, rates, got, on_device):
        y_ref, A, K = rref.resample(x, r, 16_000, 32, 0.99, int16=dtype == np.int16)
        assert y.dtype == np.float32 and y.shape == y_ref.shape == tuple(yd.shape)
        assert np.array_equal(y, yd.cpu().numpy())
        if r == 16_000:
            assert np.array_equal(y, x.astype(np.float32) / np.float32(32768.0) if dtype == np.int16 else x)
        else:
            assert np.all(np.abs(y - y_ref) <= rref.bound(A, K))
    one = rs.resample(xs[:1], 48_000, device=DEV, lowpass_filter_width=6)[0]  # one rate for all, torchaudio's width
    y_ref, A, K = rref.resample(xs[0], 48_000, 16_000, 6, 0.99, int16=dtype == np.int16)
    assert K == 37 and np.all(np.abs(one - y_ref) <= rref.bound(A, K))
