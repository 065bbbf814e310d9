"""csrc/norm.hip on a real MI355X against the float64 references and derived bounds of tests/norm_ref.py (proved on the
CPU in tests/test_norm_ref_cpu.py): the LayerNorm forward in all its forms with its saved statistics, the backward with
its row pipeline running (more than one row per wave), every template width, the partial-sum reductions including the
few-parts kernel, the column sums and the two element-wise kernels past their grid-stride threshold.  `-m gpu` only.

Every comparison prints `ratio <kernel> <largest error / bound>`; a ratio above 1 fails.

Which test reaches which path (each asserts the regime it depends on):
  backward row rotation (rows > 4 * grid)          test_layernorm_bwd_row_pipeline, test_layernorm_bwd_dropout_form
  forward grid-stride loop (rows > 16384)          test_layernorm_fwd_grid_stride_loop, test_layernorm_fwd_fp8_grid_stride_loop
  NCH = 3 and NCH = 8 (C = 2056, 4096: 128 KiB LDS)  every forward test over R.C_LIST, test_layernorm_bwd_row_pipeline,
                                                   test_layernorm_bwd_every_width_and_the_forward_kernels_statistics
  saved statistics                                 check_stats in every forward test
  large-offset rows under a derived bound          the 'mixed' matrices everywhere, ..._large_offset_rows_alone
  reduce_few_parts_kernel, tail, fallback, in place  test_reduce_few_parts_kernel(_in_place), test_reduce_boundaries_...
  colsum with ld > N, offsets, long and short slabs  test_colsum
  element-wise grid-stride loops (n > 16 777 216)  test_dgelu_mul, test_dropout
Not reached: the non-DPP backward variant (CA_LN_BWD_DPP is read once per process, so a test that set it would test
nothing)."""
import collections
import math

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
U = R.U
RATIOS = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield o
    for k in sorted(RATIOS):
        print("largest ratio %-28s %.3f" % (k, RATIOS[k]))


def within(name, got, ref, bound):
    """assert |got - ref| <= bound element-wise (an exact result is inside a zero bound) and keep the largest ratio."""
    err = (R.f64(got) - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(err, bound)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = float(torch.nan_to_num(r, nan=math.inf).max())
    RATIOS[name] = max(RATIOS[name], r)
    print("ratio %s %.3f" % (name, r))
    assert r <= 1.0, (name, r)


def grid_cap(ops, C):
    """The backward's grid cap as the library reports it (so CA_LN_BWD_GRID cannot move a case out of its regime)."""
    return ops.layernorm_bwd_partial_floats(10 ** 7, C) // (2 * C)


def dev(t):
    return None if t is None else t.to(DEV)


# ---- forward ---------------------------------------------------------------------------------------------------------
def run_fwd(ops, x, gamma, beta, act, y_dtype, stats=True):
    rows, C = x.shape
    y = torch.full((rows, C), 7.0, dtype=y_dtype, device=DEV)
    st = torch.full((rows, 2), 7.0, dtype=torch.float32, device=DEV) if stats else None
    ops.layernorm_fwd(dev(x), dev(gamma), dev(beta), y, st, rows, C, EPS, act)
    torch.cuda.synchronize()
    return y.cpu(), (st.cpu() if stats else None)


def check_stats(name, st, x):
    _, mean, rstd = R.ln_fwd_ref(x, torch.ones(x.shape[1]), torch.zeros(x.shape[1]), EPS, 0)
    ms, rs = R.fwd_stats_slack(x, EPS)
    within(name + ".mean", st[:, 0], mean, ms)
    within(name + ".rstd", st[:, 1], rstd, rs)


def check_constant_rows(x, y, st, beta, act):
    """Family (c): x - mean is exactly 0, so y is beta rounded to the output type bit for bit, mean is the value and rstd is
    rsqrt(eps) within fp32 rounding (eps as the fp32 the kernel receives, its addition to 0, a 1-ulp rsqrt: 3 u)."""
    xf = x.float()
    const = (xf == xf[:, :1]).all(1)
    if not const.any() or x.shape[1] == 1:
        return 0
    if not act:
        assert torch.equal(y[const], beta.to(y.dtype).expand(int(const.sum()), -1))
    if st is not None:
        assert torch.equal(st[const, 0], xf[const, 0])
        want = 1.0 / math.sqrt(float(torch.tensor(EPS, dtype=torch.float32)))
        assert float((st[const, 1].double() - want).abs().max()) <= 3 * U * want
    return int(const.sum())


def check_fwd(ops, name, x, gamma, beta, act, y_dtype):
    y, st = run_fwd(ops, x, gamma, beta, act, y_dtype)
    yr, _, _ = R.ln_fwd_ref(x, gamma, beta, EPS, act)
    within(name + ".y", y, yr, R.fwd_y_bound(x, gamma, beta, EPS, act, y_dtype == torch.bfloat16))
    check_stats(name, st, x)
    y2, _ = run_fwd(ops, x, gamma, beta, act, y_dtype, stats=False)   # stats = NULL: the same y
    assert torch.equal(y.view(torch.int16 if y_dtype == torch.bfloat16 else torch.int32),
                       y2.view(torch.int16 if y_dtype == torch.bfloat16 else torch.int32))
    return check_constant_rows(x, y, st, beta, act)


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1031])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", R.C_LIST)
def test_layernorm_fwd_bf16(ops, C, act, rows):
    """ca_layernorm_fwd at both ends of every template width: y and the saved statistics against float64, on a matrix that
    mixes large-offset, constant and outlier rows into N(0, 2) ones, with the plain and the zero / negative gamma."""
    x = R.make_x(rows, C, "mixed")
    nconst = 0
    for gam in ("plain", "e"):
        gamma, beta = R.make_affine(C, gam)
        nconst += check_fwd(ops, "ln_fwd", x, gamma, beta, act, torch.bfloat16)
    assert nconst > 0 or rows < 5   # (the last row is a large-offset one)


@pytest.mark.parametrize("fam", ["b300", "b30"])
@pytest.mark.parametrize("C", R.C_LIST)
def test_layernorm_fwd_bf16_large_offset_rows_alone(ops, C, fam):
    gamma, beta = R.make_affine(C)
    for act in (0, 1):
        check_fwd(ops, "ln_fwd", R.make_x(1031, C, fam), gamma, beta, act, torch.bfloat16)


FP32_FORMS = [(True, True), (True, False), (False, True)]


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1031])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("x32,y32", FP32_FORMS)
@pytest.mark.parametrize("C", [c for c in R.C_LIST if c <= 1024])
def test_layernorm_fwd_fp32_forms(ops, C, x32, y32, act, rows):
    """ca_layernorm_fwd_ex: fp32 on either side.  An fp32 y has no rounding allowance at all: slack only."""
    x = R.make_x(rows, C, "mixed", fp32=x32)
    ydt = torch.float32 if y32 else torch.bfloat16
    for gam in ("plain", "e"):
        gamma, beta = R.make_affine(C, gam)
        check_fwd(ops, "ln_fwd_ex(x32=%d,y32=%d)" % (x32, y32), x, gamma, beta, act, ydt)
    if x32:
        gamma, beta = R.make_affine(C)
        check_fwd(ops, "ln_fwd_ex(x32=%d,y32=%d)" % (x32, y32), R.make_x(rows, C, "b1000", fp32=True), gamma, beta, act, ydt)


@pytest.mark.parametrize("x32,y32", [(False, False)] + FP32_FORMS)
@pytest.mark.parametrize("C", [72, 520])
def test_layernorm_fwd_grid_stride_loop(ops, C, x32, y32):
    """More rows than 4 * the forward's 4096-block cap: some waves normalise a second row."""
    rows = 16384 + 5
    assert rows > 16384
    x = R.make_x(rows, C, "mixed", fp32=x32)
    gamma, beta = R.make_affine(C)
    name = "ln_fwd_ex(x32=%d,y32=%d)" % (x32, y32) if (x32 or y32) else "ln_fwd"
    for act in (0, 1):
        check_fwd(ops, name, x, gamma, beta, act, torch.float32 if y32 else torch.bfloat16)


def check_fp8(ops, x, gamma, beta):
    rows, C = x.shape
    y0, _ = run_fwd(ops, x, gamma, beta, 0, torch.bfloat16, stats=False)
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    outs = []
    for with_y, with_stats in ((True, True), (False, False)):   # y and stats may be NULL
        y = torch.full((rows, C), 7.0, dtype=torch.bfloat16, device=DEV) if with_y else None
        st = torch.full((rows, 2), 7.0, dtype=torch.float32, device=DEV) if with_stats else None
        q = torch.zeros(rows, C, dtype=torch.uint8, device=DEV)
        rs = torch.zeros(rows, dtype=torch.float32, device=DEV)
        ops.layernorm_fwd_fp8(xd, gd, bd, y, q, rs, rows, C, EPS, stats=st)
        torch.cuda.synchronize()
        outs.append((q.cpu(), rs.cpu()))
        if with_y:
            assert torch.equal(y.cpu().view(torch.int16), y0.view(torch.int16))
            check_stats("ln_fwd_fp8", st.cpu(), x)
    yf = y0.float()
    am = yf.abs().amax(dim=1, keepdim=True)
    assert float(am.min()) > 0
    qr = (yf * (torch.tensor(448.0) / am)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    for q, rs in outs:
        assert torch.equal(q, qr)
        assert torch.allclose(rs, (am / 448.0).squeeze(1), rtol=1e-7, atol=0)
    yr, _, _ = R.ln_fwd_ref(x, gamma, beta, EPS, 0)
    within("ln_fwd_fp8.y", y0, yr, R.fwd_y_bound(x, gamma, beta, EPS, 0, True))


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1031])
@pytest.mark.parametrize("C", [c for c in R.C_LIST if c % 16 == 0])
def test_layernorm_fwd_fp8(ops, C, rows):
    """ca_layernorm_fwd_fp8 at every width it accepts (C % 16 == 0): the bf16 y is ca_layernorm_fwd's bit for bit, the
    bytes and row scales follow from that y exactly, the statistics meet the float64 bound."""
    check_fp8(ops, R.make_x(rows, C, "mixed"), *R.make_affine(C))


@pytest.mark.parametrize("C", [80, 528])
def test_layernorm_fwd_fp8_grid_stride_loop(ops, C):
    """(C = 72 and 520 of the other forms are no multiples of 16; these are the next ones.)"""
    rows = 16384 + 5
    assert rows > 16384
    check_fp8(ops, R.make_x(rows, C, "mixed"), *R.make_affine(C))


# ---- backward --------------------------------------------------------------------------------------------------------
def fp64_stats(x):
    _, mean, rstd = R.ln_fwd_ref(x, torch.ones(x.shape[1]), torch.zeros(x.shape[1]), EPS, 0)
    return torch.stack([mean.float(), rstd.float()], 1).contiguous()


def run_bwd(ops, dy, x, gamma, beta, st, dres, act, how, init):
    """how: 'adjacent' (d gamma | d beta in one buffer: the single-launch reduction), 'separate', or 'none' (the partials
    are returned as [grid, 2, C] instead)."""
    rows, C = x.shape
    n = ops.layernorm_bwd_partial_floats(rows, C)
    part = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    dx = torch.full((rows, C), 7.0, dtype=torch.bfloat16, device=DEV)
    if how == "adjacent":
        buf = torch.full((2 * C,), init, dtype=torch.float32, device=DEV)
        dg, db = buf[:C], buf[C:]
    elif how == "separate":
        dg = torch.full((C,), init, dtype=torch.float32, device=DEV)
        db = torch.full((C + 4,), init, dtype=torch.float32, device=DEV)[4:]
    else:
        dg = db = None
    ops.layernorm_bwd(dev(dy), dev(x), dev(gamma), dev(beta), dev(st), dev(dres), dx, dg, db, part, rows, C, act)
    torch.cuda.synchronize()
    if how == "none":
        return dx.cpu(), part.cpu().view(n // (2 * C), 2, C)
    return dx.cpu(), dg.cpu(), db.cpu()


def check_bwd(ops, name, dy, x, gamma, beta, st, dres, act, arrangements=("adjacent", "separate", "none")):
    rows, C = x.shape
    grid = ops.layernorm_bwd_partial_floats(rows, C) // (2 * C)
    mean, rstd = st[:, 0], st[:, 1]
    dxr, dgr, dbr = R.ln_bwd_ref(dy, x, gamma, beta, mean, rstd, dres, act)
    b = R.bwd_bounds(dy, x, gamma, beta, mean, rstd, dres, act, 0)
    for how in arrangements:
        use_dres = how != "separate"   # 'separate' also runs without the residual gradient
        init = {"adjacent": 1.0, "separate": 0.5, "none": None}[how]
        chain = R.bwd_chain(rows, grid, how != "none")
        bg, bb = R.param_grad_bound(b, "dgamma", chain, init), R.param_grad_bound(b, "dbeta", chain, init)
        out = run_bwd(ops, dy, x, gamma, beta, st, dres if use_dres else None, act, how, init or 0.0)
        if use_dres:
            within(name + ".dx", out[0], dxr, b["dx"])
        else:
            within(name + ".dx", out[0], dxr - R.f64(dres), b["dx_nores"])
        if how == "none":
            part = R.f64(out[1])
            assert part.shape[0] == grid
            within(name + ".partials", part[:, 0].sum(0), dgr, bg)
            within(name + ".partials", part[:, 1].sum(0), dbr, bb)
        else:
            within(name + ".dgamma", R.f64(out[1]) - init, dgr, bg)
            within(name + ".dbeta", R.f64(out[2]) - init, dbr, bb)


ROW_KEYS = {"1": (0, 1), "5": (0, 5), "4g-3": (4, -3), "4g": (4, 0), "4g+1": (4, 1), "8g": (8, 0), "8g+5": (8, 5),
            "12g+2": (12, 2)}
# one width per template instantiation (and the fp32-x forms of the first two); widths no model has stop at 4g + 1
PIPELINE_CASES = [(C, x32, key) for C, x32 in [(264, False), (520, False), (1032, False), (1544, False), (2056, False),
                                                (4096, False), (264, True), (520, True)]
                  for key in ROW_KEYS if C <= 2048 or ROW_KEYS[key][0] <= 4]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C,x32,key", PIPELINE_CASES)
def test_layernorm_bwd_row_pipeline(ops, C, x32, key, act):
    """ca_layernorm_bwd / _ex at one width per template instantiation, with one, exactly four * grid, one more (a single
    wave rotates its prefetched row in), and two and three ragged passes of rows per wave.  Statistics computed in
    float64 and rounded to fp32, so nothing of the forward can mask the backward."""
    g = grid_cap(ops, C)
    rows = ROW_KEYS[key][0] * g + ROW_KEYS[key][1]
    if key in ("4g+1", "8g", "8g+5", "12g+2"):
        assert rows > 4 * g and ops.layernorm_bwd_partial_floats(rows, C) // (2 * C) == g
    x = R.make_x(rows, C, "mixed", fp32=x32)
    gamma, beta = R.make_affine(C, "e" if key in ("5", "4g", "8g", "12g+2") else "plain")
    dy, dres = R.make_dy(rows, C), R.make_dy(rows, C, seed=5)
    check_bwd(ops, "ln_bwd_ex(x32)" if x32 else "ln_bwd", dy, x, gamma, beta, fp64_stats(x), dres, act)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", R.C_LIST)
def test_layernorm_bwd_every_width_and_the_forward_kernels_statistics(ops, C, act):
    """Every width at 1031 rows, large-offset rows alone and mixed, with float64 statistics and with the statistics the
    forward kernel saved: the result must then be the backward OF THOSE statistics (the reference takes them as given)."""
    rows = 1031
    dy, dres = R.make_dy(rows, C), R.make_dy(rows, C, seed=5)
    for fam, gam in (("mixed", "plain"), ("b300", "e")):
        x = R.make_x(rows, C, fam)
        gamma, beta = R.make_affine(C, gam)
        check_bwd(ops, "ln_bwd", dy, x, gamma, beta, fp64_stats(x), dres, act, ("adjacent",))
        _, st = run_fwd(ops, x, gamma, beta, act, torch.bfloat16)
        check_bwd(ops, "ln_bwd", dy, x, gamma, beta, st, dres, act, ("separate", "none"))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", [264, 1024])
def test_layernorm_bwd_fp32_rows_with_the_forward_kernels_statistics(ops, C, act):
    rows = 1031
    dy, dres = R.make_dy(rows, C), R.make_dy(rows, C, seed=5)
    x = R.make_x(rows, C, "mixed", fp32=True)
    gamma, beta = R.make_affine(C)
    _, st = run_fwd(ops, x, gamma, beta, act, torch.float32)
    check_bwd(ops, "ln_bwd_ex(x32)", dy, x, gamma, beta, st, dres, act)


@pytest.mark.parametrize("C,key", [(C, key) for C in (8, 520, 1280, 2056) for key in ("5", "4g+1", "8g+5")
                                   if C <= 2048 or key != "8g+5"])
def test_layernorm_bwd_dropout_form(ops, C, key):
    """ca_layernorm_bwd_dropout with more than one row per wave: dx, d gamma and d beta are the plain form's bit for bit,
    dx_drop is ca_dropout_bf16 of that dx bit for bit, every element of it is 0 or bf16(dx / (1 - p)) under the mask of
    (seed, flat index), and dx meets the float64 bound."""
    g = grid_cap(ops, C)
    rows = {"5": 5, "4g+1": 4 * g + 1, "8g+5": 8 * g + 5}[key]
    if key != "5":
        assert rows > 4 * g
    p, seed = 0.1, 0x5DEECE66D1234
    x, dy, dres = R.make_x(rows, C, "mixed"), R.make_dy(rows, C), R.make_dy(rows, C, seed=5)
    gamma, beta = R.make_affine(C)
    st = fp64_stats(x)
    dx0, dg0, db0 = run_bwd(ops, dy, x, gamma, beta, st, dres, 0, "adjacent", 1.0)
    part = torch.empty(ops.layernorm_bwd_partial_floats(rows, C), dtype=torch.float32, device=DEV)
    dx = torch.full((rows, C), 7.0, dtype=torch.bfloat16, device=DEV)
    dxd = torch.full((rows, C), 7.0, dtype=torch.bfloat16, device=DEV)
    buf = torch.ones(2 * C, dtype=torch.float32, device=DEV)
    ops.layernorm_bwd_dropout(dev(dy), dev(x), dev(gamma), dev(beta), dev(st), dev(dres), dx, dxd, p, seed, buf[:C], buf[C:],
                              part, rows, C)
    two = torch.empty_like(dx)
    ops.dropout(dx, two, rows * C, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu().view(torch.int16), dx0.view(torch.int16))
    assert torch.equal(buf[:C].cpu(), dg0) and torch.equal(buf[C:].cpu(), db0)
    assert torch.equal(dxd.view(torch.int16), two.view(torch.int16))
    keep = R.dropout_keep(seed, torch.arange(rows * C), p).view(rows, C)
    ks = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    want = torch.where(keep, (dx0.float() * ks).bfloat16(), torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(dxd.cpu().view(torch.int16), want.view(torch.int16))
    dxr, _, _ = R.ln_bwd_ref(dy, x, gamma, beta, st[:, 0], st[:, 1], dres, 0)
    within("ln_bwd_dropout.dx", dx0, dxr, R.bwd_bounds(dy, x, gamma, beta, st[:, 0], st[:, 1], dres, 0, 0)["dx"])


def test_layernorm_bwd_refuses_rows_wider_than_it_serves(ops):
    """The widest row is 4096 channels; more is an argument error, not a launch."""
    C, rows = 4104, 4
    z = torch.zeros(rows, C, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(C, dtype=torch.float32, device=DEV)
    st = torch.zeros(rows, 2, dtype=torch.float32, device=DEV)
    part = torch.zeros(2 * C, dtype=torch.float32, device=DEV)
    with pytest.raises(ops.CoralAmdError):
        ops.layernorm_bwd(z, z, f, f, st, None, torch.empty_like(z), f.clone(), f.clone(), part, rows, C, 0)
    with pytest.raises(ops.CoralAmdError):
        ops.layernorm_fwd(z, f, f, torch.empty_like(z), st, rows, C, EPS, 0)


# ---- partial-sum reductions ------------------------------------------------------------------------------------------------
def check_reduce(ops, name, nparts, n, stride, accumulate, out_off=0, in_place=False, seed=0):
    g = torch.Generator().manual_seed(seed + nparts * 131 + n)
    part = torch.randn(nparts * stride, generator=g)
    init = torch.randn(n + out_off, generator=g)
    pd = part.to(DEV)
    od = pd if in_place else init.to(DEV)
    ops.reduce_rows(pd, nparts, stride, n, od[out_off:], accumulate)
    torch.cuda.synchronize()
    p64 = R.f64(part).view(nparts, stride)[:, :n]
    ref, mass = p64.sum(0), p64.abs().sum(0)
    if accumulate:
        ref, mass = ref + R.f64(init[out_off:]), mass + R.f64(init[out_off:]).abs()
    within(name, od.cpu()[out_off:out_off + n], ref, R.sum_bound(mass, nparts))
    if in_place:   # nothing past the first slice moved
        assert torch.equal(od.cpu()[n:], part[n:])
    elif out_off:
        assert torch.equal(od.cpu()[:out_off], init[:out_off])


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n,stride", [(65536, 65536), (65536 + 3, 65540), (262144, 262144)])
@pytest.mark.parametrize("nparts", [1, 2, 16])
def test_reduce_few_parts_kernel(ops, nparts, n, stride, accumulate):
    """The split-K weight-gradient sum: nparts <= 16, n >= 65536, 16-byte alignment - with the scalar tail (n % 4 != 0)."""
    assert nparts <= 16 and n >= 65536 and stride % 4 == 0
    check_reduce(ops, "reduce_few_parts", nparts, n, stride, accumulate)


@pytest.mark.parametrize("n,stride", [(65536, 65536), (65536 + 3, 65540)])
@pytest.mark.parametrize("nparts", [1, 2, 16])
def test_reduce_few_parts_kernel_in_place(ops, nparts, n, stride):
    """reduce_rows(ws, splits, M * N, M * N, ws) as wgrad_gemm calls it: out is the first partial slice."""
    assert nparts <= 16 and n >= 65536
    check_reduce(ops, "reduce_few_parts", nparts, n, stride, False, in_place=True)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("nparts,n,out_off", [(17, 65536, 0), (16, 65532, 0), (16, 65536, 1), (2, 65539, 1)])
def test_reduce_boundaries_of_the_few_parts_choice(ops, nparts, n, out_off, accumulate):
    """One part too many, four columns too few, an output one float off 16-byte alignment: the many-parts kernel."""
    check_reduce(ops, "reduce_partials", nparts, n, (n + 3) // 4 * 4, accumulate, out_off=out_off)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("nparts", [15, 16, 17, 63, 64, 65, 500])
def test_reduce_many_parts_kernel(ops, nparts, n):
    """Both ends of the `p + 48 < nparts` unrolled loop and of the 64-column block."""
    for accumulate in (False, True):
        check_reduce(ops, "reduce_partials", nparts, n, n + 3, accumulate)


def test_reduce_rows_multi_is_bit_identical_to_reduce_rows(ops):
    g = torch.Generator().manual_seed(3)
    cases = [(65, 1, 1), (16, 65, 72), (500, 64, 64), (17, 1920, 3840)]
    parts = [torch.randn(p * s, generator=g).to(DEV) for p, _, s in cases]
    init = [torch.randn(n, generator=g).to(DEV) for _, n, _ in cases]
    for accumulate in (False, True):
        one = [t.clone() for t in init]
        for (p, n, s), pt, o in zip(cases, parts, one):
            ops.reduce_rows(pt, p, s, n, o, accumulate)
        multi = [t.clone() for t in init]
        ops.reduce_rows_multi([(pt, p, s, n, o, accumulate) for (p, n, s), pt, o in zip(cases, parts, multi)])
        torch.cuda.synchronize()
        for a, b in zip(one, multi):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- column sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("N", [8, 264, 1920])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 64, 65, 3992, 32768 + 77])
def test_colsum(ops, rows, N, wide):
    """ca_colsum_bf16 dense (ld == N) and as a column slice of a matrix three times as wide (ld = 3 N, x_off = N), without
    a mask, with a random one, an all-zero one and one whose only set row is the last; accumulate both ways, out_off = 8."""
    ld, x_off, out_off = (3 * N, N, 8) if wide else (N, 0, 0)
    g = torch.Generator(device=DEV).manual_seed(rows * 7 + N)
    xd = torch.randn(rows, ld, generator=g, device=DEV).bfloat16()
    x64 = xd[:, x_off:x_off + N].double()   # (the float64 sums of up to 63 M elements are taken on the GPU)
    nslab = ops.colsum_partial_floats(rows, N) // N
    if rows > 32768:
        assert -(-rows // nslab) > 64   # a slab longer than 64 rows: the four-in-flight loop and the tail in one slab
    part = torch.empty(nslab * N, dtype=torch.float32, device=DEV)
    last = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    last[-1] = 1
    masks = [None, (torch.rand(rows, generator=g, device=DEV) < 0.4).to(torch.uint8),
             torch.zeros(rows, dtype=torch.uint8, device=DEV), last]
    for k, mask in enumerate(masks):
        accumulate = bool(k % 2) != wide
        init = torch.randn(N + out_off, generator=g, device=DEV)
        out = init.clone()
        ops.colsum(xd.view(-1), ld, rows, N, out, part, accumulate=accumulate, rowmask=mask, x_off=x_off, out_off=out_off)
        torch.cuda.synchronize()
        xm = x64 if mask is None else x64 * mask.double()[:, None]
        ref, mass = xm.sum(0), xm.abs().sum(0)
        if accumulate:
            ref, mass = ref + init[out_off:].double(), mass + init[out_off:].double().abs()
        within("colsum", out[out_off:], ref.cpu(), R.sum_bound(mass, R.colsum_chain(rows, nslab)).cpu())
        assert torch.equal(out[:out_off], init[:out_off])


# ---- element-wise kernels ------------------------------------------------------------------------------------------------
STRIDE_N = 8192 * 256 * 8
ELEMENTWISE_N = [8, STRIDE_N + 8 * 1000]


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_dgelu_mul(ops, n):
    """ca_dgelu_mul below and past its grid-stride threshold (one stride plus a ragged remainder), against float64 on the
    GPU; u = 0, +-20 and +-inf and dy = 0 included: gelu' is 1 or 0 at infinity, never NaN."""
    if n > 8:
        assert n > STRIDE_N
    g = torch.Generator(device=DEV).manual_seed(n)
    dy = torch.randn(n, generator=g, device=DEV).bfloat16()
    u = (2.0 * torch.randn(n, generator=g, device=DEV)).bfloat16()
    special = torch.tensor([0.0, math.inf, -math.inf, 20.0, -20.0, 1.0, math.inf, -math.inf], device=DEV).bfloat16()
    for at in (0, n - 8):
        u[at:at + 8] = special
    dy[-8:] = torch.tensor([1.5, -2.0, 3.0, 0.5, -0.25, 0.0, 0.0, 0.0], device=DEV).bfloat16()
    out = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.dgelu_mul(dy, u, out, n)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    d64, u64 = dy.double(), u.double()
    err = (out.double() - d64 * R.dgelu64(u64)).abs()
    r = float((err / R.dgelu_mul_bound(d64, u64).clamp(min=1e-300)).max())
    RATIOS["dgelu_mul"] = max(RATIOS["dgelu_mul"], r)
    print("ratio dgelu_mul %.3f" % r)
    assert r <= 1.0
    assert out[-8:].float().tolist()[1:3] == [-2.0, 0.0] and out[0].item() == 0.5 * dy[0].item()


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_dropout(ops, n):
    """ca_dropout_bf16 below and past its grid-stride threshold: every element is 0 or bf16(x / (1 - p)) under the mask of
    (seed, flat index) - computed here from the hash's definition for ALL indices, those of the second stride included -
    the keep rate, p = 0, in place, and a second call on the leading slice (the mask of an element depends on its flat
    index in the call, so a prefix is the slice whose indices coincide)."""
    if n > 8:
        assert n > STRIDE_N
    p, seed = 0.1, 0x9E3779B97F4A7C15 >> 1
    x = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).bfloat16()
    x[x == 0] = 1.0
    y = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.dropout(x, y, n, p, seed)
    keep = R.dropout_keep(seed, torch.arange(n, device=DEV), p)
    one = torch.tensor(1.0, dtype=torch.float32)
    ks = (one / (one - torch.tensor(p, dtype=torch.float32))).item()
    want = torch.where(keep, (x.float() * ks).bfloat16(), torch.zeros((), dtype=torch.bfloat16, device=DEV))
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    if n > 8:
        q = 1.0 - int(p * 65536) / 65536
        assert abs(float((y != 0).double().mean()) - q) <= 4 * math.sqrt(q * (1 - q) / n)
        m = 8 * 4096 + 8
        head = torch.empty(m, dtype=torch.bfloat16, device=DEV)
        ops.dropout(x[:m], head, m, p, seed)
        assert torch.equal(head.view(torch.int16), y[:m].view(torch.int16))
    ident = torch.empty_like(x)
    ops.dropout(x, ident, n, 0.0, seed)
    assert torch.equal(ident.view(torch.int16), x.view(torch.int16))
    xin = x.clone()
    ops.dropout(xin, xin, n, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(xin.view(torch.int16), y.view(torch.int16))
