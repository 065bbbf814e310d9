"""tests/frontend_ref.py checked without a GPU: the float64 references against torch's own float64 operators, the derived
bounds against an fp32 emulation of the kernels' own order of operations (at most a quarter of each fp32 slack), and
against the wrong implementations they exist to reject, on inputs the GPU test uses."""
import pytest
import torch

import frontend_ref as F
import test_norm_ref_cpu as NE   # its fp32 emulations of ca_half_erfc's GELU and of reduce_partials_kernel
from norm_ref import BF16_HALF_ULP, f64

EPS = 1e-5
WEPS = 1e-7
F32 = torch.float32


def ratio(got, ref, bound):
    err = (f64(got) - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


# ---- fp32 emulations -----------------------------------------------------------------------------------------------------
def emu_wave512(t, squares=False):
    """[F, 512] -> [F]: lane l adds its channels 8 l .. 8 l + 7 in order (fused when they are squares), then wave_sum_dpp:
    quad swaps, row rotations by 4 and 8, and the four row totals pairwise."""
    s = torch.zeros(t.shape[0], 64, dtype=F32)
    t = t.view(-1, 64, 8)
    for e in range(8):
        s = fma(t[:, :, e], t[:, :, e], s) if squares else s + t[:, :, e]
    lane = torch.arange(64)
    s = s + s[:, lane ^ 1]
    s = s + s[:, lane ^ 2]
    for r in (4, 8):
        s = s + s[:, (lane & 48) | ((lane + r) & 15)]
    return (s[:, 0] + s[:, 16]) + (s[:, 32] + s[:, 48])


def emu_conv0(x, w, bias, gamma, beta, stride, dy=None, grid=4, init=0.0, wrong=None):
    """conv0_fwd_kernel's y (fp32, before its rounding to bf16) and, with dy, conv0_bwd_kernel + reduce_partials_kernel
    on `grid` workgroups.  wrong: 'bias' (uncentred bias), 'tap' (no last tap), 'hm2' (dv without h m2), 'block' (the
    second frame block dropped)."""
    B, N = x.shape
    T0 = F.conv0_frames(N, stride)
    inv = torch.tensor(1.0 / F.C0, dtype=F32)
    wc = w - (emu_wave512(w.t().contiguous()) * inv)[None, :]
    bc = bias if wrong == "bias" else bias - emu_wave512(bias[None, :]) * inv
    X = x.unfold(1, F.K0, stride)[:, :T0].reshape(-1, F.K0)
    v = bc[None, :].expand(X.shape[0], F.C0)
    for j in range(F.K0 - (wrong == "tap")):
        v = fma(wc[None, :, j], X[:, j:j + 1], v)
    rstd = torch.rsqrt(emu_wave512(v, squares=True) * inv + torch.tensor(EPS, dtype=F32))[:, None]
    h = v * rstd
    z = fma(h, gamma, beta)
    y = NE.emu_gelu(z).view(B, T0, F.C0)
    if dy is None:
        return y
    du = dy.float().view(-1, F.C0) * NE.emu_dgelu(z)
    dh = du * gamma
    m1, m2 = (emu_wave512(dh) * inv)[:, None], (emu_wave512(dh * h) * inv)[:, None]
    dv = rstd * (dh - m1 if wrong == "hm2" else dh - m1 - h * m2)
    # order[wg, wave, step]: the frame a wave adds at that step of its register accumulation, -1 for none
    bpu = -(-T0 // F.FPB)
    nblk = B * bpu
    passes = -(-nblk // grid)
    order = torch.full((grid, 4, passes * F.FPB // 4), -1, dtype=torch.int64)
    for wg in range(grid):
        for p, blk in enumerate(range(wg, nblk, grid)):
            if wrong == "block" and blk == 1:
                continue
            b, t0 = blk // bpu, (blk % bpu) * F.FPB
            for f in range(min(F.FPB, T0 - t0)):
                order[wg, f % 4, p * F.FPB // 4 + f // 4] = b * T0 + t0 + f
    acc = {"dw": torch.zeros(grid, 4, F.C0, F.K0), "dbias": torch.zeros(grid, 4, F.C0),
           "dgamma": torch.zeros(grid, 4, F.C0), "dbeta": torch.zeros(grid, 4, F.C0)}
    for s in range(order.shape[2]):
        idx = order[:, :, s]
        live = idx >= 0
        if not live.any():
            continue
        i = idx[live]
        acc["dgamma"][live] = acc["dgamma"][live] + du[i] * h[i]
        acc["dbeta"][live] = acc["dbeta"][live] + du[i]
        acc["dbias"][live] = acc["dbias"][live] + dv[i]
        acc["dw"][live] = fma(dv[i][:, :, None], X[i][:, None, :], acc["dw"][live])
    out = {"y": y}
    for key, a in acc.items():
        part = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
        flat = part.reshape(grid, -1)
        out[key] = NE.emu_reduce(flat, torch.full((flat.shape[1],), float(init)), True).view(part.shape[1:])
    return out


def emu_block_sum(t):
    """[B, N] -> [B]: the 1024-thread utterance sum: a thread adds every 1024th sample, wave butterflies, 16 waves."""
    B, N = t.shape
    pad = torch.zeros(B, -(-N // 1024) * 1024, dtype=F32)
    pad[:, :N] = t
    pad = pad.view(B, -1, 1024)
    s = torch.zeros(B, 1024, dtype=F32)
    for m in range(pad.shape[1]):
        s = s + pad[:, m]
    s = s.view(B, 16, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    tot = torch.zeros(B, dtype=F32)
    for wv in range(16):
        tot = tot + s[:, wv, 0]
    return tot


def emu_pcm(pcm, lengths, peak, znorm, one_pass=False, fused=False):
    """pcm_prepare_kernel (and wave_normalize_kernel: fp32, no peak).  one_pass: the variance as E[x^2] - mean^2; fused: the
    gain folded into the centring as fma(v, gain, -mean) - the two wrong implementations."""
    B, N = pcm.shape
    v = pcm.float() * (1.0 / 32768.0) if pcm.dtype == torch.int16 else pcm
    n = F._clamped(lengths, B, N)
    valid = torch.arange(N)[None, :] < n[:, None]
    v = torch.where(valid, v, torch.zeros(()))
    cnt = n.clamp(min=1).float()
    m = v.abs().amax(1)
    gain = torch.where((m > 0) & bool(peak), 1.0 / m, torch.ones(()))
    if not znorm:
        return v * gain[:, None]
    mean = (emu_block_sum(v) / cnt * gain)[:, None]
    xg = v * gain[:, None]
    if one_pass:
        var = emu_block_sum(xg * xg) / cnt - mean[:, 0] * mean[:, 0]
    else:
        d = torch.where(valid, fma(v, gain[:, None], -mean) if fused else xg - mean, torch.zeros(()))
        var = emu_block_sum(d * d) / cnt
    rstd = torch.where(n > 0, torch.rsqrt(var + torch.tensor(WEPS, dtype=F32)), torch.zeros(()))
    return torch.where(valid, (fma(v, gain[:, None], -mean) if fused else xg - mean) * rstd[:, None], torch.zeros(()))


def emu_tap_sums(terms, K, drop_slab=None):
    """[rows, K] fp32 products -> [K]: tap_dot_kernel's slab partials (256 / K row lanes, four accumulators over whole
    groups of four rows, the tail into the first) and tap_finish_kernel's fixed-order finish."""
    rows = terms.shape[0]
    per = -(-rows // F.PCW_SLABS)
    nrl = 256 // K
    steps = -(-per // nrl)
    slab_rows = (rows - torch.arange(F.PCW_SLABS) * per).clamp(0, per)                      # rows of each slab
    t = torch.zeros(F.PCW_SLABS, steps * nrl, K, dtype=F32)
    src = torch.arange(F.PCW_SLABS)[:, None] * per + torch.arange(steps * nrl)[None, :]
    ok = torch.arange(steps * nrl)[None, :] < slab_rows[:, None]
    t[ok] = terms[src[ok]]
    t = t.view(F.PCW_SLABS, steps, nrl, K)
    cnt = ((slab_rows[:, None] - torch.arange(nrl)[None, :] + nrl - 1) // nrl).clamp(min=0)  # rows of each row lane
    acc = [torch.zeros(F.PCW_SLABS, nrl, K, dtype=F32) for _ in range(4)]
    for i in range(steps):
        tgt = torch.where(i < cnt // 4 * 4, i % 4, 0)
        for a in range(4):
            acc[a] = acc[a] + torch.where((tgt == a)[:, :, None], t[:, i], torch.zeros(()))
    lane = (acc[0] + acc[1]) + (acc[2] + acc[3])
    part = torch.zeros(F.PCW_SLABS, K, dtype=F32)
    for q in range(nrl):
        part = part + lane[:, q]
    if drop_slab is not None:
        part[drop_slab] = 0
    return NE.emu_reduce(part, torch.zeros(K), False)


def emu_posconv_fwd(v, g, drop_slab=None):
    d, Cg, K = v.shape
    norm = torch.sqrt(emu_tap_sums((v * v).view(-1, K), K, drop_slab))
    return norm, v * (g / norm)


def emu_posconv_bwd(dw, v, g, norm, dv0, dg0, wrong=None):
    K = v.shape[2]
    dot = emu_tap_sums((v * dw).view(-1, K), K)
    grad = (g / norm) * (dw if wrong == "projection" else dw - v * dot / (norm * norm))
    if wrong == "overwrite":
        return grad, dot / norm
    return dv0 + grad, dg0 + dot / norm


def emu_col2im(dcol, L, stride, wrong=None, rounded=True):
    B, T, k, C = dcol.shape
    dx = torch.zeros(B, L, C, dtype=F32)
    for j in range(k):
        if wrong == "overlap" and j >= stride:
            continue
        dx[:, torch.arange(T) * stride + j] += dcol[:, :, j].float()
    return dx.bfloat16() if rounded else dx


# ---- the references against torch's float64 operators ------------------------------------------------------------------------
@pytest.mark.parametrize("stride,N", [(5, 653), (1, 40), (16, 300)])
def test_conv0_reference_agrees_with_float64_autograd(stride, N):
    B = 2
    x = F.make_conv0_x(B, N, "dc")
    w, bias, gamma, beta = (f64(t).requires_grad_(True) for t in F.make_conv0_params())
    T0 = F.conv0_frames(N, stride)
    dy = F.make_conv0_dy(B, T0)
    hcv = torch.nn.functional.conv1d(f64(x)[:, None, :], w[:, None, :], bias, stride=stride).transpose(1, 2)
    y = torch.nn.functional.gelu(torch.nn.functional.layer_norm(hcv, (F.C0,), gamma, beta, EPS))
    assert y.shape[1] == T0
    y.backward(f64(dy))
    r = F.conv0_ref(x, w, bias, gamma, beta, stride, EPS, dy=dy, batch=1)
    assert rel(r["y"], y.detach()) <= 1e-12
    for key, t in (("dw", w), ("dbias", bias), ("dgamma", gamma), ("dbeta", beta)):
        assert rel(r[key], t.grad) <= 1e-12, key


@pytest.mark.parametrize("B,L,C,k,s", F.COL2IM_SHAPES[:1] + F.COL2IM_SHAPES[2:5])
def test_col2im_reference_is_fold(B, L, C, k, s):
    T = (L - k) // s + 1
    dcol = F.make_dcol(B, T, C, k)
    dx, _, covered = F.col2im_ref(dcol, L, s)
    cols = f64(dcol).permute(0, 3, 2, 1).reshape(B, C * k, T)
    Lc = (T - 1) * s + k
    want = torch.nn.functional.fold(cols, (1, Lc), (1, k), stride=(1, s)).view(B, C, Lc).transpose(1, 2)
    assert rel(dx[:, :Lc], want) <= 1e-12
    assert not bool(covered[Lc:].any()) and float(dx[:, Lc:].abs().sum()) == 0.0
    if k < s:
        assert float(dx[:, 1::2].abs().sum()) == 0.0


def test_normalisation_reference_is_torchs():
    N = 1000
    lens = F.make_lengths(N)
    x = F.make_wave(8, N, "noise")
    y, mask, _ = F.pcm_ref(x, lens, False, True, WEPS)
    for b, n in enumerate(lens.clamp(max=N).tolist()):
        assert mask[b].tolist() == [1] * n + [0] * (N - n)
        assert float(y[b, n:].abs().sum()) == 0.0
        if n > 1:
            a = f64(x[b, :n])
            assert rel(y[b, :n], (a - a.mean()) / torch.sqrt(a.var(unbiased=False) + WEPS)) <= 1e-12
        else:
            assert float(y[b].abs().sum()) == 0.0
    p = F.make_pcm16(8, N)
    y, _, _ = F.pcm_ref(p, None, True, False, WEPS)
    assert float(y[6].abs().sum()) == 0.0 and float(y[2].min()) == -1.0
    assert rel(y[0], f64(p[0]) / f64(p[0]).abs().max()) <= 1e-12


def test_frame_lengths_reference():
    m = F.make_attention_mask(5, 16001)
    n = m.sum(1)
    for k, s in zip(F.CONV_KERNELS, F.CONV_STRIDES):
        n = torch.div(n - k, s, rounding_mode="floor") + 1
    assert F.frame_lengths_ref(m, F.CONV_KERNELS, F.CONV_STRIDES) == n.tolist()
    assert F.frame_lengths_ref(m, (), ()) == m.sum(1).tolist()
    assert int(m[1].sum()) == 0 and int(m[0].sum()) == 16001 and int((m[2:].diff(dim=1) == 1).sum()) > 0   # interior zeros


@pytest.mark.parametrize("d,Cg,K", [s for s in F.POSCONV_SHAPES if s[0] < 1024])
def test_posconv_reference_is_torchs_weight_norm(d, Cg, K):
    v, g, dw = F.make_posconv(d, Cg, K, "spread")
    conv = torch.nn.Conv1d(d, d, K, groups=d // Cg, bias=False, dtype=torch.float64)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    p = conv.parametrizations.weight
    with torch.no_grad():
        p.original0.copy_(f64(g).view(1, 1, K))
        p.original1.copy_(f64(v))
    conv.weight.backward(f64(dw))
    norm, w, _, _ = F.posconv_weight_ref(v, g)
    assert rel(w, conv.weight.detach()) <= 1e-12
    dv0, dg0 = torch.randn(d, Cg, K, generator=F._gen(1)), torch.randn(K, generator=F._gen(2))
    dv, dg, _, _ = F.posconv_bwd_ref(dw, v, g, norm, dv0, dg0)
    gv, want = dv - f64(dv0), p.original1.grad
    # per tap: the spread family's taps differ by six orders of magnitude, and each is held to its own scale (dv0 is
    # N(0, 1): subtracting it back costs 1e-16 absolute, which the small taps' tolerance has to carry)
    tap_err = (gv - want).abs().amax((0, 1))
    assert bool((tap_err <= 1e-12 * want.abs().amax((0, 1)) + 4e-16).all())
    gv0, _, _, _ = F.posconv_bwd_ref(dw, v, g, norm, torch.zeros(d, Cg, K), torch.zeros(K))
    assert float(((gv0 - want).abs().amax((0, 1)) / want.abs().amax((0, 1))).max()) <= 1e-12
    assert float(((w - conv.weight.detach()).abs().amax((0, 1)) / w.abs().amax((0, 1))).max()) <= 1e-12
    assert rel(dg - f64(dg0), p.original0.grad.view(K)) <= 1e-12
    G = d // Cg
    wf, wb = F.to_wf(w, Cg), F.to_wb(w, Cg)
    assert wf.shape == (G, Cg, K, Cg) and wb.shape == (G, Cg, K, Cg)
    assert float(wf[1, 2, 3, 4]) == float(w[Cg + 2, 4, 3]) and float(wb[1, 4, 3, 2]) == float(w[Cg + 2, 4, K - 1 - 3])


def test_mask_reference_order_and_regroup():
    B, T, C = 2, 12, 32
    h = torch.randn(B, T, C, generator=F._gen(3)).bfloat16()
    emb = torch.randn(C, generator=F._gen(4)).bfloat16()
    tm, fm, fl = F.make_masks(B, T, C)
    out = F.mask_frames_ref(h, tm, fm, emb, fl)
    for b in range(B):
        n = int(fl[b])
        assert float(out[b, n:].abs().sum()) == 0.0 and bool(tm[b, n:].any())               # time and padding
        assert float(out[b, :, fm[b].bool()].abs().sum()) == 0.0 and bool(tm[b, :n].any())  # time and feature
        keep = ~fm[b].bool()
        assert torch.equal(out[b, 1, keep], emb[keep])
        free = ~tm[b, :n].bool()
        assert torch.equal(out[b, :n][free][:, keep], h[b, :n][free][:, keep])
    xg = F.regroup_pad_ref(h, 4, 3)
    assert xg.shape == (B, 4, T + 6, 8) and torch.equal(xg[1, 2, 3 + 5], h[1, 5, 16:24]) and float(xg[:, :, :3].abs().sum()) == 0.0


# ---- the bounds admit the fp32 emulation with a margin of four ---------------------------------------------------------------
CONV0_EMU = [(3, 653, 5, "noise", "plain", True), (3, 653, 5, "dc", "e", True), (2, 300, 1, "noise", "plain", False),
             (2, 1000, 16, "dc", "plain", False), (1, 95, 5, "noise", "e", False)]


def conv0_case(B, N, stride, fam, gam, tails, grid=4, init=0.0):
    lens = [N, N // 2, 37][:B] if tails else None
    x = F.make_conv0_x(B, N, fam, lens)
    params = F.make_conv0_params(gam)
    T0 = F.conv0_frames(N, stride)
    dy = F.make_conv0_dy(B, T0)
    ref = F.conv0_ref(x, *params, stride, EPS, dy=dy, chain=F.conv0_bwd_chain(B, T0, grid), init=init)
    return x, params, dy, ref


@pytest.mark.parametrize("B,N,stride,fam,gam,tails", CONV0_EMU)
def test_conv0_bounds_admit_the_fp32_emulation(B, N, stride, fam, gam, tails):
    """y rounded to bf16 against the whole bound (<= 1: the rounding itself), y before rounding against the slack alone and
    the four parameter gradients (<= 0.25).  Gradients landing on 0.5 are held to 1, as in test_norm_ref_cpu: one
    addition into a buffer whose content dwarfs the sum has u of the 2 u granted."""
    grid = 4
    x, params, dy, ref = conv0_case(B, N, stride, fam, gam, tails, grid)
    emu = emu_conv0(x, *params, stride, dy=dy, grid=grid)
    slack = ref["y_bound"] - BF16_HALF_ULP * ref["y"].abs()
    got = [ratio(emu["y"].bfloat16(), ref["y"], ref["y_bound"]), ratio(emu["y"], ref["y"], slack)]
    got += [ratio(emu[k], ref[k], ref[k + "_bound"]) for k in ("dw", "dbias", "dgamma", "dbeta")]
    print("conv0", B, N, stride, fam, gam, ["%.3f" % r for r in got])
    assert got[0] <= 1.0 and max(got[1:]) <= 0.25, got
    _, _, _, ref1 = conv0_case(B, N, stride, fam, gam, tails, grid, init=0.5)
    emu1 = emu_conv0(x, *params, stride, dy=dy, grid=grid, init=0.5)
    got1 = [ratio(f64(emu1[k]) - 0.5, ref1[k], ref1[k + "_bound"]) for k in ("dw", "dbias", "dgamma", "dbeta")]
    assert max(got1) <= 1.0, got1


@pytest.mark.parametrize("fam", ["noise", "const", "dc"])
@pytest.mark.parametrize("N", [1000, 4099])
def test_normalisation_bounds_admit_the_fp32_emulation(N, fam):
    """Largest error / bound over the rows: 0.12 with z-normalisation (<= 0.25).  Peak normalisation alone is v * (1 / m):
    two roundings against the 3 u granted (the reciprocal is allowed 1 ulp), up to 0.53 here and 2/3 with a correct
    kernel: held to 1, like every term norm_ref's margin note lists as one rounding granted in full."""
    lens = F.make_lengths(N)
    x = F.make_wave(8, N, fam)
    worst, peak_only = 0.0, 0.0
    for ln in (lens, None):
        y, _, bound = F.pcm_ref(x, ln, False, True, WEPS)
        worst = max(worst, ratio(emu_pcm(x, ln, False, True), y, bound))
    p = F.make_pcm16(8, N)
    for src in (p, p.float() / 32768.0, x):   # pcm_prepare_kernel's own centring, on the constant and DC-offset rows too
        for peak in (False, True):
            for zn in (False, True):
                y, _, bound = F.pcm_ref(src, lens, peak, zn, WEPS)
                r = ratio(emu_pcm(src, lens, peak, zn), y, bound)
                if peak and not zn:
                    peak_only = max(peak_only, r)
                else:
                    worst = max(worst, r)
    print("normalise", N, fam, "%.3f %.3f" % (worst, peak_only))
    assert worst <= 0.25 and peak_only <= 1.0


@pytest.mark.parametrize("fam", ["plain", "spread"])
@pytest.mark.parametrize("d,Cg,K", [s for s in F.POSCONV_SHAPES if s[0] < 1024])
def test_posconv_bounds_admit_the_fp32_emulation(d, Cg, K, fam):
    """norm, w before its rounding to bf16 and dg into a zeroed buffer - the quantities a chain of additions carries:
    <= 0.25 (0.05, 0.08, 0.01 here).  dv is element-wise: where the projection term is small it is (g / n) dw, three
    roundings against the 4 u granted, up to 0.63 here; it, w in bf16, and the gradients added into buffers that hold N(0, 1)
    values (one rounding of a sum the buffer dominates) are held to 1, as test_norm_ref_cpu holds its one-rounding terms:
    a constant raised to bring them under 0.25 would loosen the bound where it is tight for a reason."""
    v, g, dw = F.make_posconv(d, Cg, K, fam)
    norm, w, nb, wbound = F.posconv_weight_ref(v, g)
    en, ew = emu_posconv_fwd(v, g)
    got = [ratio(en, norm, nb), ratio(ew, w, wbound - BF16_HALF_ULP * w.abs())]
    assert ratio(ew.bfloat16(), w, wbound) <= 1.0
    n32 = norm.float()
    z3, z1 = torch.zeros(d, Cg, K), torch.zeros(K)
    dv, dg, dvb, dgb = F.posconv_bwd_ref(dw, v, g, n32, z3, z1)
    edv, edg = emu_posconv_bwd(dw, v, g, n32, z3, z1)
    got.append(ratio(edg, dg, dgb))
    print("posconv", d, Cg, K, fam, ["%.3f" % r for r in got], "dv %.3f" % ratio(edv, dv, dvb))
    assert max(got) <= 0.25 and ratio(edv, dv, dvb) <= 1.0, got
    dv0, dg0 = torch.randn(d, Cg, K, generator=F._gen(1)), torch.randn(K, generator=F._gen(2))
    dv, dg, dvb, dgb = F.posconv_bwd_ref(dw, v, g, n32, dv0, dg0)
    edv, edg = emu_posconv_bwd(dw, v, g, n32, dv0, dg0)
    assert ratio(edv, dv, dvb) <= 1.0 and ratio(edg, dg, dgb) <= 1.0


@pytest.mark.parametrize("B,L,C,k,s", F.COL2IM_SHAPES[:1] + F.COL2IM_SHAPES[2:5])
def test_col2im_bound_admits_the_fp32_emulation(B, L, C, k, s):
    """The fp32 sum before its rounding against the fp32 slack alone (<= 0.25), the bf16 result against the whole bound
    (<= 1: the rounding to bf16 itself)."""
    T = (L - k) // s + 1
    dcol = F.make_dcol(B, T, C, k)
    dx, bound, covered = F.col2im_ref(dcol, L, s)
    got = emu_col2im(dcol, L, s)
    assert ratio(got, dx, bound) <= 1.0
    slack = torch.where(bound > 0, bound - BF16_HALF_ULP * dx.abs(), bound)
    assert ratio(emu_col2im(dcol, L, s, rounded=False), dx, slack) <= 0.25
    assert float(got[:, ~covered].abs().sum()) == 0.0


# ---- the bounds reject what they exist to reject -------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 4099])
@pytest.mark.parametrize("peak", [False, True])
def test_normalisation_bound_rejects_a_one_pass_variance(peak, N):
    """On the DC-offset family, without and with peak normalisation (pcm_prepare_kernel's form).  On zero-mean PCM noise a
    one-pass variance is as good as the two-pass one and passes (ratio < 0.1): only these rows tell them apart."""
    x = F.make_wave(8, N, "dc")
    for ln in (F.make_lengths(N), None):
        y, _, bound = F.pcm_ref(x, ln, peak, True, WEPS)
        assert ratio(emu_pcm(x, ln, peak, True, one_pass=True), y, bound) > 10.0
        assert ratio(emu_pcm(x, ln, peak, True), y, bound) <= 0.25
    p = F.make_pcm16(8, N)
    y, _, bound = F.pcm_ref(p, None, peak, True, WEPS)
    assert ratio(emu_pcm(p, None, peak, True, one_pass=True), y, bound) < 1.0


@pytest.mark.parametrize("N", [1000, 4099])
def test_normalisation_bound_rejects_a_gain_fused_into_the_centring(N):
    """What pcm_prepare_kernel did before it was held to this bound: the mean is formed from the rounded product v * gain,
    the centring fused the exact one, and the utterance of one sample came out as that rounding error times rsqrt(eps)
    (~1e-4) instead of 0."""
    p, lens = F.make_pcm16(8, N), F.make_lengths(N)
    y, _, bound = F.pcm_ref(p, lens, True, True, WEPS)
    got = emu_pcm(p, lens, True, True, fused=True)
    assert float(bound[1].max()) == 0.0 and float(got[1, 0].abs()) > 1e-6
    assert ratio(got, y, bound) == float("inf")
    assert ratio(emu_pcm(p, lens, True, True), y, bound) <= 0.25


@pytest.mark.parametrize("wrong", ["bias", "tap"])
def test_conv0_forward_bound_rejects(wrong):
    x, params, dy, ref = conv0_case(3, 653, 5, "noise", "plain", True)
    y = emu_conv0(x, *params, 5, wrong=wrong)
    assert ratio(y.bfloat16(), ref["y"], ref["y_bound"]) > 2.0


@pytest.mark.parametrize("wrong", ["hm2", "block"])
def test_conv0_backward_bounds_reject(wrong):
    x, params, dy, ref = conv0_case(3, 653, 5, "noise", "plain", True)
    emu = emu_conv0(x, *params, 5, dy=dy, wrong=wrong)
    keys = ("dw", "dbias") if wrong == "hm2" else ("dw", "dbias", "dgamma", "dbeta")
    for k in keys:
        assert ratio(emu[k], ref[k], ref[k + "_bound"]) > 10.0, k


def test_col2im_bound_rejects_a_missing_frame_and_nonzero_uncovered_positions():
    B, L, C, k, s = F.COL2IM_SHAPES[0]
    T = (L - k) // s + 1
    dcol = F.make_dcol(B, T, C, k)
    dx, bound, covered = F.col2im_ref(dcol, L, s)
    assert not bool(covered[-1]) and bool(covered[:-1].all())
    assert ratio(emu_col2im(dcol, L, s, wrong="overlap"), dx, bound) > 10.0
    got = emu_col2im(dcol, L, s)
    got[:, -1] = 2.0 ** -120
    assert ratio(got, dx, bound) == float("inf")


@pytest.mark.parametrize("fam", ["plain", "spread"])
def test_posconv_bounds_reject(fam):
    d, Cg, K = F.POSCONV_SHAPES[0]
    v, g, dw = F.make_posconv(d, Cg, K, fam)
    norm, w, nb, wbound = F.posconv_weight_ref(v, g)
    en, _ = emu_posconv_fwd(v, g, drop_slab=5)
    assert ratio(en, norm, nb) > 10.0
    n32 = norm.float()
    dv0, dg0 = torch.randn(d, Cg, K, generator=F._gen(1)), torch.randn(K, generator=F._gen(2))
    dv, dg, dvb, dgb = F.posconv_bwd_ref(dw, v, g, n32, dv0, dg0)
    edv, _ = emu_posconv_bwd(dw, v, g, n32, dv0, dg0, wrong="projection")
    assert ratio(edv, dv, dvb) > 10.0
    edv, edg = emu_posconv_bwd(dw, v, g, n32, dv0, dg0, wrong="overwrite")
    assert ratio(edv, dv, dvb) > 10.0 and ratio(edg, dg, dgb) > 10.0


def test_mask_reference_tells_feature_zeros_before_the_embed():
    B, T, C = 2, 499, 1024
    h = torch.randn(B, T, C, generator=F._gen(3)).bfloat16()
    emb = torch.randn(C, generator=F._gen(4)).bfloat16()
    tm, fm, fl = F.make_masks(B, T, C)
    good = F.mask_frames_ref(h, tm, fm, emb, fl)
    bad = F.mask_frames_ref(h, tm, fm, emb, fl, order=("feature", "embed", "pad"))
    assert not torch.equal(good.view(torch.int16), bad.view(torch.int16))
