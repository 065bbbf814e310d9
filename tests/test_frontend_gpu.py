"""csrc/frontend.hip and the head of csrc/misc.hip on a real MI355X against the float64 references and derived bounds of
tests/frontend_ref.py (proved on the CPU in tests/test_frontend_ref_cpu.py).  `-m gpu` only.

Every comparison prints `ratio <kernel> <largest error / bound>`; a ratio above 1 fails.  Outputs are pre-filled with a
sentinel (7) and carry guard rows that must keep it.

Which test reaches which path (each asserts the regime it depends on):
  conv0 backward grid-stride loop (nblk > grid)              test_conv0_more_frame_blocks_than_workgroups
  leftover samples, all-zero frames, bias = 0, DC offset     test_conv0_silent_tails_and_leftover_samples
  nf = 1, 2, 5 (idle waves), 16, 17, 18, 128                 test_conv0_short_frame_blocks
  stride 1 and 16 (the ends of the LDS layout)               test_conv0_stride_ends
  col2im: uncovered tail, k = s copy, k = 10 s = 5, s = 1,   test_col2im
    gaps (k < s), the Whisper form
  col2im grid cap (chunks > 16384 * 256)                     test_col2im_past_the_grid_cap
  normalisation: len 0, 1, N, > N, NULL, N < 1024, constant  test_wave_normalize, test_pcm_prepare (its own
    and DC-offset rows; int16 -32768, silent row, peak x      centring code: the same families again)
    znorm, ld_in > N at odd offsets, mask NULL
  frame_count scalar path, 64-slice cap, counters' reset,    test_frame_lengths
    interior zeros, B = 4096 and the refusal of 4097
  masks overlapping, each NULL form, the 8192-group caps     test_mask_frames, test_regroup_pad,
                                                             test_mask_and_regroup_past_the_grid_cap
  tap_dot: four-in-flight loop, tail, row lanes, empty       test_posconv_weight
    slabs; wb = NULL; dv / dg accumulated; spread taps"""
import collections
import math

import pytest
import torch

import frontend_ref as F
from norm_ref import f64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
WEPS = 1e-7
SENT = 7.0
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
    err = (f64(got) - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(err, bound)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = float(torch.nan_to_num(r, nan=math.inf).max())
    RATIOS[name] = max(RATIOS[name], r)
    print("ratio %s %.3f" % (name, r))
    assert r <= 1.0, (name, r)


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def sentinel(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def kept(t):
    return bool((t == SENT).all())


# ---- conv0 + LayerNorm + GELU --------------------------------------------------------------------------------------------
def conv0_grid(ops, B, N, stride):
    """The backward's grid as the library reports it (so CONV0_BWD_GRID cannot move a case out of its regime)."""
    return ops.conv0_bwd_partial_floats(B, N, F.C0, F.K0, stride) // (F.C0 * (F.K0 + 3))


def check_conv0(ops, x, params, stride, init=0.0, batch=16, exact=None):
    """Forward and backward of one case against conv0_ref; `exact` [B, T0] marks frames whose bound must be zero."""
    B, N = x.shape
    T0 = F.conv0_frames(N, stride)
    grid = conv0_grid(ops, B, N, stride)
    dy = F.make_conv0_dy(B, T0)
    xd, pd, dyd = dev(x), [dev(t) for t in params], dev(dy)
    y = sentinel((B * T0 + 2, F.C0), torch.bfloat16)
    ops.conv0_fwd(xd, *pd, y, B, N, F.C0, F.K0, stride, EPS)
    grads = {"dw": sentinel((F.C0 * F.K0 + 8,), torch.float32), "dbias": sentinel((F.C0 + 8,), torch.float32),
             "dgamma": sentinel((F.C0 + 8,), torch.float32), "dbeta": sentinel((F.C0 + 8,), torch.float32)}
    for k, t in grads.items():
        t[:-8] = init
    part = torch.empty(grid * F.C0 * (F.K0 + 3), dtype=torch.float32, device=DEV)
    ops.conv0_bwd(xd, *pd, dyd, grads["dw"], grads["dbias"], grads["dgamma"], grads["dbeta"], part, B, N, F.C0, F.K0,
                  stride, EPS)
    torch.cuda.synchronize()
    yc = y.cpu()
    assert kept(yc[B * T0:])
    yc = yc[:B * T0].view(B, T0, F.C0)
    assert not bool((yc == SENT).all(2).any())    # every frame was written

    def on_y(b0, yr, yb):
        within("conv0_fwd.y", yc[b0:b0 + yr.shape[0]], yr, yb)
        if exact is not None:
            assert float(yb[exact[b0:b0 + yr.shape[0]]].max()) == 0.0   # (so `within` compared those frames exactly)

    ref = F.conv0_ref(x, *params, stride, EPS, dy=dy, chain=F.conv0_bwd_chain(B, T0, grid), init=init, batch=batch, on_y=on_y)
    for k, t in grads.items():
        t = t.cpu()
        assert kept(t[-8:])
        within("conv0_bwd." + k, f64(t[:-8]).view(ref[k].shape) - init, ref[k], ref[k + "_bound"])


def test_conv0_more_frame_blocks_than_workgroups(ops):
    """B = 320, N = 650: T0 = 129 is a full 128-frame block and a one-frame block per utterance, 640 blocks on a grid of
    512, so 128 workgroups restage LDS for a second block."""
    B, N, stride = 320, 650, 5
    T0 = F.conv0_frames(N, stride)
    grid = conv0_grid(ops, B, N, stride)
    nblk = B * -(-T0 // F.FPB)
    assert T0 == 129 and nblk == 640 and nblk > grid
    check_conv0(ops, F.make_conv0_x(B, N), F.make_conv0_params("plain"), stride, batch=32)


@pytest.mark.parametrize("fam,gam,init", [("noise", "e", 0.0), ("dc", "plain", 0.5), ("dc", "e", 0.0)])
def test_conv0_silent_tails_and_leftover_samples(ops, fam, gam, init):
    """B = 3, N = 653: three samples belong to no frame; utterances 1 and 2 end in silence, whose frames are all zero: with
    bias = 0 ('e') they have v = 0 and rstd = rsqrt(eps) exactly, and y = gelu(0) = 0 there bit for bit."""
    B, N, stride = 3, 653, 5
    lens = [N, 326, 37]
    assert (N - F.K0) % stride != 0
    x = F.make_conv0_x(B, N, fam, lens)
    T0 = F.conv0_frames(N, stride)
    silent = (x.unfold(1, F.K0, stride)[:, :T0] == 0).all(2)
    assert int(silent[1].sum()) > 50 and int(silent[2].sum()) > 100 and not bool(silent[0].any())
    check_conv0(ops, x, F.make_conv0_params(gam), stride, init=init, exact=silent if gam == "e" else None)


@pytest.mark.parametrize("N,nf", [(10, 1), (15, 2), (30, 5), (85, 16), (90, 17), (95, 18), (645, 128)])
def test_conv0_short_frame_blocks(ops, N, nf):
    """One utterance of nf frames: waves without a frame (nf < 4), one pass of the forward's four-frames-per-wave loop
    (nf <= 16), one frame past it, and the full block."""
    assert F.conv0_frames(N, 5) == nf
    check_conv0(ops, F.make_conv0_x(1, N, "dc" if nf % 2 else "noise"), F.make_conv0_params("e" if nf % 2 else "plain"), 5)


@pytest.mark.parametrize("stride,N", [(1, 209), (16, 3197)])
def test_conv0_stride_ends(ops, stride, N):
    assert F.conv0_frames(N, stride) == 200
    check_conv0(ops, F.make_conv0_x(2, N, "dc"), F.make_conv0_params("plain"), stride)


# ---- col2im ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,C,k,s", F.COL2IM_SHAPES)
def test_col2im(ops, B, L, C, k, s):
    T = (L - k) // s + 1
    dcol = F.make_dcol(B, T, C, k)
    dx = sentinel((B * L + 2, C), torch.bfloat16)
    ops.col2im_1d(dev(dcol), dx, B, T, L, C, k, s)
    torch.cuda.synchronize()
    dx = dx.cpu()
    assert kept(dx[B * L:])
    got = dx[:B * L].view(B, L, C)
    ref, bound, covered = F.col2im_ref(dcol, L, s)
    if (B, L, C, k, s) in (F.COL2IM_SHAPES[0], F.COL2IM_SHAPES[1], F.COL2IM_SHAPES[5]):
        assert not bool(covered[-1])                 # an uncovered tail position
    if k < s:
        assert not bool(covered[1::2].any())         # gaps
    within("col2im", got, ref, bound)
    assert bool((bits(got[:, ~covered]) == 0).all())   # +0, not merely == 0
    if k <= s:   # no overlap: a copy, and `within` compared it exactly
        assert float(bound.max()) == 0.0


def test_col2im_past_the_grid_cap(ops):
    """4 198 400 chunks of 8 channels against 16384 workgroups of 256: the last 4096 chunks are a second trip of the
    grid-stride loop.  k = s = 2: dx is dcol re-read as [B, 2 T, C], compared on the device."""
    B, L, C, k, s = 2, 32800, 512, 2, 2
    T = (L - k) // s + 1
    assert B * L * (C // 8) > 16384 * 256 and T * s == L   # the cap is `if (g > 16384)` in ca_col2im_1d: no accessor
    dcol = torch.randn(B, T, k, C, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV).bfloat16()
    dx = sentinel((B * L + 2, C), torch.bfloat16)
    ops.col2im_1d(dcol, dx, B, T, L, C, k, s)
    torch.cuda.synchronize()
    assert kept(dx[B * L:])
    assert torch.equal(bits(dx[:B * L]), bits(dcol.view(B * L, C)))


# ---- normalisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["noise", "const", "dc"])
@pytest.mark.parametrize("N", [1000, 4099])
def test_wave_normalize(ops, N, fam):
    """Eight rows in one launch with lengths 0, 1, N, N + 5, 17 and a ragged rest, then lengths = NULL.  Rows of length 0
    and 1, and everything past a length, have a zero bound: they must be exactly 0."""
    B = 8
    x = F.make_wave(B, N, fam)
    for lens in (F.make_lengths(N), None):
        y = sentinel((B + 1, N), torch.float32)
        ops.wave_normalize(dev(x), dev(lens), y, B, N, WEPS)
        torch.cuda.synchronize()
        y = y.cpu()
        assert kept(y[B])
        ref, _, bound = F.pcm_ref(x, lens, False, True, WEPS)
        if lens is not None:
            assert float(bound[:2].max()) == 0.0 and float(bound[4, 17:].max()) == 0.0
        within("wave_normalize", y[:B], ref, bound)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("peak,znorm", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("kind", ["int16", "fp32", "const", "dc"])
@pytest.mark.parametrize("N", [1000, 4099])
def test_pcm_prepare(ops, N, kind, peak, znorm, strided):
    """int16 PCM (with -32768 and a silent row), the same as fp32, and the fp32 constant and 1 + 1e-3 noise rows of
    test_wave_normalize (the DC offset is what a one-pass variance in this kernel's own centring would fail on); peak x
    znorm, dense rows and rows of pitch N + 3 that start one element into their buffer (int16 rows at odd element
    offsets), with the mask (exact) and with mask = NULL (the same y bit for bit); lengths as in test_wave_normalize and
    NULL."""
    B = 8
    if kind in ("const", "dc"):
        p = F.make_wave(B, N, kind)
    else:
        p = F.make_pcm16(B, N)
        if kind == "fp32":
            p = p.float() / 32768.0
    if strided:
        ld = N + 3
        flat = torch.zeros(1 + B * ld, dtype=p.dtype, device=DEV)
        src = flat[1:].view(B, ld)[:, :N]
        src.copy_(p)
        assert (src.data_ptr() - flat.data_ptr()) == flat.element_size()   # rows start at odd element offsets
    else:
        ld, src = N, dev(p)
    for lens in (F.make_lengths(N), None):
        ref, mref, bound = F.pcm_ref(p, lens, peak, znorm, WEPS)
        outs = []
        for with_mask in (True, False):
            y = sentinel((B + 1, N), torch.float32)
            mask = torch.full((B + 1, N), 7, dtype=torch.int32, device=DEV) if with_mask else None
            ops.pcm_prepare(src, dev(lens), y, mask, B, N, ld, peak_normalize=peak, zero_mean_unit_var=znorm, eps=WEPS)
            torch.cuda.synchronize()
            y = y.cpu()
            assert kept(y[B])
            if with_mask:
                mask = mask.cpu()
                assert torch.equal(mask[:B], mref) and bool((mask[B] == 7).all())
            outs.append(y[:B])
        within("pcm_prepare", outs[0], ref, bound)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        if not peak and not znorm:
            assert float(bound.max()) == 0.0        # a conversion: exact


# ---- frame lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(5, 16001), (3, 7), (2, 600000), (4096, 64)])
def test_frame_lengths(ops, B, N):
    """Rows off 16-byte alignment (N % 4 != 0, b >= 1: the scalar path), N below the first kernel, N past 64 slices of
    8192, every counter the library has; masks with interior zeros and an all-zero row; the model's conv stack and
    nconv = 0; two calls in a row on one stream, each result its own (the counters reset themselves)."""
    if (B, N) == (5, 16001):
        assert N % 4 != 0
    if (B, N) == (2, 600000):
        assert N > 64 * 8192
    m1, m2 = F.make_attention_mask(B, N, seed=13), F.make_attention_mask(B, N, seed=14).flip(0).contiguous()
    assert not torch.equal(m1.sum(1), m2.sum(1)) and int(m1[1].sum()) == 0
    for kernels, strides in ((F.CONV_KERNELS, F.CONV_STRIDES), ((), ())):
        o1, o2 = (torch.full((B + 1,), 7, dtype=torch.int32, device=DEV) for _ in range(2))
        ops.frame_lengths(dev(m1), kernels, strides, o1)
        ops.frame_lengths(dev(m2), kernels, strides, o2)
        torch.cuda.synchronize()
        assert o1[:B].cpu().tolist() == F.frame_lengths_ref(m1, kernels, strides)
        assert o2[:B].cpu().tolist() == F.frame_lengths_ref(m2, kernels, strides)
        assert int(o1[B]) == 7 and int(o2[B]) == 7


def test_frame_lengths_refuses_more_rows_than_counters(ops):
    B = 4097
    m = torch.ones(B, 8, dtype=torch.int32, device=DEV)
    with pytest.raises(ops.CoralAmdError):
        ops.frame_lengths(m, F.CONV_KERNELS, F.CONV_STRIDES, torch.zeros(B, dtype=torch.int32, device=DEV))


# ---- masks, regroup --------------------------------------------------------------------------------------------------
def mask_inputs(B, T, C, device="cpu"):
    g = torch.Generator(device=device).manual_seed(B + T)
    h = torch.randn(B, T, C, generator=g, device=device).bfloat16()
    emb = torch.randn(C, generator=g, device=device).bfloat16()
    return h, emb


def test_mask_frames(ops):
    """Model shape.  Every row has frames that are time-masked inside a feature span, time-masked and padded, and feature
    spans across padded frames; then each argument NULL in turn, and all of them (h untouched)."""
    B, T, C = 2, 499, 1024
    h, emb = mask_inputs(B, T, C)
    tm, fm, fl = F.make_masks(B, T, C)
    pad = torch.arange(T)[None, :] >= fl[:, None]
    assert bool((tm.bool() & pad).any(1).all()) and bool((tm.bool() & ~pad).any(1).all()) and bool(fm.bool().any(1).all())
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        a = [m if u else None for m, u in zip((tm, fm, fl), use)]
        hd = sentinel((B * T + 2, C), torch.bfloat16)
        hd[:B * T] = dev(h).view(B * T, C)
        ops.mask_frames(hd, dev(a[0]), dev(a[1]), dev(emb), dev(a[2]), B, T, C)
        torch.cuda.synchronize()
        hd = hd.cpu()
        assert kept(hd[B * T:])
        want = F.mask_frames_ref(h, a[0], a[1], emb, a[2])
        assert torch.equal(bits(hd[:B * T].view(B, T, C)), bits(want))
        assert torch.equal(bits(want), bits(h)) == (use == (0, 0, 0))


@pytest.mark.parametrize("pad", [64, 0])
def test_regroup_pad(ops, pad):
    B, T, G, Cg = 2, 499, 16, 64
    h, _ = mask_inputs(B, T, G * Cg)
    n = B * G * (T + 2 * pad)
    xg = sentinel((n + 2, Cg), torch.bfloat16)
    ops.regroup_pad(dev(h), xg, B, T, G, Cg, pad)
    torch.cuda.synchronize()
    xg = xg.cpu()
    assert kept(xg[n:])
    assert torch.equal(bits(xg[:n].view(B, G, T + 2 * pad, Cg)), bits(F.regroup_pad_ref(h, G, pad)))


def test_mask_and_regroup_past_the_grid_cap(ops):
    """B = 17, T = 1000, C = 1024: 2 176 000 chunks of 8 channels against 8192 workgroups of 256, for both kernels (the
    regrouped tensor is larger still); the references run on the device."""
    B, T, C, G, pad = 17, 1000, 1024, 16, 64
    assert B * T * (C // 8) > 8192 * 256   # the cap is `if (g > 8192)` in ca_mask_frames and ca_regroup_pad: no accessor
    h, emb = mask_inputs(B, T, C, DEV)
    tm, fm, fl = (dev(t) for t in F.make_masks(B, T, C))
    hd = sentinel((B * T + 2, C), torch.bfloat16)
    hd[:B * T] = h.view(B * T, C)
    ops.mask_frames(hd, tm, fm, emb, fl, B, T, C)
    n = B * G * (T + 2 * pad)
    xg = sentinel((n + 2, C // G), torch.bfloat16)
    ops.regroup_pad(h, xg, B, T, G, C // G, pad)
    torch.cuda.synchronize()
    assert kept(hd[B * T:]) and kept(xg[n:])
    assert torch.equal(bits(hd[:B * T].view(B, T, C)), bits(F.mask_frames_ref(h, tm, fm, emb, fl)))
    assert torch.equal(bits(xg[:n].view(B, G, T + 2 * pad, C // G)), bits(F.regroup_pad_ref(h, G, pad)))


# ---- positional-conv weight norm -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["plain", "spread"])
@pytest.mark.parametrize("d,Cg,K", F.POSCONV_SHAPES)
def test_posconv_weight(ops, d, Cg, K, fam):
    """ca_posconv_weight (norm, wf, wb, and wb = NULL) and ca_posconv_weight_bwd into buffers that already hold values,
    with the norm given in float64-rounded form and with the norm the forward kernel wrote."""
    slabs = ops.posconv_partial_floats(K) // K - 1
    rows = d * Cg
    per = -(-rows // slabs)
    assert slabs == F.PCW_SLABS
    if (d, Cg, K) == F.POSCONV_SHAPES[0]:
        assert per == 11 and 256 // K == 2          # an unrolled pass and a tail in both row lanes
    if (d, Cg, K) == F.POSCONV_SHAPES[1]:
        assert per == 9 and slabs - -(-rows // per) == 64   # 64 empty slabs
    if (d, Cg, K) == F.POSCONV_SHAPES[2]:
        assert per == 64
    if (d, Cg, K) in F.POSCONV_SHAPES[:3]:
        assert per >= 8                              # rows per slab: the four-in-flight loop runs
    v, g, dw = F.make_posconv(d, Cg, K, fam)
    if fam == "spread":
        nj = f64(v).pow(2).sum((0, 1)).sqrt()
        assert float(nj.max() / nj.min()) > 1e5
    G = d // Cg
    vd, gd = dev(v), dev(g)
    part = torch.empty(ops.posconv_partial_floats(K), dtype=torch.float32, device=DEV)
    norm_ref, w, nb, wbound = F.posconv_weight_ref(v, g)
    outs = []
    for with_wb in (True, False):
        wf = sentinel((d * K * Cg + 8,), torch.bfloat16)
        wb = sentinel((d * K * Cg + 8,), torch.bfloat16)
        norm = sentinel((K + 1,), torch.float32)
        ops.posconv_weight(vd, gd, wf, wb if with_wb else None, norm, part, d, Cg, K)
        torch.cuda.synchronize()
        assert kept(wf[-8:]) and kept(wb[-8:] if with_wb else wb) and kept(norm[K:])
        outs.append((wf.cpu()[:-8], wb.cpu()[:-8], norm[:K].clone()))
    wf, wb, norm = outs[0]
    assert torch.equal(bits(wf), bits(outs[1][0])) and torch.equal(norm, outs[1][2])
    within("posconv_weight.norm", norm, norm_ref, nb)
    within("posconv_weight.wf", wf.view(G, Cg, K, Cg), F.to_wf(w, Cg), F.to_wf(wbound, Cg))
    within("posconv_weight.wb", wb.view(G, Cg, K, Cg), F.to_wb(w, Cg), F.to_wb(wbound, Cg))
    dwf = dev(F.to_wf(dw, Cg))
    gen = torch.Generator().manual_seed(d + K)
    dv0, dg0 = torch.randn(d, Cg, K, generator=gen), torch.randn(K, generator=gen)
    for n32 in (norm_ref.float(), norm.cpu()):
        dv = sentinel((d * Cg * K + 8,), torch.float32)
        dg = sentinel((K + 8,), torch.float32)
        dv[:-8], dg[:-8] = dev(dv0).view(-1), dev(dg0)
        ops.posconv_weight_bwd(dwf, vd, gd, dev(n32), dv, dg, part, d, Cg, K)
        torch.cuda.synchronize()
        dv, dg = dv.cpu(), dg.cpu()
        assert kept(dv[-8:]) and kept(dg[-8:])
        rv, rg, bv, bg = F.posconv_bwd_ref(dw, v, g, n32, dv0, dg0)
        within("posconv_weight_bwd.dv", dv[:-8].view(d, Cg, K), rv, bv)
        within("posconv_weight_bwd.dg", dg[:-8], rg, bg)
