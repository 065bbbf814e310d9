"""Test-side float64 references of the kernels that feed and leave the wav2vec2 encoder - csrc/frontend.hip (utterance
normalisation, PCM preparation, frame lengths, the fused conv0 + LayerNorm + GELU forward and backward, col2im) and the
head of csrc/misc.hip (SpecAugment / padding masks, regroup + pad, the positional conv's weight norm and its backward) -
with the error bounds a correct fp32 kernel is held to and the seeded inputs that tests/test_frontend_ref_cpu.py (no GPU)
and tests/test_frontend_gpu.py build identically.  Plain torch; nothing here imports `coral_amd`.  The bit-exact
references (masks, regroup, col2im without overlap) are integer / copy operations and run on whatever device their
arguments live on, so the GPU test can apply them to tensors too large to bring back.

Notation and margin rule are those of tests/norm_ref.py: u = 2^-24, a sum along a chain of k fp32 additions has error
<= k u sum|term|, a bf16 result carries 2^-8 |ref| more; every bound is the worst case with no constant fitted to a
kernel, and an fp32 emulation of the kernel's own order of operations uses at most a quarter of each fp32 slack.
"""
from __future__ import annotations

import torch

from norm_ref import BF16_HALF_ULP, DGELU_LIP, ERF_APPROX, GELU_LIP, U, dgelu64, f64, gelu64, make_affine

C0, K0 = 512, 10                  # conv0: channels, taps
FPB = 128                         # CONV0_FPB: frames per frame block
WAVE_DEPTH = 8 + 6                # a sum over 512 channels: 8 in the lane, 6 cross-lane steps
PCW_SLABS = 1024                  # slabs of tap_dot_kernel
CONV_KERNELS, CONV_STRIDES = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- utterance normalisation, PCM preparation ----------------------------------------------------------------------------
def make_lengths(N: int) -> torch.Tensor:
    """int32 [8]: 0, 1, N, N + 5 (clamped by the kernel), 17 and a ragged rest."""
    return torch.tensor([0, 1, N, N + 5, 17, N - 1, N // 2 + 1, 1023 if N > 1023 else N // 3], dtype=torch.int32)


def make_wave(B: int, N: int, family: str, seed: int = 11) -> torch.Tensor:
    """fp32 [B, N]: 'noise' 0.1 N(0, 1) + 0.01, 'const' one value per row, 'dc' 1 + 1e-3 N(0, 1) (the offset is a thousand
    standard deviations: a one-pass variance loses everything there)."""
    g = _gen(seed)
    n = torch.randn(B, N, generator=g)
    if family == "noise":
        return 0.1 * n + 0.01
    if family == "const":
        return (0.3 * n[:, :1]).expand(B, N).clone()
    if family == "dc":
        return 1.0 + 1e-3 * n
    raise ValueError(family)


def make_pcm16(B: int, N: int, seed: int = 12) -> torch.Tensor:
    """int16 [B, N]: noise of a different loudness per row, -32768 planted in rows 2 and 5, row 6 silent."""
    g = _gen(seed)
    x = (torch.randn(B, N, generator=g) * (3000.0 / (1 + torch.arange(B)[:, None]))).round().clamp(-32768, 32767)
    x[2, N // 3] = -32768
    x[5, 5] = -32768
    x[6] = 0
    return x.to(torch.int16)


def _clamped(lengths, B, N):
    return torch.full((B,), N, dtype=torch.int64) if lengths is None else lengths.to(torch.int64).clamp(max=N)


def norm_depth(N: int) -> int:
    """Longest chain of a 1024-thread utterance sum: ceil(N / 1024) in the thread, 6 butterfly steps, 16 waves."""
    return -(-N // 1024) + 6 + 16


def pcm_ref(pcm, lengths, peak: bool, znorm: bool, eps: float):
    """(y [B, N] float64, mask [B, N] int32, bound [B, N]) of ca_pcm_prepare; ca_wave_normalize is the fp32, no-peak,
    znorm form of it.  int16 samples are v = s / 32768 exactly.  Peak: v / max|v| over the valid samples (gain 1 for a
    silent row).  znorm: (v - mean) / sqrt(var + eps), two-pass, over the valid samples.  Rows of length 0 and everything
    past the length are 0, and so is a row of length 1 (v - mean is exactly 0).

    Bound.  e_x, the error of the gained sample: the kernel's gain 1 / m rounds once (2 u granted) and the product once:
    3 u |x| with peak, 0 without.  mean^ = t / len * g: the sum runs along depth = ceil(N / 1024) + 6 + 16 additions, the
    division and the product round: ms = (depth + 4) u mean|x|.  Variance of (x^ - mean^): as norm_ref.fwd_stats_slack,
    (depth / 2 + 6) u + (ms rstd)^2 / 2 relative on rstd, plus what e_x does to it: d var = 2 mean(d e_x), so
    rstd^2 mean(|d| e_x) relative.  y = (x^ - mean^) rstd^: two roundings relative to (|x| + |mean|) rstd, and the input
    errors: bound = (e_x + ms + 2 u (|x| + |mean|)) rstd + |x - mean| rs.  Without znorm y = x^ and the bound is e_x (an
    exact copy when there is no peak either)."""
    B, N = pcm.shape
    v = f64(pcm) / 32768.0 if pcm.dtype == torch.int16 else f64(pcm)
    n = _clamped(lengths, B, N)
    valid = torch.arange(N)[None, :] < n[:, None]
    v = torch.where(valid, v, torch.zeros(()).double())
    cnt = n.clamp(min=1).double()[:, None]
    e_x = torch.zeros_like(v)
    if peak:
        m = v.abs().amax(1, keepdim=True)
        v = v / torch.where(m > 0, m, torch.ones_like(m))
        e_x = 3 * U * v.abs()
    if not znorm:
        return v, valid.to(torch.int32), e_x
    depth = norm_depth(N)
    mean = v.sum(1, keepdim=True) / cnt
    d = torch.where(valid, v - mean, torch.zeros(()).double())
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / cnt + eps)
    ms = (depth + 4) * U * v.abs().sum(1, keepdim=True) / cnt
    rs = rstd * ((depth / 2 + 6) * U + 0.5 * (ms * rstd) ** 2 + rstd ** 2 * (d.abs() * e_x).sum(1, keepdim=True) / cnt)
    y = d * rstd
    bound = (e_x + ms + 2 * U * (v.abs() + mean.abs())) * rstd + d.abs() * rs
    live = valid & (n > 1)[:, None]
    zero = torch.zeros(()).double()
    return torch.where(live, y, zero), valid.to(torch.int32), torch.where(live, bound, zero)


# ---- frame lengths -------------------------------------------------------------------------------------------------------
def frame_lengths_ref(mask: torch.Tensor, kernels, strides) -> list:
    """Python floor division of the row sums through floor((n - k) / s) + 1."""
    out = []
    for n in mask.to(torch.int64).sum(1).tolist():
        for k, s in zip(kernels, strides):
            n = (n - k) // s + 1
        out.append(n)
    return out


def make_attention_mask(B: int, N: int, seed: int = 13) -> torch.Tensor:
    """int32 [B, N]: ragged prefixes with interior zeros punched in; row 1 all zero (when B > 1), row 0 full."""
    g = _gen(seed + B + N)
    lens = torch.randint(0, N + 1, (B,), generator=g)
    lens[0] = N
    m = (torch.arange(N)[None, :] < lens[:, None]).to(torch.int32)
    holes = torch.randint(0, N, (B, 3), generator=g)
    m[torch.arange(B)[:, None], holes] = 0
    m[0] = 1
    if B > 1:
        m[1] = 0
    return m


# ---- conv0 + LayerNorm + GELU ----------------------------------------------------------------------------------------
def make_conv0_params(gam: str = "plain"):
    """(w [512, 10], bias, gamma, beta) fp32.  'plain': a bias with a mean (so centring it matters) and the plain affine;
    'e': bias = 0, gamma with zeros and negative entries, beta = 0 (norm_ref.make_affine(..., 'e'))."""
    g = _gen(21)
    w = 0.3 * torch.randn(C0, K0, generator=g)
    bias = 0.05 * torch.randn(C0, generator=g) + 0.02
    gamma, beta = make_affine(C0, gam, seed=22)
    if gam == "e":
        bias = torch.zeros(C0)
    return w, bias, gamma, beta


def make_conv0_x(B: int, N: int, family: str = "noise", lengths=None, seed: int = 23) -> torch.Tensor:
    """fp32 [B, N]: zero-mean unit-variance noise as the model sees it, 'dc': the same plus 0.5; zeros past lengths."""
    x = torch.randn(B, N, generator=_gen(seed + B + N))
    if family == "dc":
        x = x + 0.5
    if lengths is not None:
        x = torch.where(torch.arange(N)[None, :] < torch.as_tensor(lengths)[:, None], x, torch.zeros(()))
    return x.contiguous()


def make_conv0_dy(B: int, T0: int, seed: int = 24) -> torch.Tensor:
    return torch.randn(B, T0, C0, generator=_gen(seed + B + T0)).bfloat16()


def conv0_frames(N: int, stride: int) -> int:
    return (N - K0) // stride + 1


def conv0_bwd_chain(B: int, T0: int, grid: int) -> int:
    """Longest addition chain of a conv0 parameter-gradient element: the frames a wave accumulates in registers (32 of a
    128-frame block, for each of the ceil(nblk / grid) blocks its workgroup walks), the 4 waves through LDS, then
    reduce_partials_kernel over `grid` workgroups (ceil(grid / 64) + 3 + 16) and 1 into the output."""
    nblk = B * -(-T0 // FPB)
    return (FPB // 4) * -(-nblk // grid) + 4 + -(-grid // 64) + 3 + 16 + 1


def _conv0_chunk(X, w, bias, gamma, beta, eps):
    """Forward of frames X [F, 10] (float64) with its error terms; see conv0_ref."""
    wc, bc = w - w.mean(0, keepdim=True), bias - bias.mean()
    vc = X @ wc.t() + bc
    var = (vc * vc).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    aX = X.abs()
    ms = (WAVE_DEPTH + 1) * U * (aX @ w.abs().mean(0)[:, None] + bias.abs().mean())   # [F, 1]
    e_vc = (K0 + 1) * U * (aX @ wc.abs().t() + bc.abs())                               # [F, C]
    rs = rstd * ((WAVE_DEPTH / 2 + 6) * U + 0.5 * (ms * rstd) ** 2 + rstd ** 2 * (vc.abs() * e_vc).mean(1, keepdim=True))
    h = vc * rstd
    z = h * gamma + beta
    e_h = (e_vc + ms) * rstd + vc.abs() * rs
    return vc, rstd, rs, h, z, e_h


def conv0_ref(x, w, bias, gamma, beta, stride, eps, dy=None, chain=0, init=0.0, batch=16, on_y=None):
    """Conv1d(1, 512, k = 10, stride) -> LayerNorm over the channels -> exact GELU of x [B, N], channels last, in float64,
    and (with dy [B, T0, 512]) its backward for the parameters.  Returns a dict:
      'y' [B, T0, 512], 'y_bound', and with dy 'dw' [512, 10], 'dbias', 'dgamma', 'dbeta' with 'dw_bound' ...
    Utterances are walked `batch` at a time.  With on_y, y and its bound are not kept: on_y(b0, y, y_bound) is called with
    each batch's [<= batch, T0, 512] pair instead, so nothing larger than that is ever alive.

    Forward bound.  The kernel centres weights and bias over the channels (w~ = w - mean_c w), so the taps yield v - mean
    directly.  A channel mean is a sum of depth 8 + 6 and a product: off by <= 15 u mean_c|w_j|, THE SAME for every
    channel, so the frame's values are shifted together by at most ms = 15 u (sum_j |x_j| mean_c|w_j| + mean|bias|) - the
    role mean_slack has in norm_ref.  Per channel, the subtraction that centres (u |w~|) and ten fused multiply-adds
    starting from the centred bias give e_vc = 11 u (|b~| + sum_j |w~_j| |x_j|).  The variance is mean(v^2) along a chain
    of depth 8 + 6: as norm_ref.fwd_stats_slack, rs = rstd ((depth / 2 + 6) u + (ms rstd)^2 / 2 + rstd^2 mean(|vc| e_vc)),
    the last term being what the per-channel errors do to it (d var = 2 mean(vc dv)).  Then z = v rstd gamma + beta:
      slack_z = 4 u (|h gamma| + |beta|) + e_h |gamma|,  e_h = (e_vc + ms) rstd + |vc| rs,
    and y = gelu(z) in bf16 as norm_ref.fwd_y_bound: 1.13 slack_z + |z| (1.5e-7 + 8 u) + u |y| + 2^-8 |y|.

    Backward bound.  With h^ off by e_h (+ u |h| for its product):
      e_du = |dy| (0.8 (e_h |gamma| + 4 u (|h gamma| + |beta|)) + 1.5e-7 + 8 u) + u |du|
      dgamma = sum du h: terms off by |h| e_du + |du| e_h + 3 u |du h|;  dbeta = sum du: terms off by e_du
      dh = du gamma, m1 = mean dh, m2 = mean dh h (depth 8 + 6):
        e_m1 = (depth + 2) u mean|dh| + mean(|gamma| e_du)
        e_m2 = (depth + 5) u mean|dh h| + mean(|gamma| e_du |h| + |dh| e_h)
      dv = rstd (dh - m1 - h m2):
        e_dv = rstd (|gamma| e_du + e_m1 + |h| e_m2 + e_h |m2| + 6 u (|dh| + |m1| + |h m2|)) + rs |dh - m1 - h m2|
      dbias = sum dv, dw_j = sum dv x_j (x exact, fused).
    Every sum runs along `chain` = conv0_bwd_chain(...) additions and lands on `init`:
      bound = (chain + 4) u sum|term| + sum e_term + u (|init| + |grad + init|)."""
    x = f64(x)
    w, bias, gamma, beta = f64(w), f64(bias), f64(gamma), f64(beta)
    B, N = x.shape
    T0 = conv0_frames(N, stride)
    out = {}
    if on_y is None:
        out = {"y": torch.empty(B, T0, C0, dtype=torch.float64), "y_bound": torch.empty(B, T0, C0, dtype=torch.float64)}
    acc = {k: [0.0, 0.0, 0.0] for k in ("dw", "dbias", "dgamma", "dbeta")}   # value, sum|term|, sum e_term
    for b0 in range(0, B, batch):
        xb = x[b0:b0 + batch]
        X = xb.unfold(1, K0, stride)[:, :T0].reshape(-1, K0)
        vc, rstd, rs, h, z, e_h = _conv0_chunk(X, w, bias, gamma, beta, eps)
        y = gelu64(z)
        slack_z = 4 * U * ((h * gamma).abs() + beta.abs()) + e_h * gamma.abs()
        yb = GELU_LIP * slack_z + z.abs() * (ERF_APPROX + 8 * U) + (U + BF16_HALF_ULP) * y.abs()
        if on_y is None:
            out["y"][b0:b0 + batch] = y.view(-1, T0, C0)
            out["y_bound"][b0:b0 + batch] = yb.view(-1, T0, C0)
        else:
            on_y(b0, y.view(-1, T0, C0), yb.view(-1, T0, C0))
        if dy is None:
            continue
        d = f64(dy[b0:b0 + batch]).reshape(-1, C0)
        du = d * dgelu64(z)
        e_du = d.abs() * (DGELU_LIP * (e_h * gamma.abs() + 4 * U * ((h * gamma).abs() + beta.abs())) + ERF_APPROX + 8 * U)
        e_du = e_du + U * du.abs()
        dh = du * gamma
        ge = gamma.abs() * e_du
        m1, m2 = dh.mean(1, keepdim=True), (dh * h).mean(1, keepdim=True)
        e_m1 = (WAVE_DEPTH + 2) * U * dh.abs().mean(1, keepdim=True) + ge.mean(1, keepdim=True)
        e_m2 = (WAVE_DEPTH + 5) * U * (dh * h).abs().mean(1, keepdim=True) + (ge * h.abs() + dh.abs() * e_h).mean(1, keepdim=True)
        inner = dh - m1 - h * m2
        dv = rstd * inner
        e_dv = rstd * (ge + e_m1 + h.abs() * e_m2 + e_h * m2.abs() + 6 * U * (dh.abs() + m1.abs() + (h * m2).abs()))
        e_dv = e_dv + rs * inner.abs()
        aX = X.abs()
        for key, val, mass, err in (("dgamma", (du * h).sum(0), (du * h).abs().sum(0),
                                     (h.abs() * e_du + du.abs() * e_h + 3 * U * (du * h).abs()).sum(0)),
                                    ("dbeta", du.sum(0), du.abs().sum(0), e_du.sum(0)),
                                    ("dbias", dv.sum(0), dv.abs().sum(0), e_dv.sum(0)),
                                    ("dw", dv.t() @ X, dv.abs().t() @ aX, e_dv.t() @ aX)):
            a = acc[key]
            a[0], a[1], a[2] = a[0] + val, a[1] + mass, a[2] + err
    if dy is not None:
        for key, (val, mass, err) in acc.items():
            out[key] = val
            out[key + "_bound"] = (chain + 4) * U * mass + err + U * (abs(init) + (val + init).abs())
    return out


# ---- col2im ----------------------------------------------------------------------------------------------------------------
COL2IM_SHAPES = [(2, 42, 16, 3, 2), (2, 1999, 512, 2, 2), (1, 57, 64, 10, 5), (1, 20, 8, 3, 1), (1, 9, 8, 1, 2),
                 (2, 3002, 64, 3, 2)]


def make_dcol(B, T, C, k, seed: int = 31) -> torch.Tensor:
    return torch.randn(B, T, k, C, generator=_gen(seed + T + C)).bfloat16()


def col2im_ref(dcol, L: int, stride: int):
    """(dx [B, L, C] float64, bound, covered [L] bool) of dcol [B, T, k, C]: dx[b, t s + j] += dcol[b, t, j], an index-add.
    The kernel adds the <= ceil(k / s) frames that cover a position in fp32 and rounds to bf16:
    bound = 2^-8 |dx| + ceil(k / s) u sum|term|; positions no frame covers have bound 0 and must be 0, and where one frame
    covers a position the fp32 sum is that bf16 value itself, so the result is exact (the caller compares bits)."""
    B, T, k, C = dcol.shape
    d = f64(dcol)
    pos = (torch.arange(T)[:, None] * stride + torch.arange(k)[None, :]).reshape(-1)
    dx = torch.zeros(B, L, C, dtype=torch.float64).index_add_(1, pos, d.reshape(B, T * k, C))
    mass = torch.zeros(B, L, C, dtype=torch.float64).index_add_(1, pos, d.abs().reshape(B, T * k, C))
    count = torch.zeros(L).index_add_(0, pos, torch.ones(T * k))
    bound = torch.where((count > 1)[None, :, None], BF16_HALF_ULP * dx.abs() + -(-k // stride) * U * mass, torch.zeros(()).double())
    return dx, bound, count > 0


# ---- masks, regroup --------------------------------------------------------------------------------------------------
def make_masks(B: int, T: int, C: int, seed: int = 41):
    """(tmask uint8 [B, T], fmask uint8 [B, C], flen int32 [B]) in which every row has a time-masked frame inside a
    feature span, a time-masked padded frame, and feature spans that cross padded frames."""
    g = _gen(seed + B + T)
    tmask = (torch.rand(B, T, generator=g) < 0.2).to(torch.uint8)
    fmask = (torch.rand(B, C, generator=g) < 0.1).to(torch.uint8)
    flen = torch.randint(T // 2, T - 2, (B,), generator=g).to(torch.int32)
    flen[0] = T - 3
    tmask[:, 1] = 1
    tmask[:, T - 1] = 1            # time and padding
    fmask[:, 3] = 1                # one masked channel inside a chunk of 8, and
    fmask[:, 16:24] = 1            # one whole chunk: with tmask[:, 1], time and feature
    return tmask, fmask, flen


def mask_frames_ref(h, tmask, fmask, embed, flen, order=("embed", "feature", "pad")):
    """h [B, T, C] bf16 -> masked copy, bit-exact: masked_spec_embed on time-masked frames, then zeros on masked
    channels, then zeros on padded frames.  `order` exists for the test that a different order is told apart."""
    h = h.clone()
    B, T, C = h.shape
    zero = torch.zeros((), dtype=h.dtype, device=h.device)
    for step in order:
        if step == "embed" and tmask is not None:
            h = torch.where(tmask.bool()[:, :, None], embed[None, None, :], h)
        elif step == "feature" and fmask is not None:
            h = torch.where(fmask.bool()[:, None, :], zero, h)
        elif step == "pad" and flen is not None:
            pad = torch.arange(T, device=h.device)[None, :] >= flen[:, None]
            h = torch.where(pad[:, :, None], zero, h)
    return h


def regroup_pad_ref(x, G: int, pad: int):
    """x [B, T, G Cg] -> [B, G, T + 2 pad, Cg] with zero time padding, bit-exact."""
    B, T, C = x.shape
    out = torch.zeros(B, G, T + 2 * pad, C // G, dtype=x.dtype, device=x.device)
    out[:, :, pad:pad + T] = x.view(B, T, G, C // G).permute(0, 2, 1, 3)
    return out


# ---- positional-conv weight norm -----------------------------------------------------------------------------------------
POSCONV_SHAPES = [(352, 32, 128), (360, 24, 128), (1024, 64, 128), (64, 8, 256), (64, 8, 16)]


def make_posconv(d, Cg, K, family: str = "plain", seed: int = 51):
    """(v [d, Cg, K], g [K], dw [d, Cg, K]) fp32.  'spread': the taps of v scaled over 1e-3 .. 1e3, so their norms differ
    by six orders of magnitude."""
    gen = _gen(seed + d + K)
    v = 0.1 * torch.randn(d, Cg, K, generator=gen)
    if family == "spread":
        v = v * torch.logspace(-3, 3, K)[torch.randperm(K, generator=gen)]
    g = 1.0 + 0.2 * torch.rand(K, generator=gen)
    dw = torch.randn(d, Cg, K, generator=gen)
    return v, g, dw


def posconv_chain(d: int, Cg: int, K: int) -> int:
    """Longest chain of a per-tap sum over the d Cg rows: a row lane of tap_dot_kernel adds every (256 / K)th row of its
    slab (four accumulators, joined in 2 more steps), the row lanes are added through LDS, then tap_finish_kernel over
    the 1024 slabs: 16 per accumulator, 3 to join, 16 part lanes."""
    per = -(-(d * Cg) // PCW_SLABS)
    nrl = 256 // K
    return -(-per // nrl) + 2 + nrl + PCW_SLABS // 64 + 3 + 16


def to_wf(w, Cg):
    """[d, Cg, K] -> the forward GEMM layout [G, co, j, ci]."""
    d, _, K = w.shape
    return w.view(d // Cg, Cg, Cg, K).permute(0, 1, 3, 2).contiguous()


def to_wb(w, Cg):
    """[d, Cg, K] -> the backward GEMM layout [G, ci, K - 1 - j, co]."""
    d, _, K = w.shape
    return w.flip(-1).view(d // Cg, Cg, Cg, K).permute(0, 2, 3, 1).contiguous()


def posconv_weight_ref(v, g):
    """(norm [K], w [d, Cg, K], norm_bound, w_bound (bf16)): w = g v / ||v||_(0,1).
    ||v||_j^2 is a sum of squares along posconv_chain additions, every term rounded once: relative (chain + 1) u, halved
    by the square root, which rounds itself (2 u granted): norm_bound = ((chain + 1) / 2 + 2) u norm.  w = v (g / norm^):
    a division and a product, 3 u more, and the rounding to bf16: w_bound = (2^-8 + ((chain + 1) / 2 + 5) u) |w|."""
    d, Cg, K = v.shape
    chain = posconv_chain(d, Cg, K)
    v, g = f64(v), f64(g)
    norm = torch.sqrt((v * v).sum((0, 1)))
    w = g * v / norm
    return norm, w, ((chain + 1) / 2 + 2) * U * norm, (BF16_HALF_ULP + ((chain + 1) / 2 + 5) * U) * w.abs()


def posconv_bwd_ref(dw, v, g, norm, dv0, dg0):
    """(dv, dg, dv_bound, dg_bound) with `norm` taken as given (the fp32 values the kernel reads) and dv0 / dg0 what the
    gradient buffers held: dot_j = sum dw v, dv = dv0 + (g / n) (dw - v dot / n^2), dg = dg0 + dot / n.
    dot: chain additions of once-rounded products: e_dot = (chain + 1) u sum|dw v|.  dg: the division and the addition:
    e_dot / n + 2 u |dot / n| + u |dg|.  dv: t = v dot / n^2 carries e_dot and four roundings (n n, v dot, the division,
    the subtraction's share), dw the subtraction's, the factor g / n two more, the addition into the buffer the last:
      |g / n| (|v| e_dot / n^2 + 4 u |t| + u |dw|) + 2 u |grad| + u |dv|."""
    d, Cg, K = v.shape
    chain = posconv_chain(d, Cg, K)
    dw, v, g, n, dv0, dg0 = f64(dw), f64(v), f64(g), f64(norm), f64(dv0), f64(dg0)
    dot = (dw * v).sum((0, 1))
    e_dot = (chain + 1) * U * (dw * v).abs().sum((0, 1))
    t = v * dot / (n * n)
    grad = (g / n) * (dw - t)
    dv, dg = dv0 + grad, dg0 + dot / n
    dv_bound = (g / n).abs() * (v.abs() * e_dot / (n * n) + 4 * U * t.abs() + U * dw.abs()) + 2 * U * grad.abs() + U * dv.abs()
    dg_bound = e_dot / n + 2 * U * (dot / n).abs() + U * dg.abs()
    return dv, dg, dv_bound, dg_bound

