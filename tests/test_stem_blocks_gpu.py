"""coral_amd/stem_blocks.py on a real MI355X: StridedConvBlock and LMHead, forward and backward, against float64
torch.nn.functional.conv1d / matmul / layer_norm on the CPU.  `-m gpu` only.

Inputs, weights and incoming gradients are rounded to bf16 first, so the float64 statement sees exactly what the kernels
read and products of two of them are exact in fp32.  Bounds (the `within()` / ratio convention of test_frontend_gpu.py:
every comparison prints `ratio <name> <largest error / bound>`, a ratio above 1 fails), with U = 2^-24 the fp32 unit
roundoff and H = 2^-8 the largest relative error of a rounding to bf16:

  a sum of n fp32 terms t_i, in whatever order         |err| <= (n + 2) U sum |t_i|    =: acc(n, sum |t_i|)
                                                       (n - 1 additions, and one each for a bias and a final += into
                                                       the gradient buffer)
  ... stored as bf16                                   acc + H (|exact| + acc)

  conv / head forward (bf16 out)     n = k Ci / d
  bias, weight gradients (fp32)      n = the rows summed over, B T
  conv data gradient                 every window's im2col-layout entry is a bf16-stored sum over Co, col2im adds the
                                     (at most ceil(k / stride)) entries that overlap in fp32 and stores bf16
  head data gradient                 dhf = dl W is a bf16-stored sum over V; the LayerNorm backward behind it is compared
                                     with norm_ref's bound for it (LMHead adds nothing to that kernel)
"""
import collections
import math

import pytest
import torch
import torch.nn.functional as F

from norm_ref import BF16_HALF_ULP as H
from norm_ref import U, f64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0
RATIOS = collections.defaultdict(float)


def within(name, got, ref, bound):
    """assert |got - ref| <= bound element-wise (an exact result is inside a zero bound) and print the largest ratio."""
    err = (f64(got) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = float(torch.nan_to_num(r, nan=math.inf).max())
    RATIOS[name] = max(RATIOS[name], r)
    print("ratio %s %.3f" % (name, r))
    assert r <= 1.0, (name, r)


def acc(n, mag):
    return (n + 2) * U * mag


def as_bf16(n, mag, exact):
    a = acc(n, mag)
    return a + H * (exact.abs() + a)


def rb(t):
    """Rounded to bf16, as float64."""
    return t.bfloat16().double()


def store_of(shapes, values):
    from coral_amd.wav2vec2 import ParamStore

    st = ParamStore([(n, tuple(v.shape), "b") for n, v in zip(shapes, values)], torch.device(DEV))
    for n, v in zip(shapes, values):
        st.view(n).copy_(v.float())
    st.refresh_bf16()
    return st


def zeros(n, dt=torch.bfloat16):
    """The blocks' allocator."""
    return torch.zeros(n, dtype=dt, device=DEV)


def flat(t, dtype=torch.bfloat16, pad=4096):
    """t on the device as a flat buffer with `pad` elements of sentinel behind it."""
    out = torch.full((t.numel() + pad,), SENT, dtype=dtype, device=DEV)
    out[:t.numel()] = t.reshape(-1).to(DEV, dtype)
    return out


# geometry: k, stride, rows_in, rows_out (None: the T output frames, dense), y_off, whether the backward gets a dx
GEOMETRIES = {"a_k3_s2_uncovered_tail": (3, 2, 12, None, 0, True), "b_k2_s2": (2, 2, 11, None, 0, True),
              "c_whisper_conv1": (3, 1, 12, 12, 1, False)}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_strided_conv_block(geo):
    from coral_amd import ops
    from coral_amd.stem_blocks import ConvScratch, StridedConvBlock

    k, stride, rows_in, rows_out, y_off, with_dx = GEOMETRIES[geo]
    B, Ci, Co = 2, 16, 40   # off the 128-wide tile
    T = (rows_in - k) // stride + 1
    assert T == {"a_k3_s2_uncovered_tail": 5, "b_k2_s2": 5, "c_whisper_conv1": 10}[geo]
    g = torch.Generator().manual_seed(k * 100 + stride * 10 + rows_in)
    x, w, b = rb(torch.randn(B, rows_in, Ci, generator=g)), rb(torch.randn(Co, Ci, k, generator=g) * 0.2), rb(torch.randn(Co, generator=g))
    st = store_of(["w", "b"], [w, b])
    blk = StridedConvBlock(st, "w", "b", Ci, Co, k, stride, rows_in=rows_in, rows_out=rows_out, y_off=y_off)
    blk.refresh()
    R = blk.rows_out
    assert blk.T == T and R == (T if rows_out is None else rows_out)

    # forward: every row of y outside y_off .. y_off + T keeps the sentinel
    xd = flat(x)
    y = torch.full((B * R + 2, Co), SENT, dtype=torch.bfloat16, device=DEV)
    blk.forward(xd, y.view(-1), B)
    torch.cuda.synchronize()
    yc = y.cpu()
    ref = F.conv1d(x.transpose(1, 2), w, b, stride=stride).transpose(1, 2)                       # [B, T, Co]
    mag = F.conv1d(x.abs().transpose(1, 2), w.abs(), b.abs(), stride=stride).transpose(1, 2)
    got = yc[:B * R].view(B, R, Co)
    within("conv_fwd.y", got[:, y_off:y_off + T], ref, as_bf16(k * Ci, mag, ref))
    rest = torch.ones(R, dtype=torch.bool)
    rest[y_off:y_off + T] = False
    assert bool((got[:, rest] == SENT).all()) and bool((yc[B * R:] == SENT).all())

    # backward.  Geometry c: the padding rows of dy hold a large value that no gradient may see
    dy = rb(torch.randn(B, R, Co, generator=g))
    dy[:, rest] = 1000.0
    dyv = dy[:, y_off:y_off + T]                                                                   # the rows that count
    part = torch.zeros(max(4096, ops.colsum_partial_floats(B * R, Co)), dtype=torch.float32, device=DEV)
    sc = ConvScratch(zeros, B, (blk,), (blk,), part)
    dx = torch.full((B * rows_in + 2, Ci), SENT, dtype=torch.bfloat16, device=DEV) if with_dx else None
    blk.backward(flat(dy), xd, B, sc, dx=None if dx is None else dx.view(-1))
    torch.cuda.synchronize()
    n = B * T
    within("conv_bwd.dbias", st.view("b", "g32"), dyv.sum((0, 1)), acc(n, dyv.abs().sum((0, 1))))
    win = x.unfold(1, k, stride)                                                                    # [B, T, Ci, k]
    within("conv_bwd.dw", st.view("w", "g32"), torch.einsum("bto,btck->ock", dyv, win),
           acc(n, torch.einsum("bto,btck->ock", dyv.abs(), win.abs())))
    if not with_dx:
        return
    dxc = dx.cpu()
    assert bool((dxc[B * rows_in:] == SENT).all())
    col = torch.einsum("bto,ock->btkc", dyv, w)                                                     # [B, T, k, Ci]
    colb = as_bf16(Co, torch.einsum("bto,ock->btkc", dyv.abs(), w.abs()), col)
    dref, dmag, dbound = (torch.zeros(B, rows_in, Ci, dtype=torch.float64) for _ in range(3))
    covered = torch.zeros(rows_in, dtype=torch.bool)
    for t in range(T):
        for j in range(k):
            dref[:, t * stride + j] += col[:, t, j]
            dmag[:, t * stride + j] += col[:, t, j].abs() + colb[:, t, j]
            dbound[:, t * stride + j] += colb[:, t, j]
            covered[t * stride + j] = True
    dbound = dbound + as_bf16(-(-k // stride), dmag, dref.abs() + dbound)
    got = dxc[:B * rows_in].view(B, rows_in, Ci)
    within("conv_bwd.dx", got[:, covered], dref[:, covered], dbound[:, covered])
    if geo == "a_k3_s2_uncovered_tail":
        assert not bool(covered[11]) and int((~covered).sum()) == 1
    assert bool((got[:, ~covered].view(torch.int16) == 0).all())     # rows no window covers: exactly +0 over the sentinel


@pytest.mark.parametrize("bias", [True, False])
def test_lm_head(bias):
    import norm_ref
    from coral_amd import ops
    from coral_amd.stem_blocks import LMHead

    M, d, V, eps = 7, 32, 45, 1e-5
    g = torch.Generator().manual_seed(5 + bias)
    h, W = rb(torch.randn(M, d, generator=g) * 2 + 0.5), rb(torch.randn(V, d, generator=g) * 0.3)
    gamma, beta, bv = ((1.0 + 0.1 * torch.randn(d, generator=g)).double(), torch.randn(d, generator=g).double(),
                       torch.randn(V, generator=g).double())                 # fp32 values: the kernels read these from p32
    st = store_of(["ln.weight", "ln.bias", "w", "b"], [gamma, beta, W, bv])
    head = LMHead(st, "ln", "w", "b" if bias else None, d, V, eps)
    Vp = head.Vp
    assert Vp == 48
    sv = head.alloc(M, zeros)

    # forward
    hd = flat(h)
    logits = torch.full((M + 1, Vp), SENT, dtype=torch.float32, device=DEV)
    out = head.forward(hd, sv, M, logits=logits.view(-1))
    torch.cuda.synchronize()
    assert out.data_ptr() == logits.data_ptr()
    hf = f64(sv["hf"]).view(M, d)            # the LayerNorm output as the projection read it (bf16)
    hf_ref = F.layer_norm(h, (d,), gamma, beta, eps)
    within("head_fwd.hf", hf, hf_ref, norm_ref.fwd_y_bound(h, gamma, beta, eps, 0, True))   # (the LayerNorm kernel's bound)
    b64 = bv if bias else torch.zeros(V, dtype=torch.float64)
    lref = hf @ W.T + b64
    lc = logits.cpu()
    within("head_fwd.logits", lc[:M, :V], lref, acc(d, hf.abs() @ W.abs().T + b64.abs()))
    assert bool((lc[:M, V:] == SENT).all()) and bool((lc[M] == SENT).all())     # pad columns are never written
    # last_of: the last row of each of B sequences, here 7 sequences of 1 row and 1 sequence of 7 rows
    for B in (7, 1):
        got = head.forward(hd, sv, M, last_of=B)
        torch.cuda.synchronize()
        assert got.shape == (B, Vp)
        assert torch.equal(got[:, :V].cpu(), lc[:M, :V].view(B, M // B, V)[:, -1])

    # backward
    dl = rb(torch.randn(M, Vp, generator=g))
    dl[:, V:] = 0
    dld = flat(dl)
    part = torch.zeros(max(4096, ops.layernorm_bwd_partial_floats(M, d), ops.colsum_partial_floats(M, Vp)),
                       dtype=torch.float32, device=DEV)
    dhf, dh = (torch.full((M + 1, d), SENT, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    head.backward(dld, hd, dhf.view(-1), dh.view(-1), sv, M, part, freeze=True)
    torch.cuda.synchronize()
    dlv = dl[:, :V]
    within("head_bwd.dw", st.view("w", "g32"), dlv.T @ hf, acc(M, dlv.abs().T @ hf.abs()))
    if bias:
        within("head_bwd.db", st.view("b", "g32"), dlv.sum(0), acc(M, dlv.abs().sum(0)))
    else:
        assert not bool(st.view("b", "g32").any())
    # freeze: nothing below the projection - the data-gradient buffers are untouched, no LayerNorm gradient
    assert bool((dhf == SENT).all()) and bool((dh == SENT).all())
    assert not bool(st.view("ln.weight", "g32").any()) and not bool(st.view("ln.bias", "g32").any())
    st.g32.zero_()
    head.backward(dld, hd, dhf.view(-1), dh.view(-1), sv, M, part)
    torch.cuda.synchronize()
    within("head_bwd.dw", st.view("w", "g32"), dlv.T @ hf, acc(M, dlv.abs().T @ hf.abs()))
    dhf_ref = dlv @ W
    within("head_bwd.dhf", dhf[:M], dhf_ref, as_bf16(V, dlv.abs() @ W.abs(), dhf_ref))
    assert bool((dhf[M] == SENT).all()) and bool((dh[M] == SENT).all())
    # the LayerNorm backward of the dhf and the statistics the kernels produced: norm_ref's float64 statement and bounds
    # (tests/test_norm_gpu.py), the parameter gradients through the kernel's own second stage into a zeroed buffer
    stats = f64(sv["st"]).view(M, 2)
    args = (f64(dhf[:M]), h, gamma, beta, stats[:, 0], stats[:, 1], None, 0)
    dxr, dgr, dbr = norm_ref.ln_bwd_ref(*args)
    grid = ops.layernorm_bwd_partial_floats(M, d) // (2 * d)
    b = norm_ref.bwd_bounds(*args, norm_ref.bwd_chain(M, grid))
    within("head_bwd.dh", dh[:M], dxr, b["dx"])
    within("head_bwd.dgamma", st.view("ln.weight", "g32"), dgr, b["dgamma"])
    within("head_bwd.dbeta", st.view("ln.bias", "g32"), dbr, b["dbeta"])
