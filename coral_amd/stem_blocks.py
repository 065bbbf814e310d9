"""What stands in front of and behind the encoder / decoder layers of blocks.py, as blocks of the same kind: forward with
saved activations + hand-written backward as sequences of libcoral_amd kernels, over a `ParamStore`, flat row-major
buffers and the caller's allocator z(n, dt=torch.bfloat16) (zero-filled).

  StridedConvBlock     a 1-D conv over channels-last rows as an implicit GEMM: the six strided convs of the wav2vec2
                       feature encoder and Whisper's conv1 / conv2
  ConvFeatureEncoder   wav2vec2: the fused layer 0 and six StridedConvBlock + LayerNorm + GELU
  FeatureProjection    wav2vec2: LayerNorm, projection, the `feat_proj` dropout site
  PosConvEmbed         wav2vec2: h0 + gelu(weight-normed grouped conv(h0))
  LMHead               final LayerNorm, optional dropout site, output projection (wav2vec2: lm_head with a bias; Whisper:
                       the tied token embedding)

Every name and offset is resolved once, in the constructors.  The loss kernels (CTC, cross-entropy), SpecAugment and the
activation backward of a conv (LayerNorm+GELU for wav2vec2, GELU for Whisper) stay with the engines.
"""

from __future__ import annotations

import torch

from . import ops
from .blocks import layernorm_bwd
from .ops import EPI_GELU_RESIDUAL, EPI_RESIDUAL, MNMAJOR

F32 = torch.float32


class ConvScratch:
    """Backward scratch of a stack of StridedConvBlocks for B clips: the fp32 weight-gradient partials of the convs
    `wgrad`, the im2col-layout data gradient of the convs `dgrad` (the ones whose backward gets a dx), and `part`, the
    caller's column-sum partials."""

    def __init__(self, z, B, wgrad, dgrad, part):
        nw = max(c.Co * c.k * c.Ci for c in wgrad)
        self.dwr_part, self.dwr = z(B * nw, F32), z(nw, F32)
        self.dcol = z(max(B * c.T * c.k * c.Ci for c in dgrad))
        self.part = part


class StridedConvBlock:
    """y[b, y_off + t, :] = W [x[b, stride t, :] | ... | x[b, stride t + k - 1, :]] + bias, t < T = (rows_in - k) / stride
    + 1, over clips of `rows_in` rows of Ci channels and `rows_out` rows of Co channels (default T): the A operand of the
    GEMM is the input itself, read as overlapping rows of k Ci elements stride Ci apart.  Time padding is the buffers'
    business: Whisper's conv1 (padding 1) reads a (Tin + 2)-row clip whose first and last rows stay zero and writes rows
    1 .. Tin of another one (y_off = 1), which conv2 reads.  The block owns the weight in GEMM layout [Co][k][Ci] (bf16)."""

    def __init__(self, store, weight: str, bias: str, Ci: int, Co: int, k: int, stride: int, rows_in=None, rows_out=None,
                 y_off: int = 0):
        self.st, self.Ci, self.Co, self.k, self.stride, self.y_off = store, Ci, Co, k, stride, y_off
        self.w_off, self.b_off = store.off(weight), store.off(bias)
        self.wr = torch.zeros(Co * k * Ci, dtype=torch.bfloat16, device=store.device)
        if rows_in is not None:
            self.set_rows(rows_in, rows_out)

    def set_rows(self, rows_in: int, rows_out=None):
        self.rows_in = rows_in
        self.T = (rows_in - self.k) // self.stride + 1
        self.rows_out = self.T if rows_out is None else rows_out
        assert self.y_off + self.T <= self.rows_out

    def refresh(self):
        ops.conv_weight_reorder(self.st.p32, self.wr, self.Co, self.Ci, self.k, w_off=self.w_off)

    def forward(self, x, y, B, **epilogue):
        """epilogue: the GEMM's (epilogue=, C2=, R=, r_off=, ldr=, sR=); y may be None with a C2."""
        Ci, Co, k = self.Ci, self.Co, self.k
        ops.gemm(x, self.wr, y, c_off=self.y_off * Co, M=self.T, N=Co, K=k * Ci, lda=self.stride * Ci, ldb=k * Ci, ldc=Co,
                 bias=self.st.p32, bias_off=self.b_off, batch2=B, sA=(0, self.rows_in * Ci), sC=(0, self.rows_out * Co),
                 **epilogue)

    def backward(self, dy, x, B, sc: ConvScratch, dx=None):
        """dy: the gradient wrt the conv's own output, in the output's layout (rows outside y_off .. y_off + T of a clip
        are not read); x: the forward's input.  Bias and weight gradients (+=) and, with dx, the gradient wrt x - every
        row of it is written, rows no window covers with 0."""
        Ci, Co, k, T = self.Ci, self.Co, self.k, self.T
        g32, nw = self.st.g32, Co * k * Ci
        # bias: the column sums of the T rows that count, of all clips at once where they are adjacent
        clips, rows = (1, B * T) if self.rows_out == T else (B, T)
        for b in range(clips):
            ops.colsum(dy, Co, rows, Co, g32, sc.part, x_off=(b * self.rows_out + self.y_off) * Co, out_off=self.b_off)
        # one TN GEMM per clip (batch dimension) into fp32 partials, summed afterwards: the single long-K GEMM has only
        # Co/128 x k*Ci/128 tiles
        ops.gemm(dy, x, sc.dwr_part, M=Co, N=k * Ci, K=T, a_layout=MNMAJOR, lda=Co, a_off=self.y_off * Co, b_layout=MNMAJOR,
                 ldb=self.stride * Ci, ldc=k * Ci, out_f32=True, batch2=B, sA=(0, self.rows_out * Co),
                 sB=(0, self.rows_in * Ci), sC=(0, nw))
        ops.reduce_rows(sc.dwr_part, B, nw, nw, sc.dwr)
        ops.conv_weight_grad_reorder(sc.dwr, g32, Co, Ci, k, dw_off=self.w_off)
        if dx is not None:
            assert self.rows_out == T, "the data gradient reads dy as one [B * T, Co] matrix"
            ops.gemm(dy, self.wr, sc.dcol, M=B * T, N=k * Ci, K=Co, lda=Co, b_layout=MNMAJOR, ldb=k * Ci, ldc=k * Ci)
            ops.col2im_1d(sc.dcol, dx, B, T, self.rows_in, Ci, k, self.stride)


class ConvFeatureEncoder:
    """The wav2vec2 feature encoder ($TF/models/wav2vec2/modeling_wav2vec2.py:291-298, 429-434): conv + LayerNorm + GELU
    seven times, layer 0 (one input channel) as the fused conv0 kernels, layers 1..6 as StridedConvBlocks followed by the
    LayerNorm+GELU kernel.  f32: the pre-norm tensors and the last layer's output stay fp32."""

    def __init__(self, store, prefix: str, conv_dim, conv_kernel, conv_stride, eps: float, f32: bool):
        assert conv_dim[0] == 512 and conv_kernel[0] == 10, "layer-0 kernel expects C=512,k=10"
        self.st, self.eps, self.f32 = store, eps, f32
        self.dims, self.k0, self.stride0 = tuple(conv_dim), conv_kernel[0], conv_stride[0]
        names = [[f"{prefix}{i}.{n}" for n in ("conv.weight", "conv.bias", "layer_norm.weight", "layer_norm.bias")]
                 for i in range(len(conv_dim))]
        self.p = [[store.view(n) for n in ns] for ns in names]          # weight, bias, gamma, beta of layer i
        self.g = [[store.view(n, "g32") for n in ns] for ns in names]   # ... and their gradients
        self.convs = [None] + [StridedConvBlock(store, names[i][0], names[i][1], conv_dim[i - 1], conv_dim[i], conv_kernel[i],
                                                conv_stride[i]) for i in range(1, len(conv_dim))]

    def refresh(self):
        for c in self.convs[1:]:
            c.refresh()

    def alloc(self, B, Ts, z, part):
        """Ts: the frames per clip behind each layer.  a[i]: layer i's output; y[i]: its conv's (pre-norm) output; dconv[i]:
        the gradient wrt a[i]; dy: the gradient wrt the current y[i] (the caller's scratch once the backward is through)."""
        n = [B * T * C for T, C in zip(Ts, self.dims)]
        bf, cdt = torch.bfloat16, F32 if self.f32 else torch.bfloat16
        for i, c in enumerate(self.convs[1:], 1):
            c.set_rows(Ts[i - 1])
        return dict(Ts=Ts, a=[z(m, dt=bf) for m in n[:-1]] + [z(n[-1], dt=cdt)], y=[None] + [z(m, dt=cdt) for m in n[1:]],
                    cstats=[None] + [z(B * T * 2, dt=F32) for T in Ts[1:]], dconv=[z(m) for m in n], dy=z(max(n[1:])),
                    sc=ConvScratch(z, B, self.convs[1:], self.convs[1:], part))

    def forward(self, x, sv, B, N):
        """x f32 [B, N] -> the last layer's output [B * Ts[-1], C]."""
        a, y, Ts = sv["a"], sv["y"], sv["Ts"]
        ops.conv0_fwd(x, *self.p[0], a[0], B, N, self.dims[0], self.k0, self.stride0, self.eps)
        for i, c in enumerate(self.convs[1:], 1):
            c.set_rows(Ts[i - 1])  # (of this saved state, whichever alloc came last)
            c.forward(a[i - 1], y[i], B)
            ops.layernorm_fwd(y[i], self.p[i][2], self.p[i][3], a[i], sv["cstats"][i], B * Ts[i], c.Co, self.eps, act=1)
        return a[-1]

    def backward(self, x, sv, B, N):
        """From sv["dconv"][-1], the gradient wrt the last layer's output, down to the parameters of layer 0."""
        dconv, dy, sc, Ts = sv["dconv"], sv["dy"], sv["sc"], sv["Ts"]
        for i in range(len(self.convs) - 1, 0, -1):
            c, (_, _, gamma, beta), (_, _, dgamma, dbeta) = self.convs[i], self.p[i], self.g[i]
            ops.layernorm_bwd(dconv[i], sv["y"][i], gamma, beta, sv["cstats"][i], None, dy, dgamma, dbeta, sc.part,
                              B * Ts[i], c.Co, act=1)
            c.backward(dy, sv["a"][i - 1], B, sc, dx=dconv[i - 1])
        ops.conv0_bwd(x, *self.p[0], dconv[0], *self.g[0], sc.part, B, N, self.dims[0], self.k0, self.stride0, self.eps)


class FeatureProjection:
    """h0 = dropout(LN(x) W^T + b) ($TF/models/wav2vec2/modeling_wav2vec2.py:429-434), x fp32 or bf16 [M, C]."""

    def __init__(self, store, prefix: str, C: int, d: int, eps: float):
        self.st, self.C, self.d, self.eps = store, C, d, eps
        ln = prefix + "layer_norm."
        self.gamma, self.beta = store.view(ln + "weight"), store.view(ln + "bias")
        self.dgamma, self.dbeta = store.view(ln + "weight", "g32"), store.view(ln + "bias", "g32")
        self.w_off, self.b_off = store.off(prefix + "projection.weight"), store.off(prefix + "projection.bias")

    def alloc(self, M, z):
        return dict(xln=z(M * self.C), st=z(M * 2, dt=F32))

    def forward(self, x, h0, sv, M, drop=(0.0, 0)):
        st, C, d = self.st, self.C, self.d
        ops.layernorm_fwd(x, self.gamma, self.beta, sv["xln"], sv["st"], M, C, self.eps)
        ops.gemm(sv["xln"], st.p16, h0, M=M, N=d, K=C, lda=C, ldb=C, ldc=d, b_off=self.w_off, bias=st.p32, bias_off=self.b_off)
        if drop[0] > 0:
            ops.dropout(h0, h0, M * d, *drop)

    def backward(self, dh0, x, dxln, dx, sv, M, part, drop=(0.0, 0)):
        """dh0: the gradient wrt h0 (masked in place with the forward's `drop`); dxln: scratch [M, C]; dx: out."""
        st, C, d = self.st, self.C, self.d
        if drop[0] > 0:
            ops.dropout(dh0, dh0, M * d, *drop)
        ops.colsum(dh0, d, M, d, st.g32, part, out_off=self.b_off)
        ops.gemm(dh0, sv["xln"], st.g32, M=d, N=C, K=M, a_layout=MNMAJOR, lda=d, b_layout=MNMAJOR, ldb=C, ldc=C,
                 c_off=self.w_off, out_f32=True, accumulate=True)
        ops.gemm(dh0, st.p16, dxln, M=M, N=C, K=d, lda=d, b_layout=MNMAJOR, ldb=C, ldc=C, b_off=self.w_off)
        ops.layernorm_bwd(dxln, x, self.gamma, None, sv["st"], None, dx, self.dgamma, self.dbeta, part, M, C)


class PosConvEmbed:
    """h = h0 + gelu(conv(h0) + b), the weight-normed grouped positional conv (K taps, G groups of Cg channels,
    $TF/models/wav2vec2/modeling_wav2vec2.py:765) as a grouped implicit GEMM over the regrouped, time-padded input
    xg [B, G, T + K, Cg].  The block owns the weights in GEMM layout, forward (wf) and flipped for the data gradient
    (wb), and the norm the weight-norm backward reads."""

    def __init__(self, store, prefix: str, d: int, G: int, K: int):
        self.st, self.d, self.G, self.K, self.Cg = store, d, G, K, d // G
        dev = store.device
        self.wf = torch.zeros(d * K * self.Cg, dtype=torch.bfloat16, device=dev)
        self.wb = torch.zeros(d * K * self.Cg, dtype=torch.bfloat16, device=dev)
        self.norm = torch.zeros(K, dtype=F32, device=dev)
        self.partial = torch.zeros(ops.posconv_partial_floats(K), dtype=F32, device=dev)
        w = prefix + "parametrizations.weight."
        self.v, self.g = store.view(w + "original1"), store.view(w + "original0")
        self.dv, self.dg = store.view(w + "original1", "g32"), store.view(w + "original0", "g32")
        self.b_off = store.off(prefix + "bias")

    def refresh(self):
        ops.posconv_weight(self.v, self.g, self.wf, self.wb, self.norm, self.partial, self.d, self.Cg, self.K)

    def alloc(self, B, T, z):
        """(+ 8 Cg: the GEMM's tile loads run past the last clip; xg / dxg's time padding stays the allocator's zeros)"""
        n = B * self.G * (T + self.K) * self.Cg + 8 * self.Cg
        return dict(xg=z(n), pc_pre=z(B * T * self.d), dxg=z(n), dwf=z(self.d * self.K * self.Cg, dt=F32))

    def _conv(self, T, Tpad):
        G, K, Cg, d = self.G, self.K, self.Cg, self.d
        return dict(M=T, N=Cg, K=K * Cg, lda=Cg, ldb=K * Cg, ldc=d, ldr=d, batch2=G, sA=(G * Tpad * Cg, Tpad * Cg),
                    sB=(0, Cg * K * Cg), sC=(T * d, Cg), sR=(T * d, Cg))

    def forward(self, h0, h, sv, B, T):
        st, G, K, Cg = self.st, self.G, self.K, self.Cg
        ops.regroup_pad(h0, sv["xg"], B, T, G, Cg, K // 2)
        ops.gemm(sv["xg"], self.wf, sv["pc_pre"], C2=h, R=h0, bias=st.p32, bias_off=self.b_off, epilogue=EPI_GELU_RESIDUAL,
                 batch1=B, sBias=(0, Cg), **self._conv(T, T + K))

    def backward(self, dh, dpc, dh0, sv, B, T, part):
        """dh: the gradient wrt h; dpc: scratch [B * T, d] for the one wrt the conv's output; dh0: out."""
        st, d, G, K, Cg = self.st, self.d, self.G, self.K, self.Cg
        M, Tpad = B * T, T + K
        ops.dgelu_mul(dh, sv["pc_pre"], dpc, M * d)
        ops.colsum(dpc, d, M, d, st.g32, part, out_off=self.b_off)
        # weight gradient in GEMM layout [G][Cg][K][Cg], then through the weight norm
        ops.gemm(dpc, sv["xg"], sv["dwf"], M=Cg, N=K * Cg, K=M, a_layout=MNMAJOR, lda=d, b_layout=MNMAJOR, ldb=Cg, b_kseg=T,
                 b_kseg_stride=G * Tpad * Cg, ldc=K * Cg, batch2=G, sA=(0, Cg), sB=(0, Tpad * Cg), sC=(0, Cg * K * Cg),
                 out_f32=True)
        ops.posconv_weight_bwd(sv["dwf"], self.v, self.g, self.norm, self.dv, self.dg, self.partial, d, Cg, K)
        # data gradient: correlation of the (left K/2 - 1 / right K/2) padded dpc with flipped weights
        ops.regroup_pad(dpc, sv["dxg"], B, T, G, Cg, K // 2)
        ops.gemm(sv["dxg"], self.wb, dh0, a_off=Cg, epilogue=EPI_RESIDUAL, R=dh, batch1=B, **self._conv(T, Tpad))


class LMHead:
    """logits = dropout(LN(h)) W^T (+ b), fp32 [rows, Vp] (Vp: V rounded up to 8; the pad columns are never written)."""

    def __init__(self, store, ln: str, weight: str, bias: str | None, d: int, V: int, eps: float):
        self.st, self.d, self.V, self.Vp, self.eps = store, d, V, (V + 7) // 8 * 8, eps
        self.gamma, self.beta = store.view(ln + ".weight"), store.view(ln + ".bias")
        self.dgamma, self.dbeta = store.view(ln + ".weight", "g32"), store.view(ln + ".bias", "g32")
        self.w_off = store.off(weight)
        self.b_off = store.off(bias) if bias is not None else None

    def alloc(self, M, z, train=True):
        return dict(hf=z(M * self.d), st=z(M * 2, dt=F32) if train else None)

    def forward(self, h, sv, M, logits=None, last_of=None, drop=(0.0, 0)):
        """The final LayerNorm of M rows of h into sv["hf"] (dropped in place: the weight gradient reads the dropped values)
        and the projection of every row, or with last_of=B of the last row of each of B sequences, into `logits`
        (default: a fresh buffer)."""
        d, hf = self.d, sv["hf"]
        ops.layernorm_fwd(h, self.gamma, self.beta, hf, sv["st"], M, d, self.eps)
        if drop[0] > 0:
            ops.dropout(hf, hf, M * d, *drop)
        if last_of is None:
            return self.project(hf, M, logits)
        return self.project(hf.view(last_of, M // last_of, d)[:, -1, :].contiguous(), last_of, logits)

    def project(self, rows, n, logits=None):
        """The projection of n rows of LayerNorm output."""
        if logits is None:
            # (torch.empty: the GEMM writes all V columns, the Vp - V pad columns are never read - no fill kernel per call)
            logits = torch.empty(n, self.Vp, dtype=F32, device=rows.device)
        d = self.d
        ops.gemm(rows, self.st.p16, logits, M=n, N=self.V, K=d, lda=d, ldb=d, ldc=self.Vp, b_off=self.w_off,
                 bias=None if self.b_off is None else self.st.p32, bias_off=self.b_off or 0)
        return logits

    def backward(self, dl, h, dhf, dh, sv, M, part, freeze=False, drop=(0.0, 0), xdrop=None):
        """dl: bf16 d logits [M, Vp]; h: the forward's input; dhf: scratch [M, d]; dh: out, the gradient wrt h (xdrop:
        blocks.layernorm_bwd).  Weight and bias gradients (+=); freeze: nothing below the projection is trained - the
        data gradient is not computed and dhf / dh stay as they are."""
        st, d, V, Vp = self.st, self.d, self.V, self.Vp
        ops.gemm(dl, sv["hf"], st.g32, M=V, N=d, K=M, a_layout=MNMAJOR, lda=Vp, b_layout=MNMAJOR, ldb=d, ldc=d,
                 c_off=self.w_off, out_f32=True, accumulate=True)
        if self.b_off is not None:
            ops.colsum(dl, Vp, M, Vp, st.g32, part, out_off=self.b_off)
        if freeze:
            return
        ops.gemm(dl, st.p16, dhf, M=M, N=d, K=V, lda=Vp, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=self.w_off)
        if drop[0] > 0:
            ops.dropout(dhf, dhf, M * d, *drop)
        layernorm_bwd(dhf, h, self.gamma, sv["st"], None, dh, self.dgamma, self.dbeta, part, M, d, xdrop)
