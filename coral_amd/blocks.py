"""Pre-LN transformer sub-blocks (forward with saved activations + hand-written backward) as sequences
of libcoral_amd kernels, and the backward schedule of a stack of pre-LN encoder layers (encoder_backward).
The three block kinds are exactly the ones of `WhisperEncoderLayer` / `WhisperDecoderLayer`
($TF/models/whisper/modeling_whisper.py:379-413, 448-505): residual self-attention, residual cross-attention,
residual GELU feed-forward.  The Whisper engines build their encoder and decoder layers from them (the training
forward, `encode`, the teacher-forced `decode` and the feed-forward of the incremental decoding paths); the
wav2vec2 engine its XLS-R encoder layers (the stable-LayerNorm layer, $TF/models/wav2vec2/modeling_wav2vec2.py:
611-654, is the same pre-LN self-attention + feed-forward pair).  What stands around the layers - the strided convs of
both front ends, the wav2vec2 feature projection and positional conv, the final LayerNorm + output projection of both
models - are blocks of the same kind in stem_blocks.py.

Every block works on flat row-major bf16 activations [B*T, d] and a `ParamStore` (fp32 masters `p32`,
bf16 compute copies `p16`, fp32 gradients `g32`); weight gradients are accumulated in fp32.  Workspaces come
from the caller's allocator z(n, dt=torch.bfloat16) (zero-filled).  alloc(..., train=False) is the inference form:
the buffers only a backward reads (LayerNorm statistics, Dq, the FFN pre-activation) are None, a forward into it
writes only what its next launch consumes and keeps nothing for a backward, and the FFN of M <= 128 rows runs its
LayerNorm inside fc1's prologue (LN_IN_GEMM).

Packed rows: SelfAttnBlock.forward / .backward and encoder_backward take rows=(row_off, Mp) - the valid
frames of the B utterances laid end to end, utterance b at rows row_off[b] .. row_off[b + 1] (int32 [B + 1] on the
device) of every [rows, *] buffer, Mp = row_off[B] as a host integer.  Every GEMM, LayerNorm, column sum and
weight-gradient problem then runs on Mp rows and the attention kernels address the utterances through
CaAttnDesc.row_off; T stays the longest utterance's frame count (grid and lse / Dq layout).  None = the [B, T] layout.

fp8: a forward takes its e4m3 operands per call, dict(w=(p8, scale, x8, rs)) for q|k|v / fc1 (the
e4m3 weights, the matrix's dequantisation factor, the LayerNorm output as e4m3 and its row scales); the training
forward adds out= / fc2= (the attention / GELU output as e4m3, see WhisperTrainEngine._train_ws) and bwd= / du= (the
fp8 data gradients), which the backward finds in the saved states.
"""

from __future__ import annotations

import os

import torch

from . import ops
from .ops import EPI_DGELU, EPI_GELU, EPI_RESIDUAL, MNMAJOR


# A decoded token's LayerNorms inside the following projection's prologue (CA_DECODE_LN_FUSED=0: their own launches -
# the A/B switch; the results are bit-identical): the inference FFN of M <= 128 rows, and the incremental decoding paths
LN_IN_GEMM = os.environ.get("CA_DECODE_LN_FUSED", "1") != "0"


def _z(n, dev, dt=torch.bfloat16):
    return torch.zeros(n, dtype=dt, device=dev)


def zeros_on(dev):
    """The allocator of a workspace made of separate zero-filled tensors."""
    return lambda n, dt=torch.bfloat16: _z(n, dev, dt)


class Scratch:
    """Shared backward scratch for one (rows, d, f) problem size.  masks=False: no dropout(dh) buffers (the caller
    hands the blocks their masked gradients, encoder_backward's `mring`)."""

    def __init__(self, M, d, f, z, Mkv=0, masks=True):
        self.dx = z(M * d)
        # (a self-attention block's dctx is dead before its dx is written; the cross-attention block needs both)
        self.dctx = z(M * d) if Mkv else self.dx
        self.dqkv = z(M * 3 * d)
        self.du = z(M * f)
        self.dkv = z(Mkv * 2 * d) if Mkv else None
        self.dq = z(M * d) if Mkv else None  # cross-attention dq: lives until the layer's deferred weight gradients
        # dropout(dh): the gradient entering a sub-layer whose output was dropped (hidden dropout); one buffer per block
        # kind so that a layer's deferred weight gradients can read both
        self.dm = {"attn": z(M * d), "ffn": z(M * d), "cross": z(M * d)} if masks else None
        npart = max(ops.layernorm_bwd_partial_floats(M, d), ops.colsum_partial_floats(max(M, Mkv), max(f, 3 * d)), 4096)
        self.part = z(npart, torch.float32)


def _masked_grad(dh, sv, sc: "Scratch", n, kind):
    """Gradient wrt the sub-layer output: dh itself, or dropout(dh) with the forward's mask when the output went
    through hidden-state dropout before the residual add."""
    p, seed = sv.get("hdrop", (0.0, 0))
    if p <= 0.0:
        return dh
    ops.dropout(dh, sc.dm[kind], n, p, seed)
    return sc.dm[kind]


def _masked_grad_fp8(dh, sv, sc: "Scratch", M, d, kind, fb):
    """_masked_grad on the fp8 path: the same bf16 dropout(dh) (or dh itself) for the weight gradient, and in the same pass
    the rows as e4m3 with one scale per row (fb = (p8t, w_off, dy8, row_scale, inv_w)) - the A operand of the sub-layer's
    data gradient through ca_gemm_fp8 against the transposed e4m3 weight copy."""
    p, seed = sv.get("hdrop", (0.0, 0))
    ops.dropout_rows_fp8(dh, sc.dm[kind] if p > 0.0 else None, fb[2], fb[3], M, d, p, seed)
    return sc.dm[kind] if p > 0.0 else dh


def layernorm_bwd(dy, x, gamma, stats, dres, dx, dgamma, dbeta, part, M, d, xdrop=None):
    """dx = dres + LN'(dy).  xdrop = (p, seed, buf): the same pass also leaves dropout(dx) in buf - the gradient of the
    sub-layer below when its output went through hidden dropout (ca_layernorm_bwd_dropout)."""
    if xdrop is None:
        ops.layernorm_bwd(dy, x, gamma, None, stats, dres, dx, dgamma, dbeta, part, M, d)
    else:
        ops.layernorm_bwd_dropout(dy, x, gamma, None, stats, dres, dx, xdrop[2], xdrop[0], xdrop[1], dgamma, dbeta, part,
                                  M, d)


def _ln_bwd(st, ln, dx, sv, dh, dhin, sc: "Scratch", M, d, ln_part, pending, xdrop=None):
    """The pre-norm's backward: dhin = dh + LN'(dx) (and dropout(dhin), see layernorm_bwd).  d gamma | d beta (adjacent
    in the flat buffer) either reduced right away, or left as partials in `ln_part` with the reduction appended to
    `pending`."""
    if pending is None:
        layernorm_bwd(dx, sv["hin"], st.view(ln + ".weight"), sv["st"], dh, dhin, st.view(ln + ".weight", "g32"),
                      st.view(ln + ".bias", "g32"), sc.part, M, d, xdrop)
        return
    layernorm_bwd(dx, sv["hin"], st.view(ln + ".weight"), sv["st"], dh, dhin, None, None, ln_part, M, d, xdrop)
    pending.append((ln_part, ops.layernorm_bwd_partial_floats(M, d) // (2 * d), 2 * d, 2 * d, st.g32[st.off(ln + ".weight"):], True))


class SelfAttnBlock:
    """h_out = h_in + out_proj(attn(q, k, v)),  q|k|v = LN(h_in) Wqkv^T + bqkv."""

    def __init__(self, store, ln: str, attn: str, H: int, d: int, eps: float, causal: bool, qbias: str):
        self.st, self.ln, self.attn, self.H, self.d, self.eps, self.causal = store, ln, attn, H, d, eps, causal
        self.qbias = qbias  # name of the first of the three adjacent bias vectors (q, k, v)
        # positions of this block's bias gradients in the layer's contiguous bias vector (fused column sums of a
        # grouped weight-gradient launch); the encoder layout, a decoder layer sets its own
        self.cs_qkv, self.cs_o = 0, 3 * d

    def alloc(self, B, T, z, train=True):
        d, H = self.d, self.H
        Tqp = (T + 31) // 32 * 32
        return dict(x=z(B * T * d), st=z(B * T * 2, torch.float32) if train else None, qkv=z(B * T * 3 * d),
                    ctx=z(B * T * d), lse=z(B * H * Tqp, torch.float32),
                    Dq=z(B * H * Tqp, torch.float32) if train else None, Tqp=Tqp)

    def _akw(self, B, T, Tqp, klen, adrop, rows=None):
        d, H = self.d, self.H
        hd = d // H
        if rows is not None:  # packed rows: the utterance's own length is its key count (no klen)
            return dict(self._akw(B, T, Tqp, None, adrop), row_off=rows[0])
        return dict(B=B, H=H, Tq=T, Tk=T, hd=hd, Tqp=Tqp, scale=hd ** -0.5, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d,
                    sqb=T * 3 * d, skb=T * 3 * d, svb=T * 3 * d, sob=T * d, q_off=0, k_off=d, v_off=2 * d, klen=klen,
                    causal=self.causal, dropout_p=adrop[0], dropout_seed=adrop[1])

    def forward(self, hin, hout, sv, B, T, klen=None, hdrop=(0.0, 0), adrop=(0.0, 0), fp8=None, rows=None):
        """hdrop: (p, seed) of the hidden-state dropout on the block's output; adrop: of the dropout on the attention
        probabilities ($TF/models/whisper/modeling_whisper.py:234); fp8: this call's e4m3 operands (module docstring);
        rows: packed rows (module docstring; bf16 path only, klen is then implied)."""
        st, d = self.st, self.d
        M = B * T if rows is None else rows[1]
        if rows is not None and fp8 is not None:
            raise ops.CoralAmdError("SelfAttnBlock: packed rows are not implemented on the fp8 path")
        train = sv["st"] is not None
        if fp8 is not None:
            p8, scale, x8, rs = fp8["w"]
            ops.layernorm_fwd_fp8(hin, st.view(self.ln + ".weight"), st.view(self.ln + ".bias"), sv["x"] if train else None,
                                  x8, rs, M, d, self.eps, stats=sv["st"])
            ops.gemm_fp8(x8, p8, sv["qkv"], a_row_scale=rs, b_scale=scale, M=M, N=3 * d, K=d, lda=d, ldb=d, ldc=3 * d,
                         b_off=st.off(self.attn + "q_proj.weight"), bias=st.p32, bias_off=st.off(self.qbias))
        else:
            ops.layernorm_fwd(hin, st.view(self.ln + ".weight"), st.view(self.ln + ".bias"), sv["x"], sv["st"], M, d, self.eps)
            ops.gemm(sv["x"], st.p16, sv["qkv"], M=M, N=3 * d, K=d, lda=d, ldb=d, ldc=3 * d,
                     b_off=st.off(self.attn + "q_proj.weight"), bias=st.p32, bias_off=st.off(self.qbias))
        akw = self._akw(B, T, sv["Tqp"], klen, adrop, rows)
        o8 = fp8.get("out") if (fp8 is not None and T >= 100 and adrop[0] == 0.0) else None
        if o8 is not None:
            # out_proj on the fp8 path: the attention kernel's output stage also writes the context as e4m3 (delayed
            # per-tensor scale, CaAttnDesc.O8)
            ops.attn_fwd(sv["qkv"], sv["qkv"], sv["qkv"], sv["ctx"], sv["lse"], O8=o8[0], o8_scale=o8[1], o8_amax=o8[3], **akw)
            ops.gemm_fp8(o8[0], p8, hout, a_scale=o8[2], b_scale=o8[4], M=M, N=d, K=d, lda=d, ldb=d, ldc=d,
                         b_off=st.off(self.attn + "out_proj.weight"), bias=st.p32, bias_off=st.off(self.attn + "out_proj.bias"),
                         epilogue=EPI_RESIDUAL, R=hin, ldr=d, dropout_p=hdrop[0], dropout_seed=hdrop[1])
        else:
            ops.attn_fwd(sv["qkv"], sv["qkv"], sv["qkv"], sv["ctx"], sv["lse"], **akw)
            ops.gemm(sv["ctx"], st.p16, hout, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=st.off(self.attn + "out_proj.weight"),
                     bias=st.p32, bias_off=st.off(self.attn + "out_proj.bias"), epilogue=EPI_RESIDUAL, R=hin, ldr=d,
                     dropout_p=hdrop[0], dropout_seed=hdrop[1])
        if train:
            sv.update(hin=hin, klen=klen, hdrop=hdrop, adrop=adrop, fp8=fp8, rows=rows)

    def backward(self, dh, dhin, sv, sc: Scratch, B, T, defer=None, acc=True, sq=None, ln_part=None, pending=None,
                 dy=None, xdrop=None, deferred=None, rows=None):
        """dh: grad wrt h_out (kept intact); dhin: output buffer for grad wrt h_in (may alias nothing of sv).
        ln_part / pending: leave the norm's d gamma | d beta partials in `ln_part` and append their second-stage
        reduction to `pending` (the caller runs a layer's reductions as one launch, ops.reduce_rows_multi).
        defer: list collecting the block's weight-gradient problems instead of launching them (the caller launches
        the whole layer's group once dh and sc.dqkv are no longer needed elsewhere); deferred(): called as soon as
        they are in the list, before the q|k|v data gradient.  acc=False: the weight gradients overwrite (first
        micro-batch of a step, matrices not cleared); sq: {"o": (slots, off), "qkv": ...} where the weight-gradient GEMMs
        leave their per-tile sums of squares (CaGemmDesc.c_sumsq).  dy: the gradient wrt the output before hidden
        dropout, computed by the caller (default: dropout(dh) here); xdrop: see layernorm_bwd.  rows: the forward's
        packed rows (module docstring)."""
        sq = sq or {}
        st, d = self.st, self.d
        M = B * T if rows is None else rows[1]
        o, g32, p16 = st.off, st.g32, st.p16
        fb = sv["fp8"].get("bwd") if sv["fp8"] is not None else None
        if dy is None:
            dy = _masked_grad(dh, sv, sc, M * d, "attn") if fb is None else _masked_grad_fp8(dh, sv, sc, M, d, "attn", fb)
        # with `defer` the bias gradients travel with the problems (fused into the grouped launch or done by it)
        if defer is None:
            ops.colsum(dy, d, M, d, g32, sc.part, out_off=o(self.attn + "out_proj.bias"))
        wg = [dict(dY=dy, X=sv["ctx"], M=d, N=d, K=M, lda=d, ldb=d, c_off=o(self.attn + "out_proj.weight"), accumulate=acc,
                   sq=sq.get("o"),
                   **(dict(bias_off=o(self.attn + "out_proj.bias"), part=sc.part, cs_off=self.cs_o) if defer is not None else {}))]
        if fb is not None:  # data gradient of out_proj on the fp8 path: e4m3 dY (row scales) x transposed e4m3 weights
            ops.gemm_fp8(fb[2], fb[0], sc.dctx, a_row_scale=fb[3], b_scale=fb[4], M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=fb[1])
        else:
            ops.gemm(dy, p16, sc.dctx, M=M, N=d, K=d, lda=d, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=o(self.attn + "out_proj.weight"))
        qkv, dqkv = sv["qkv"], sc.dqkv
        ops.attn_bwd(qkv, qkv, qkv, sv["ctx"], sv["lse"], sc.dctx, sv["Dq"], dqkv, dqkv, dqkv, lddo=d, sdob=T * d, lddq=3 * d,
                     lddk=3 * d, lddv=3 * d, sdqb=T * 3 * d, sdkb=T * 3 * d, sdvb=T * 3 * d, dq_off=0, dk_off=d, dv_off=2 * d,
                     **self._akw(B, T, sv["Tqp"], sv["klen"], sv["adrop"], rows))
        if defer is None:
            ops.colsum(dqkv, 3 * d, M, 3 * d, g32, sc.part, out_off=o(self.qbias))
        wg.append(dict(dY=dqkv, X=sv["x"], M=3 * d, N=d, K=M, lda=3 * d, ldb=d, c_off=o(self.attn + "q_proj.weight"),
                       accumulate=acc, sq=sq.get("qkv"),
                       **(dict(bias_off=o(self.qbias), part=sc.part, cs_off=self.cs_qkv) if defer is not None else {})))
        if defer is not None:
            defer.extend(wg)
            if deferred is not None:
                deferred()
        else:
            ops.wgrad_gemm_group(wg, g32)  # both weight gradients of the block in one grouped launch
        ops.gemm(dqkv, p16, sc.dx, M=M, N=d, K=3 * d, lda=3 * d, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=o(self.attn + "q_proj.weight"))
        _ln_bwd(st, self.ln, sc.dx, sv, dh, dhin, sc, M, d, ln_part, pending, xdrop)


class CrossAttnBlock:
    """h_out = h_in + out_proj(attn(q, K, V)) with q from LN(h_in) and K|V = enc Wkv^T + [0|bv] [B*Te, 2d]."""

    def __init__(self, store, ln: str, attn: str, H: int, d: int, eps: float):
        self.st, self.ln, self.attn, self.H, self.d, self.eps = store, ln, attn, H, d, eps

    def alloc(self, B, L, Te, z, train=True):
        """(train=False: no K|V buffer either - the forward then takes the caller's, `kv=`)"""
        d, H = self.d, self.H
        Lqp = (L + 31) // 32 * 32
        return dict(x=z(B * L * d), st=z(B * L * 2, torch.float32) if train else None, q=z(B * L * d), ctx=z(B * L * d),
                    kv=z(B * Te * 2 * d) if train else None, lse=z(B * H * Lqp, torch.float32),
                    Dq=z(B * H * Lqp, torch.float32) if train else None, Tqp=Lqp)

    def _akw(self, B, L, Te, Tqp, adrop):
        d, H = self.d, self.H
        hd = d // H
        return dict(B=B, H=H, Tq=L, Tk=Te, hd=hd, Tqp=Tqp, scale=hd ** -0.5, ldq=d, ldk=2 * d, ldv=2 * d, ldo=d,
                    sqb=L * d, skb=Te * 2 * d, svb=Te * 2 * d, sob=L * d, k_off=0, v_off=d, dropout_p=adrop[0],
                    dropout_seed=adrop[1])

    def project_kv(self, enc, sv, B, Te):
        """K|V of the encoder states into sv["kv"] (returned)."""
        st, d = self.st, self.d
        ops.gemm(enc, st.p16, sv["kv"], M=B * Te, N=2 * d, K=d, lda=d, ldb=d, ldc=2 * d, b_off=st.off(self.attn + "k_proj.weight"),
                 bias=st.p32, bias_off=st.off(self.attn + "k_proj.bias__zero"))
        sv["enc"] = enc
        return sv["kv"]

    def forward(self, hin, hout, sv, B, L, Te, kv=None, hdrop=(0.0, 0), adrop=(0.0, 0)):
        """kv: the K|V of the encoder states (default: sv["kv"], project_kv's)."""
        st, d = self.st, self.d
        M = B * L
        kv = sv["kv"] if kv is None else kv
        ops.layernorm_fwd(hin, st.view(self.ln + ".weight"), st.view(self.ln + ".bias"), sv["x"], sv["st"], M, d, self.eps)
        ops.gemm(sv["x"], st.p16, sv["q"], M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=st.off(self.attn + "q_proj.weight"),
                 bias=st.p32, bias_off=st.off(self.attn + "q_proj.bias"))
        ops.attn_fwd(sv["q"], kv, kv, sv["ctx"], sv["lse"], **self._akw(B, L, Te, sv["Tqp"], adrop))
        ops.gemm(sv["ctx"], st.p16, hout, M=M, N=d, K=d, lda=d, ldb=d, ldc=d, b_off=st.off(self.attn + "out_proj.weight"),
                 bias=st.p32, bias_off=st.off(self.attn + "out_proj.bias"), epilogue=EPI_RESIDUAL, R=hin, ldr=d,
                 dropout_p=hdrop[0], dropout_seed=hdrop[1])
        if sv["st"] is not None:
            sv.update(hin=hin, hdrop=hdrop, adrop=adrop)

    def backward(self, dh, dhin, sv, sc: Scratch, denc32, B, L, Te, defer=None, cs=(0, 0), ln_part=None, pending=None,
                 acc=True):
        """denc32: fp32 [B*Te, d] accumulator of the gradient wrt the encoder states (+=).  defer: list collecting
        the two token-side weight-gradient problems (out_proj, q_proj; bias gradients fused at cs = (cs_q, cs_o) of the
        layer's bias vector) for the layer's grouped launch; the k|v projection's (K = B*Te rows) goes out at once.
        acc=False: the three weight gradients overwrite their (uncleared) slots instead of adding to them."""
        st, d = self.st, self.d
        M, Mk = B * L, B * Te
        o, g32, p16 = st.off, st.g32, st.p16
        dy = _masked_grad(dh, sv, sc, M * d, "cross")
        if defer is None:
            ops.colsum(dy, d, M, d, g32, sc.part, out_off=o(self.attn + "out_proj.bias"))
            ops.wgrad_gemm(dy, sv["ctx"], g32, M=d, N=d, K=M, lda=d, ldb=d,
                           c_off=o(self.attn + "out_proj.weight"), accumulate=acc)
        else:
            defer.append(dict(dY=dy, X=sv["ctx"], M=d, N=d, K=M, lda=d, ldb=d, c_off=o(self.attn + "out_proj.weight"),
                              accumulate=acc, bias_off=o(self.attn + "out_proj.bias"), part=sc.part, cs_off=cs[1]))
        ops.gemm(dy, p16, sc.dctx, M=M, N=d, K=d, lda=d, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=o(self.attn + "out_proj.weight"))
        dq, dkv = (sc.dx if defer is None else sc.dq), sc.dkv
        ops.attn_bwd(sv["q"], sv["kv"], sv["kv"], sv["ctx"], sv["lse"], sc.dctx, sv["Dq"], dq, dkv, dkv, lddo=d, sdob=L * d,
                     lddq=d, lddk=2 * d, lddv=2 * d, sdqb=L * d, sdkb=Te * 2 * d, sdvb=Te * 2 * d, dk_off=0, dv_off=d,
                     **self._akw(B, L, Te, sv["Tqp"], sv["adrop"]))
        # q projection
        if defer is None:
            ops.colsum(dq, d, M, d, g32, sc.part, out_off=o(self.attn + "q_proj.bias"))
            ops.wgrad_gemm(dq, sv["x"], g32, M=d, N=d, K=M, lda=d, ldb=d,
                           c_off=o(self.attn + "q_proj.weight"), accumulate=acc)
        else:
            defer.append(dict(dY=dq, X=sv["x"], M=d, N=d, K=M, lda=d, ldb=d, c_off=o(self.attn + "q_proj.weight"),
                              accumulate=acc, bias_off=o(self.attn + "q_proj.bias"), part=sc.part, cs_off=cs[0]))
        ops.gemm(dq, p16, sc.dctx, M=M, N=d, K=d, lda=d, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=o(self.attn + "q_proj.weight"))
        _ln_bwd(st, self.ln, sc.dctx, sv, dh, dhin, sc, M, d, ln_part, pending)
        # k|v projection of the encoder states
        ops.colsum(dkv, 2 * d, Mk, 2 * d, g32, sc.part, out_off=o(self.attn + "k_proj.bias__zero"))
        ops.wgrad_gemm(dkv, sv["enc"], g32, M=2 * d, N=d, K=Mk, lda=2 * d, ldb=d,
                       c_off=o(self.attn + "k_proj.weight"), accumulate=acc)
        ops.gemm(dkv, p16, denc32, M=Mk, N=d, K=2 * d, lda=2 * d, b_layout=MNMAJOR, ldb=d, ldc=d,
                 b_off=o(self.attn + "k_proj.weight"), out_f32=True, accumulate=True)


class FFNBlock:
    """h_out = h_in + fc2(dropout(gelu(fc1(LN(h_in)))))."""

    def __init__(self, store, ln: str, fc1: str, fc2: str, d: int, f: int, eps: float):
        self.st, self.ln, self.fc1, self.fc2, self.d, self.f, self.eps = store, ln, fc1, fc2, d, f, eps
        self.cs_fc1, self.cs_fc2 = 4 * d, 4 * d + f  # (the encoder layer's bias vector; see SelfAttnBlock)

    def alloc(self, M, z, train=True):
        """(train=False: no pre-activation u either - fc1 then writes only the GELU output)"""
        return dict(x=z(M * self.d), st=z(M * 2, torch.float32) if train else None, u=z(M * self.f) if train else None,
                    g=z(M * self.f))

    def forward(self, hin, hout, sv, M, dropout_p=0.0, seed=0, hdrop=(0.0, 0), fp8=None):
        st, d, f = self.st, self.d, self.f
        train = sv["st"] is not None
        gamma, beta = st.view(self.ln + ".weight"), st.view(self.ln + ".bias")
        fc1 = dict(M=M, N=f, K=d, lda=d, ldb=d, ldc=f, b_off=st.off(self.fc1 + ".weight"), bias=st.p32,
                   bias_off=st.off(self.fc1 + ".bias"), epilogue=EPI_GELU, dropout_p=dropout_p, dropout_seed=seed,
                   stream_out=train and ops.STREAM_U)
        fc2_8 = fp8.get("fc2") if fp8 is not None else None
        if fp8 is not None:
            p8, scale, x8, rs = fp8["w"]
            ops.layernorm_fwd_fp8(hin, gamma, beta, sv["x"] if train else None, x8, rs, M, d, self.eps, stats=sv["st"])
            # (fc2 on the fp8 path: the GELU output also leaves fc1's epilogue as e4m3, delayed per-tensor scale)
            c8 = dict(C8=fc2_8[0], c8_scale=fc2_8[1], c8_amax=fc2_8[3]) if fc2_8 is not None else {}
            ops.gemm_fp8(x8, p8, sv["u"], C2=sv["g"], a_row_scale=rs, b_scale=scale, **fc1, **c8)
        elif not train and M <= 128 and d <= 2048 and LN_IN_GEMM:
            # a decoded token: the LayerNorm runs in fc1's prologue (CaGemmDesc.a_ln_gamma, bit-identical)
            ops.gemm(hin, st.p16, None, C2=sv["g"], a_ln=(gamma, beta, self.eps), **fc1)
        else:
            ops.layernorm_fwd(hin, gamma, beta, sv["x"], sv["st"], M, d, self.eps)
            ops.gemm(sv["x"], st.p16, sv["u"], C2=sv["g"], **fc1)
        if fc2_8 is not None:
            ops.gemm_fp8(fc2_8[0], p8, hout, a_scale=fc2_8[2], b_scale=fc2_8[4], M=M, N=d, K=f, lda=f, ldb=f, ldc=d,
                         b_off=st.off(self.fc2 + ".weight"), bias=st.p32, bias_off=st.off(self.fc2 + ".bias"),
                         epilogue=EPI_RESIDUAL, R=hin, ldr=d, dropout_p=hdrop[0], dropout_seed=hdrop[1])
        else:
            ops.gemm(sv["g"], st.p16, hout, M=M, N=d, K=f, lda=f, ldb=f, ldc=d, b_off=st.off(self.fc2 + ".weight"), bias=st.p32,
                     bias_off=st.off(self.fc2 + ".bias"), epilogue=EPI_RESIDUAL, R=hin, ldr=d, dropout_p=hdrop[0],
                     dropout_seed=hdrop[1])
        if train:
            sv.update(hin=hin, drop=(dropout_p, seed), hdrop=hdrop, fp8=fp8)

    def backward(self, dh, dhin, sv, sc: Scratch, M, defer=None, acc=True, sq=None, ln_part=None, pending=None, dy=None,
                 xdrop=None):
        """(SelfAttnBlock.backward)"""
        sq = sq or {}
        st, d, f = self.st, self.d, self.f
        o, g32, p16 = st.off, st.g32, st.p16
        p, seed = sv["drop"]
        fb = sv["fp8"].get("bwd") if sv["fp8"] is not None else None
        if dy is None:
            dy = _masked_grad(dh, sv, sc, M * d, "ffn") if fb is None else _masked_grad_fp8(dh, sv, sc, M, d, "ffn", fb)
        if defer is None:
            ops.colsum(dy, d, M, d, g32, sc.part, out_off=o(self.fc2 + ".bias"))
        wg = [dict(dY=dy, X=sv["g"], M=d, N=f, K=M, lda=d, ldb=f, c_off=o(self.fc2 + ".weight"), accumulate=acc,
                   sq=sq.get("fc2"),
                   **(dict(bias_off=o(self.fc2 + ".bias"), part=sc.part, cs_off=self.cs_fc2) if defer is not None else {}))]
        du8 = sv["fp8"].get("du") if fb is not None else None
        if fb is not None:  # fc2's data gradient on the fp8 path (GELU' epilogue as on the bf16 path)
            # (fc1's data gradient on it too: dU also leaves this epilogue as e4m3, delayed per-tensor scale - CaGemmDesc.C8)
            c8 = dict(C8=du8["buf"], c8_scale=du8["scale"], c8_amax=du8["amax"]) if du8 is not None else {}
            ops.gemm_fp8(fb[2], fb[0], sc.du, a_row_scale=fb[3], b_scale=fb[4], M=M, N=f, K=d, lda=d, ldb=d, ldc=f, b_off=fb[1],
                         epilogue=EPI_DGELU, R=sv["u"], ldr=f, dropout_p=p, dropout_seed=seed, **c8)
        else:
            ops.gemm(dy, p16, sc.du, M=M, N=f, K=d, lda=d, b_layout=MNMAJOR, ldb=f, ldc=f, b_off=o(self.fc2 + ".weight"),
                     epilogue=EPI_DGELU, R=sv["u"], ldr=f, dropout_p=p, dropout_seed=seed)
        if defer is None:
            ops.colsum(sc.du, f, M, f, g32, sc.part, out_off=o(self.fc1 + ".bias"))
        wg.append(dict(dY=sc.du, X=sv["x"], M=f, N=d, K=M, lda=f, ldb=d, c_off=o(self.fc1 + ".weight"), accumulate=acc,
                       sq=sq.get("fc1"),
                       **(dict(bias_off=o(self.fc1 + ".bias"), part=sc.part, cs_off=self.cs_fc1) if defer is not None else {})))
        if defer is not None:
            defer.extend(wg)
        else:
            ops.wgrad_gemm_group(wg, g32)
        if du8 is not None and du8["ready"][0]:
            # dX = dU W1 through ca_gemm_fp8: e4m3 dU x the transposed e4m3 copy of W1 (the scale of dU comes from the
            # previous step's amax; until one backward has measured it the bf16 GEMM below runs)
            ops.gemm_fp8(du8["buf"], fb[0], sc.dx, a_scale=du8["inv"], b_scale=du8["inv_w"], M=M, N=d, K=f, lda=f, ldb=f, ldc=d,
                         b_off=du8["w_off"])
        else:
            ops.gemm(sc.du, p16, sc.dx, M=M, N=d, K=f, lda=f, b_layout=MNMAJOR, ldb=d, ldc=d, b_off=o(self.fc1 + ".weight"))
        _ln_bwd(st, self.ln, sc.dx, sv, dh, dhin, sc, M, d, ln_part, pending, xdrop)


def wgrad_stream(engine):
    """The side stream of an engine's encoder weight gradients (None = everything on the current stream;
    CA_WGRAD_STREAM=0)."""
    if os.environ.get("CA_WGRAD_STREAM", "1") == "0":
        return None
    if engine._wstream is None:
        engine._wstream = ops.side_stream(engine.device, "wgrad", int(os.environ.get("CA_WGRAD_PRIO", "0")))
    return engine._wstream


def norm_plan(store, matrices, device):
    """Squared gradient norm without a pass over the listed weight matrices, (layer, key, name, rows, cols): their
    weight-gradient GEMMs leave per-tile sums of squares in `slots` at slot_off[(layer, key)] (CaGemmDesc.c_sumsq;
    encoder_backward passes the slices), everything else of the flat gradient buffer is listed as chunks of <= 64 Ki
    floats for ca_sumsq_ranges_f32.  None without matrices."""
    if not matrices:
        return None
    off, soff, mats = 0, {}, []
    for l, key, name, M, N in matrices:
        soff[(l, key)] = off
        off += ops.sumsq_slots(M, N)
        mats.append((store.off(name), M * N))
    chunks, pos = [], 0
    for a, n in sorted(mats) + [(store.numel, 0)]:
        while pos < a:
            m = min(65536, a - pos)
            chunks.append((pos, m))
            pos += m
        pos = max(pos, a + n)
    return dict(slots=torch.zeros(off, dtype=torch.float32, device=device), nslots=off, slot_off=soff,
                chunks=torch.tensor(chunks, dtype=torch.int64, device=device), nchunks=len(chunks),
                partial=torch.zeros(max(4096, len(chunks)), dtype=torch.float32, device=device))


def encoder_backward(blocks, svs, keep, B, T, ring, scs, bias_ws, ln_parts, *, gm, acc, plan, names, side, wgrad_early,
                     matrix_range, done, below=None, mring=None, epilogue=None, rows=None):
    """Backward through a stack of pre-LN encoder layers, blocks[l] = (SelfAttnBlock, FFNBlock) with saved states
    svs[l], from the gradient wrt the stack's output in ring[0] down to the one wrt its input.

    A layer's four weight gradients go out as one grouped launch into `gm` (g32, or the bf16 g16; fused bias column sums
    into g32), its second stages (both norms' d gamma | d beta, the bias vector) as one reduce_rows_multi.  With a `side`
    stream both run there beside the next layers' data-gradient chain: what they read rotates through the six buffers
    `ring` (layer i: 2i, 2i+1, 2i+2 mod 6) and two sets of `scs` / `bias_ws` / `ln_parts`, and the main stream waits for
    layer i's side work before layer i + 2 reuses them.  wgrad_early: the grouped launch goes out right after the
    attention backward (its second stage at the end of the layer), else both at the end.  epilogue(l) runs behind the
    second stage, then done(names[l]) - with the side stream current.  acc=False: the matrices' gradients are
    overwritten, and those of a dropped layer (keep[l] False, matrix_range(l) = (lo, hi)) cleared with its norm slots.

    below(l) -> (p, seed): the hidden dropout on the output of the sub-layer below layer l (dropped layers skipped).
    With it the LayerNorm backwards also write the dropped gradients of the sub-layers below into `mring` (parallel to
    `ring`; the caller writes mring[0]) and the blocks read them from there; without it each block masks its own.
    rows: the forward's packed rows (module docstring) - every layer then works on rows[1] rows.
    Returns (the gradient wrt the stack's input, its masked copy or None, a free ring buffer)."""
    main = torch.cuda.current_stream()
    M = B * T if rows is None else rows[1]
    kw_rows = {} if rows is None else dict(rows=rows)  # (nothing new in the calls of an unpacked stack)

    def on_side(fn):
        """Run fn on the side stream once the main stream has passed this point (in line without a side stream)."""
        if side is None:
            return fn()
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            return fn()

    wdone, it = {}, 0
    for l in reversed(range(len(blocks))):
        if not keep[l]:
            if not acc:  # dropped layer: its (uncleared) matrices get no gradient this step
                lo, hi = matrix_range(l)
                ops.clear_ranges(gm, ((lo, hi - lo),))
                if plan is not None:
                    a0 = plan["slot_off"][(l, "qkv")]
                    ops.clear_f32(plan["slots"], plan["slot_off"].get((l + 1, "qkv"), plan["nslots"]) - a0, off=a0)
            done(names[l])
            continue
        sa, ff = blocks[l]
        sv_a, sv_f = svs[l]
        st, g32 = sa.st, sa.st.g32
        nb = 5 * sa.d + ff.f  # the layer's bias vector: q|k|v, out_proj, fc1, fc2
        if side is not None and it - 2 in wdone:
            main.wait_event(wdone.pop(it - 2))
        sc, bw, lnp = scs[it & 1], bias_ws[it & 1], ln_parts[it & 1]
        i0, i1, i2 = (2 * it) % 6, (2 * it + 1) % 6, (2 * it + 2) % 6
        sq = {k: (plan["slots"], plan["slot_off"][(l, k)]) for k in ("qkv", "o", "fc1", "fc2")} if plan is not None else None
        kw_f = kw_a = {}
        if below is not None:
            pa, pb = sv_a["hdrop"], below(l)
            kw_f = dict(dy=mring[i0] if sv_f["hdrop"][0] > 0 else ring[i0], xdrop=(*pa, mring[i1]) if pa[0] > 0 else None)
            kw_a = dict(dy=mring[i1] if pa[0] > 0 else ring[i1], xdrop=(*pb, mring[i2]) if pb[0] > 0 else None)
        wg, second, fused = [], [], [False]

        def wgrads():
            fused[0] = ops.wgrad_gemm_group(wg, gm, colsum_ws=bw, colsum_ld=nb, Gb=g32)

        ff.backward(ring[i0], ring[i1], sv_f, sc, M, defer=wg, acc=acc, sq=sq, ln_part=lnp[0], pending=second, **kw_f)
        sa.backward(ring[i1], ring[i2], sv_a, sc, B, T, defer=wg, acc=acc, sq=sq, ln_part=lnp[1], pending=second,
                    deferred=(lambda: on_side(wgrads)) if wgrad_early else None, **kw_a, **kw_rows)

        def finish():
            if not wgrad_early:
                wgrads()
            if fused[0]:
                second.append((bw, ops.COLSUM_PARTS, nb, nb, g32[st.off(sa.qbias):], True))
            ops.reduce_rows_multi(second)
            if epilogue is not None:
                epilogue(l)
            if side is not None:
                wdone[it] = torch.cuda.Event()
                wdone[it].record(side)
            done(names[l])

        on_side(finish)
        it += 1
    if side is not None:
        main.wait_stream(side)
    k = (2 * it) % 6
    return ring[k], (mring[k] if mring is not None else None), ring[(k + 1) % 6]
