"""Test-side float64 restatements of the kernels that end every training step: the cross-entropy forward and backward
(csrc/softmax.hip), the embedding gather and its scatter-add, the squared norm and the fused AdamW with the clip folded
in (csrc/misc.hip).  Each is written from the operation's definition, not from the kernel; tests/test_step_ref_cpu.py
proves them against torch (no GPU) and tests/test_step_kernels_gpu.py holds the kernels to them.  Plain torch on the
CPU; nothing here imports `coral_amd`.

The float32 restatements (`ce_f32`, `adamw_f32`) are the yardsticks of the GPU tests: what a straightforward fp32
evaluation of the same formula loses against float64 on the same inputs.  A kernel is allowed a fixed multiple of that.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff


def f64(t):
    return t.detach().to("cpu", torch.float64)


def f32r(x: float) -> float:
    """`x` rounded to float32, as a Python float: the value a kernel's `float` argument really holds."""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- cross-entropy ----------------------------------------------------------------------------------------------------
def ce_kept(labels, V, ignore=-100):
    lab = labels.to(torch.int64)
    return (lab != ignore) & (lab >= 0) & (lab < V)


def ce_rows_ref(logits, labels, V, ignore=-100):
    """-> (loss_row [rows] float64, 0 on skipped rows; kept [rows] bool; grad [rows, ldv] float64).  Only columns < V of
    `logits` are read.  A row whose label is `ignore`, negative or >= V is skipped: zero loss, zero gradient, not counted.
    Otherwise loss = logsumexp(x) - x[label] and grad = softmax(x) - onehot(label) in columns < V, 0 in columns >= V."""
    rows, ldv = logits.shape
    x = f64(logits[:, :V])
    kept = ce_kept(labels, V, ignore)
    grad = torch.zeros(rows, ldv, dtype=torch.float64)
    loss = torch.zeros(rows, dtype=torch.float64)
    for r in range(rows):
        if not kept[r]:
            continue
        lab = int(labels[r])
        lse = torch.logsumexp(x[r], dim=0)
        loss[r] = lse - x[r, lab]
        grad[r, :V] = torch.exp(x[r] - lse)
        grad[r, lab] -= 1.0
    return loss, kept, grad


def ce_ref(logits, labels, V, ignore=-100):
    """-> (loss_sum float, count int, grad [rows, ldv] float64)."""
    loss, kept, grad = ce_rows_ref(logits, labels, V, ignore)
    return float(loss.sum()), int(kept.sum()), grad


def ce_f32(logits, labels, V, ignore=-100):
    """The fp32 restatement: torch.log_softmax in float32, exp, minus the one-hot.  -> (loss_row [rows] float32, grad
    [rows, ldv] float32), zeros on skipped rows and in columns >= V."""
    rows, ldv = logits.shape
    kept = ce_kept(labels, V, ignore)
    grad = torch.zeros(rows, ldv, dtype=torch.float32)
    loss = torch.zeros(rows, dtype=torch.float32)
    for r in range(rows):
        if not kept[r]:
            continue
        lab = int(labels[r])
        lp = torch.log_softmax(logits[r, :V].to(torch.float32), dim=0)
        loss[r] = -lp[lab]
        grad[r, :V] = torch.exp(lp)
        grad[r, lab] -= 1.0
    return loss, grad


# ---- embedding --------------------------------------------------------------------------------------------------------
def embed_ref(table, pos, ids, pos_ids):
    """y[r] = table[ids[r]] + pos[pos_ids[r]] in float64 (pos None: the table rows alone)."""
    y = f64(table)[ids.long()]
    if pos is not None:
        y = y + f64(pos)[pos_ids.long()]
    return y


def embed_bwd_ref(dy, ids, pos_ids, dtable, dpos):
    """dtable[ids[r]] += dy[r], dpos[pos_ids[r]] += dy[r] in float64; either of dtable / dpos may be None.
    -> (dtable, dpos) as new tensors."""
    g = f64(dy)
    dt = dp = None
    if dtable is not None:
        dt = f64(dtable).clone().index_add_(0, ids.long(), g)
    if dpos is not None:
        dp = f64(dpos).clone().index_add_(0, pos_ids.long(), g)
    return dt, dp


# ---- AdamW with the clip folded in ------------------------------------------------------------------------------------
def clip_coef(grad_scale, max_norm, gnorm_sq):
    """grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6)); the min factor only when gnorm_sq is given
    and max_norm > 0 (clip_grad_norm_ applied to g * grad_scale)."""
    coef = float(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        coef *= min(1.0, max_norm / (math.sqrt(float(gnorm_sq)) * grad_scale + 1e-6))
    return coef


def adamw_ref(p, m, v, g, lr, b1, b2, eps, wd, step, grad_scale=1.0, max_norm=0.0, gnorm_sq=None):
    """One step of decoupled-decay AdamW (torch.optim.AdamW) on the gradient g * coef, float64.  -> (p, m, v)."""
    p, m, v, g = f64(p), f64(m), f64(v), f64(g)
    gi = g * clip_coef(grad_scale, max_norm, gnorm_sq)
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adamw_f32(p, m, v, g, lr, b1, b2, eps, wd, step, grad_scale=1.0, max_norm=0.0, gnorm_sq=None):
    """The fp32 restatement, every operation a torch.float32 operation in the order of the kernel's comment:
    gi = g coef, p *= 1 - lr wd, m = b1 m + (1 - b1) gi, v = b2 v + (1 - b2) gi gi, p -= (lr / bc1) m / (sqrt(v) /
    sqrt(bc2) + eps).  -> (p, m, v) float32."""
    t = lambda x: torch.tensor(float(x), dtype=torch.float32)  # noqa: E731
    lr, b1, b2, eps, wd, gs, mn = t(lr), t(b1), t(b2), t(eps), t(wd), t(grad_scale), t(max_norm)
    one = t(1.0)
    coef = gs.clone()
    if gnorm_sq is not None and max_norm > 0:
        c = mn / (torch.sqrt(t(gnorm_sq)) * gs + t(1e-6))
        coef = coef * torch.minimum(c, one)
    bc1 = one - torch.pow(b1, t(step))
    bc2_sqrt = torch.sqrt(one - torch.pow(b2, t(step)))
    step_size = lr / bc1
    decay = one - lr * wd
    p, m, v = (x.detach().to("cpu", torch.float32) for x in (p, m, v))
    gi = g.detach().to("cpu", torch.float32) * coef
    pi = p * decay
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    denom = torch.sqrt(vi) / bc2_sqrt + eps
    pi = pi - step_size * mi / denom
    return pi, mi, vi
