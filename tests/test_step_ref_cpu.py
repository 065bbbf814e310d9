"""The float64 restatements of tests/step_ref.py are themselves right: each agrees with torch's own float64 operation
to 1e-12 relative (no GPU).  tests/test_step_kernels_gpu.py holds the kernels to them."""
import pytest
import torch
import torch.nn.functional as F

import step_ref as R

RTOL = 1e-12


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def close(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a - b).abs() <= RTOL * b.abs().max().clamp_min(1e-300)).all())


@pytest.mark.parametrize("ignore", [-100, 3])
@pytest.mark.parametrize("rows,V,ldv", [(6, 7, 8), (9, 1003, 1008), (4, 4100, 4100)])
def test_ce_ref_matches_torch_cross_entropy(rows, V, ldv, ignore):
    x = rnd(rows, ldv, seed=1, scale=3.0)
    x[:, V:] = float("nan")  # the reference never reads the pad columns
    x[1, 5] = float("-inf")
    labels = torch.tensor(([0, V - 1, ignore, 5, 2, 1] * 2)[:rows])  # (every label in range or the ignored one)
    xv = x[:, :V].clone().requires_grad_(True)
    loss = F.cross_entropy(xv, labels, ignore_index=ignore, reduction="sum")
    loss.backward()
    ls, cnt, grad = R.ce_ref(x, labels, V, ignore)
    assert cnt == int((labels != ignore).sum())
    assert close(ls, loss.detach())
    assert close(grad[:, :V], xv.grad)
    assert bool((grad[:, V:] == 0).all())
    skipped = labels == ignore
    assert bool((grad[skipped] == 0).all())


def test_ce_ref_skips_out_of_range_labels():
    V, ldv = 7, 8
    x = rnd(5, ldv, seed=2)
    labels = torch.tensor([2, -1, V, ldv - 1, -100])
    ls, cnt, grad = R.ce_ref(x, labels, V)
    one, _, g1 = R.ce_ref(x[:1], labels[:1], V)
    assert cnt == 1 and ls == one
    assert torch.equal(grad[:1], g1) and bool((grad[1:] == 0).all())


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("gscale,active", [(1.0, True), (1e-3, False)])
def test_adamw_ref_matches_torch_adamw_after_clip(gscale, active, wd):
    n, lr, b1, b2, eps, grad_scale, max_norm = 257, 1e-3, 0.9, 0.98, 1e-8, 0.25, 1.0
    p0 = rnd(n, seed=3)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = rnd(n, seed=10 + step, scale=gscale)
        assert (float(g.norm()) * grad_scale > max_norm) == active
        pt.grad = g * grad_scale
        torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        p, m, v = R.adamw_ref(p, m, v, g, lr, b1, b2, eps, wd, step, grad_scale, max_norm, float((g * g).sum()))
        if not active:
            assert R.clip_coef(grad_scale, max_norm, float((g * g).sum())) == grad_scale
    st = opt.state[pt]
    assert close(p, pt.detach()) and close(m, st["exp_avg"]) and close(v, st["exp_avg_sq"])
    assert not torch.equal(p, p0)


def test_adamw_ref_without_norm_or_max_norm_only_scales():
    n = 33
    p, m, v, g = rnd(n, seed=4), rnd(n, seed=5, scale=0.01), rnd(n, seed=6).abs() * 1e-4, rnd(n, seed=7)
    a = R.adamw_ref(p, m, v, g, 1e-3, 0.9, 0.98, 1e-8, 0.1, 3, 0.25, 1.0, None)
    b = R.adamw_ref(p, m, v, g, 1e-3, 0.9, 0.98, 1e-8, 0.1, 3, 0.25, 0.0, float((g * g).sum()))
    c = R.adamw_ref(p, m, v, g * 0.25, 1e-3, 0.9, 0.98, 1e-8, 0.1, 3)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_adamw_f32_restatement_tracks_the_reference():
    n = 4099
    p, m, v, g = rnd(n, seed=4), rnd(n, seed=5, scale=0.01), rnd(n, seed=6).abs() * 1e-4, rnd(n, seed=7)
    p, m, v, g = (x.float() for x in (p, m, v, g))
    h = [R.f32r(x) for x in (1e-3, 0.9, 0.98, 1e-8, 0.1)]
    nsq = R.f32r(float((g.double() ** 2).sum()))
    ref = R.adamw_ref(p, m, v, g, *h, 1000, 0.25, 1.0, nsq)
    got = R.adamw_f32(p, m, v, g, *h, 1000, 0.25, 1.0, nsq)
    for x, y in zip(got, ref):
        assert x.dtype == torch.float32
        assert float((x.double() - y).abs().max()) <= 1e-5 * float(y.abs().max())


@pytest.mark.parametrize("C", [8, 264])
def test_embed_refs_match_torch_embedding(C):
    vocab, npos, rows = 11, 7, 300
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
    pos_ids = torch.randint(0, npos, (rows,), generator=g, dtype=torch.int32)
    table = rnd(vocab, C, seed=9).requires_grad_(True)
    pos = rnd(npos, C, seed=10).requires_grad_(True)
    dy = rnd(rows, C, seed=11)
    y = F.embedding(ids.long(), table) + F.embedding(pos_ids.long(), pos)
    y.backward(dy)
    assert close(R.embed_ref(table, pos, ids, pos_ids), y.detach())
    assert torch.equal(R.embed_ref(table, None, ids, None), table.detach()[ids.long()])
    dt0, dp0 = rnd(vocab, C, seed=12), rnd(npos, C, seed=13)
    dt, dp = R.embed_bwd_ref(dy, ids, pos_ids, dt0, dp0)
    assert close(dt - dt0, table.grad) and close(dp - dp0, pos.grad)
    only_t, none_p = R.embed_bwd_ref(dy, ids, pos_ids, dt0, None)
    assert none_p is None and torch.equal(only_t, dt)
