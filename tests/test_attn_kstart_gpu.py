"""CaAttnDesc.kstart on a real MI355X: a per-row first key in the causal tiled forward (the decoder prefill: the 64-query
and the 128-query kernel) and in the single-query decode form, against a float64 torch statement of the masked softmax.

Bounds are those of the unmasked forms' tests: 2e-2 absolute on randn inputs for the single-query kernel
(test_attention_every_planned_instantiation_computes_attention) and for the tiled forward's output
(test_fused_attention_fwd_bwd).  Exact: kstart of zeros is kstart=None bit for bit; what the masked cache rows hold does
not reach the output; a query without an allowed key gets zeros; nothing non-finite is written; a refused combination
returns the error and launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = 2e-2


@pytest.fixture(scope="module")
def ops():
    from coral_amd import ops as o

    o.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return o


def _reference(q, k, v, H, hd, klen, kstart, causal):
    """float64 softmax(scale q k^T + masks) v with keys kstart[b] <= t < klen[b] (and t <= i when causal); rows without
    an allowed key are zero.  q [B, Tq, d], k / v [B, Tk, d] -> [B, Tq, d] and the [B, Tq] map of rows with a key."""
    B, Tq, d = q.shape
    Tk = k.shape[1]

    def heads(x, T):
        return x.double().cpu().view(B, T, H, hd).transpose(1, 2)

    s = heads(q, Tq) @ heads(k, Tk).transpose(-1, -2) * hd ** -0.5
    t = torch.arange(Tk)[None, None, None, :]
    mask = (t >= kstart.cpu()[:, None, None, None]) & (t < klen.cpu()[:, None, None, None])
    if causal:
        mask = mask & (t <= torch.arange(Tq)[None, None, :, None])
    mask = mask.expand(B, 1, Tq, Tk)
    alive = mask.any(-1)  # [B, 1, Tq]
    s = s.masked_fill(~mask, float("-inf"))
    s = torch.where(alive[..., None], s, torch.zeros_like(s))  # (a row of -inf has no softmax)
    o = (torch.softmax(s, -1) * mask) @ heads(v, Tk)
    o = o * alive[..., None]
    return o.transpose(1, 2).reshape(B, Tq, d), alive[:, 0]


# ---- the single-query form ---------------------------------------------------------------------------------------------
SQ_B, SQ_H, SQ_LMAX = 6, 2, 200
SQ_KLEN = (200, 130, 66, 65, 64, 1)
SQ_STARTS = ("0", "1", "63", "64", "65", "klen-1", "klen")


def _sq_kstart(which):
    """`which` for every row, held to klen (a first key past the last one means the same as at it); 'mixed': one per row."""
    def val(w, kl):
        return kl - 1 if w == "klen-1" else kl if w == "klen" else min(int(w), kl)

    if which == "mixed":
        return torch.tensor([val(w, kl) for w, kl in zip(("65", "klen-1", "1", "64", "63", "klen"), SQ_KLEN)], dtype=torch.int32)
    return torch.tensor([val(which, kl) for kl in SQ_KLEN], dtype=torch.int32)


@pytest.fixture(scope="module")
def sq_data():
    out = {}
    for hd in (64, 32):
        d = SQ_H * hd
        g = torch.Generator().manual_seed(1000 + hd)
        kv = torch.randn(SQ_B, SQ_LMAX, 2 * d, generator=g).to(torch.bfloat16)
        q = torch.randn(SQ_B, 1, d, generator=g).to(torch.bfloat16)
        out[hd] = (q.to(DEV), kv.to(DEV))
    return out


def _sq_run(ops, q, kv, hd, kstart, klen=None, keep=None, **extra):
    """One launch over the K|V cache [B, Lmax, 2d]; the output buffer starts as ones (and is handed out through `keep`
    before the launch, for the launches that are refused)."""
    d = SQ_H * hd
    klen = torch.tensor(SQ_KLEN, dtype=torch.int32, device=DEV) if klen is None else klen
    got = torch.ones(SQ_B, 1, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(SQ_B * SQ_H * 32, device=DEV)
    if keep is not None:
        keep.append(got)
    ops.attn_fwd(q, kv, kv, got, lse, B=SQ_B, H=SQ_H, Tq=1, Tk=SQ_LMAX, hd=hd, Tqp=32, scale=hd ** -0.5, ldq=d, ldk=2 * d,
                 ldv=2 * d, ldo=d, sqb=d, skb=SQ_LMAX * 2 * d, svb=SQ_LMAX * 2 * d, sob=d, k_off=0, v_off=d, klen=klen,
                 kstart=None if kstart is None else kstart.to(DEV), **extra)
    torch.cuda.synchronize()
    return got, lse


@pytest.mark.parametrize("hd,which", [(64, w) for w in SQ_STARTS + ("mixed",)] + [(32, "mixed")])
def test_single_query_first_key(ops, sq_data, hd, which):
    q, kv = sq_data[hd]
    d = SQ_H * hd
    ks = _sq_kstart(which)
    klen = torch.tensor(SQ_KLEN, dtype=torch.int32)
    got, lse = _sq_run(ops, q, kv, hd, ks)
    ref, alive = _reference(q, kv[..., :d], kv[..., d:], SQ_H, hd, klen, ks, causal=False)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"single query hd {hd} kstart {ks.tolist()}: max |err| {err:.3e} (bound {BOUND})")
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(lse).all())
    assert err <= BOUND, err
    dead = ~alive[:, 0]
    assert dead.tolist() == [int(a) >= int(b) for a, b in zip(ks, klen)]
    assert bool((got[dead.to(DEV)] == 0).all()), "a row without an allowed key must be exactly zero"
    # what the masked cache rows hold does not matter
    outs = []
    for value in (0.0, 1e30, -1e30):
        kv2 = kv.clone()
        for b in range(SQ_B):
            kv2[b, :int(ks[b])] = value
        outs.append(_sq_run(ops, q, kv2, hd, ks)[0])
    assert all(torch.equal(o, got) for o in outs)


def test_single_query_kstart_of_zeros_is_no_kstart(ops, sq_data):
    for hd in (64, 32):
        q, kv = sq_data[hd]
        a, lse_a = _sq_run(ops, q, kv, hd, None)
        b, lse_b = _sq_run(ops, q, kv, hd, torch.zeros(SQ_B, dtype=torch.int32))
        assert torch.equal(a, b) and torch.equal(lse_a, lse_b)


# ---- the causal tiled forward ------------------------------------------------------------------------------------------
PF_B, PF_H, PF_HD = 4, 2, 64


@pytest.fixture(scope="module")
def pf_data():
    d = PF_H * PF_HD
    out = {}
    for n in (5, 70, 130):
        g = torch.Generator().manual_seed(2000 + n)
        out[n] = torch.randn(PF_B, n, 3 * d, generator=g).to(torch.bfloat16).to(DEV)
    return out


def _pf_run(ops, qkv, n, kstart, klen=None, keep=None, hd=PF_HD, H=PF_H, **extra):
    """Causal self-attention over a fused [B, n, 3d] projection buffer, as the decoder prefill launches it; `keep` as in
    _sq_run."""
    d = H * hd
    Tqp = (n + 31) // 32 * 32
    got = torch.ones(PF_B, n, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(PF_B, H, Tqp, device=DEV)
    if keep is not None:
        keep.append(got)
    kw = dict(B=PF_B, H=H, Tq=n, Tk=n, hd=hd, Tqp=Tqp, scale=hd ** -0.5, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d,
              sqb=n * 3 * d, skb=n * 3 * d, svb=n * 3 * d, sob=n * d, q_off=0, k_off=d, v_off=2 * d, causal=True,
              klen=None if klen is None else klen.to(DEV), kstart=None if kstart is None else kstart.to(DEV))
    kw.update(extra)
    ops.attn_fwd(qkv, qkv, qkv, got, lse, **kw)
    torch.cuda.synchronize()
    return got, lse


@pytest.mark.parametrize("n,pad", [(5, False), (70, False), (130, False), (130, True)])
def test_causal_prefill_first_key(ops, pf_data, n, pad):
    """n = 5, 70: the 64-query kernel (one and two key tiles); n = 130: the 128-query kernel, two workgroups per head."""
    qkv = pf_data[n]
    d = PF_H * PF_HD
    ks = torch.tensor([0, 1, 64, n - 1], dtype=torch.int32)
    klen = torch.tensor([n, n - 3, n, n], dtype=torch.int32) if pad else torch.full((PF_B,), n, dtype=torch.int32)
    got, lse = _pf_run(ops, qkv, n, ks, klen if pad else None)
    ref, alive = _reference(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], PF_H, PF_HD, klen, ks, causal=True)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"causal prefill n {n} klen {klen.tolist()} kstart {ks.tolist()}: max |err| {err:.3e} (bound {BOUND})")
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(lse).all())
    assert err <= BOUND, err
    # rows in front of their first key (and every row of a clip whose first key lies past its last): exactly zero
    want_dead = torch.arange(n)[None, :] < torch.minimum(ks, klen)[:, None]
    want_dead = want_dead | (ks >= klen)[:, None]
    assert torch.equal(~alive, want_dead) and bool(want_dead.any())
    assert bool((got[want_dead.to(DEV)] == 0).all())
    outs = []
    for value in (0.0, 1e30, -1e30):
        x = qkv.clone()
        for b in range(PF_B):
            x[b, :int(ks[b]), d:] = value  # the K and V columns of the masked rows
        outs.append(_pf_run(ops, x, n, ks, klen if pad else None)[0])
    assert all(torch.equal(o, got) for o in outs)


@pytest.mark.parametrize("n", [5, 70, 130])
def test_causal_prefill_kstart_of_zeros_is_no_kstart(ops, pf_data, n):
    a, lse_a = _pf_run(ops, pf_data[n], n, None)
    b, lse_b = _pf_run(ops, pf_data[n], n, torch.zeros(PF_B, dtype=torch.int32))
    assert torch.equal(a, b) and torch.equal(lse_a[:, :, :n], lse_b[:, :, :n])


# ---- refused forms -----------------------------------------------------------------------------------------------------
def test_refused_combinations_launch_nothing(ops, sq_data, pf_data):
    from coral_amd._lib import CoralAmdError

    q, kv = sq_data[64]
    ks6, ks4 = torch.ones(SQ_B, dtype=torch.int32), torch.ones(PF_B, dtype=torch.int32)
    dummy = torch.zeros(4096, dtype=torch.int32, device=DEV)
    keep = []

    def refused(what, run, *args, **kw):
        with pytest.raises(CoralAmdError, match="kstart"):
            run(*args, keep=keep, **kw)
        torch.cuda.synchronize()
        assert bool((keep[-1] == 1.0).all()), f"{what}: the refused launch wrote its output"

    # the single-query form
    d = SQ_H * 64
    refused("key_slot", _sq_run, ops, q, kv, 64, ks6, key_slot=torch.zeros(SQ_B, SQ_LMAX, dtype=torch.int32, device=DEV))
    refused("split_ws", _sq_run, ops, q, kv, 64, ks6, split_ws=ops.attn_split_workspace(SQ_B, SQ_H, DEV))
    refused("dropout", _sq_run, ops, q, kv, 64, ks6, dropout_p=0.1, dropout_seed=3)
    # the tiled forward
    x = pf_data[130]
    refused("dropout, causal", _pf_run, ops, x, 130, ks4, dropout_p=0.1, dropout_seed=3)
    refused("not causal", _pf_run, ops, x, 130, ks4, causal=False)
    refused("row_off", _pf_run, ops, x, 130, ks4, causal=False, row_off=dummy)
    o8 = torch.zeros(PF_B, 130, PF_H * PF_HD, dtype=torch.uint8, device=DEV)
    refused("O8", _pf_run, ops, x, 130, ks4, O8=o8, o8_scale=torch.ones(1, device=DEV),
            o8_amax=torch.zeros(64, dtype=torch.int32, device=DEV))
    wide = torch.randn(PF_B, 130, 3 * 128, device=DEV).to(torch.bfloat16)
    refused("head_dim 128", _pf_run, ops, wide, 130, ks4, hd=128, H=1)
    assert len(keep) == 8

    # the backward and the fused query-projection entry point
    n, dm = 130, PF_H * PF_HD
    O = torch.ones(PF_B, n, dm, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(PF_B, PF_H, 160, device=DEV)
    dbuf = torch.ones(PF_B, n, 3 * dm, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(CoralAmdError, match="kstart"):
        ops.attn_bwd(x, x, x, O, lse, O, torch.zeros_like(lse), dbuf, dbuf, dbuf, lddo=dm, sdob=n * dm, lddq=3 * dm, lddk=3 * dm,
                     lddv=3 * dm, sdqb=n * 3 * dm, sdkb=n * 3 * dm, sdvb=n * 3 * dm, dq_off=0, dk_off=dm, dv_off=2 * dm,
                     B=PF_B, H=PF_H, Tq=n, Tk=n, hd=PF_HD, Tqp=160, scale=0.125, ldq=3 * dm, ldk=3 * dm, ldv=3 * dm, ldo=dm,
                     sqb=n * 3 * dm, skb=n * 3 * dm, svb=n * 3 * dm, sob=n * dm, q_off=0, k_off=dm, v_off=2 * dm, causal=True,
                     kstart=ks4.to(DEV))
    torch.cuda.synchronize()
    assert bool((dbuf == 1.0).all())
    xr = torch.randn(SQ_B, d, device=DEV).to(torch.bfloat16)
    W = torch.zeros(d, d, dtype=torch.bfloat16, device=DEV)
    one, zero = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    out = torch.ones(SQ_B, 1, d, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(CoralAmdError, match="kstart"):
        ops.decode_attn_qproj(xr, one, zero, W, zero, kv, kv, out, d_model=d, eps=1e-5, ldx=d, ldw=d, sob=d, B=SQ_B, H=SQ_H,
                              Tk=SQ_LMAX, hd=64, scale=0.125, ldk=2 * d, ldv=2 * d, ldo=d, skb=SQ_LMAX * 2 * d,
                              svb=SQ_LMAX * 2 * d, k_off=0, v_off=d, klen=torch.tensor(SQ_KLEN, dtype=torch.int32, device=DEV),
                              kstart=ks6.to(DEV))
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
