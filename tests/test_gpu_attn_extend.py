"""-m gpu: sd_attn_extend (a block of new query rows over a live KV cache) and sd_kvcache_store_at.

Yardsticks: plain fp64 torch under the visibility rule of tests/extend_ref.py (checked on the CPU by
tests/test_session_cpu.py) and the existing sd_attn_fwd on the whole sequence.  The bit contract -- a row's output depends
on its query, its position and the visible K / V only -- is checked bit for bit."""
import pytest
import torch

import attn_ref as A
import extend_ref as E
from gpu_util import dev, record
from test_gpu_generate import _inputs, same_bits

pytestmark = pytest.mark.gpu

D = 128
HEADS = [(16, 8), (4, 2), (2, 1)]
KINDS = ["randn", "rising", "falling"]
PASTS = (0, 1, 63, 64, 65, 256)
NEWS = (1, 2, 63, 64, 65, 129)
LF = 640          # longest sequence of the file: 511 + 129


@pytest.fixture(scope="module")
def ops():
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    return ops_


_CACHE = {}


def _seqs(kind, Hq, Hkv):
    """q [3, LF, Hq*128], k, v [3, LF, Hkv*128] bf16 (CPU), made once per (kind, heads) and never changed."""
    key = (kind, Hq, Hkv)
    if key not in _CACHE:
        q, k, v = _inputs(kind, 3, LF, Hq, Hkv, seed=7 + Hq)
        _CACHE[key] = (q.view(3, LF, Hq * D), k.view(3, LF, Hkv * D), v.view(3, LF, Hkv * D))
    return _CACHE[key]


def _junk(shape_cols):
    return torch.where(torch.arange(shape_cols) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)


def _planes(k, v, rows, ends, cap, junk=False):
    """Cache planes [B, cap, KD] on the device holding sequence rows[b]'s K / V in slots [0, ends[b]); the rest zeros, or
    +-1e4 with junk=True."""
    B, KD = len(rows), k.shape[-1]
    kp = torch.zeros(B, cap, KD, dtype=torch.bfloat16)
    vp = torch.zeros(B, cap, KD, dtype=torch.bfloat16)
    if junk:
        kp[:], vp[:] = _junk(KD), -_junk(KD)
    for i, (b, n) in enumerate(zip(rows, ends)):
        kp[i, :n], vp[i, :n] = k[b, :n], v[b, :n]
    return kp.to(dev()), vp.to(dev())


def _block(q, rows, pasts, T):
    """q block [B*T, QD]: row (i, t) is sequence rows[i]'s query at position pasts[i] + t."""
    return torch.stack([q[b, p:p + T] for b, p in zip(rows, pasts)]).reshape(len(rows) * T, -1).contiguous()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=dev())


def _extend(ops, q, k, v, rows, pasts, news, T, cap, Hq, Hkv, junk=False, q_blk=None):
    kp, vp = _planes(k, v, rows, [p + n for p, n in zip(pasts, news)], cap, junk)
    qb = (_block(q, rows, pasts, T) if q_blk is None else q_blk).to(dev())
    o, lse = ops.attn_extend(qb, kp, vp, _i32(pasts), _i32(news), T, Hq, Hkv)
    return o.view(len(rows), T, Hq * D), lse, (qb, kp, vp)


# ---------------------------------------------------------------------------------------------------- 1. against fp64
def _against_fp64(ops, kind, Hq, Hkv, rows, pasts, news, T, cap, tag):
    q, k, v = _seqs(kind, Hq, Hkv)
    B = len(rows)
    o, lse, (qb, kp, vp) = _extend(ops, q, k, v, rows, pasts, news, T, cap, Hq, Hkv)
    vis = E.extend_visible(pasts, news, T, cap)
    ref, lse_ref = E.attend(qb.cpu().view(B, T, Hq * D), kp.cpu(), vp.cpu(), vis, Hq, Hkv)      # [B,T,Hq,D], [B,Hq,T]
    got = o.double().cpu().view(B, T, Hq, D)
    # yardstick: sd_attn_fwd on the whole sequences with kv_len = past + new, the same rows
    Lf = max(p + T for p in pasts)
    qf = torch.stack([q[b, :Lf] for b in rows]).reshape(B * Lf, -1).to(dev())
    kf = torch.stack([k[b, :Lf] for b in rows]).reshape(B * Lf, -1).to(dev())
    vf = torch.stack([v[b, :Lf] for b in rows]).reshape(B * Lf, -1).to(dev())
    o_full, _ = ops.attn_fwd(qf, kf, vf, B, Lf, Hq, Hkv, kv_len=_i32(p + n for p, n in zip(pasts, news)))
    o_full = o_full.double().cpu().view(B, Lf, Hq, D)
    yard = torch.stack([o_full[i, p:p + T] for i, p in enumerate(pasts)])
    err_ext = (got - ref).abs().amax(-1)                  # [B,T,Hq] worst column of every row
    err_yard = (yard - ref).abs().amax(-1)
    worst_yard = float(err_yard.max())
    ulp = 2.0 ** -8 * ref.abs().amax(-1)
    allow = torch.maximum(torch.full_like(ulp, A.F_ROW * worst_yard), ulp)
    print(f"attn_extend {tag} Hq={Hq} Hkv={Hkv} {kind} past={list(pasts)} new={list(news)} T={T}: worst row err extend "
          f"{float(err_ext.max()):.3e}  sd_attn_fwd {worst_yard:.3e}")
    record("attn_extend", Hq=Hq, kind=kind, tag=tag, past=list(pasts), new=list(news), err_extend=float(err_ext.max()),
           err_attn_fwd=worst_yard)
    assert bool(torch.isfinite(got).all())
    assert bool((err_ext <= allow).all()), (tag, pasts, news, float(err_ext.max()), worst_yard)
    e_lse = float((lse.double().cpu() - lse_ref).abs().max())
    assert e_lse <= 1e-3 * max(1.0, float(lse_ref.abs().max())), (tag, pasts, news, e_lse)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_extend_attention_against_fp64(ops, Hq, Hkv, kind):
    """Worst-row absolute error of sd_attn_extend against fp64 <= max(F_ROW x the worst-row error of sd_attn_fwd run on the
    whole sequence of past + new rows with kv_len = past + new, on the same rows, 2^-8 x max|o_ref| of the row); LSE within
    1e-3 max(1, |LSE|) (the rule of test_decode_attention_against_fp64).  One ragged batch, then the (past, new) grid at
    B = 1 with cap = 385, so that past = 256, new = 129 fills the cache exactly."""
    _against_fp64(ops, kind, Hq, Hkv, [0, 1, 2], [0, 65, 511], [129, 1, 64], 129, 640, "batch")
    for past in PASTS:
        for new in NEWS:
            _against_fp64(ops, kind, Hq, Hkv, [0], [past], [new], new, 385, "grid")


# ------------------------------------------------------------------------------------------------ 2. split invariance
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_extend_attention_bits_do_not_depend_on_the_split(ops, Hq, Hkv, kind):
    """130 new rows behind 37 cached ones: one call, then (1 + 129), (64 + 66), (65 + 65) -- the later call of a pair reads
    the slots the earlier one's K / V occupy, and every slot >= past + new holds +-1e4.  Rows of the same absolute position
    have identical o and lse bits; also for cap in {256, 512}, T padded to 192, inside a batch of 3, and run twice."""
    q, k, v = _seqs(kind, Hq, Hkv)
    P, N = 37, 130
    o0, l0, _ = _extend(ops, q, k, v, [0], [P], [N], N, 256, Hq, Hkv, junk=True)
    o0, l0 = o0[0], l0[0]                                       # [N, QD], [Hq, N]
    o1, l1, _ = _extend(ops, q, k, v, [0], [P], [N], N, 256, Hq, Hkv, junk=True)
    assert same_bits(o0, o1[0]) and same_bits(l0, l1[0])
    for first in (1, 64, 65):
        oa, la, _ = _extend(ops, q, k, v, [0], [P], [first], first, 256, Hq, Hkv, junk=True)
        ob, lb, _ = _extend(ops, q, k, v, [0], [P + first], [N - first], N - first, 256, Hq, Hkv, junk=True)
        assert same_bits(torch.cat([oa[0], ob[0]]), o0), first
        assert same_bits(torch.cat([la[0], lb[0]], -1), l0), first
    for cap, T in ((512, N), (256, 192), (512, 192)):
        oc, lc, _ = _extend(ops, q, k, v, [0], [P], [N], T, cap, Hq, Hkv, junk=True)
        assert same_bits(oc[0, :N], o0) and same_bits(lc[0, :, :N].contiguous(), l0), (cap, T)
    # sequence 0 as the middle row of a batch of 3 whose other rows have other pasts and lengths
    od, ld, _ = _extend(ops, q, k, v, [1, 0, 2], [200, P, 0], [7, N, 192], 192, 512, Hq, Hkv, junk=True)
    assert same_bits(od[1, :N], o0) and same_bits(ld[1, :, :N].contiguous(), l0)


# ------------------------------------------------------------------------------------------------------- 3. no leak
@pytest.mark.parametrize("kind", ["randn", "rising"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_extend_attention_does_not_leak(ops, Hq, Hkv, kind):
    q, k, v = _seqs(kind, Hq, Hkv)
    N, T, cap = 70, 96, 256
    for past in (64, 65, 63):                                    # past % 64 in {0, 1, 63}: the diagonal at any offset
        clean, lclean, (qb, kp, vp) = _extend(ops, q, k, v, [0], [past], [N], T, cap, Hq, Hkv)
        # slots >= past + new and query rows >= new hold +-1e4: no bit of a valid row moves
        qj = qb.clone()
        qj.view(1, T, -1)[0, N:] = _junk(Hq * D).to(dev())
        oj, lj, _ = _extend(ops, q, k, v, [0], [past], [N], T, cap, Hq, Hkv, junk=True, q_blk=qj)
        assert same_bits(oj[0, :N], clean[0, :N]) and same_bits(lj[0, :, :N].contiguous(), lclean[0, :, :N].contiguous())
        # the future-key probe: every slot > past + t holds +-1e4, row t does not move
        for t in (0, 1, 62, 63, 64, N - 1):
            kq, vq = kp.clone(), vp.clone()
            kq[0, past + t + 1:], vq[0, past + t + 1:] = _junk(Hkv * D).to(dev()), -_junk(Hkv * D).to(dev())
            op, lp = ops.attn_extend(qb, kq, vq, _i32([past]), _i32([N]), T, Hq, Hkv)
            assert same_bits(op.view(T, -1)[t], clean[0, t]), (past, t)
            assert same_bits(lp[0, :, t].contiguous(), lclean[0, :, t].contiguous()), (past, t)
    # nothing cached and nothing new: zero rows, lse = -inf (the planes hold junk: nothing is read)
    o, lse, _ = _extend(ops, q, k, v, [0], [0], [0], 3, 64, Hq, Hkv, junk=True)
    assert float(o.float().abs().max()) == 0.0 and bool(torch.isinf(lse).all()) and bool((lse < 0).all())
    # 5 cached keys and nothing new: every row runs over keys [0, 5)
    o5, l5, (qb, kp, vp) = _extend(ops, q, k, v, [0], [5], [0], 3, 64, Hq, Hkv, junk=True)
    ref, lse_ref = E.attend(qb.cpu().view(1, 3, -1), kp.cpu(), vp.cpu(), E.extend_visible([5], [0], 3, 64), Hq, Hkv)
    err = (o5.double().cpu().view(1, 3, Hq, D) - ref).abs().amax(-1)
    assert bool((err <= 2.0 ** -7 * ref.abs().amax(-1).clamp_min(2.0 ** -7)).all())
    assert float((l5.double().cpu() - lse_ref).abs().max()) <= 1e-3 * max(1.0, float(lse_ref.abs().max()))
    # ... which is what the one block row of (past 4, new 1) sees: the same bits for the same query over the same keys
    o41, l41 = ops.attn_extend(qb.view(1, 3, -1)[:, 1:2].reshape(1, -1).contiguous(), kp, vp, _i32([4]), _i32([1]), 1, Hq, Hkv)
    assert same_bits(o41[0], o5[0, 1]) and same_bits(l41[0, :, 0].contiguous(), l5[0, :, 1].contiguous())


# ----------------------------------------------------------------------------------------------- 4. the sink at an offset
def test_kvcache_store_at_writes_exactly_its_slots(ops):
    g = torch.Generator().manual_seed(3)
    B, T, cap, Hq, Hkv = 6, 5, 16, 4, 2
    qk = torch.randn(B * T, (Hq + Hkv) * D, generator=g).to(torch.bfloat16).to(dev())
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(dev())
    past, new = [0, 3, 14, 16, 20, -3], [5, 2, 5, 3, 1, 9]
    sentinel = torch.full((B, cap, Hkv * D), 0x7FC1, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    kp, vp, want_k, want_v = sentinel.clone(), sentinel.clone(), sentinel.clone(), sentinel.clone()
    ops.kvcache_store_at(qk, qkv, kp, vp, _i32(past), _i32(new), B, T, Hq, Hkv)
    st = E.stored_slots(past, new, T, cap)
    assert st.sum((1, 2)).tolist() == [5, 2, 2, 0, 0, 5]         # past + t >= cap writes nothing
    for b, t, j in st.nonzero().tolist():
        want_k[b, j] = qk[b * T + t, Hq * D:]
        want_v[b, j] = qkv[b * T + t, (Hq + Hkv) * D:]
    assert same_bits(kp, want_k) and same_bits(vp, want_v)


# -------------------------------------------------------------------------------------------------- 5. return codes
def test_attn_extend_refuses_before_any_launch(ops):
    lib = ops.load_lib()
    B, T, cap = 1, 4, 16
    SENT = 0x7FC1

    def call(Hq=4, Hkv=2, head_dim=128, T_=T, null=None):
        q = torch.zeros(B * T, Hq * D, dtype=torch.bfloat16, device=dev())
        kp = torch.zeros(B, cap, Hkv * D, dtype=torch.bfloat16, device=dev())
        o = torch.full((B * T, Hq * D), SENT, dtype=torch.int16, device=dev())
        lse = torch.full((B, Hq, T), 7.0, device=dev())
        past, new = _i32([0]), _i32([T])
        ptr = dict(q=q.data_ptr(), k=kp.data_ptr(), v=kp.data_ptr(), o=o.data_ptr(), past=past.data_ptr(), new=new.data_ptr())
        if null:
            ptr[null] = 0
        rc = lib.sd_attn_extend(ptr["q"], ptr["k"], ptr["v"], ptr["o"], lse.data_ptr(), ptr["past"], ptr["new"], Hq * D,
                                Hq * D, B, T_, cap, Hq, Hkv, head_dim, D ** -0.5, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((o == SENT).all()) and bool((lse == 7.0).all())
        return rc
    SHAPE, UNSUPPORTED = -1, -3
    assert call(head_dim=64) == UNSUPPORTED
    assert call(Hq=3, Hkv=1) == UNSUPPORTED
    assert call(T_=0) == SHAPE
    for name in ("q", "k", "v", "o", "past", "new"):
        assert call(null=name) == SHAPE, name
    assert lib.sd_attn_extend(0x1000, 0x1000, 0x1000, 0x1000, None, 0x1000, 0x1000, 512, 512, 1, 4, 0, 4, 2, 128, 0.1,
                              None) == SHAPE                                   # cap = 0
    assert lib.sd_kvcache_store_at(0x1000, 0x1000, 0x1000, 0x1000, None, 0x1000, 1, 4, 16, 4, 2, None) == SHAPE
