"""The visibility rule of include/sd_hip.h ``sd_attn_extend`` / ``sd_kvcache_store_at`` and an fp64 attention over a cache
plane: TEST INFRASTRUCTURE ONLY (never imported by the product).  tests/test_session_cpu.py checks the rule on the CPU
against the causal / kv_len mask of tests/attn_ref.py; the GPU tests use it as their reference."""
from __future__ import annotations

import math

import torch

D = 128


def clamp_past_new(past, new_len, T, cap):
    """int64 [B] each: past clamped to [0, cap], new_len to [0, min(T, cap - past)], as the kernels do."""
    p = torch.as_tensor(past).to(torch.int64).clamp(0, cap)
    n = torch.minimum(torch.as_tensor(new_len).to(torch.int64).clamp(min=0), (cap - p).clamp(max=T))
    return p, n


def extend_visible(past, new_len, T, cap):
    """bool [B, T, cap]: block row (b, t), whose position is past[b] + t, sees cache slot j  <=>
    j < min(past[b] + t + 1, past[b] + new_len[b]).  Rows t >= new_len[b] (padding) see every key of the sequence."""
    p, n = clamp_past_new(past, new_len, T, cap)
    t = torch.arange(T)[None, :, None]
    j = torch.arange(cap)[None, None, :]
    return j < torch.minimum(p[:, None, None] + t + 1, (p + n)[:, None, None])


def stored_slots(past, new_len, T, cap):
    """bool [B, T, cap]: sd_kvcache_store_at copies block row (b, t) into slot j  <=>  t < new_len[b] and j = past[b] + t."""
    p, n = clamp_past_new(past, new_len, T, cap)
    t = torch.arange(T)[None, :, None]
    j = torch.arange(cap)[None, None, :]
    return (t < n[:, None, None]) & (j == p[:, None, None] + t)


def attend(q_blk, k_plane, v_plane, vis, Hq, Hkv, scale=D ** -0.5):
    """fp64: q_blk [B,T,Hq*128], planes [B,cap,Hkv*128], vis bool [B,T,cap] -> o [B,T,Hq,128], lse [B,Hq,T] (natural log).
    A row that sees nothing is zeros with lse = -inf.  Masked slots are dropped before the products, whatever they hold."""
    B, T, _ = q_blk.shape
    cap = k_plane.shape[1]
    G = Hq // Hkv
    q = q_blk.double().reshape(B, T, Hkv, G, D)
    k = k_plane.double().reshape(B, cap, Hkv, D)
    v = v_plane.double().reshape(B, cap, Hkv, D)
    m = vis[:, None, None]                                                 # [B,1,1,T,cap]
    s = scale * torch.einsum("bthgd,bnhd->bhgtn", q, k)
    s = s.masked_fill(~m, -math.inf)
    lse = torch.logsumexp(s, -1)                                            # -inf where nothing is visible
    p = torch.where(m, torch.exp(s - lse.clamp_min(-1e300)[..., None]), torch.zeros_like(s))
    v0 = torch.where(vis.any(1)[:, :, None, None], v, torch.zeros_like(v))  # junk in never-visible slots: 0 * junk = 0
    o = torch.einsum("bhgtn,bnhd->bthgd", p, v0)
    return o.reshape(B, T, Hq, D), lse.reshape(B, Hq, T)
