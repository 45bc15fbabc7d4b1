"""Causal GQA attention in plain fp64 torch: TEST INFRASTRUCTURE ONLY (never imported by the product).

``attn_ref`` writes the forward and the backward of include/sd_hip.h ``sd_attn_fwd`` / ``sd_attn_bwd`` out term by term
(S, mask, logsumexp, P, delta, dP, dS and the three products), without autograd and without oracle/ (whose attention
takes its softmax in fp32 even for fp64 inputs).  With ``emulate=True`` the same computation rounds to bf16 where the HIP
path stores bf16 or feeds the matrix unit with it; the error of that run against the unrounded one is the NOISE MODEL:
what a correct bf16 kernel is expected to show.  It never looks at the code under test.

``row_err`` / ``judge`` are the acceptance rule of tests/test_gpu_attn_edges.py, and tests/test_attn_ref_cpu.py shows on
the CPU that the rule rejects wrong masks and accepts the clean emulation.

Layout as in the C ABI: q, do [B*T, Hq*128]; k, v [B*T, Hkv*128]; head h at columns h*128 .. h*128+127; LSE [B, Hq, T].
"""
from __future__ import annotations

import math

import torch

D = 128
F32_TINY = 2.0 ** -126
BF16_ROW_EPS = 2.0 ** -9   # relative error of one bf16 rounding: no bf16 result can be held to less per row
F_ROW = 2.0                # per-row error budget: HIP row error <= F_ROW x the emulation's worst row of the same tile
# the global limits of tests/test_gpu_kernels.py::test_attention_fwd_bwd (max / rms of the whole tensor), unchanged
GLOBAL_LIMITS = {"o": (1.5e-2, 4e-3), "dq": (2e-2, 6e-3), "dk": (2e-2, 6e-3), "dv": (2e-2, 6e-3)}
NAMES = ("o", "lse", "dq", "dk", "dv")


def _bf(x):
    """bf16 storage of an fp64 value: magnitudes below the smallest normal fp32 number go to zero first (the kernels
    compute in fp32 with hardware exp2, which has no denormal results), then round to nearest even."""
    x = torch.where(x.abs() < F32_TINY, torch.zeros_like(x), x)
    return x.to(torch.bfloat16).double()


def clamp_kv_len(kv_len, B, T):
    """int64 [B]; None -> T; clamped to [1, T] as the kernels do."""
    if kv_len is None:
        return torch.full((B,), T, dtype=torch.int64)
    return torch.as_tensor(kv_len).to(torch.int64).clamp(1, T)


def visible_mask(B, T, kv_len=None):
    """bool [B, T, T]: query i of batch entry b sees key j  <=>  j <= i and j < kv_len[b].  Query rows >= kv_len are
    ordinary rows (they see the keys below kv_len)."""
    kl = clamp_kv_len(kv_len, B, T)
    i = torch.arange(T)
    return (i[None, None, :] <= i[None, :, None]) & (i[None, None, :] < kl[:, None, None])


def attn_ref(q, k, v, do, B, T, Hq, Hkv, kv_len=None, scale=D ** -0.5, emulate=False, mask=None, o_given=None):
    """-> dict o [M,Hq*128], lse [B,Hq,T], dq [M,Hq*128], dk, dv [M,Hkv*128], all fp64.

    ``mask`` (bool [B,T,T] or [T,T], True = visible) replaces the causal / kv_len mask: the mutation tests edit it.
    emulate=True rounds to bf16: P before P.V and dO^T.P, dS before the dQ / dK products, O before delta, and
    O, dQ, dK, dV on the way out; LSE is rounded to fp32 (the kernels store it so).
    emulate="unnorm": the same, except that the forward rounds the UNNORMALISED probabilities exp(S - rowmax) and divides
    P.V by the unrounded row sum, as a flash forward does (the backward still rounds the normalised P it recomputes from
    LSE).  A second, equally legitimate draw of the rounding noise: the CPU tests judge it as they would a kernel.
    ``o_given`` [M, Hq*128]: the backward as the OPERATOR sd_attn_bwd is, whose ``o`` is an input: delta = rowsum(dO *
    o_given) instead of the O computed here (everything else unchanged, the returned "o" included)."""
    G = Hq // Hkv
    assert G * Hkv == Hq
    if mask is None:
        mask = visible_mask(B, T, kv_len)
    mask = torch.as_tensor(mask)
    if mask.dim() == 2:
        mask = mask[None].expand(B, T, T)
    rnd = _bf if emulate else (lambda x: x)
    q4 = q.double().reshape(B, T, Hkv, G, D).permute(0, 2, 3, 1, 4)    # [B, Hkv, G, T, D]
    do4 = do.double().reshape(B, T, Hkv, G, D).permute(0, 2, 3, 1, 4)
    k4 = k.double().reshape(B, T, Hkv, D).permute(0, 2, 1, 3)          # [B, Hkv, T, D]
    v4 = v.double().reshape(B, T, Hkv, D).permute(0, 2, 1, 3)
    o = torch.empty(B, Hkv, G, T, D, dtype=torch.float64)
    dq = torch.empty_like(o)
    lse = torch.empty(B, Hkv, G, T, dtype=torch.float64)
    dk = torch.empty(B, Hkv, T, D, dtype=torch.float64)
    dv = torch.empty_like(dk)
    og4 = None if o_given is None else o_given.detach().double().cpu().reshape(B, T, Hkv, G, D).permute(0, 2, 3, 1, 4)
    for b in range(B):  # one batch entry at a time keeps the [Hq, T, T] temporaries small
        qb, dob, kb, vb = q4[b], do4[b], k4[b][:, None], v4[b][:, None]        # k, v broadcast over the group axis
        s = scale * (qb @ kb.transpose(-1, -2))                                 # S [Hkv, G, T, T]
        s = s.masked_fill(~mask[b][None, None], -math.inf)
        lb = torch.logsumexp(s, -1)                                             # LSE (natural log)
        p = torch.exp(s - lb[..., None])                                        # P
        pr = rnd(p)
        if emulate == "unnorm":
            pu = torch.exp(s - s.amax(-1, keepdim=True))
            ob = (rnd(pu) @ vb) / pu.sum(-1, keepdim=True)
        else:
            ob = pr @ vb                                                        # O = P V
        delta = (dob * (rnd(ob) if og4 is None else og4[b])).sum(-1, keepdim=True)   # delta = rowsum(dO * O)
        dp = dob @ vb.transpose(-1, -2)                                         # dP = dO V^T
        ds = rnd(p * (dp - delta))                                              # dS = P (dP - delta)
        o[b], lse[b] = ob, lb
        dq[b] = scale * (ds @ kb)                                               # dQ = scale dS K
        dk[b] = scale * (ds.transpose(-1, -2) @ qb).sum(1)                      # dK = scale sum_group dS^T Q
        dv[b] = (pr.transpose(-1, -2) @ dob).sum(1)                             # dV = sum_group P^T dO
    M = B * T
    out = {"o": rnd(o.permute(0, 3, 1, 2, 4).reshape(M, Hq * D)),
           "lse": lse.reshape(B, Hq, T).float().double() if emulate else lse.reshape(B, Hq, T),
           "dq": rnd(dq.permute(0, 3, 1, 2, 4).reshape(M, Hq * D)),
           "dk": rnd(dk.permute(0, 2, 1, 3).reshape(M, Hkv * D)),
           "dv": rnd(dv.permute(0, 2, 1, 3).reshape(M, Hkv * D))}
    return out


def score_magnitude(q, k, B, T, Hq, Hkv, scale):
    """max over (query, key, head) of scale * sum_d |q_d| |k_d|: what the fp32 accumulation of one score adds up."""
    G = Hq // Hkv
    qa = q.double().abs().reshape(B, T, Hkv, G, D).permute(0, 2, 3, 1, 4)
    ka = k.double().abs().reshape(B, T, Hkv, D).permute(0, 2, 1, 3)[:, :, None]
    return float(max((scale * (qa[b] @ ka[b].transpose(-1, -2))).max() for b in range(B)))


def lse_tolerance(q, k, lse_ref, B, T, Hq, Hkv, scale):
    """Bound on |LSE_hip - LSE_fp64| from the number formats, not from any kernel's output.  LSE = m * scale + log(l):
    a score is an fp32 sum of exact bf16 products whose partial sums are at most A = score_magnitude (a few ulps of A;
    LSE is a softmax-weighted mean of the scores, so it errs no more than they do), m * scale and the final sum round at
    |LSE|, and the fast log adds an absolute error of about 2^-21.  Budget: 8 ulps of max(A, 1), 4 ulps of |LSE|, 2^-20."""
    A = score_magnitude(q, k, B, T, Hq, Hkv, scale)
    ulp = 2.0 ** -23
    return 8 * ulp * max(A, 1.0) + 4 * ulp * float(lse_ref.abs().max()) + 2.0 ** -20


def row_err(got, ref):
    """Per (token, head) row of 128: ||got - ref||_2 / max(||ref||_2, 0.05 * median row norm of ref); the vector of all
    rows, token-major.  The floor only keeps exactly-zero rows (dQ of token 0) from dividing by zero; no row is excluded.
    Where that median is zero (more than half of the rows are exactly zero: dK / dV of a batch that is mostly padding)
    the median of the non-zero rows takes its place; with no such row, a row that equals the reference has error 0 and
    any other row has error inf."""
    g = got.detach().double().cpu().reshape(-1, D)
    r = ref.detach().double().cpu().reshape(-1, D)
    dn = (g - r).norm(dim=-1)
    rn = r.norm(dim=-1)
    med = rn.median()
    if med == 0 and bool((rn > 0).any()):
        med = rn[rn > 0].median()
    den = torch.maximum(rn, 0.05 * med)
    err = dn / den
    err = torch.where(dn == 0, torch.zeros_like(err), err)
    return torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)


def tile_bound(emu_err, B, T, F=F_ROW):
    """Per-row allowance from the emulation's row errors [B*T*H]: F x the worst emulated row among the rows (all heads)
    of the same 64-token tile of the same batch entry, and never less than F x one bf16 rounding.  Local on purpose: the
    emulated dQ error peaks in the first rows (few keys, small gradients), and one maximum over the whole tensor would
    lend that allowance to every late row, where a mask error shows."""
    H = emu_err.numel() // (B * T)
    e = emu_err.reshape(B, T, H)
    out = torch.empty_like(e)
    for t0 in range(0, T, 64):
        out[:, t0:t0 + 64] = e[:, t0:t0 + 64].amax(dim=(1, 2), keepdim=True)
    return F * out.clamp_min(BF16_ROW_EPS).reshape(-1)


def global_err(got, ref):
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    mx = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-30)
    rms = float((g - r).pow(2).mean().sqrt()) / max(float(r.pow(2).mean().sqrt()), 1e-30)
    return mx, rms


F_RMS = 1.5               # the project's per-tensor gradient budget (gpu_util.assert_grad_budget)


def judge(got, ref, emu, ref_g, ref_e, B, T, lse_tol, per_row=("o", "dq", "dk", "dv"), rms_budget=()):
    """The acceptance rule.  got / ref / emu: dicts as attn_ref returns them.  Per tensor: finite; the global max / rms
    limits against ``ref``; for the names in ``per_row`` every row within tile_bound of the emulation; LSE within
    ``lse_tol`` of the fp64 value.  Returns {name: {"ok", "ratio" (worst row error / (allowance / F_ROW)), ...}}.

    ``ref_g`` / ``ref_e``: attn_ref(..., o_given=got["o"]) and attn_ref(..., o_given=emu["o"]).  The per-row rule of dQ,
    dK, dV measures got against ref_g and emu against ref_e: the backward as the operator it is, on the ``o`` it was
    handed.  Why: delta = rowsum(dO * O) carries the bf16 rounding of the stored O (about 0.03 absolute) into every dS
    of the row as a common offset, and in rows with a handful of visible keys, where dS nearly cancels, that alone is
    0.1 - 0.5 of the dQ row.  The kernel's O and the emulation's O are two different roundings (unnormalised against
    normalised P), hence two independent draws of that heavy-tailed term, and their ratio is not bounded by any F
    (measured on the MI355X: up to 7.1 at row 1 of a batch entry, every other output within 1.7; on the CPU between
    the two emulations: tests/test_attn_ref_cpu.py::test_first_rows_of_dq_need_the_o_given_reference).  Conditioning
    both sides on their own O removes the draw and leaves what the backward kernels compute.  O itself, and the
    gradients under the global limits, are still measured against the plain reference ``ref``.

    ``rms_budget`` names tensors whose rms limit becomes F_RMS x the emulation's own rms error, and only where that
    error ITSELF exceeds the global limit ("rms_widened" in the result says whether it did).  That is dQ on the rising
    ramps: a dS row sums to zero while columns 0 / 1 of K reach 63, so the bf16 rounding of dS alone puts the emulated
    dQ at 1.1e-2 (step 0.25) to 2.7e-2 (step 1.0) rms, above the 6e-3 that holds everywhere else; no bf16 kernel can
    do better there."""
    res = {}
    for n in NAMES:
        g = got[n].detach().double().cpu()
        finite = bool(torch.isfinite(g).all())
        if n == "lse":
            err = float((g - ref[n]).abs().max())
            res[n] = {"ok": finite and err <= lse_tol, "abs_err": err, "tol": lse_tol, "ratio": err / lse_tol}
            continue
        mx, rms = global_err(g, ref[n])
        max_lim, rms_lim = GLOBAL_LIMITS[n]
        emu_rms = global_err(emu[n], ref[n])[1]
        widened = n in rms_budget and emu_rms > rms_lim
        if widened:
            rms_lim = F_RMS * emu_rms
        he = row_err(g, ref[n] if n == "o" else ref_g[n])
        ee = row_err(emu[n], ref[n] if n == "o" else ref_e[n])
        ratio_v = he / tile_bound(ee, B, T, 1.0)
        worst = int(ratio_v.argmax())
        ratio = float(ratio_v[worst])
        ok = finite and mx <= max_lim and rms <= rms_lim and (n not in per_row or ratio <= F_ROW)
        res[n] = {"ok": ok, "max_rel": mx, "rms_rel": rms, "rms_lim": rms_lim, "rms_widened": widened, "rms_emu": emu_rms,
                  "row_hip": float(he.max()), "row_emu": float(ee.max()), "ratio": ratio, "worst_row": worst,
                  "per_row": n in per_row}
    return res


def rejected(res):
    return [n for n, r in res.items() if not r["ok"]]


# ------------------------------------------------------------------------------------------------ the kv_len grid
KV_SET = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # plus T - 1 and T


def kv_values(T):
    return sorted({x for x in KV_SET + (T - 1, T) if 1 <= x <= T})


def kv_launches(T):
    """Batches of 8 kv_len values that together cover kv_values(T)."""
    vals = kv_values(T)
    n = (len(vals) + 7) // 8
    return [tuple(vals[(8 * i + j) % len(vals)] for j in range(8)) for i in range(n)]


# ------------------------------------------------------------------------------------------------ input builders
def randn_inputs(B, T, Hq, Hkv, seed, gain=1.0):
    """q, k, v, do ~ gain * N(0, 1), rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    M = B * T
    return tuple((gain * torch.randn(M, h * D, generator=g)).to(torch.bfloat16) for h in (Hq, Hkv, Hkv, Hq))


def ramp_inputs(B, T, Hq, Hkv, seed, sign, step):
    """Scores that move with the key index: q, k = 0.25 randn, then column 0 of k = sign * (j // 64), column 1 =
    sign * (j % 64) and columns 0 / 1 of every q row = (64 g, g) with g = bf16(step * sqrt(128)), so that with the
    kernels' scale 128^-1/2 score(i, j) = sign * step * j nats plus O(0.1) noise; every value is exact in bf16.
    sign = +1 (rising): every future key outscores every visible one, so a causal or padding leak takes the row over, and
    the running maximum moves in every tile.  sign = -1 (falling): key 0 dominates and later tiles underflow, so a
    dropped first tile or a broken light-tile path shows."""
    g = torch.Generator().manual_seed(seed)
    M = B * T
    q, k = (0.25 * torch.randn(M, h * D, generator=g) for h in (Hq, Hkv))
    v, do = (torch.randn(M, h * D, generator=g) for h in (Hkv, Hq))
    j = torch.arange(M) % T
    gq = float(torch.tensor(step * math.sqrt(D)).to(torch.bfloat16))
    k = k.reshape(M, Hkv, D)
    k[:, :, 0] = (sign * (j // 64)).double()[:, None]
    k[:, :, 1] = (sign * (j % 64)).double()[:, None]
    q = q.reshape(M, Hq, D)
    q[:, :, 0] = 64 * gq
    q[:, :, 1] = gq
    return tuple(t.reshape(M, -1).to(torch.bfloat16) for t in (q, k, v, do))


def poison(k, v, B, T, kv_len, seed=12345):
    """Copies of k, v with every key row >= kv_len[b] replaced by large FINITE values (k: 50 randn, v: 1000 randn).
    Finite on purpose: a flash kernel multiplies masked probabilities (exact zeros) into V, and 0 * inf is NaN in any
    such kernel, flash_attn included; the contract under test is "masked keys have no influence", not "masked memory may
    hold NaN"."""
    g = torch.Generator().manual_seed(seed)
    kl = clamp_kv_len(kv_len, B, T)
    pad = (torch.arange(T)[None, :] >= kl[:, None]).reshape(B * T)
    kp, vp = k.clone(), v.clone()
    kp[pad] = (50 * torch.randn(int(pad.sum()), k.shape[1], generator=g)).to(k.dtype)
    vp[pad] = (1000 * torch.randn(int(pad.sum()), v.shape[1], generator=g)).to(v.dtype)
    return kp, vp
