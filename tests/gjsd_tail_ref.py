"""fp64 reference of the three divergences against a top-K teacher with a tail bucket (sd_gjsd_tail_*_rows, divergences
"forward_kl_tail", "reverse_kl_tail", "jsd_tail"), of the tail itself (sd_topk_tail), their case tables and their measured
tolerances.  TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product).

Definitions, per selected row (s [V] student logits; (v_k, i_k), k < K, the teacher's stored log-probs and indices; tau the
teacher's mass outside its top-K at the temperature T; 0 < b < 1; y the label; N the number of valid rows):
    p_k = softmax(v / T)_k over the kept entries;  P_j = (1 - tau) sum_{k: i_k = j} p_k;  S = {j : P_j >= FLT_MIN};  P_0 = tau
    q = softmax(s / T);  q_j on S;  q_0 = sum_{j not in S} q_j            (buckets: the elements of S, and 0 = "anything else")
    forward_kl_tail   D = sum_b P_b (log P_b - log q_b)                    g_b = -P_b / q_b
    reverse_kl_tail   D = sum_b q_b (log q_b - log P_b)                    g_b = log q_b - log P_b + 1
    jsd_tail          D = b sum_b P_b (log P_b - log m_b) + (1-b) sum_b q_b (log q_b - log m_b),  m = (1-b) q + b P
                                                                           g_b = (1-b)(log q_b - log m_b)
    d D / d s_j = q_j (g_b(j) - c) / T,  c = sum_b q_b g_b;  b(j) = j on S, 0 off it
    distill = T^2 mean D,  task = mean (lse(s) - s_y),  total = a task + (1-a) distill;  teacher / n_hits as gjsd_topk_ref
with 0 log 0 = 0.  Kept entries as gjsd_topk_ref (index inside [0, V), value finite).  S is cut at fp32's smallest normal
(the kernels' rule, which for a reverse KL is part of the definition: an element with P_j = 1e-40 would otherwise carry
q_j log(q_j / 1e-40)).  A row is masked when its label is -100 or outside [0, V), when no entry is kept, or when its tau is
NaN, < 0 or >= 1; a tau in [0, 2^-100) counts as 2^-100.

``tail_rows`` evaluates these closed forms in ``acc`` (fp64: the reference; fp32: the floor measurement), log q_0 in log
space from the off-support elements' own maximum; ``tail_total_autograd`` is the from-the-definition form (P scattered
dense, q_0 an explicit sum, torch's autograd) that tests/test_gjsd_tail_ref_cpu.py holds the closed forms against.

Tolerances follow gjsd_ref.py's method: ``measure_floors`` evaluates the closed forms in fp32 on the CPU against fp64 on
exactly the inputs of the GPU tests; the worst figures are the *_MEASURED constants below and each bound is 4 x its
measurement, rounded up to two digits.  Nothing here comes from a kernel's output.
"""
from __future__ import annotations

import functools
import math

import torch

import gjsd_ref as G
import gjsd_topk_ref as K
import parity_ref as P
from parity_ref import BF, F32

DIVERGENCES = ("forward_kl_tail", "reverse_kl_tail", "jsd_tail")
MODES = K.MODES                      # (beta, temperature); beta is read by jsd_tail only
UNDERFLOW_MODES = K.UNDERFLOW_MODES
EDGE_V, TABLE_V, TABLE_K, ALPHA = K.EDGE_V, K.TABLE_V, K.TABLE_K, K.ALPHA
UNDERFLOW_V, DROP_V = K.UNDERFLOW_V, K.DROP_V
FLT_MIN = 2.0 ** -126
TAIL_MIN = 2.0 ** -100
SPREAD = (0.5, 1e-3, 1e-7, 1e-12)    # the tails of rows without a generating teacher row, cycled over the rows
BAD_TAILS = (math.nan, -0.1, 1.0, 0.0)


def case_id(div, mode):
    return f"{div}_{K.mode_id(mode)}"


# ------------------------------------------------------------------------------------------------- the tail itself
def tail_direct(t, ti, temperature, V=None, acc=torch.float64):
    """sum_{j not in {i_k}} exp(t_j / T) / sum_j exp(t_j / T) over the first V columns, summed directly over the non-members
    in ``acc``; indices outside [0, V) are ignored.  t [R, >=V], ti [R, K] -> [R]."""
    V = t.shape[-1] if V is None else V
    x = t[:, :V].to(acc) / temperature
    idx = ti.long()
    ok = (idx >= 0) & (idx < V)
    member = torch.zeros(x.shape[0], V + 1, dtype=torch.bool)          # (column V collects the ignored indices)
    member.scatter_(1, torch.where(ok, idx, torch.full_like(idx, V)), True)
    member = member[:, :V]
    e = (x - x.amax(-1, keepdim=True)).exp()
    return torch.where(member, torch.zeros_like(e), e).sum(-1) / e.sum(-1)


def spread_tails(n_rows):
    return torch.tensor([SPREAD[r % len(SPREAD)] for r in range(n_rows)], dtype=torch.float32)


# ------------------------------------------------------------------------------------------------- reference
def bucket_P(tv, ti, tau, V, temperature, acc=torch.float64):
    """-> P [R,V] (0 off S), on [R,V], tau clamped [R], usable [R] (an entry kept and tau in [0, 1)), all in ``acc``."""
    Pd, some = K.scatter_P(tv, ti, V, temperature, acc)
    t = tau.to(acc)
    ok = (t >= 0) & (t < 1)
    t = torch.where(ok, t.clamp_min(TAIL_MIN), torch.full_like(t, 0.5))
    Pd = (1.0 - t)[:, None] * Pd
    on = Pd >= FLT_MIN
    return torch.where(on, Pd, torch.zeros_like(Pd)), on, t, some & ok


def divergence_terms(s, Pd, on, t, divergence, beta, temperature, acc=torch.float64):
    """-> D [R] and the distillation gradient's bracket W [R,V] with d D / d s_j = W_j / T (so W_j = q_j (g_b(j) - c)), in
    ``acc``.  log q_0 comes from the off-support elements with their own maximum."""
    x = s.to(acc) / temperature
    a = G._log_softmax(x)
    q = a.exp()
    ninf = torch.full_like(x, -math.inf)
    m = x.amax(-1, keepdim=True)
    xo = torch.where(on, ninf, x)
    m0 = xo.amax(-1, keepdim=True)
    lq0 = ((m0 - m) + (xo - m0).exp().sum(-1, keepdim=True).log() - (x - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)
    q0, lt = lq0.exp(), t.log()
    one, zero = torch.ones_like(Pd), torch.zeros_like(q)
    lP = torch.where(on, Pd, one).log()
    if divergence == "forward_kl_tail":
        D = torch.where(on, Pd * (lP - a), zero).sum(-1) + t * (lt - lq0)
        W = torch.where(on, q - Pd, q - t[:, None] * (a - lq0[:, None]).exp())
        return D, W
    if divergence == "reverse_kl_tail":
        D = torch.where(on, G._xlog(q, a - lP), zero).sum(-1) + G._xlog(q0, lq0 - lt)
        g = torch.where(on, a - lP, (lq0 - lt)[:, None].expand_as(a))
        return D, G._xlog(q, g - D[:, None])
    if divergence != "jsd_tail" or not 0.0 < beta < 1.0:
        raise ValueError((divergence, beta))
    lm = torch.where(on, (1.0 - beta) * q + beta * Pd, one).log()
    lm0 = torch.logaddexp(math.log(1.0 - beta) + lq0, math.log(beta) + lt)
    klp = torch.where(on, Pd * (lP - lm), zero).sum(-1) + t * (lt - lm0)
    klq = torch.where(on, G._xlog(q, a - lm), zero).sum(-1) + G._xlog(q0, lq0 - lm0)
    g = (1.0 - beta) * torch.where(on, a - lm, (lq0 - lm0)[:, None].expand_as(a))
    return beta * klp + (1.0 - beta) * klq, G._xlog(q, g - (1.0 - beta) * klq[:, None])


def tail_rows(s, tv, ti, tau, labels, divergence, beta=0.5, temperature=2.0, alpha=0.5, acc=torch.float64):
    """-> ((total, task, distill, teacher) floats, N, n_hits, D [R] (0 on masked rows), grad [R,V]) in ``acc``."""
    R, V = s.shape
    Pd, on, t, usable = bucket_P(tv, ti, tau, V, temperature, acc)
    valid = (labels >= 0) & (labels < V) & usable
    n = int(valid.sum())
    y = labels.clamp(0, V - 1)
    x = s.to(acc)
    ls = G._log_softmax(x)
    task = -ls.gather(-1, y[:, None]).squeeze(-1)
    D, W = divergence_terms(s, Pd, on, t, divergence, beta, temperature, acc)
    zero = torch.zeros_like(D)
    D = torch.where(valid, D, zero)
    hit = K.kept(tv, ti, V) & (ti.long() == labels[:, None]) & valid[:, None]
    hits = int(hit.sum())
    teacher = -float(torch.where(hit, tv.to(acc), torch.zeros((), dtype=acc)).sum()) / hits if hits else 0.0
    if n == 0:
        return (0.0, 0.0, 0.0, 0.0), 0, 0, D, torch.zeros_like(x)
    task_m = torch.where(valid, task, zero).sum() / n
    dist_m = D.sum() / n * temperature * temperature
    total = alpha * task_m + (1.0 - alpha) * dist_m
    ce = ls.exp()
    ce[torch.arange(R), y] -= 1.0
    grad = (alpha * ce + (1.0 - alpha) * temperature * W) / n
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return (float(total), float(task_m), float(dist_m), teacher), n, hits, D, grad


def tail_total_autograd(s64, tv, ti, tau, labels, divergence, beta, temperature, alpha):
    """``total`` as a differentiable fp64 scalar, from the definition: P scattered dense, the bucket sums written out (q_0 an
    explicit sum over the off-support elements), torch's log_softmax / xlogy, no closed-form gradient (for inputs without
    underflow)."""
    V = s64.shape[1]
    Pd, on, t, usable = bucket_P(tv, ti, tau, V, temperature)
    valid = (labels >= 0) & (labels < V) & usable
    n = int(valid.sum())
    a = torch.log_softmax(s64 / temperature, -1)
    q = a.exp()
    q0 = torch.where(on, torch.zeros_like(q), q).sum(-1)
    qb = torch.cat([torch.where(on, q, torch.zeros_like(q)), q0[:, None]], -1)     # [R, V + 1]: S scattered, bucket 0 last
    Pb = torch.cat([Pd, t[:, None]], -1)
    if divergence == "forward_kl_tail":
        D = (torch.xlogy(Pb, Pb) - torch.xlogy(Pb, qb)).sum(-1)
    elif divergence == "reverse_kl_tail":
        live = torch.cat([on, torch.ones_like(on[:, :1])], -1)
        D = torch.where(live, torch.xlogy(qb, qb) - qb * torch.where(live, Pb, torch.ones_like(Pb)).log(),
                        torch.zeros_like(qb)).sum(-1)
    else:
        mb = (1.0 - beta) * qb + beta * Pb
        D = (beta * (torch.xlogy(Pb, Pb) - torch.xlogy(Pb, mb)) + (1.0 - beta) * (torch.xlogy(qb, qb) - torch.xlogy(qb, mb))).sum(-1)
    task = -torch.log_softmax(s64, -1).gather(-1, labels.clamp(0, V - 1)[:, None]).squeeze(-1)
    return (alpha * task[valid].sum() + (1.0 - alpha) * temperature ** 2 * D[valid].sum()) / n


# ------------------------------------------------------------------------------------------------- inputs
# Each is gjsd_topk_ref's set with a tau column: (s, tv, ti, tau, labels).  Where the set's top-K was extracted from a
# teacher row that parity_ref still has (the table sets), tau is that row's true tail at the mode's temperature, in fp32 as
# sd_topk_tail stores it; elsewhere the fixed spread.
def _true_tails(V, dtype, Kk, temperature):
    t = P.loss_inputs(V, dtype)[1]
    return tail_direct(t.float(), P.loss_topk(V, dtype, Kk)[1], temperature).float()


@functools.lru_cache(maxsize=None)
def table_inputs(V, dtype, temperature, Kk=100):
    s, tv, ti, lab = K.table_inputs(V, dtype, Kk)
    return s, tv, ti, _true_tails(V, dtype, K._k_for(V, Kk), temperature), lab


@functools.lru_cache(maxsize=None)
def extras_inputs(V, dtype, temperature, name):
    s, tv, ti, lab = K.extras_inputs(V, dtype, name)
    return s, tv, ti, _true_tails(V, dtype, 100, temperature), lab


@functools.lru_cache(maxsize=None)
def peaked_inputs(V, dtype):
    s, tv, ti, lab = K.peaked_inputs(V, dtype)
    return s, tv, ti, spread_tails(len(lab)), lab


@functools.lru_cache(maxsize=None)
def underflow_inputs(V, dtype):
    """gjsd_topk_ref's underflow rows (T = 1): with the student spike of 200 on a support index (rows 0, 3) q_0 is ~1e-80
    and only its logarithm exists in fp32; tails 0.5, 1e-3, 1e-7, 1e-12."""
    s, tv, ti, lab = K.underflow_inputs(V, dtype)
    return s, tv, ti, spread_tails(len(lab)), lab


@functools.lru_cache(maxsize=None)
def dropped_inputs(V, dtype, temperature):
    """-> (with, without) of gjsd_topk_ref.dropped_inputs, both with the true tails of the rows the live entries came from."""
    (s, tv, ti, lab), (_, tv0, ti0, lab0) = K.dropped_inputs(V, dtype)
    tau = _true_tails(V, dtype, ti0.shape[1], temperature)
    return (s, tv, ti, tau, lab), (s, tv0, ti0, tau, lab0)


@functools.lru_cache(maxsize=None)
def bad_tail_inputs(V, dtype, temperature):
    """The table set with the tails of rows 0-3 replaced by NaN, -0.1, 1.0 (masked rows) and 0.0 (counts as 2^-100)."""
    s, tv, ti, tau, lab = table_inputs(V, dtype, temperature)
    tau = tau.clone()
    tau[:4] = torch.tensor(BAD_TAILS, dtype=torch.float32)
    return s, tv, ti, tau, lab


def family_cases(family):
    """[(inputs tuple, mode)] of one tolerance family, exactly what tests/test_gpu_gjsd_tail.py runs (for each divergence)."""
    out = []
    if family == "table":
        for dt in (BF, F32):
            for m in MODES:
                out += [(table_inputs(V, dt, m[1]), m) for V in (TABLE_V,) + EDGE_V]
            for Kk in TABLE_K[1:]:
                out += [(table_inputs(TABLE_V, dt, m[1], Kk), m) for m in MODES[:2]]
            for name in ("duplicates", "ends", "no_hit"):
                out += [(extras_inputs(TABLE_V, dt, m[1], name), m) for m in MODES[:2]]
            out += [(dropped_inputs(DROP_V, dt, m[1])[1], m) for m in MODES[:2]]
            out += [(bad_tail_inputs(DROP_V, dt, m[1]), m) for m in MODES[:2]]
    elif family == "peaked":
        out = [(peaked_inputs(TABLE_V, dt), m) for dt in (BF, F32) for m in MODES]
    else:
        out = [(underflow_inputs(UNDERFLOW_V, dt), m) for dt in (BF, F32) for m in UNDERFLOW_MODES]
    return out


# ------------------------------------------------------------------------------------------------- tolerances
# Measured by measure_floors(): the closed forms in fp32 on the CPU against fp64, worst over every case of the family and
# the three divergences.  Gradient, relative to the row maximum, per row CLASS (peaked rows, every other row), the classes
# of gjsd_topk_ref.  Scalars by gjsd_topk_ref's rules (task and teacher pooled; distill per family over the entries with
# |ref| >= SMALL, the smaller ones by atol: 4 x their worst fp32 error, never below parity_ref's 1e-6).
PEAKED_ROWS = K.PEAKED_ROWS
GRAD_MEASURED = {"table": (1.40e-6, 1.95e-6), "peaked": (1.47e-5, 1.24e-7), "underflow": (2.45e-7, 6.30e-7)}
GRAD_FLOOR = {"table": (5.6e-6, 7.8e-6), "peaked": (5.9e-5, 5.0e-7), "underflow": (9.8e-7, 2.6e-6)}
SMALL = G.SMALL
CE_MEASURED = 1.53e-6
CE_RTOL = 6.2e-6
TEACHER_MEASURED = 0.0   # sums of a few fp16 values are exact in fp32: the bound is the atol alone
TEACHER_RTOL = 0.0
DISTILL_MEASURED = {"table": 3.16e-5, "peaked": 3.00e-5, "underflow": 2.08e-7}
DISTILL_RTOL = {"table": 1.3e-4, "peaked": 1.2e-4, "underflow": 8.4e-7}
SMALL_ABS_MEASURED = {"table": 0.0, "peaked": 5.92e-7, "underflow": 1.0e-12}   # peaked: 4 x 5.92e-7 is above parity_ref's 1e-6
SCALAR_ATOL = {"table": P.LOSS_SCALAR_ATOL, "peaked": 2.4e-6, "underflow": P.LOSS_SCALAR_ATOL}
# sd_topk_tail against tail_direct in fp64, relative: the direct sum in fp32 on the CPU over TAIL_CASES (measure_tail_floor)
TAIL_MEASURED = 8.12e-7
TAIL_RTOL = 3.3e-6


def scalar_bounds(ref_losses, family, alpha=ALPHA):
    """-> the four absolute bounds of (total, task, distill, teacher) at the reference values (gjsd_topk_ref's rules)."""
    total, task, distill, teacher = (abs(float(x)) for x in ref_losses)
    atol = SCALAR_ATOL[family]
    b_task, b_teacher = CE_RTOL * task + atol, TEACHER_RTOL * teacher + atol
    b_distill = DISTILL_RTOL[family] * distill + atol
    return [alpha * b_task + (1.0 - alpha) * b_distill + 2.0 ** -23 * total, b_task, b_distill, b_teacher]


def scalars_close(got_losses, ref_losses, family, alpha=ALPHA):
    """-> (ok, worst entry, its err / bound): every entry finite and within its bound."""
    ratios = []
    for g, r, b in zip(got_losses, ref_losses, scalar_bounds(ref_losses, family, alpha)):
        err = abs(float(g) - float(r))
        ratios.append(err / b if err == err and err != float("inf") else float("inf"))
    i = max(range(4), key=lambda k: ratios[k])
    return all(x <= 1.0 for x in ratios), i, ratios[i]


def grad_floor_rows(family, n_rows, rows=None):
    """[R, 1] fp64 tensor of the gradient floor of each row of a family's inputs (``rows``: a subset, in order)."""
    peaked, other = GRAD_FLOOR[family]
    f = torch.full((n_rows, 1), other, dtype=torch.float64)
    f[[r for r in PEAKED_ROWS[family] if r < n_rows]] = peaked
    return f if rows is None else f[rows]


def measure_floors(families=("table", "peaked", "underflow")):
    """-> {family: dict(grad=(peaked, other), ce, teacher, distill_rel, small_abs)} of the fp32 evaluation against fp64 on
    the inputs of the GPU tests: every batch and every single valid row, the three divergences."""
    out = {}
    for fam in families:
        grad, ce, teach, dist, small = [0.0, 0.0], 0.0, 0.0, 0.0, 0.0
        for (s, tv, ti, tau, labels), (beta, T) in family_cases(fam):
            n_rows = len(labels)
            for div in DIVERGENCES:
                for rows in [slice(None)] + [slice(r, r + 1) for r in range(n_rows) if labels[r] >= 0]:
                    a = (s[rows], tv[rows], ti[rows], tau[rows], labels[rows], div, beta, T, ALPHA)
                    l64, _, _, _, g64 = tail_rows(*a)
                    l32, _, _, _, g32 = tail_rows(*a, acc=torch.float32)
                    rel = (lambda i: abs(l32[i] - l64[i]) / abs(l64[i]) if l64[i] != 0.0 else 0.0)
                    ce, teach = max(ce, rel(1)), max(teach, rel(3))
                    if abs(l64[2]) >= SMALL:
                        dist = max(dist, rel(2))
                    else:
                        small = max(small, abs(l32[2] - l64[2]))
                    if rows == slice(None):
                        for r in range(n_rows):
                            if float(g64[r].abs().max()) > 0.0:
                                k = 0 if r in PEAKED_ROWS[fam] else 1
                                grad[k] = max(grad[k], P._row_rel(g32[r:r + 1], g64[r:r + 1]))
        out[fam] = dict(grad=tuple(grad), ce=ce, teacher=teach, distill_rel=dist, small_abs=small)
    return out


def tail_close(got_losses, got_grad, ref_losses, ref_grad, grad_dtype, family):
    """The acceptance rule of one call on a family's whole input: four scalars (scalars_close) and the gradient per row and
    per element (parity_ref.rowwise_close with each row's floor).  -> (ok, text)."""
    s_ok, i, ratio = scalars_close(got_losses, ref_losses, family)
    v = P.rowwise_close(got_grad, ref_grad, grad_dtype, grad_floor_rows(family, ref_grad.shape[0]))
    return s_ok and v.ok, (f"scalars ok={s_ok} worst={('total', 'task', 'distill', 'teacher')[i]} err/bound={ratio:.3f}; "
                           f"grad {v}")


# ------------------------------------------------------------------------------------------------- sd_topk_tail's cases
TAIL_TEMPERATURES = (1.0, 2.0, 3.0)
TAIL_BIG_V = 159488
TAIL_MAX_V = 524288    # the largest vocabulary sd_topk_tail takes: its bitmap is the whole 64 KB of LDS


@functools.lru_cache(maxsize=None)
def tail_case(name, dtype):
    """-> (logits [R, stride] in ``dtype``, top_i int32 [R, K], V) of one sd_topk_tail case; the columns V..stride, where
    there are any, hold NaN / +inf (never to be read)."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (1 if dtype == BF else 0))
    if name.startswith("randn"):                     # "randn_V<V>_K<K>"
        V, Kk = (int(x[1:]) for x in name.split("_")[1:])
        R = 2 if V >= TAIL_BIG_V else 4
        t = (torch.randn(R, V, generator=gen) * 3).to(dtype)
        return t, P.topk_ref(t.float(), Kk)[1].int(), V
    V, Kk, R = 16392, 100, 4
    t = (torch.randn(R, V, generator=gen) * 3).to(dtype)
    if name == "spike":                              # one logit 37 above a narrow rest: tails of ~1e-12 at T = 1, ~1e-4 at T = 2
        t = (torch.randn(R, V, generator=gen) * 0.5).to(dtype)
        t[:, 77] = 37.0
        return t, P.topk_ref(t.float(), Kk)[1].int(), V
    if name == "ties":                               # 300 equal logits across the K-th boundary: membership is by index
        t[:, 1000:1300] = 9.0
        return t, P.topk_ref(t.float(), Kk)[1].int(), V
    ti = P.topk_ref(t.float(), Kk)[1].int()
    if name == "bad_indices":                        # duplicates, -1, V, 2^31 - 1 among the indices
        ti[:, 5] = ti[:, 4]
        ti[:, 6] = ti[:, 4]
        ti[0, 7], ti[1, 8], ti[2, 9], ti[3, 0] = -1, V, 2 ** 31 - 1, -(2 ** 31)
        return t, ti, V
    assert name == "stride"                          # row_stride > V, poison behind the row
    wide = torch.full((R, V + 24), math.nan, dtype=dtype)
    wide[:, V + 8:] = math.inf
    wide[:, :V] = t
    return wide, ti, V


TAIL_CASES = (["randn_V8_K4"] + [f"randn_V{V}_K{Kk}" for V in EDGE_V[1:] + (TABLE_V,) for Kk in (1, 100, 1024)]
              + [f"randn_V{TAIL_BIG_V}_K100", f"randn_V{TAIL_MAX_V}_K100", "spike", "ties", "bad_indices", "stride"])


def measure_tail_floor():
    """The worst relative error of the direct sum in fp32 on the CPU against fp64 over TAIL_CASES x temperatures x dtypes."""
    worst = 0.0
    for name in TAIL_CASES:
        for dt in (BF, F32):
            t, ti, V = tail_case(name, dt)
            for T in TAIL_TEMPERATURES:
                r64 = tail_direct(t.float(), ti, T, V)
                r32 = tail_direct(t.float(), ti, T, V, acc=torch.float32).double()
                worst = max(worst, float(((r32 - r64).abs() / r64).max()))
    return worst
