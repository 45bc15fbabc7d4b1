"""fp64 reference of the skewed Jensen-Shannon loss against a top-K teacher (sd_gjsd_topk_*_rows, divergence
"jsd_topk"), its case tables and its measured tolerances.  TEST INFRASTRUCTURE ONLY, CPU only (never imported by the
product).

Definitions, per selected row (s [V] student logits; (v_k, i_k), k < K, the teacher's stored log-probs and indices; T the
temperature, 0 < b < 1, y the label the row predicts, N the number of valid rows):
    p_k = softmax(v / T)_k over the K entries;  P_j = sum_{k: i_k = j} p_k;  S = {j : P_j > 0};  q = softmax(s / T)
    m = (1-b) q + b P
    D  = b sum_S P_j (log P_j - log m_j) + (1-b) sum_S q_j (log q_j - log m_j) + (1 - Q_S) g0
    Q_S = sum_S q_j,  g0 = -(1-b) log(1-b)      (off S: m_j = (1-b) q_j, so (1-b)(log q_j - log m_j) = g0)
    g_j = (1-b)(log q_j - log m_j) on S, g0 off S;   c = sum_v q_v g_v = sum_S q_j g_j + (1 - Q_S) g0
    d total / d s_j = [ a (softmax(s)_j - e_y) + (1-a) T q_j (g_j - c) ] / N     on valid rows, exactly 0 elsewhere
    distill = T^2 mean D,  task = mean (lse(s) - s_y),  total = a task + (1-a) distill
    teacher = -(mean of v_k over the entries with i_k = y), n_hits their number (the sparse forward KL's monitor)
with 0 log 0 = 0.  An entry whose index is outside [0, V) or whose value is not finite carries no mass and behaves as
absent; a row without any entry left, like a row whose label is -100 or outside [0, V), is masked.

``topk_rows`` evaluates exactly these closed forms in ``acc`` (fp64: the reference; fp32: the floor measurement);
tests/test_gjsd_topk_ref_cpu.py shows that its gradient is the fp64 autograd gradient of ``topk_total_autograd`` (written
from the definition with P scattered dense, no closed form) and that D is gjsd_ref's "jsd" on a dense teacher built from P.

Tolerances follow gjsd_ref.py's method: ``measure_floors`` evaluates the closed forms in fp32 on the CPU against fp64 on
exactly the inputs of the GPU tests; the worst figures are the *_MEASURED constants below and each bound is 4 x its
measurement, rounded up to two digits.  Nothing here comes from a kernel's output.
"""
from __future__ import annotations

import functools
import math

import torch

import gjsd_ref as G
import parity_ref as P
from oracle import distill_loss as L
from parity_ref import BF, F32

# (beta, temperature) of every loss case: both T2 instantiations of the kernels run
MODES = [(0.5, 2.0), (0.1, 3.0), (0.9, 1.0)]
UNDERFLOW_MODES = [(0.5, 1.0), (0.9, 1.0)]
EDGE_V = G.GJSD_EDGE_V          # one chunk in all, one chunk per thread, exactly one prefetch trip, one chunk more
TABLE_V = P.LOSS_V              # 40 008: more than one prefetch trip per thread
ALPHA = P.LOSS_ALPHA
TABLE_K = (100, 512, 513, 1024)  # the last K of the 512-thread forward, the first of the 1024-thread one, KMAX
UNDERFLOW_V = 16392
DROP_V = 16392
SPIKE = 200.0


def mode_id(mode):
    return f"b{mode[0]:g}_T{mode[1]:g}"


# ------------------------------------------------------------------------------------------------- reference
def kept(tv, ti, V):
    """[R,K] bool: the entries that carry mass (index inside [0, V), value finite)."""
    return (ti.long() >= 0) & (ti.long() < V) & torch.isfinite(tv.float())


def scatter_P(tv, ti, V, temperature, acc=torch.float64):
    """-> P [R,V] in ``acc`` (rows without a kept entry are all zero), any_kept [R]."""
    keep = kept(tv, ti, V)
    x = torch.where(keep, tv.to(acc) / temperature, torch.full((), -math.inf, dtype=acc))
    some = keep.any(-1)
    x = torch.where(some[:, None], x, torch.zeros_like(x))   # (a row without an entry: no NaN from -inf - -inf)
    p = torch.where(keep & some[:, None], G._log_softmax(x).exp(), torch.zeros_like(x))
    Pd = torch.zeros(tv.shape[0], V, dtype=acc)
    Pd.scatter_add_(1, torch.where(keep, ti.long(), torch.zeros_like(ti.long())), p)
    return Pd, some


def divergence_terms(s, Pd, beta, temperature, acc=torch.float64):
    """-> D [R], q [R,V], g [R,V], c [R] of the definitions above, in ``acc``, from the dense P."""
    a = G._log_softmax(s.to(acc) / temperature)
    q = a.exp()
    on = Pd > 0
    one = torch.ones_like(Pd)
    lm = ((1.0 - beta) * q + beta * Pd).log()
    lP = torch.where(on, Pd, one).log()
    zero = torch.zeros_like(q)
    g0 = -(1.0 - beta) * math.log(1.0 - beta)
    klp = torch.where(on, Pd * (lP - lm), zero).sum(-1)
    klq = torch.where(on & (q > 0), q * (a - lm), zero).sum(-1)
    off = (1.0 - torch.where(on, q, zero).sum(-1)).clamp_min(0.0)
    c = (1.0 - beta) * klq + off * g0
    g = torch.where(on, (1.0 - beta) * (a - lm), torch.full_like(q, g0))
    return beta * klp + c, q, g, c


def topk_rows(s, tv, ti, labels, beta=0.5, temperature=2.0, alpha=0.5, acc=torch.float64):
    """-> ((total, task, distill, teacher) floats, N, n_hits, D [R] (0 on masked rows), grad [R,V]) in ``acc``."""
    R, V = s.shape
    Pd, some = scatter_P(tv, ti, V, temperature, acc)
    valid = (labels >= 0) & (labels < V) & some
    n = int(valid.sum())
    y = labels.clamp(0, V - 1)
    x = s.to(acc)
    ls = G._log_softmax(x)
    task = -ls.gather(-1, y[:, None]).squeeze(-1)
    D, q, g, c = divergence_terms(s, Pd, beta, temperature, acc)
    zero = torch.zeros_like(D)
    D = torch.where(valid, D, zero)
    hit = kept(tv, ti, V) & (ti.long() == labels[:, None]) & valid[:, None]
    hits = int(hit.sum())
    teacher = -float(torch.where(hit, tv.to(acc), torch.zeros((), dtype=acc)).sum()) / hits if hits else 0.0
    if n == 0:
        return (0.0, 0.0, 0.0, 0.0), 0, 0, D, torch.zeros_like(x)
    task_m = torch.where(valid, task, zero).sum() / n
    dist_m = D.sum() / n * temperature * temperature
    total = alpha * task_m + (1.0 - alpha) * dist_m
    ce = ls.exp()
    ce[torch.arange(R), y] -= 1.0
    grad = (alpha * ce + (1.0 - alpha) * temperature * G._xlog(q, g - c[:, None])) / n
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return (float(total), float(task_m), float(dist_m), teacher), n, hits, D, grad


def topk_total_autograd(s64, tv, ti, labels, beta, temperature, alpha):
    """``total`` as a differentiable fp64 scalar, written from the definition with P scattered dense and torch's own
    log_softmax / xlogy (no closed-form gradient, no collapsed off-support sum)."""
    V = s64.shape[1]
    Pd, some = scatter_P(tv, ti, V, temperature)
    valid = (labels >= 0) & (labels < V) & some
    n = int(valid.sum())
    a = torch.log_softmax(s64 / temperature, -1)
    q = a.exp()
    m = (1.0 - beta) * q + beta * Pd
    D = beta * (torch.xlogy(Pd, Pd) - Pd * m.log()).sum(-1) + (1.0 - beta) * (q * (a - m.log())).sum(-1)
    task = -torch.log_softmax(s64, -1).gather(-1, labels.clamp(0, V - 1)[:, None]).squeeze(-1)
    return (alpha * task[valid].sum() + (1.0 - alpha) * temperature ** 2 * D[valid].sum()) / n


def dense_teacher_logits(tv, ti, V, temperature):
    """fp64 logits t with softmax(t / T) = P: T log P_j on S, -inf off it (duplicates merged)."""
    Pd, _ = scatter_P(tv, ti, V, temperature)
    return temperature * torch.where(Pd > 0, Pd, torch.zeros_like(Pd)).log()


# ------------------------------------------------------------------------------------------------- inputs
def _k_for(V, K):
    return 4 if V == 8 else K


@functools.lru_cache(maxsize=None)
def table_inputs(V, dtype, K=100):
    """parity_ref's eight ROW_KINDS against the top-K of its random teacher rows -> s, tv, ti, labels (row 7 ignored)."""
    s, _ = P.loss_inputs(V, dtype)
    tv, ti = P.loss_topk(V, dtype, _k_for(V, K))
    return s, tv, ti, P.loss_labels(V, dtype)


@functools.lru_cache(maxsize=None)
def extras_inputs(V, dtype, name):
    """parity_ref.sparse_extras: "duplicates", "ends", "no_hit" at K = 100."""
    s, _ = P.loss_inputs(V, dtype)
    tv, ti, lab = P.sparse_extras(V, dtype, 100)[name]
    return s, tv, ti, lab


@functools.lru_cache(maxsize=None)
def peaked_inputs(V, dtype, K=100):
    """The spike row (one logit 60 above the rest) three times and a random row.  Row 0: a near teacher (t = s + 0.25 randn),
    the peak inside S and D small; row 1: a random teacher whose top-K leaves the peak out, all student mass off support
    (Q_S ~ 0); row 2: the near teacher with the peak's entry held TWICE (the duplicate merge on the element that carries
    the mass); row 3: a random row against its near teacher; row 4 ignored."""
    base, _ = P.loss_inputs(V, dtype)
    gen = torch.Generator().manual_seed(V * 2 + 23 + (1 if dtype == BF else 0))
    s = torch.stack([base[5], base[5], base[5], base[0], base[1]])
    peak = (V * 2) // 3
    t = (s.float() + 0.25 * torch.randn(s.shape, generator=gen)).to(dtype)
    t[1] = (torch.randn(V, generator=gen) * 3).to(dtype)
    t[1, peak] = -30.0
    tv, ti = L.extract_topk(t.float(), _k_for(V, K))
    assert bool((ti[0] == peak).any()) and not bool((ti[1] == peak).any())
    ti[2, -1] = ti[2, 0]
    tv[2, -1] = tv[2, 0]
    return s, tv, ti, torch.tensor([1, 1, 1, int(ti[3, 3]), -100], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def underflow_inputs(V, dtype, K=100):
    """T = 1.  Row 0: a student spike of 200 on a support index; row 1: on an off-support index; row 2: a teacher value
    spike (v_0 = 0, the rest <= -60 000 in fp16: p underflows everywhere else); row 3: both spikes on one index;
    row 4: ignored.  No label sits on a student spike (there the whole gradient row is ~1e-80)."""
    gen = torch.Generator().manual_seed(V * 2 + 29 + (1 if dtype == BF else 0))
    s = (torch.randn(5, V, generator=gen) * 3).to(dtype)
    t = torch.randn(5, V, generator=gen) * 3
    tv, ti = L.extract_topk(t, K)
    tv, ti = tv.clone(), ti.clone()
    cold = (-60000.0 - torch.arange(K - 1, dtype=torch.float32) * 4).to(torch.float16)
    for r in (2, 3):
        tv[r, 0] = 0.0
        tv[r, 1:] = cold
    off = P._not_in(ti[1], V)
    s[0, int(ti[0, 7])] = SPIKE
    s[1, off] = SPIKE
    s[3, int(ti[3, 0])] = SPIKE
    # (row 3's label is no hit: a hit on a -60 000 entry would make the teacher monitor a test of fp32 sums of 1e4s)
    labels = torch.tensor([int(ti[0, 2]), int(ti[1, 2]), int(ti[2, 0]), P._not_in(ti[3], V), -100], dtype=torch.int64)
    return s, tv, ti, labels


DROP = 4   # entries dropped from every row of dropped_inputs


@functools.lru_cache(maxsize=None)
def dropped_inputs(V, dtype, K=36):
    """-> (with, without): the same rows once with DROP massless entries spliced into every row -- an index of -1, of V
    and of 2^31 - 1, and a -inf value on a valid index, at positions that differ per row -- and once without them
    (K - DROP columns).  Row 6 of ``with`` has EVERY entry dropped (a mix of the four kinds); in ``without`` it is masked
    by its label instead.  Row 7 is ignored in both."""
    s, _ = P.loss_inputs(V, dtype)
    tv0, ti0 = P.loss_topk(V, dtype, K - DROP)
    labels = P.loss_labels(V, dtype).clone()
    labels[6] = int(ti0[6, 1])
    R = s.shape[0]
    tv = torch.zeros(R, K, dtype=torch.float16)
    ti = torch.zeros(R, K, dtype=torch.int32)
    bad_i = [-1, V, 2 ** 31 - 1, None]
    for r in range(R):
        pos = sorted({(r * 5) % K, (r * 5 + 7) % K, (r * 3 + 16) % K, K - 1 - r})
        assert len(pos) == DROP
        keep = [k for k in range(K) if k not in pos]
        tv[r, keep], ti[r, keep] = tv0[r], ti0[r]
        for n, k in enumerate(pos):
            if bad_i[(n + r) % 4] is None:
                tv[r, k], ti[r, k] = -math.inf, int(ti0[r, 0])   # a duplicate of a live index, without mass
            else:
                tv[r, k], ti[r, k] = -1.0 - n, bad_i[(n + r) % 4]
    for k in range(K):   # row 6: nothing left
        if k % 4 == 3:
            tv[6, k] = -math.inf
        else:
            ti[6, k] = bad_i[k % 4]
    without_labels = labels.clone()
    without_labels[6] = -100
    return (s, tv, ti, labels), (s, tv0, ti0, without_labels)


def family_cases(family):
    """[(inputs tuple, mode)] of one tolerance family, exactly what tests/test_gpu_gjsd_topk.py runs."""
    out = []
    if family == "table":
        for dt in (BF, F32):
            for m in MODES:
                out += [(table_inputs(V, dt), m) for V in (TABLE_V,) + EDGE_V]
            for K in TABLE_K[1:]:
                out += [(table_inputs(TABLE_V, dt, K), m) for m in MODES[:2]]
            for name in ("duplicates", "ends", "no_hit"):
                out += [(extras_inputs(TABLE_V, dt, name), m) for m in MODES[:2]]
            out += [(dropped_inputs(DROP_V, dt)[1], m) for m in MODES[:2]]
    elif family == "peaked":
        out = [(peaked_inputs(TABLE_V, dt), m) for dt in (BF, F32) for m in MODES]
    else:
        out = [(underflow_inputs(UNDERFLOW_V, dt), m) for dt in (BF, F32) for m in UNDERFLOW_MODES]
    return out


# ------------------------------------------------------------------------------------------------- tolerances
# Measured by measure_floors(): the closed forms in fp32 on the CPU against fp64, worst over every case of the family.
# Gradient, relative to the row maximum, per row CLASS (peaked rows, every other row); a peaked row is one whose q is all
# but one-hot: parity_ref's "spike" row (row 5 of the table sets, rows 0-2 of the peaked set) and the student-spike rows
# 0, 1, 3 of the underflow set (gjsd_ref.py says why the closed form loses digits there and only there).
PEAKED_ROWS = {"table": (5,), "peaked": (0, 1, 2), "underflow": (0, 1, 3)}
GRAD_MEASURED = {"table": (8.34e-8, 2.99e-6), "peaked": (2.81e-7, 1.05e-7), "underflow": (3.98e-8, 1.41e-7)}
GRAD_FLOOR = {"table": (3.4e-7, 1.2e-5), "peaked": (1.2e-6, 4.2e-7), "underflow": (1.6e-7, 5.7e-7)}
# Scalars, each with its own bound rtol |ref| + atol (scalar_bounds):
#   task      the cross-entropy lse(s) - s_y, pooled over the families (one formula whatever the teacher);
#   teacher   a mean of at most a few fp16 values: its fp32 evaluation, pooled likewise;
#   distill   per family, over the entries with |ref| >= SMALL; an entry below SMALL (a peaked row on a near teacher) is
#             in effect judged by atol: 4 x the worst fp32 error of those entries, never below parity_ref's 1e-6;
#   total     a x (task's bound) + (1-a) x (distill's bound) + one fp32 rounding of the total: derived.
SMALL = G.SMALL
CE_MEASURED = 1.53e-6
CE_RTOL = 6.2e-6
TEACHER_MEASURED = 0.0   # sums of a few fp16 values are exact in fp32: the bound is the atol alone
TEACHER_RTOL = 0.0
DISTILL_MEASURED = {"table": 1.48e-6, "peaked": 6.44e-7, "underflow": 2.27e-7}
DISTILL_RTOL = {"table": 6.0e-6, "peaked": 2.6e-6, "underflow": 9.1e-7}
SMALL_ABS_MEASURED = {"table": 0.0, "peaked": 9.02e-8, "underflow": 0.0}   # 4 x 9.02e-8 < 1e-6: the atol stays parity_ref's
SCALAR_ATOL = {"table": P.LOSS_SCALAR_ATOL, "peaked": P.LOSS_SCALAR_ATOL, "underflow": P.LOSS_SCALAR_ATOL}


def scalar_bounds(ref_losses, family, alpha=ALPHA):
    """-> the four absolute bounds of (total, task, distill, teacher) at the reference values, by the rules above."""
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
    the inputs of the GPU tests: every batch and every single valid row."""
    out = {}
    for fam in families:
        grad, ce, teach, dist, small = [0.0, 0.0], 0.0, 0.0, 0.0, 0.0
        for (s, tv, ti, labels), (beta, T) in family_cases(fam):
            n_rows = len(labels)
            for rows in [slice(None)] + [slice(r, r + 1) for r in range(n_rows) if labels[r] >= 0]:
                a = (s[rows], tv[rows], ti[rows], labels[rows], beta, T, ALPHA)
                l64, _, _, _, g64 = topk_rows(*a)
                l32, _, _, _, g32 = topk_rows(*a, acc=torch.float32)
                rel = (lambda i: abs(l32[i] - l64[i]) / abs(l64[i]) if l64[i] != 0.0 else 0.0)
                ce, teach = max(ce, rel(1)), max(teach, rel(3))
                if abs(l64[2]) >= SMALL:
                    dist = max(dist, rel(2))
                else:
                    small = max(small, abs(l32[2] - l64[2]))
                if rows == slice(None):
                    for r in range(n_rows):
                        if labels[r] >= 0:
                            k = 0 if r in PEAKED_ROWS[fam] else 1
                            grad[k] = max(grad[k], P._row_rel(g32[r:r + 1], g64[r:r + 1]))
        out[fam] = dict(grad=tuple(grad), ce=ce, teacher=teach, distill_rel=dist, small_abs=small)
    return out


def topk_close(got_losses, got_grad, ref_losses, ref_grad, grad_dtype, family):
    """The acceptance rule of one call on a family's whole input: four scalars (scalars_close) and the gradient per row and
    per element (parity_ref.rowwise_close with each row's floor).  -> (ok, text)."""
    s_ok, i, ratio = scalars_close(got_losses, ref_losses, family)
    v = P.rowwise_close(got_grad, ref_grad, grad_dtype, grad_floor_rows(family, ref_grad.shape[0]))
    return s_ok and v.ok, (f"scalars ok={s_ok} worst={('total', 'task', 'distill', 'teacher')[i]} err/bound={ratio:.3f}; "
                           f"grad {v}")
