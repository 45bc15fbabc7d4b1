"""fp64 reference of the reverse-KL / skewed Jensen-Shannon distillation loss (sd_gjsd_*_rows), its case tables and
its measured tolerances.  TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product).

Definitions, per selected row (s student logits, t teacher logits, T temperature, y the label the row predicts, N the
number of valid rows; q = softmax(s/T), p = softmax(t/T)):
    reverse_kl   D = KL(q || p) = sum q (log q - log p)
    jsd          m = (1-b) q + b p,   D = b KL(p || m) + (1-b) KL(q || m),   0 < b < 1
    distill = T^2 mean D,  task = mean (lse(s) - s_y),  total = a task + (1-a) distill,  teacher = mean (lse(t) - t_y)
    d total / d s_j = [ a (softmax(s)_j - e_y) + (1-a) T q_j (g_j - c) ] / N     on valid rows, exactly 0 elsewhere
        reverse_kl: g_j = log q_j - log p_j,         c = sum_v q_v g_v = KL(q || p)
        jsd:        g_j = (1-b)(log q_j - log m_j),  c = sum_v q_v g_v = (1-b) KL(q || m)
with 0 log 0 = 0: an element whose q (or p) underflows contributes 0.  A label of -100 or outside [0, V) masks a row.

``gjsd_rows`` evaluates exactly these closed forms in ``acc`` (fp64: the reference; fp32: the floor measurement, as
parity_ref.oracle_rows has it); tests/test_gjsd_ref_cpu.py shows that its gradient is the fp64 autograd gradient of its
own loss (``gjsd_total_autograd``, written from the definitions with torch's log_softmax, not from the closed form).

Tolerances follow parity_ref.py's method: ``measure_floors`` evaluates the same formulas in fp32 on the CPU against fp64
on the inputs the GPU tests use; the worst per-row figures are the *_MEASURED constants below and each bound is 4 x its
measurement, rounded up to two digits (v_exp_f32 / v_log_f32 are about an ulp looser than libm).  Nothing here comes
from a kernel's output.
"""
from __future__ import annotations

import functools

import torch

import parity_ref as P
from parity_ref import BF, F32

MODES = ("reverse_kl", "jsd")
# (divergence, beta, temperature) of every loss case; beta is ignored by reverse_kl
GJSD_MODES = [("reverse_kl", 0.5, 2.0), ("reverse_kl", 0.5, 3.0), ("jsd", 0.5, 2.0), ("jsd", 0.1, 3.0), ("jsd", 0.9, 1.0)]
UNDERFLOW_MODES = [("reverse_kl", 0.5, 1.0), ("jsd", 0.5, 1.0), ("jsd", 0.9, 1.0)]
# vocabulary edges of gjsd_*_kernel's streaming loop (512 threads per row, 4 chunks of 8 in flight per thread: row_sweep of
# csrc/sd_rows.cuh, as kd_fwd_kernel's dense variant): one chunk in all, one chunk per thread, exactly one prefetch trip, one chunk more
GJSD_EDGE_V = (8, 4096, 16384, 16392)
GJSD_V = P.LOSS_V
GJSD_ALPHA = P.LOSS_ALPHA
UNDERFLOW_V = 16392
SPIKE = 200.0


def mode_id(mode):
    return f"{mode[0]}_b{mode[1]:g}_T{mode[2]:g}" if mode[0] == "jsd" else f"{mode[0]}_T{mode[2]:g}"


# ------------------------------------------------------------------------------------------------- reference
def _log_softmax(x):
    """(x - max) - log sum exp(x - max), in that order: exact at the maximum and a small log, where x - (max + log sum)
    rounds every entry at the magnitude of lse.  The same mathematics; in fp32 it is the order the kernels use."""
    d = x - x.amax(-1, keepdim=True)
    return d - d.exp().sum(-1, keepdim=True).log()


def _xlog(w, d):
    """w * d with 0 * anything = 0 (the guarded term of a KL sum)."""
    return torch.where(w > 0, w * d, torch.zeros_like(w))


def divergence_terms(s, t, divergence, beta, temperature, acc=torch.float64):
    """-> D [R], q [R,V], g [R,V], c [R] of the definitions above, in ``acc``."""
    a = _log_softmax(s.to(acc) / temperature)
    b = _log_softmax(t.to(acc) / temperature)
    q, p = a.exp(), b.exp()
    if divergence == "reverse_kl":
        g = a - b
        D = _xlog(q, g).sum(-1)
        return D, q, g, D
    if divergence != "jsd" or not 0.0 < beta < 1.0:
        raise ValueError((divergence, beta))
    lm = ((1.0 - beta) * q + beta * p).log()
    klq, klp = _xlog(q, a - lm).sum(-1), _xlog(p, b - lm).sum(-1)
    return beta * klp + (1.0 - beta) * klq, q, (1.0 - beta) * (a - lm), (1.0 - beta) * klq


def gjsd_rows(s, t, labels, divergence, beta=0.5, temperature=2.0, alpha=0.5, acc=torch.float64):
    """-> ((total, task, distill, teacher) floats, N, D [R] (0 on masked rows), grad [R,V]) in ``acc``."""
    R, V = s.shape
    valid = (labels >= 0) & (labels < V)
    n = int(valid.sum())
    y = labels.clamp(0, V - 1)
    x, xt = s.to(acc), t.to(acc)
    ls, lt = _log_softmax(x), _log_softmax(xt)
    task = -ls.gather(-1, y[:, None]).squeeze(-1)
    teach = -lt.gather(-1, y[:, None]).squeeze(-1)
    D, q, g, c = divergence_terms(s, t, divergence, beta, temperature, acc)
    zero = torch.zeros_like(D)
    D = torch.where(valid, D, zero)
    if n == 0:
        return (0.0, 0.0, 0.0, 0.0), 0, D, torch.zeros_like(x)
    mean = (lambda v: torch.where(valid, v, zero).sum() / n)
    task_m, dist_m, teach_m = mean(task), mean(D) * temperature * temperature, mean(teach)
    total = alpha * task_m + (1.0 - alpha) * dist_m
    ce = ls.exp()
    ce[torch.arange(R), y] -= 1.0
    grad = (alpha * ce + (1.0 - alpha) * temperature * _xlog(q, g - c[:, None])) / n
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return (float(total), float(task_m), float(dist_m), float(teach_m)), n, D, grad


def gjsd_total_autograd(s64, t, labels, divergence, beta, temperature, alpha):
    """``total`` as a differentiable fp64 scalar, written from the definitions with torch's own log_softmax (no closed-form
    gradient, no guards: for inputs without underflow)."""
    V = s64.shape[1]
    valid = (labels >= 0) & (labels < V)
    n = int(valid.sum())
    a = torch.log_softmax(s64 / temperature, -1)
    b = torch.log_softmax(t.double() / temperature, -1)
    q, p = a.exp(), b.exp()
    if divergence == "reverse_kl":
        D = (q * (a - b)).sum(-1)
    else:
        lm = ((1.0 - beta) * q + beta * p).log()
        D = beta * (p * (b - lm)).sum(-1) + (1.0 - beta) * (q * (a - lm)).sum(-1)
    task = -torch.log_softmax(s64, -1).gather(-1, labels.clamp(0, V - 1)[:, None]).squeeze(-1)
    return (alpha * task[valid].sum() + (1.0 - alpha) * temperature ** 2 * D[valid].sum()) / n


# ------------------------------------------------------------------------------------------------- inputs
def table_inputs(V, dtype):
    """parity_ref's eight ROW_KINDS (student) against random teacher rows, and their labels (row 7 is ignored)."""
    s, t = P.loss_inputs(V, dtype)
    return s, t, P.loss_labels(V, dtype)


@functools.lru_cache(maxsize=None)
def near_inputs(V, dtype):
    """t = s + 0.25 randn: D is small, the regime of a half-trained student."""
    s, _ = P.loss_inputs(V, dtype)
    gen = torch.Generator().manual_seed(V * 2 + 7 + (1 if dtype == BF else 0))
    t = (s.float() + 0.25 * torch.randn(s.shape, generator=gen)).to(dtype)
    return s, t, P.loss_labels(V, dtype)


@functools.lru_cache(maxsize=None)
def underflow_inputs(V, dtype):
    """Spikes of 200 at T = 1: q (rows 0, 2, 3) or p (rows 1, 2, 3) underflows everywhere else in fp32.  Row 0: the
    student spikes; row 1: the teacher; row 2: both on one element; row 3: on different elements; row 4: ignored."""
    gen = torch.Generator().manual_seed(V * 2 + 11 + (1 if dtype == BF else 0))
    s = (torch.randn(5, V, generator=gen) * 3).to(dtype)
    t = (torch.randn(5, V, generator=gen) * 3).to(dtype)
    i, j = V // 3, (2 * V) // 3 + 1
    s[0, i] = SPIKE
    t[1, i] = SPIKE
    s[2, i] = SPIKE
    t[2, i] = SPIKE
    s[3, i] = SPIKE
    t[3, j] = SPIKE
    # no label sits on a student spike: there lse(s) - s_y and the whole gradient row are ~1e-80, nothing to compare
    return s, t, torch.tensor([5, i, 7, j, -100], dtype=torch.int64)


FAMILIES = {"table": table_inputs, "near": near_inputs, "underflow": underflow_inputs}


def family_cases(family):
    """[(V, dtype, mode)] of one family: the table at V = 40 008 and at the vocabulary edges, near at V = 40 008, underflow
    at V = 16 392 (T = 1 only)."""
    if family == "table":
        return [(V, dt, m) for V in (GJSD_V,) + GJSD_EDGE_V for dt in (BF, F32) for m in GJSD_MODES]
    if family == "near":
        return [(GJSD_V, dt, m) for dt in (BF, F32) for m in GJSD_MODES]
    return [(UNDERFLOW_V, dt, m) for dt in (BF, F32) for m in UNDERFLOW_MODES]


# ------------------------------------------------------------------------------------------------- tolerances
# Measured by measure_floors(): the closed forms in fp32 on the CPU against fp64, worst over every case of the family.
#
# Gradient, relative to the row maximum, per row CLASS: (peaked rows, every other row).  A peaked row is one whose q is
# all but one-hot -- parity_ref's "spike" row (row 5 of the table and near sets: one logit 60 above the rest) and the
# student-spike rows 0, 2, 3 of the underflow set.  There q_i (g_i - c) at the peak is a difference of two numbers that
# agree to 1 - q_i, and c = sum q g is itself a rounded fp32 sum: the closed form loses digits on such a row and only
# there (with the max-subtracted log-softmax above, too), so one floor for all rows would be fifty times too wide for the
# others.
GJSD_GRAD_MEASURED = {"table": (9.87e-5, 2.16e-6), "near": (4.54e-8, 1.78e-7), "underflow": (3.98e-8, 2.48e-6)}
GJSD_GRAD_FLOOR = {"table": (4.0e-4, 8.7e-6), "near": (1.9e-7, 7.2e-7), "underflow": (1.6e-7, 1.0e-5)}
PEAKED_ROWS = {"table": (5,), "near": (5,), "underflow": (0, 2, 3)}
# Scalars of every batch and every single row, each entry with its own bound (scalar_bounds):
#   task, teacher   rtol |ref| + atol, rtol = 4 x GJSD_CE_MEASURED: both are the cross-entropy lse(x) - x_y of a row, one
#                   formula whose error does not depend on the family, so the measurement is pooled over the families;
#   distill         rtol |ref| + atol, rtol = 4 x the family's measurement over the entries with |ref| >= SMALL.  The error
#                   of a divergence has an absolute part of about an ulp of the log-normalisers (sum q = 1 carries it into
#                   D undiminished) that does not shrink with D, so the relative error grows as D falls (near set) and
#                   an entry below SMALL (a peaked row whose teacher is near, 1e-10 .. 3e-6; two coinciding spikes,
#                   ~1e-80) is in effect judged by atol: 4 x the worst fp32 error of those entries, never below the
#                   suite's existing absolute term (1e-6, parity_ref's for a loss that is exactly 0 in the reference);
#   total           = a task + (1-a) distill, so a x (task's bound) + (1-a) x (distill's bound) + one fp32 rounding of
#                   the total: derived, not measured.
SMALL = 1e-3
GJSD_CE_MEASURED = 1.53e-6
GJSD_CE_RTOL = 6.2e-6
GJSD_DISTILL_MEASURED = {"table": 5.44e-6, "near": 2.21e-4, "underflow": 1.76e-7}
GJSD_DISTILL_RTOL = {"table": 2.2e-5, "near": 8.9e-4, "underflow": 7.1e-7}
GJSD_SMALL_ABS_MEASURED = {"table": 0.0, "near": 6.5e-7, "underflow": 1.74e-80}
GJSD_SCALAR_ATOL = {"table": P.LOSS_SCALAR_ATOL, "near": 2.6e-6, "underflow": P.LOSS_SCALAR_ATOL}


def scalar_bounds(ref_losses, family, alpha=GJSD_ALPHA):
    """-> the four absolute bounds of (total, task, distill, teacher) at the reference values, by the rules above."""
    total, task, distill, teacher = (abs(float(x)) for x in ref_losses)
    atol = GJSD_SCALAR_ATOL[family]
    b_task, b_teacher = GJSD_CE_RTOL * task + atol, GJSD_CE_RTOL * teacher + atol
    b_distill = GJSD_DISTILL_RTOL[family] * distill + atol
    return [alpha * b_task + (1.0 - alpha) * b_distill + 2.0 ** -23 * total, b_task, b_distill, b_teacher]


def scalars_close(got_losses, ref_losses, family, alpha=GJSD_ALPHA):
    """-> (ok, worst entry, its err / bound): every entry finite and within its bound."""
    ratios = []
    for g, r, b in zip(got_losses, ref_losses, scalar_bounds(ref_losses, family, alpha)):
        err = abs(float(g) - float(r))
        ratios.append(err / b if err == err and err != float("inf") else float("inf"))
    i = max(range(4), key=lambda k: ratios[k])
    return all(x <= 1.0 for x in ratios), i, ratios[i]


def grad_floor_rows(family, rows=None):
    """[R, 1] fp64 tensor of the gradient floor of each row of the family's inputs (``rows``: a subset, in order)."""
    n = len(FAMILIES[family](UNDERFLOW_V if family == "underflow" else 8, F32)[2])
    peaked, other = GJSD_GRAD_FLOOR[family]
    f = torch.full((n, 1), other, dtype=torch.float64)
    f[list(PEAKED_ROWS[family])] = peaked
    return f if rows is None else f[rows]


def measure_floors(families=("table", "near", "underflow")):
    """-> {family: dict(grad=(peaked, other), scalar_rel=(total, task, distill, teacher), small_abs=...)} of the fp32
    evaluation against fp64 on the inputs of the GPU tests."""
    out = {}
    for fam in families:
        grad, scal, small = [0.0, 0.0], [0.0] * 4, 0.0
        for V, dt, (div, beta, T) in family_cases(fam):
            s, t, labels = FAMILIES[fam](V, dt)
            for rows in [slice(None)] + [slice(r, r + 1) for r in range(len(labels)) if labels[r] >= 0]:
                l64, _, _, g64 = gjsd_rows(s[rows], t[rows], labels[rows], div, beta, T, GJSD_ALPHA)
                l32, _, _, g32 = gjsd_rows(s[rows], t[rows], labels[rows], div, beta, T, GJSD_ALPHA, acc=torch.float32)
                for i, (x, y) in enumerate(zip(l32, l64)):
                    if abs(y) >= SMALL:
                        scal[i] = max(scal[i], abs(x - y) / abs(y))
                    else:
                        small = max(small, abs(x - y))
                if rows == slice(None):
                    for r in range(len(labels)):
                        if labels[r] >= 0:
                            k = 0 if r in PEAKED_ROWS[fam] else 1
                            grad[k] = max(grad[k], P._row_rel(g32[r:r + 1], g64[r:r + 1]))
        out[fam] = dict(grad=tuple(grad), scalar_rel=tuple(scal), small_abs=small)
    return out


def gjsd_close(got_losses, got_grad, ref_losses, ref_grad, grad_dtype, family, rows=None):
    """The acceptance rule of one call: four scalars (scalars_close) and the gradient per row and per element
    (parity_ref.rowwise_close with each row's floor).  -> (ok, text)."""
    s_ok, i, ratio = scalars_close(got_losses, ref_losses, family)
    v = P.rowwise_close(got_grad, ref_grad, grad_dtype, grad_floor_rows(family, rows))
    return s_ok and v.ok, (f"scalars ok={s_ok} worst={('total', 'task', 'distill', 'teacher')[i]} err/bound={ratio:.3f}; "
                           f"grad {v}")
