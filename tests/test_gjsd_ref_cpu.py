"""The tools of tests/test_gpu_gjsd.py (tests/gjsd_ref.py), on the CPU: the reference's closed-form gradient is the fp64
autograd gradient of its own loss; the acceptance rule accepts the rounded reference and rejects each named wrong formula at
the inputs the GPU tests use; the recorded tolerances are what the fp32 evaluation measures; and three properties that tie
the reference to mathematics it does not restate (symmetry, the entropy bound, the project's own forward-KL oracle)."""
import math

import pytest
import torch

import gjsd_ref as G
import parity_ref as P
from parity_ref import BF, F32

V_SMALL = 16392  # the largest vocabulary edge: two prefetch trips of the kernel, quick in fp64 on the CPU


def _ids(m):
    return G.mode_id(m)


@pytest.mark.parametrize("mode", G.GJSD_MODES, ids=_ids)
@pytest.mark.parametrize("V", [8, V_SMALL, G.GJSD_V])
def test_reference_gradient_is_the_autograd_gradient_of_its_loss(V, mode):
    div, beta, T = mode
    for dt in (BF, F32):
        s, t, labels = G.table_inputs(V, dt)
        losses, n, D, grad = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA)
        x = s.double().requires_grad_(True)
        total = G.gjsd_total_autograd(x, t, labels, div, beta, T, G.GJSD_ALPHA)
        total.backward()
        assert n == 7 and abs(float(total.detach()) - losses[0]) <= 1e-12 * abs(losses[0])
        err = (grad - x.grad).abs().amax(-1) / x.grad.abs().amax(-1).clamp_min(1e-300)
        assert float(err[:7].max()) <= 1e-12, err
        assert float(grad[7].abs().max()) == 0.0 and float(D[7]) == 0.0
        # total = a task + (1 - a) distill
        assert abs(losses[0] - (G.GJSD_ALPHA * losses[1] + (1 - G.GJSD_ALPHA) * losses[2])) <= 1e-12 * abs(losses[0])


def test_masked_rows_and_the_empty_batch():
    s, t, labels = G.table_inputs(8, F32)
    lab = labels.clone()
    lab[0], lab[1] = 8, -5  # outside [0, V): masked like -100
    losses, n, D, grad = G.gjsd_rows(s, t, lab, "jsd", 0.5, 2.0, 0.3)
    assert n == 5 and float(grad[[0, 1, 7]].abs().max()) == 0.0 and float(D[[0, 1, 7]].abs().max()) == 0.0
    ref = G.gjsd_rows(s[2:7], t[2:7], labels[2:7], "jsd", 0.5, 2.0, 0.3)
    assert losses == pytest.approx(ref[0], rel=1e-14) and torch.equal(grad[2:7], ref[3])
    losses, n, D, grad = G.gjsd_rows(s, t, torch.full_like(labels, -100), "reverse_kl", 0.5, 2.0, 0.3)
    assert losses == (0.0, 0.0, 0.0, 0.0) and n == 0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- the rule
def _variant(mut, s, t, labels, div, beta, T, alpha):
    """gjsd_rows' gradient and distill with one named mistake (None: no mistake)."""
    R, V = s.shape
    valid = (labels >= 0) & (labels < V)
    n = int(valid.sum())
    D, q, g, c = G.divergence_terms(s, t, div, 1.0 - beta if mut == "beta_swapped" else beta, T)
    if mut == "g_factor_dropped":
        g, c = g / (1.0 - beta), c / (1.0 - beta)
    if mut == "c_omitted":
        c = torch.zeros_like(c)
    term = q * (g - c[:, None])
    if mut == "forward_for_reverse":  # the forward KL's loss and gradient, T (q - p), oracle/distill_loss.py
        p = torch.softmax(t.double() / T, -1)
        term = q - p
        D = (p * (p.log() - q.log())).sum(-1)
    ce = torch.softmax(s.double(), -1)
    ce[torch.arange(R), labels.clamp(0, V - 1)] -= 1.0
    grad = (alpha * ce + (1.0 - alpha) * (1.0 if mut == "T_dropped" else T) * term) / n
    return torch.where(valid[:, None], grad, torch.zeros_like(grad)), float(D[valid].sum() / n * T * T)


# name -> where the mistake changes anything.  A mutant that is (nearly) the right formula somewhere is not asked for there:
# beta = 1/2 swaps to itself, T = 1 has no factor to drop, and on the near set c = O(D) ~ 1e-3 of g, so omitting it moves
# the gradient by less than the rounding of the stored type.
MUTANTS = {"beta_swapped": lambda fam, d, b, T: d == "jsd" and b != 0.5,
           "g_factor_dropped": lambda fam, d, b, T: d == "jsd",
           "T_dropped": lambda fam, d, b, T: T != 1.0,
           "c_omitted": lambda fam, d, b, T: fam == "table",
           "forward_for_reverse": lambda fam, d, b, T: d == "reverse_kl"}


@pytest.mark.parametrize("mode", G.GJSD_MODES, ids=_ids)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_rule_accepts_the_rounded_reference_and_rejects_each_wrong_formula(dtype, mode):
    div, beta, T = mode
    for fam, V in (("table", V_SMALL), ("near", G.GJSD_V)):
        s, t, labels = G.FAMILIES[fam](V, dtype)
        losses, n, _, grad = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA)
        exact, d_exact = _variant(None, s, t, labels, div, beta, T, G.GJSD_ALPHA)
        assert float((exact - grad).abs().max()) <= 1e-13 * float(grad.abs().max())
        assert abs(d_exact - losses[2]) <= 1e-12 * abs(losses[2])
        rounded = [float(torch.tensor(x, dtype=torch.float32)) for x in losses]
        ok, why = G.gjsd_close(rounded, grad.to(dtype), losses, grad, dtype, fam)
        assert ok, why
        for mut, applies in MUTANTS.items():
            if not applies(fam, div, beta, T):
                continue
            bad, d_bad = _variant(mut, s, t, labels, div, beta, T, G.GJSD_ALPHA)
            v = P.rowwise_close(bad.to(dtype), grad, dtype, G.grad_floor_rows(fam))
            assert not v.ok, (fam, mut, v)
            # the two that change the loss itself; on the near set all divergences agree to second order in t - s, so
            # there only the gradient (first order) tells them apart
            if mut in ("beta_swapped", "forward_for_reverse") and fam == "table":
                wrong = [losses[0] + (1 - G.GJSD_ALPHA) * (d_bad - losses[2]), losses[1], d_bad, losses[3]]
                assert not G.gjsd_close(wrong, grad, losses, grad, F32, fam)[0], (fam, mut)


def test_recorded_tolerances_are_what_the_fp32_evaluation_measures():
    """Each bound is 4 x its recorded measurement, and the measurement reproduces (25 % slack for another libm)."""
    m = G.measure_floors()
    for fam in G.FAMILIES:
        pairs = list(zip(m[fam]["grad"], G.GJSD_GRAD_MEASURED[fam], G.GJSD_GRAD_FLOOR[fam]))
        pairs.append((m[fam]["scalar_rel"][2], G.GJSD_DISTILL_MEASURED[fam], G.GJSD_DISTILL_RTOL[fam]))
        for now, measured, floor in pairs:
            assert 0 < now <= 1.25 * measured, (fam, now, measured)
            assert 4 * measured <= floor * (1 + 1e-9) and floor <= 4.4 * measured, (fam, measured, floor)  # two digits, rounded up
        small, atol = G.GJSD_SMALL_ABS_MEASURED[fam], G.GJSD_SCALAR_ATOL[fam]
        assert m[fam]["small_abs"] <= 1.25 * small or small == 0.0 == m[fam]["small_abs"], (fam, m[fam]["small_abs"])
        assert atol >= P.LOSS_SCALAR_ATOL and 4 * small <= atol * (1 + 1e-9) and atol <= max(4.4 * small, P.LOSS_SCALAR_ATOL)
    # orientation: the ordinary rows stay near the figures of the forward-KL kernels' floors
    # task and teacher: one formula (a row's cross-entropy), one measurement pooled over the families and both entries
    ce = max(max(m[fam]["scalar_rel"][1], m[fam]["scalar_rel"][3]) for fam in G.FAMILIES)
    assert 0 < ce <= 1.25 * G.GJSD_CE_MEASURED and 4 * G.GJSD_CE_MEASURED <= G.GJSD_CE_RTOL * (1 + 1e-9) <= 4.4 * G.GJSD_CE_MEASURED
    # the total's bound is derived from its parts: the fp32 evaluation itself stays inside a quarter of it
    for fam in G.FAMILIES:
        for V, dt, (div, beta, T) in G.family_cases(fam):
            s, t, labels = G.FAMILIES[fam](V, dt)
            l64 = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA)[0]
            l32 = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA, acc=torch.float32)[0]
            assert abs(l32[0] - l64[0]) <= 0.25 * G.scalar_bounds(l64, fam)[0], (fam, V, div)
    # orientation: the ordinary rows stay near the figures of the forward-KL kernels' floors
    assert G.GJSD_GRAD_FLOOR["table"][1] <= 2e-5 and G.GJSD_DISTILL_RTOL["table"] <= 3e-5 and G.GJSD_CE_RTOL <= 2e-5


def test_underflow_rows_are_finite_in_fp32_and_close_to_fp64():
    """0 log 0 = 0: with a spike of 200 at T = 1, q or p underflows everywhere else in fp32; the guarded closed form stays
    finite and passes its own rule."""
    for V, dt, (div, beta, T) in G.family_cases("underflow"):
        s, t, labels = G.underflow_inputs(V, dt)
        assert float(torch.softmax(s[0].float(), -1).min()) == 0.0 and float(torch.softmax(t[1].float(), -1).min()) == 0.0
        l64, n, D, g64 = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA)
        l32, _, _, g32 = G.gjsd_rows(s, t, labels, div, beta, T, G.GJSD_ALPHA, acc=torch.float32)
        assert n == 4 and all(math.isfinite(x) for x in l32) and bool(torch.isfinite(g32).all())
        ok, why = G.gjsd_close(l32, g32, l64, g64, F32, "underflow")
        assert ok, why


# ------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("T", [1.0, 2.0, 3.0])
def test_jsd_at_half_is_symmetric_and_bounded_by_the_mixing_entropy(T):
    for fam, V in (("table", V_SMALL), ("underflow", G.UNDERFLOW_V)):
        s, t, _ = G.FAMILIES[fam](V, F32)
        a = G.divergence_terms(s, t, "jsd", 0.5, T)[0]
        b = G.divergence_terms(t, s, "jsd", 0.5, T)[0]
        assert float((a - b).abs().max()) <= 1e-13
        for beta in (0.1, 0.5, 0.9):
            D = G.divergence_terms(s, t, "jsd", beta, T)[0]
            H = -beta * math.log(beta) - (1 - beta) * math.log(1 - beta)   # <= ln 2, reached by disjoint supports
            assert float(D.min()) >= 0.0 and float(D.max()) <= H * (1 + 1e-12) <= math.log(2) * (1 + 1e-12)
            labels = torch.zeros(len(s), dtype=torch.int64)
            distill = G.gjsd_rows(s, t, labels, "jsd", beta, T, 0.3)[0][2]
            assert distill <= T * T * math.log(2)
    s, t, _ = G.underflow_inputs(G.UNDERFLOW_V, F32)   # row 3: the spikes sit on different elements -> the bound is reached
    assert abs(float(G.divergence_terms(s[3:4], t[3:4], "jsd", 0.5, 1.0)[0]) - math.log(2)) <= 1e-12


@pytest.mark.parametrize("T", [2.0, 3.0])
def test_reverse_kl_is_the_oracles_forward_kl_with_the_roles_swapped(T):
    for dt in (BF, F32):
        s, t, labels = G.table_inputs(V_SMALL, dt)
        ours = G.gjsd_rows(s, t, labels, "reverse_kl", 0.5, T, 0.3)[0]
        swapped = P.oracle_rows(t, labels, teacher=s, temperature=T, alpha=0.3)[0]
        assert abs(ours[2] - swapped[2]) <= 1e-10 * abs(swapped[2])
        assert abs(ours[1] - swapped[3]) <= 1e-12 * abs(ours[1])  # our task loss is its teacher monitor, and vice versa
        assert abs(ours[3] - swapped[1]) <= 1e-12 * abs(ours[3])
