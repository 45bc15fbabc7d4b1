"""-m gpu: the reverse-KL / skewed Jensen-Shannon loss kernels (sd_gjsd_fwd_rows / sd_gjsd_bwd_rows) against the fp64
reference of tests/gjsd_ref.py, per row and per element; tests/test_gjsd_ref_cpu.py shows on the CPU that the rule has
teeth and where its tolerances come from.

Shapes.  gjsd_fwd_kernel / gjsd_bwd_kernel stream a row with 512 threads and four 8-element chunks in flight per thread,
the row_sweep of csrc/sd_rows.cuh that kd_fwd_kernel's dense variant calls too, so the vocabulary edges are the same four: V = 8 (one chunk in all), 4096 (one
chunk per thread), 16 384 (exactly one prefetch trip), 16 392 (one chunk more); the case table runs at V = 40 008 (9.8
chunks per thread: several trips, a ragged last one).  Every case covers both sweeps of the forward and the backward.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gjsd_ref as G
import parity_ref as P
from gpu_util import dev, record, to_dev
from parity_ref import BF, F32

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -24
SHAPE, ALIGN, UNSUPPORTED, NO_TEACHER = -1, -2, -3, -4
MODE = {"reverse_kl": 1, "jsd": 2}


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    return ops_


def _dt_name(dt):
    return "bf16" if dt == BF else "fp32"


def _fwd_bwd(s, t, labels, mode, grad_scale=None, inplace=False):
    """DistillationLoss.forward_rows + backward -> ([total, task, distill, teacher] floats, gradient of the logits)."""
    from speech_distill_amd import DistillationLoss
    div, beta, T = mode
    leaf = to_dev(s).requires_grad_(True)
    x = leaf * 1 if inplace else leaf  # a non-leaf, so that its buffer may be overwritten
    fn = DistillationLoss(T, G.GJSD_ALPHA, inplace_grad=inplace, divergence=div, beta=beta)
    out = fn.forward_rows(x, to_dev(labels), teacher_logits=to_dev(t))
    losses = [float(v.detach()) for v in out]
    (out[0] if grad_scale is None else out[0] * grad_scale).backward()
    return losses, leaf.grad


def _out(ops, s, t, labels, mode):
    """The raw out[0..7] of the same entry (forward only)."""
    div, beta, T = mode
    with torch.no_grad():
        _, out = ops.GJSDLossRowsFn.apply(to_dev(s), to_dev(labels), to_dev(t), T, G.GJSD_ALPHA, beta, div, False)
    return [float(v) for v in out.cpu()]


@functools.lru_cache(maxsize=None)
def _ref(family, V, dtype, mode, row=None):
    s, t, labels = G.FAMILIES[family](V, dtype)
    r = slice(None) if row is None else slice(row, row + 1)
    return G.gjsd_rows(s[r], t[r], labels[r], mode[0], mode[1], mode[2], G.GJSD_ALPHA)


def _check_case(ops, family, V, dtype, mode):
    name = f"{family}_V{V}_{_dt_name(dtype)}_{G.mode_id(mode)}"
    s, t, labels = G.FAMILIES[family](V, dtype)
    ref_l, n, _, ref_g = _ref(family, V, dtype, mode)
    losses, grad = _fwd_bwd(s, t, labels, mode)
    out = _out(ops, s, t, labels, mode)
    ok, why = G.gjsd_close(losses, grad, ref_l, ref_g, dtype, family)
    v = P.rowwise_close(grad, ref_g, dtype, G.grad_floor_rows(family))
    rec = dict(losses=losses, ref=list(ref_l), scalar_err_over_bound=G.scalars_close(losses, ref_l, family)[2],
               scalar_bounds=G.scalar_bounds(ref_l, family), grad_worst_rel=v.worst_rel, grad_floor=list(G.GJSD_GRAD_FLOOR[family]),
               grad_worst=[v.row, v.col, v.got, v.ref, v.err, v.bound])
    print(name, rec)
    record("parity_gjsd_" + name, **rec)
    assert all(math.isfinite(x) for x in losses) and bool(torch.isfinite(grad).all()), name
    assert out[:4] == losses, (out, losses)
    assert out[4] == n and out[5] == n and out[6] == 0.0 and out[7] == 0.0, (out, n)  # exact
    assert ok, f"{name}: {why}"
    ignored = labels < 0
    assert float(grad[to_dev(ignored)].abs().max()) == 0.0
    # each row on its own against the reference on that row; the batch is the mean of the rows
    rows = []
    for r in torch.nonzero(~ignored).reshape(-1).tolist():
        got = _out(ops, s[r:r + 1], t[r:r + 1], labels[r:r + 1], mode)
        want = _ref(family, V, dtype, mode, r)[0]
        s_ok, i, ratio = G.scalars_close(got[:4], want, family)
        print(name, "row", r, got[:4], "err/bound", ratio)
        assert s_ok, f"{name} row {r}: got {got[:4]} want {want} (entry {i}, err / bound {ratio:.3f})"
        assert got[4] == 1.0 and got[5] == 1.0
        rows.append(got)
    rows = np.array(rows, dtype=np.float64)
    # kd_finalize_kernel<GjsdStats, false> adds at most 8 row terms in fp32 and divides: a dozen roundings of numbers no larger than the
    # sum of the rows' magnitudes (the bound of tests/test_gpu_loss_topk_optim.py)
    for j, what in enumerate(("total", "task", "distill", "teacher")):
        mean, tol = rows[:, j].mean(), 16 * ULP32 * np.abs(rows[:, j]).sum() / n
        assert abs(out[j] - mean) <= tol, f"{name}: batch {what} {out[j]} != mean of its rows {mean} (tol {tol:.2e})"


_DT = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
_MODES = pytest.mark.parametrize("mode", G.GJSD_MODES, ids=G.mode_id)


@_MODES
@_DT
def test_gjsd_rows_case_table(ops, dtype, mode):
    """Eight row kinds at V = 40 008: the four scalars per batch and per single row, N exact, the gradient per row and
    per element, the ignored row exactly 0, the batch = the mean of its rows."""
    _check_case(ops, "table", G.GJSD_V, dtype, mode)


@_MODES
@_DT
@pytest.mark.parametrize("V", G.GJSD_EDGE_V)
def test_gjsd_rows_vocabulary_edges(ops, V, dtype, mode):
    _check_case(ops, "table", V, dtype, mode)


@_MODES
@_DT
def test_gjsd_rows_near_teacher(ops, dtype, mode):
    """t = s + 0.25 randn: D ~ 1e-3, the regime of a half-trained student."""
    _check_case(ops, "near", G.GJSD_V, dtype, mode)


@pytest.mark.parametrize("mode", G.UNDERFLOW_MODES, ids=G.mode_id)
@_DT
def test_gjsd_rows_underflow(ops, dtype, mode):
    """A spike of 200 on one element of s, of t, of both: q or p underflows elsewhere at T = 1.  Finite and within
    tolerance: no NaN from 0 log 0."""
    _check_case(ops, "underflow", G.UNDERFLOW_V, dtype, mode)


# ------------------------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("mode", [G.GJSD_MODES[0], G.GJSD_MODES[3]], ids=G.mode_id)
@_DT
def test_gjsd_inplace_upstream_gradient_and_teacher_untouched(ops, dtype, mode):
    s, t, labels = G.table_inputs(G.GJSD_EDGE_V[3], dtype)
    losses, grad = _fwd_bwd(s, t, labels, mode)
    losses_i, grad_i = _fwd_bwd(s, t, labels, mode, inplace=True)
    assert losses_i == losses and torch.equal(grad_i, grad)
    # the upstream gradient scales the gradient (0.5: exact in fp32, and in bf16 short of a subnormal result)
    _, half = _fwd_bwd(s, t, labels, mode, grad_scale=0.5)
    ref_g = G.gjsd_rows(s, t, labels, mode[0], mode[1], mode[2], G.GJSD_ALPHA)[3]
    v = P.rowwise_close(half, 0.5 * ref_g, dtype, G.grad_floor_rows("table"))
    assert v.ok, v
    assert not torch.equal(half, grad)
    # the teacher buffer is read only
    from speech_distill_amd import DistillationLoss
    td = to_dev(t)
    keep = td.clone()
    x = to_dev(s).requires_grad_(True)
    DistillationLoss(mode[2], G.GJSD_ALPHA, divergence=mode[0], beta=mode[1]).forward_rows(
        x, to_dev(labels), teacher_logits=td)[0].backward()
    assert torch.equal(td, keep)


def _raw(lib, s, t, labels, stats, out, mode, beta, T, dt, grad=None, go=None, V=None, s_ptr=None):
    """The C entry points with raw pointers.  -> return code of the forward (grad None) or the backward."""
    R, Vs = s.shape
    V = Vs if V is None else V
    sp = s.data_ptr() if s_ptr is None else s_ptr
    if grad is None:
        return lib.sd_gjsd_fwd_rows(sp, t.data_ptr(), labels.data_ptr(), stats.data_ptr(), out.data_ptr(), R, V, T,
                                    G.GJSD_ALPHA, beta, mode, dt, torch.cuda.current_stream().cuda_stream)
    return lib.sd_gjsd_bwd_rows(sp, t.data_ptr(), labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                0 if go is None else go.data_ptr(), grad, R, V, T, G.GJSD_ALPHA, beta, mode, dt,
                                torch.cuda.current_stream().cuda_stream)


@_DT
def test_gjsd_backward_writes_only_its_rows(ops, dtype):
    """Guard rows of NaN in front of and behind an [R, V] gradient view stay NaN; a NULL grad_total means 1."""
    lib = ops.load_lib()
    V = G.GJSD_EDGE_V[3]
    mode = G.GJSD_MODES[2]
    s, t, labels = (to_dev(x) for x in G.table_inputs(V, dtype))
    R = s.shape[0]
    stats = torch.empty(lib.sd_gjsd_stats_bytes(R), dtype=torch.uint8, device=dev())
    out = torch.empty(8, dtype=torch.float32, device=dev())
    buf = torch.full((R + 2, V), float("nan"), dtype=dtype, device=dev())
    dt = 0 if dtype == BF else 1
    assert _raw(lib, s, t, labels, stats, out, MODE[mode[0]], mode[1], mode[2], dt) == 0
    assert _raw(lib, s, t, labels, stats, out, MODE[mode[0]], mode[1], mode[2], dt, grad=buf[1:R + 1].data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[R + 1]).all())
    _, grad = _fwd_bwd(s.cpu(), t.cpu(), labels.cpu(), mode)
    assert torch.equal(buf[1:R + 1], grad)


def test_gjsd_misuse_is_refused_before_any_launch(ops):
    """A misaligned pointer, V = 12, beta = 0 / 1 / NaN for jsd, an unknown mode or dtype, a temperature <= 0 and a NULL
    teacher each return their code; the sentinel-filled stats, scalars and gradient are unchanged."""
    lib = ops.load_lib()
    V = 16
    s = torch.randn(4, V, device=dev()).bfloat16()
    t = torch.randn(4, V, device=dev()).bfloat16()
    labels = torch.tensor([1, 2, 3, -100], device=dev())
    stats = torch.full((lib.sd_gjsd_stats_bytes(4),), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((8,), -7.0, dtype=torch.float32, device=dev())
    grad = torch.full((4, V), 3.0, dtype=torch.bfloat16, device=dev())
    keep = [x.clone() for x in (stats, out, grad, s, t)]
    nan = float("nan")
    cases = [("misaligned student", ALIGN, dict(s_ptr=s.data_ptr() + 2)),
             ("V = 12", ALIGN, dict(V=12)),
             ("jsd beta 0", SHAPE, dict(mode=2, beta=0.0)), ("jsd beta 1", SHAPE, dict(mode=2, beta=1.0)),
             ("jsd beta NaN", SHAPE, dict(mode=2, beta=nan)),
             ("unknown mode", UNSUPPORTED, dict(mode=0)), ("unknown mode 3", UNSUPPORTED, dict(mode=3)),
             ("unknown dtype", UNSUPPORTED, dict(dt=2)),
             ("temperature 0", SHAPE, dict(T=0.0)), ("temperature NaN", SHAPE, dict(T=nan))]
    for what, code, kw in cases:
        a = dict(mode=1, beta=0.5, T=2.0, dt=0)
        a.update({k: v for k, v in kw.items() if k in a})
        extra = {k: v for k, v in kw.items() if k not in a}
        assert _raw(lib, s, t, labels, stats, out, a["mode"], a["beta"], a["T"], a["dt"], **extra) == code, what
        assert _raw(lib, s, t, labels, stats, out, a["mode"], a["beta"], a["T"], a["dt"], grad=grad.data_ptr(), **extra) == code, what
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sd_gjsd_fwd_rows(s.data_ptr(), None, labels.data_ptr(), stats.data_ptr(), out.data_ptr(), 4, V, 2.0, 0.3, 0.5,
                                1, 0, stream) == NO_TEACHER
    assert _raw(lib, s, t, labels, stats, out, 1, 0.5, 2.0, 0, grad=grad.data_ptr() + 2) == ALIGN   # misaligned gradient
    assert lib.sd_gjsd_fwd_rows(s.data_ptr(), t.data_ptr() + 2, labels.data_ptr(), stats.data_ptr(), out.data_ptr(), 4, V,
                                2.0, 0.3, 0.5, 1, 0, stream) == ALIGN
    torch.cuda.synchronize()
    for now, before in zip((stats, out, grad, s, t), keep):
        assert torch.equal(now, before)
    # reverse_kl ignores beta: 0 is fine there
    assert _raw(lib, s, t, labels, stats, out, 1, 0.0, 2.0, 0) == 0
    torch.cuda.synchronize()
    assert float(out[4]) == 3.0


def test_gjsd_no_valid_row_gives_zeros(ops):
    s = torch.randn(3, 4096, device=dev()).bfloat16().requires_grad_(True)
    t = torch.randn(3, 4096, device=dev()).bfloat16()
    from speech_distill_amd import DistillationLoss
    out = DistillationLoss(2.0, 0.3, divergence="jsd", beta=0.5).forward_rows(
        s, torch.tensor([-100, 4096, -1], device=dev()), teacher_logits=t)
    assert [float(x.detach()) for x in out] == [0.0, 0.0, 0.0, 0.0]
    out[0].backward()
    assert float(s.grad.abs().max()) == 0.0


@pytest.mark.parametrize("divergence", ["reverse_kl", "jsd"])
def test_gjsd_batch_without_a_loss_row_gives_connected_zeros(ops, divergence):
    """N == 0 on the [B,T,V] form (what the trainer sends such a batch through) and R == 0 on the rows form: four zeros,
    connected to autograd, a zero gradient, nothing launched on zero rows."""
    from speech_distill_amd import DistillationLoss
    B, Tn, V = 2, 5, 4096
    fn = DistillationLoss(2.0, 0.3, divergence=divergence, beta=0.5)
    t = to_dev(torch.randn(B, Tn, V).bfloat16())
    for inplace in (False, True):
        fn.inplace_grad = inplace
        x = to_dev(torch.randn(B, Tn, V).bfloat16()).requires_grad_(True)
        out = fn(x * 1, torch.full((B, Tn), -100, device=dev()), teacher_logits=t)
        assert [float(v.detach()) for v in out] == [0.0, 0.0, 0.0, 0.0] and out[0].requires_grad
        out[0].backward()
        assert x.grad is not None and x.grad.shape == x.shape and float(x.grad.abs().max()) == 0.0
        y = torch.empty(0, V, dtype=torch.bfloat16, device=dev()).requires_grad_(True)
        part = fn.forward_rows(y * 1, torch.empty(0, dtype=torch.int64, device=dev()),
                               teacher_logits=torch.empty(0, V, dtype=torch.bfloat16, device=dev()))
        assert [float(v.detach()) for v in part] == [0.0, 0.0, 0.0, 0.0] and part[0].requires_grad
        part[0].backward()
        assert y.grad.shape == (0, V)


# ------------------------------------------------------------------------------------------------- cross-checks
@_DT
@pytest.mark.parametrize("T", [2.0, 3.0])
def test_reverse_kl_equals_the_forward_kl_kernel_with_the_roles_swapped(ops, T, dtype):
    """No reference: KL(q || p) by sd_gjsd_fwd_rows against the existing dense sd_kdloss_fwd_rows with the teacher as
    student and the student as teacher.  Bound: the sum of the two kernels' scalar tolerances."""
    s, t, labels = (to_dev(x) for x in G.table_inputs(G.GJSD_V, dtype))
    with torch.no_grad():
        _, ours = ops.GJSDLossRowsFn.apply(s, labels, t, T, G.GJSD_ALPHA, 0.5, "reverse_kl", False)
        _, theirs = ops.KDLossRowsFn.apply(t, labels, s, None, None, T, G.GJSD_ALPHA, False)
    a, b = float(ours[2]), float(theirs[2])
    bound = (G.GJSD_DISTILL_RTOL["table"] + P.LOSS_SCALAR_RTOL["dense"]) * abs(b) + G.GJSD_SCALAR_ATOL["table"] + P.LOSS_SCALAR_ATOL
    print("reverse vs swapped forward", a, b, abs(a - b), bound)
    assert abs(a - b) <= bound, (a, b, bound)
    # our task loss is its teacher monitor and vice versa: the same sums over the same rows
    ce = G.GJSD_CE_RTOL + P.LOSS_SCALAR_RTOL["dense"]
    assert abs(float(ours[1]) - float(theirs[3])) <= ce * abs(float(ours[1]))
    assert abs(float(ours[3]) - float(theirs[1])) <= ce * abs(float(ours[3]))


@pytest.mark.parametrize("mode", [G.GJSD_MODES[0], G.GJSD_MODES[2]], ids=G.mode_id)
@pytest.mark.parametrize("with_mask", [False, True], ids=["labels", "speech_mask"])
def test_forward_on_btv_equals_forward_rows_on_the_selected_rows(ops, mode, with_mask):
    from speech_distill_amd import DistillationLoss
    div, beta, T = mode
    B, Tn, V = 3, 9, 4096
    g = torch.Generator().manual_seed(5)
    s = (torch.randn(B, Tn, V, generator=g) * 3).bfloat16()
    t = (torch.randn(B, Tn, V, generator=g) * 3).bfloat16()
    labels = torch.randint(0, V, (B, Tn), generator=g)
    labels[0, :4] = -100
    labels[2, 6:] = -100
    mask = None
    if with_mask:
        mask = torch.ones(B, Tn, dtype=torch.int64)
        mask[1, :5] = 0
    fn = DistillationLoss(T, 0.4, divergence=div, beta=beta)
    x = to_dev(s).requires_grad_(True)
    full = fn(x, to_dev(labels), teacher_logits=to_dev(t), speech_token_mask=None if mask is None else to_dev(mask))
    full[0].backward()
    rows, row_labels = ops.loss_rows(to_dev(labels), None if mask is None else to_dev(mask))
    assert 0 < rows.numel() < B * (Tn - 1)
    y = to_dev(s).reshape(-1, V)[rows].requires_grad_(True)
    part = fn.forward_rows(y, row_labels, teacher_logits=to_dev(t).reshape(-1, V)[rows])
    part[0].backward()
    assert [float(v.detach()) for v in full] == [float(v.detach()) for v in part]
    scattered = torch.zeros(B * Tn, V, dtype=torch.bfloat16, device=dev())
    scattered[rows] = y.grad
    assert torch.equal(x.grad.reshape(-1, V), scattered)
    with pytest.raises(ValueError, match="dense teacher"):
        fn(x, to_dev(labels), teacher_top_k_v=torch.zeros(B, Tn, 4), teacher_top_k_i=torch.zeros(B, Tn, 4, dtype=torch.int64))
