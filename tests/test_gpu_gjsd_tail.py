"""-m gpu: forward KL, reverse KL and the skewed JSD against a top-K teacher with a tail bucket (sd_gjsd_tail_fwd_rows /
sd_gjsd_tail_bwd_rows, divergences "forward_kl_tail", "reverse_kl_tail", "jsd_tail") against the fp64 reference of
tests/gjsd_tail_ref.py, per row and per element; tests/test_gjsd_tail_ref_cpu.py shows on the CPU where the reference and
its tolerances come from.

Shapes.  gjsd_tail_fwd_kernel streams a row with 512 threads (1024 when K > 512) and four 8-element chunks in flight per
thread, gjsd_tail_bwd_kernel with 512: the vocabulary edges are gjsd_ref's four (V = 8, 4096, 16 384, 16 392), the case
table runs at V = 40 008 (several prefetch trips, a ragged last one), K at 100, 512, 513 and 1024.
"""
import math

import numpy as np
import pytest
import torch

import gjsd_tail_ref as R
import gjsd_topk_ref as K
import parity_ref as P
from gpu_util import dev, record, to_dev
from parity_ref import BF, F32

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -24
SHAPE, ALIGN, UNSUPPORTED, NO_TEACHER = -1, -2, -3, -4


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    return ops_


def _dt_name(dt):
    return "bf16" if dt == BF else "fp32"


def _fwd_bwd(inputs, div, mode, grad_scale=None, inplace=False):
    """DistillationLoss.forward_rows + backward -> ([total, task, distill, teacher] floats, gradient of the logits)."""
    from speech_distill_amd import DistillationLoss
    s, tv, ti, tau, labels = inputs
    beta, T = mode
    leaf = to_dev(s).requires_grad_(True)
    x = leaf * 1 if inplace else leaf  # a non-leaf, so that its buffer may be overwritten
    fn = DistillationLoss(T, R.ALPHA, inplace_grad=inplace, divergence=div, beta=beta)
    out = fn.forward_rows(x, to_dev(labels), teacher_top_k_v=to_dev(tv), teacher_top_k_i=to_dev(ti),
                          teacher_top_k_tail=to_dev(tau))
    losses = [float(v.detach()) for v in out]
    (out[0] if grad_scale is None else out[0] * grad_scale).backward()
    return losses, leaf.grad


def _out(ops, inputs, div, mode, rows=slice(None)):
    """The raw out[0..7] of the same entry (forward only) on a subset of the rows."""
    s, tv, ti, tau, labels = (x[rows] for x in inputs)
    with torch.no_grad():
        _, out = ops.GJSDTailLossRowsFn.apply(to_dev(s), to_dev(labels), to_dev(tv), to_dev(ti), to_dev(tau), mode[1], R.ALPHA,
                                              mode[0], div, False)
    return [float(v) for v in out.cpu()]


def _ref(inputs, div, mode, row=None):
    r = slice(None) if row is None else slice(row, row + 1)
    s, tv, ti, tau, labels = (x[r] for x in inputs)
    return R.tail_rows(s, tv, ti, tau, labels, div, mode[0], mode[1], R.ALPHA)


def _check_case(ops, name, family, inputs, dtype, div, mode, ref_inputs=None, single_rows=True):
    """The batch: four scalars, N and n_hits exact, the gradient per row and per element, masked rows exactly zero; then
    each row on its own against the reference on that row (bit for bit the row's share of the batch is checked in
    test_tail_bit_contracts), and the batch against the mean of its rows.  ``ref_inputs``: the inputs the reference is
    evaluated on (the dropped-entry cases: the same rows with those entries removed)."""
    name = f"{name}_{_dt_name(dtype)}_{R.case_id(div, mode)}"
    labels = inputs[4]
    ref_in = inputs if ref_inputs is None else ref_inputs
    ref_l, n, hits, _, ref_g = _ref(ref_in, div, mode)
    losses, grad = _fwd_bwd(inputs, div, mode)
    out = _out(ops, inputs, div, mode)
    ok, why = R.tail_close(losses, grad, ref_l, ref_g, dtype, family)
    v = P.rowwise_close(grad, ref_g, dtype, R.grad_floor_rows(family, len(labels)))
    rec = dict(losses=losses, ref=list(ref_l), scalar_err_over_bound=R.scalars_close(losses, ref_l, family)[2],
               scalar_bounds=R.scalar_bounds(ref_l, family), grad_worst_rel=v.worst_rel, grad_floor=list(R.GRAD_FLOOR[family]),
               grad_worst=[v.row, v.col, v.got, v.ref, v.err, v.bound])
    print(name, rec)
    record("parity_gjsd_tail_" + name, **rec)
    assert all(math.isfinite(x) for x in losses) and bool(torch.isfinite(grad).all()), name
    assert out[:4] == losses, (out, losses)
    assert out[4] == n and out[5] == hits and out[6] == 0.0 and out[7] == 0.0, (out, n, hits)  # exact
    assert ok, f"{name}: {why}"
    masked = ref_g.abs().amax(-1) == 0
    assert bool(masked[labels < 0].all())
    if bool(masked.any()):
        assert float(grad[to_dev(masked)].abs().max()) == 0.0
    if not single_rows:
        return
    rows = []
    for r in torch.nonzero(~masked).reshape(-1).tolist():
        got = _out(ops, inputs, div, mode, slice(r, r + 1))
        want = _ref(ref_in, div, mode, r)
        s_ok, i, ratio = R.scalars_close(got[:4], want[0], family)
        print(name, "row", r, got[:4], "err/bound", ratio)
        assert s_ok, f"{name} row {r}: got {got[:4]} want {want[0]} (entry {i}, err / bound {ratio:.3f})"
        assert got[4] == 1.0 and got[5] == want[2]
        rows.append(got)
    rows = np.array(rows, dtype=np.float64)
    # kd_finalize_kernel adds at most 8 row terms in fp32 and divides: a dozen roundings of numbers no larger than the sum
    # of the rows' magnitudes (the bound of tests/test_gpu_gjsd.py)
    for j, what in enumerate(("total", "task", "distill")):
        mean, tol = rows[:, j].mean(), 16 * ULP32 * np.abs(rows[:, j]).sum() / n
        assert abs(out[j] - mean) <= tol, f"{name}: batch {what} {out[j]} != mean of its rows {mean} (tol {tol:.2e})"


_DIV = pytest.mark.parametrize("div", R.DIVERGENCES)
_DT = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
_MODES = pytest.mark.parametrize("mode", R.MODES, ids=K.mode_id)
_MODES2 = pytest.mark.parametrize("mode", R.MODES[:2], ids=K.mode_id)


@_DIV
@_MODES
@_DT
@pytest.mark.parametrize("V", (R.TABLE_V,) + R.EDGE_V)
def test_tail_rows_case_table_and_vocabulary_edges(ops, V, dtype, mode, div):
    """parity_ref's eight row kinds at V = 40 008 and at the streaming edges (K = 100; K = 4 at V = 8), each row with the
    true tail of the teacher row its top-K came from."""
    _check_case(ops, f"table_V{V}", "table", R.table_inputs(V, dtype, mode[1]), dtype, div, mode)


@_DIV
@_MODES2
@_DT
@pytest.mark.parametrize("Kk", R.TABLE_K[1:])
def test_tail_rows_k_edges(ops, Kk, dtype, mode, div):
    """K = 512 (the last of the 512-thread forward), 513 (the first of the 1024-thread one), 1024 (KMAX)."""
    _check_case(ops, f"table_K{Kk}", "table", R.table_inputs(R.TABLE_V, dtype, mode[1], Kk), dtype, div, mode, single_rows=False)


@_DIV
@_MODES2
@_DT
@pytest.mark.parametrize("extra", ["duplicates", "ends", "no_hit"])
def test_tail_rows_sparse_extras(ops, extra, dtype, mode, div):
    """Duplicated indices sum their mass (and the label held three times counts three hits), the label at both ends of
    the top-K, no hit at all."""
    _check_case(ops, extra, "table", R.extras_inputs(R.TABLE_V, dtype, mode[1], extra), dtype, div, mode, single_rows=False)


@_DIV
@_MODES
@_DT
def test_tail_rows_peaked(ops, dtype, mode, div):
    """The spike row against a near teacher, against a teacher that leaves the peak out (all student mass in bucket 0) and
    with the peak's entry duplicated; tails 0.5, 1e-3, 1e-7, 1e-12."""
    _check_case(ops, "peaked", "peaked", R.peaked_inputs(R.TABLE_V, dtype), dtype, div, mode)


@_DIV
@pytest.mark.parametrize("mode", R.UNDERFLOW_MODES, ids=K.mode_id)
@_DT
def test_tail_rows_underflow(ops, dtype, mode, div):
    """A student spike of 200 on a support index (q_0 ~ 1e-80: only log q_0 exists in fp32), on an off-support index, and a
    teacher whose mass underflows everywhere but on one entry, at T = 1: finite and within tolerance."""
    _check_case(ops, "underflow", "underflow", R.underflow_inputs(R.UNDERFLOW_V, dtype), dtype, div, mode)


@_DIV
@_MODES2
@_DT
def test_tail_dropped_entries_behave_as_absent(ops, dtype, mode, div):
    """Indices of -1, V and 2^31 - 1 and a -inf value, spliced into every row: the results are those of the rows without
    these entries, and the row with every entry dropped is a masked row: not counted, gradient exactly zero."""
    with_, without = R.dropped_inputs(R.DROP_V, dtype, mode[1])
    _check_case(ops, "dropped", "table", with_, dtype, div, mode, ref_inputs=without, single_rows=False)
    _check_case(ops, "dropped_removed", "table", without, dtype, div, mode, single_rows=False)
    l_w, g_w = _fwd_bwd(with_, div, mode)
    assert float(g_w[6].abs().max()) == 0.0 and float(g_w[7].abs().max()) == 0.0
    assert _out(ops, with_, div, mode, slice(6, 7)) == [0.0] * 8


@_DIV
@_MODES2
@_DT
def test_tail_bad_tails_mask_their_rows(ops, dtype, mode, div):
    """tau = NaN, -0.1 and 1.0 mask their rows (stats zero, gradient exactly zero, not in N); tau = 0.0 counts as 2^-100,
    bit for bit."""
    inputs = R.bad_tail_inputs(R.DROP_V, dtype, mode[1])
    _check_case(ops, "bad_tails", "table", inputs, dtype, div, mode, single_rows=False)
    losses, grad = _fwd_bwd(inputs, div, mode)
    assert float(grad[:3].abs().max()) == 0.0 and float(grad[3].abs().max()) > 0.0
    for r in range(3):
        assert _out(ops, inputs, div, mode, slice(r, r + 1)) == [0.0] * 8
    s, tv, ti, tau, labels = inputs
    tiny = tau.clone()
    tiny[3] = R.TAIL_MIN
    losses_t, grad_t = _fwd_bwd((s, tv, ti, tiny, labels), div, mode)
    assert losses_t == losses and torch.equal(grad_t, grad)


# ------------------------------------------------------------------------------------------------- memory
def _raw(lib, s, tv, ti, tau, labels, stats, out, beta, T, mode, dt, grad=None, go=None, V=None, Kk=None, s_ptr=None,
         tv_ptr="own", ti_ptr="own", tau_ptr="own"):
    """The C entry points with raw pointers.  -> return code of the forward (grad None) or the backward."""
    Rn, Vs = s.shape
    V = Vs if V is None else V
    Kk = tv.shape[1] if Kk is None else Kk
    sp = s.data_ptr() if s_ptr is None else s_ptr
    tvp = tv.data_ptr() if tv_ptr == "own" else tv_ptr
    tip = ti.data_ptr() if ti_ptr == "own" else ti_ptr
    tap = tau.data_ptr() if tau_ptr == "own" else tau_ptr
    stream = torch.cuda.current_stream().cuda_stream
    if grad is None:
        return lib.sd_gjsd_tail_fwd_rows(sp, tvp, tip, tap, labels.data_ptr(), stats.data_ptr(), out.data_ptr(), Rn, V, Kk, T,
                                         R.ALPHA, beta, mode, dt, stream)
    return lib.sd_gjsd_tail_bwd_rows(sp, tvp, tip, tap, labels.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                     0 if go is None else go.data_ptr(), grad, Rn, V, Kk, T, R.ALPHA, beta, mode, dt, stream)


@_DIV
@pytest.mark.parametrize("which", ["table", "dropped"])
@_DT
def test_tail_backward_writes_only_its_rows(ops, dtype, which, div):
    """Guard rows of NaN in front of and behind a sentinel-filled [R, V] gradient view stay NaN (also with out-of-range
    indices among the entries), masked rows are exactly zero, every element is written; a NULL grad_total means 1."""
    lib = ops.load_lib()
    V = R.DROP_V
    mode = R.MODES[0]
    md = R.DIVERGENCES.index(div)
    inputs = R.table_inputs(V, dtype, mode[1]) if which == "table" else R.dropped_inputs(V, dtype, mode[1])[0]
    s, tv, ti, tau, labels = (to_dev(x) for x in inputs)
    Rn = s.shape[0]
    stats = torch.empty(lib.sd_gjsd_tail_stats_bytes(Rn), dtype=torch.uint8, device=dev())
    out = torch.empty(8, dtype=torch.float32, device=dev())
    buf = torch.full((Rn + 2, V), float("nan"), dtype=dtype, device=dev())
    dt = 0 if dtype == BF else 1
    assert _raw(lib, s, tv, ti, tau, labels, stats, out, mode[0], mode[1], md, dt) == 0
    assert _raw(lib, s, tv, ti, tau, labels, stats, out, mode[0], mode[1], md, dt, grad=buf[1:Rn + 1].data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[Rn + 1]).all())
    assert bool(torch.isfinite(buf[1:Rn + 1]).all())
    assert float(buf[Rn].abs().max()) == 0.0   # row 7: ignored
    _, grad = _fwd_bwd(inputs, div, mode)
    assert torch.equal(buf[1:Rn + 1], grad)


@_DIV
@_MODES2
@_DT
def test_tail_bit_contracts(ops, dtype, mode, div):
    """torch.equal: the in-place backward against the out-of-place one; two runs of one call; each row alone against the
    same row among masked rows (N = 1 in both) and a row's gradient inside the batch against the batch in reversed row
    order (a row's stats depend on no other row); grad_total = 0.5 against the scaled reference."""
    inputs = R.extras_inputs(R.TABLE_V, dtype, mode[1], "duplicates")
    s, tv, ti, tau, labels = inputs
    losses, grad = _fwd_bwd(inputs, div, mode)
    losses_i, grad_i = _fwd_bwd(inputs, div, mode, inplace=True)
    assert losses_i == losses and torch.equal(grad_i, grad)
    losses_2, grad_2 = _fwd_bwd(inputs, div, mode)
    assert losses_2 == losses and torch.equal(grad_2, grad)
    flip = tuple(x.flip(0) for x in inputs)
    _, grad_f = _fwd_bwd(flip, div, mode)
    assert torch.equal(grad_f.flip(0), grad)
    for r in (0, 3, 5):
        one = tuple(x[r:r + 1] for x in inputs)
        lab = torch.full_like(labels, -100)
        lab[r] = labels[r]
        l1, g1 = _fwd_bwd(one, div, mode)
        lm, gm = _fwd_bwd((s, tv, ti, tau, lab), div, mode)
        assert l1 == lm and torch.equal(g1[0], gm[r])
        assert float(gm[[i for i in range(len(labels)) if i != r]].abs().max()) == 0.0
    _, half = _fwd_bwd(inputs, div, mode, grad_scale=0.5)
    ref_g = _ref(inputs, div, mode)[4]
    v = P.rowwise_close(half, 0.5 * ref_g, dtype, R.grad_floor_rows("table", len(labels)))
    assert v.ok, v
    assert not torch.equal(half, grad)


@_DIV
@_DT
@pytest.mark.parametrize("Kk", [513, 1024])
def test_tail_inplace_backward_at_two_entries_per_thread(ops, Kk, dtype, div):
    """K > 512: a backward thread holds two entries and gathers logits out of every other wave's chunks before the dense
    pass overwrites them.  The gradient written over the logits equals the out-of-place one bit for bit, and two in-place
    runs agree; the same with seven indices held twice."""
    mode = R.MODES[0]
    inputs = R.table_inputs(R.TABLE_V, dtype, mode[1], Kk)
    losses, grad = _fwd_bwd(inputs, div, mode)
    for _ in range(2):
        losses_i, grad_i = _fwd_bwd(inputs, div, mode, inplace=True)
        assert losses_i == losses and torch.equal(grad_i, grad)
    s, tv, ti, tau, labels = inputs
    dup_i = ti.clone()
    dup_i[:, Kk - 7:] = ti[:, :7]          # seven indices held twice, their second entries in the upper half of the block
    dup = (s, tv, dup_i, tau, labels)
    losses_d, grad_d = _fwd_bwd(dup, div, mode)
    losses_di, grad_di = _fwd_bwd(dup, div, mode, inplace=True)
    assert losses_di == losses_d and torch.equal(grad_di, grad_d) and not torch.equal(grad_d, grad)


@_DIV
@pytest.mark.parametrize("inplace", [False, True])
def test_tail_no_row_and_all_masked_give_connected_zeros(ops, inplace, div):
    """R == 0 (nothing is launched) and a batch whose rows are all masked -- by their labels, by a teacher without a usable
    entry or by their tails: four zeros connected to autograd, a zero gradient."""
    from speech_distill_amd import DistillationLoss
    V, Kk = 4096, 8
    fn = DistillationLoss(2.0, 0.3, divergence=div, beta=0.5, inplace_grad=inplace)
    y = torch.empty(0, V, dtype=torch.bfloat16, device=dev()).requires_grad_(True)
    part = fn.forward_rows(y * 1, torch.empty(0, dtype=torch.int64, device=dev()),
                           teacher_top_k_v=torch.empty(0, Kk, dtype=torch.float16, device=dev()),
                           teacher_top_k_i=torch.empty(0, Kk, dtype=torch.int32, device=dev()),
                           teacher_top_k_tail=torch.empty(0, dtype=torch.float32, device=dev()))
    assert [float(v.detach()) for v in part] == [0.0, 0.0, 0.0, 0.0] and part[0].requires_grad
    part[0].backward()
    assert y.grad.shape == (0, V)
    tv = torch.zeros(3, Kk, dtype=torch.float16, device=dev())
    ti = torch.arange(Kk, dtype=torch.int32, device=dev()).repeat(3, 1)
    good, nan = torch.full((3,), 0.25), float("nan")
    for labels, idx, tau in ((torch.tensor([-100, V, -1]), ti, good), (torch.tensor([1, 2, 3]), torch.full_like(ti, -1), good),
                             (torch.tensor([1, 2, 3]), ti, torch.tensor([nan, 1.0, -1e-9]))):
        x = torch.randn(3, V, device=dev()).bfloat16().requires_grad_(True)
        out = fn.forward_rows(x * 1, labels.to(dev()), teacher_top_k_v=tv, teacher_top_k_i=idx, teacher_top_k_tail=tau.to(dev()))
        assert [float(v.detach()) for v in out] == [0.0, 0.0, 0.0, 0.0] and out[0].requires_grad
        out[0].backward()
        assert float(x.grad.abs().max()) == 0.0


@_DIV
def test_tail_forward_on_btv_equals_forward_rows_on_the_selected_rows(ops, div):
    from speech_distill_amd import DistillationLoss
    B, Tn, V, Kk = 3, 9, 4096, 16
    g = torch.Generator().manual_seed(5)
    s = (torch.randn(B, Tn, V, generator=g) * 3).bfloat16()
    t = to_dev((torch.randn(B, Tn, V, generator=g) * 3).bfloat16())
    labels = torch.randint(0, V, (B, Tn), generator=g)
    labels[0, :4] = -100
    labels[2, 6:] = -100
    mask = torch.ones(B, Tn, dtype=torch.int64)
    mask[1, :5] = 0
    tv, ti = ops.logsoftmax_topk(t, Kk)
    tau = ops.topk_tail(t, ti, 2.0)
    fn = DistillationLoss(2.0, 0.4, divergence=div, beta=0.3)
    x = to_dev(s).requires_grad_(True)
    full = fn(x, to_dev(labels), teacher_top_k_v=tv, teacher_top_k_i=ti, speech_token_mask=to_dev(mask), teacher_top_k_tail=tau)
    full[0].backward()
    rows, row_labels = ops.loss_rows(to_dev(labels), to_dev(mask))
    assert 0 < rows.numel() < B * (Tn - 1)
    y = to_dev(s).reshape(-1, V)[rows].requires_grad_(True)
    part = fn.forward_rows(y, row_labels, teacher_top_k_v=tv.reshape(-1, Kk)[rows], teacher_top_k_i=ti.reshape(-1, Kk)[rows],
                           teacher_top_k_tail=tau.reshape(-1)[rows])
    part[0].backward()
    assert [float(v.detach()) for v in full] == [float(v.detach()) for v in part] and float(full[2].detach()) > 0
    scattered = torch.zeros(B * Tn, V, dtype=torch.bfloat16, device=dev())
    scattered[rows] = y.grad
    assert torch.equal(x.grad.reshape(-1, V), scattered)
    with pytest.raises(ValueError, match=f"divergence='{div[:-5]}'"):
        fn(x, to_dev(labels), teacher_logits=t)
    # T = 1: the tail the stored log-probs imply stands in for a missing one
    fn1 = DistillationLoss(1.0, 0.4, divergence=div, beta=0.3)
    a = fn1.forward_rows(y.detach(), row_labels, teacher_top_k_v=tv.reshape(-1, Kk)[rows], teacher_top_k_i=ti.reshape(-1, Kk)[rows])
    b = fn1.forward_rows(y.detach(), row_labels, teacher_top_k_v=tv.reshape(-1, Kk)[rows], teacher_top_k_i=ti.reshape(-1, Kk)[rows],
                         teacher_top_k_tail=ops.tail_from_logprobs(tv.reshape(-1, Kk)[rows]))
    assert [float(v) for v in a] == [float(v) for v in b]


def test_tail_misuse_is_refused_before_any_launch(ops):
    """A misaligned pointer, V = 12, K = 0 / 1025 / V, beta = 0 / 1 / NaN for the JSD only, an unknown mode or dtype, a
    temperature <= 0, a vocabulary beyond the bitmap and a NULL top_k_v / top_k_i / top_k_tail each return their code; the
    sentinel-filled stats, scalars and gradient are unchanged."""
    lib = ops.load_lib()
    V, Kk = 16, 4
    s = torch.randn(4, V, device=dev()).bfloat16()
    tv = torch.zeros(4, Kk, dtype=torch.float16, device=dev())
    ti = torch.arange(Kk, dtype=torch.int32, device=dev()).repeat(4, 1).contiguous()
    tau = torch.full((4,), 0.25, dtype=torch.float32, device=dev())
    labels = torch.tensor([1, 2, 3, -100], device=dev())
    stats = torch.full((lib.sd_gjsd_tail_stats_bytes(4),), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((8,), -7.0, dtype=torch.float32, device=dev())
    grad = torch.full((4, V), 3.0, dtype=torch.bfloat16, device=dev())
    keep = [x.clone() for x in (stats, out, grad, s, tv, ti, tau)]
    nan = float("nan")
    cases = [("misaligned student", ALIGN, dict(s_ptr=s.data_ptr() + 2)), ("V = 12", ALIGN, dict(V=12)),
             ("K = 0", SHAPE, dict(Kk=0)), ("K = -1", SHAPE, dict(Kk=-1)), ("K = 1025", SHAPE, dict(Kk=1025)),
             ("K = V", SHAPE, dict(Kk=16)), ("K > V", SHAPE, dict(Kk=24)),
             ("beta 0", SHAPE, dict(beta=0.0, mode=2)), ("beta 1", SHAPE, dict(beta=1.0, mode=2)), ("beta NaN", SHAPE, dict(beta=nan, mode=2)),
             ("mode 3", UNSUPPORTED, dict(mode=3)), ("mode -1", UNSUPPORTED, dict(mode=-1)),
             ("unknown dtype", UNSUPPORTED, dict(dt=2)), ("V beyond the bitmap", UNSUPPORTED, dict(V=458760)),
             ("temperature 0", SHAPE, dict(T=0.0)), ("temperature NaN", SHAPE, dict(T=nan)), ("temperature inf", SHAPE, dict(T=float("inf"))),
             ("NULL values", NO_TEACHER, dict(tv_ptr=None)), ("NULL indices", NO_TEACHER, dict(ti_ptr=None)),
             ("NULL tail", NO_TEACHER, dict(tau_ptr=None))]
    for what, code, kw in cases:
        a = dict(beta=0.5, T=2.0, mode=1, dt=0)
        a.update({k: v for k, v in kw.items() if k in a})
        extra = {k: v for k, v in kw.items() if k not in a}
        args = (lib, s, tv, ti, tau, labels, stats, out, a["beta"], a["T"], a["mode"], a["dt"])
        assert _raw(*args, **extra) == code, what
        assert _raw(*args, grad=grad.data_ptr(), **extra) == code, what
    assert _raw(lib, s, tv, ti, tau, labels, stats, out, 0.5, 2.0, 1, 0, grad=grad.data_ptr() + 2) == ALIGN   # misaligned gradient
    torch.cuda.synchronize()
    for now, before in zip((stats, out, grad, s, tv, ti, tau), keep):
        assert torch.equal(now, before)
    # the same arguments without a mistake are accepted; beta is the JSD's alone
    for mode, beta in ((0, nan), (1, 0.0), (2, 0.5)):
        assert _raw(lib, s, tv, ti, tau, labels, stats, out, beta, 2.0, mode, 0) == 0
        torch.cuda.synchronize()
        assert float(out[4]) == 3.0 and float(out[6]) == 0.0 and float(out[7]) == 0.0 and math.isfinite(float(out[0]))
