"""-m gpu: the distillation loss, the cross-entropy loss, the teacher top-K and the fused AdamW against fp64 references,
per row and per element, on every kernel path (tests/parity_ref.py holds the references, the acceptance rule, the floors
and the case tables; tests/test_parity_ref_cpu.py shows on the CPU that the rule rejects wrong formulas and that each
case reaches the path it is named for).

Loss cases run the rows entry points the trainer uses (DistillationLoss.forward_rows, ops.celoss_rows) on eight rows of
different kinds at V = 40 008: 9.8 chunks per thread of kd_fwd_kernel at 512 threads and 4.9 at 1024, so the streaming
loop makes several prefetch trips with a ragged last one and rescales its running maximum.
"""
import numpy as np
import pytest
import torch

import parity_ref as P
from parity_ref import BF, F32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    yield ops_
    _lib.debug_set("reset", 0)


from gpu_util import dev, record, to_dev  # noqa: E402
from speech_distill_amd import _lib  # noqa: E402

ULP32 = 2.0 ** -24  # one fp32 rounding, relative


def _dt_name(dt):
    return "bf16" if dt == BF else "fp32"


# ------------------------------------------------------------------------------------------------- loss
_KW = {"teacher": "teacher_logits", "top_v": "teacher_top_k_v", "top_i": "teacher_top_k_i"}


def _kw_dev(kw):
    return {_KW[k]: to_dev(v) for k, v in kw.items()}


def _rows_fwd_bwd(s, labels, kw, T, grad_scale=None, inplace=False):
    """DistillationLoss.forward_rows + backward -> ([total, task, distill, teacher] floats, gradient of the logits)."""
    from speech_distill_amd import DistillationLoss
    leaf = to_dev(s).requires_grad_(True)
    x = leaf * 1 if inplace else leaf  # a non-leaf, so that its buffer may be overwritten
    out = DistillationLoss(T, P.LOSS_ALPHA, inplace_grad=inplace).forward_rows(x, to_dev(labels), **_kw_dev(kw))
    losses = [float(v) for v in out]
    (out[0] if grad_scale is None else out[0] * grad_scale).backward()
    return losses, leaf.grad


def _rows_out(ops, s, labels, kw, T):
    """The raw out[0..5] = total, task, distill, teacher, N, hits of the same entry (forward only)."""
    d = _kw_dev(kw)
    with torch.no_grad():
        _, out = ops.KDLossRowsFn.apply(to_dev(s), to_dev(labels), d.get("teacher_logits"), d.get("teacher_top_k_v"),
                                        d.get("teacher_top_k_i"), T, P.LOSS_ALPHA, False)
    return [float(v) for v in out[:6].cpu()]


def _check_loss_case(ops, name, s, labels, kw, T, dtype, per_row=True):
    form = "dense" if "teacher" in kw else "sparse"
    rtol = P.LOSS_SCALAR_RTOL[form]
    ref_l, n, hits, ref_g = P.oracle_rows(s, labels, temperature=T, alpha=P.LOSS_ALPHA, **kw)
    losses, grad = _rows_fwd_bwd(s, labels, kw, T)
    out = _rows_out(ops, s, labels, kw, T)
    ok, why = P.loss_close(losses, grad, ref_l, ref_g, dtype, form)
    v = P.rowwise_close(grad, ref_g, dtype, P.LOSS_GRAD_FLOOR)
    rec = dict(losses=losses, ref=list(ref_l), scalar_rel=P.scalar_close(losses, ref_l, rtol)[2], scalar_bound=rtol,
               grad_worst_rel=v.worst_rel, grad_floor=P.LOSS_GRAD_FLOOR, grad_fp32_measured=P.LOSS_GRAD_MEASURED,
               scalar_fp32_measured=P.LOSS_SCALAR_MEASURED[form], grad_worst=[v.row, v.col, v.got, v.ref])
    print(name, rec)
    record("parity_loss_" + name, **rec)
    assert out[:4] == losses, (out, losses)
    assert out[4] == n and out[5] == hits, (out, n, hits)  # exact
    assert ok, f"{name}: {why}"
    ignored = labels == -100
    assert float(grad[to_dev(ignored)].abs().max()) == 0.0
    if not per_row:
        return out
    # each row on its own against the oracle on that row; the batch is the mean of the rows
    rows = []
    for r in torch.nonzero(~ignored).reshape(-1).tolist():
        kr = {k: x[r:r + 1] for k, x in kw.items()}
        got = _rows_out(ops, s[r:r + 1], labels[r:r + 1], kr, T)
        want, _, h, _ = P.oracle_rows(s[r:r + 1], labels[r:r + 1], temperature=T, alpha=P.LOSS_ALPHA, **kr)
        s_ok, i, rel = P.scalar_close(got[:4], want, rtol)
        print(name, "row", r, P.ROW_KINDS[r] if len(labels) == 8 else "", got[:4], "rel", rel)
        assert s_ok, f"{name} row {r}: got {got[:4]} want {want} (entry {i}, rel {rel:.3e} > {rtol:.1e})"
        assert got[4] == 1.0 and got[5] == h
        rows.append(got)
    rows = np.array(rows, dtype=np.float64)
    # kd_finalize_kernel adds at most 8 row terms in fp32 and divides: a dozen roundings of numbers no larger than the
    # sum of the rows' magnitudes (the single-row values carry one rounding each of their own)
    for j, what in enumerate(("total", "task", "distill")):
        mean, tol = rows[:, j].mean(), 16 * ULP32 * np.abs(rows[:, j]).sum() / n
        assert abs(out[j] - mean) <= tol, f"{name}: batch {what} {out[j]} != mean of its rows {mean} (tol {tol:.2e})"
    teach = (rows[:, 3] * rows[:, 5]).sum() / max(hits, 1)  # dense: every row counts once; sparse: every hit
    assert abs(out[3] - teach) <= 16 * ULP32 * np.abs(rows[:, 3] * rows[:, 5]).sum() / max(hits, 1), (out[3], teach)
    return out


def _case_id(c):
    return c[0]


@pytest.mark.parametrize("case", P.LOSS_CASES, ids=_case_id)
def test_loss_rows_all_instantiations(ops, case):
    """The 12 kd_fwd_kernel<T, T2, NF, DENSE> instantiations (and temperature 1 on the generic ones) at V = 40 008, eight
    row kinds: losses per row and per batch, N and hits exact, gradient per row and per element, ignored row exactly 0."""
    name, V, dtype, T, te = case
    s, _ = P.loss_inputs(V, dtype)
    _check_loss_case(ops, name, s, P.loss_labels(V, dtype), P.loss_case_teacher(V, dtype, te), T, dtype)


@pytest.mark.parametrize("case", P.LOSS_EDGE_CASES, ids=_case_id)
def test_loss_rows_vocabulary_edges(ops, case):
    """V = 8 (one chunk in all, K = 4), 4096 (one chunk per thread), 16 384 (exactly one prefetch trip), 16 392 (one
    chunk more)."""
    name, V, dtype, T, te = case
    s, _ = P.loss_inputs(V, dtype)
    _check_loss_case(ops, name, s, P.loss_labels(V, dtype), P.loss_case_teacher(V, dtype, te), T, dtype)


@pytest.mark.parametrize("extra", ["duplicates", "ends", "no_hit"])
@pytest.mark.parametrize("dtype,T", [(BF, 2.0), (F32, 3.0)], ids=["bf16_T2", "fp32_T3"])
def test_loss_rows_sparse_extras(ops, dtype, T, extra):
    """Top-K teachers at K = 100: an index twice and the label three times in one row (the reference sums their q and
    counts every hit); the label at top-K position 0 and K - 1; no hit anywhere (teacher monitor 0, hits 0)."""
    tv, ti, labels = P.sparse_extras(P.LOSS_V, dtype)[extra]
    s, _ = P.loss_inputs(P.LOSS_V, dtype)
    out = _check_loss_case(ops, f"{extra}_{_dt_name(dtype)}", s, labels, dict(top_v=tv, top_i=ti), T, dtype)
    assert out[5] == {"duplicates": 6.0, "ends": 2.0, "no_hit": 0.0}[extra]
    if extra == "no_hit":
        assert out[3] == 0.0


@pytest.mark.parametrize("form", ["dense", "sparse", "duplicates"])
@pytest.mark.parametrize("dtype,T", [(BF, 2.0), (F32, 3.0)], ids=["bf16_T2", "fp32_T3"])
def test_loss_rows_upstream_gradient_and_inplace(ops, dtype, T, form):
    """(loss * 0.25).backward() is 0.25 x the reference gradient, and inplace_grad=True (the gradient written over the
    logits, as the trainer runs it) is bit-equal to the out-of-place gradient."""
    s, _ = P.loss_inputs(P.LOSS_V, dtype)
    labels = P.loss_labels(P.LOSS_V, dtype)
    kw = P.loss_case_teacher(P.LOSS_V, dtype, "dense" if form == "dense" else 100)
    if form == "duplicates":
        tv, ti, labels = P.sparse_extras(P.LOSS_V, dtype)["duplicates"]
        kw = dict(top_v=tv, top_i=ti)
    _, _, _, ref_g = P.oracle_rows(s, labels, temperature=T, alpha=P.LOSS_ALPHA, **kw)
    _, g_scaled = _rows_fwd_bwd(s, labels, kw, T, grad_scale=0.25)
    v = P.rowwise_close(g_scaled, 0.25 * ref_g, dtype, P.LOSS_GRAD_FLOOR)
    record(f"parity_loss_upstream_{form}_{_dt_name(dtype)}", worst_rel=v.worst_rel, floor=P.LOSS_GRAD_FLOOR,
           fp32_measured=P.LOSS_GRAD_MEASURED)
    assert v.ok, v
    l_out, g_out = _rows_fwd_bwd(s, labels, kw, T)
    l_in, g_in = _rows_fwd_bwd(s, labels, kw, T, inplace=True)
    assert l_out == l_in
    assert torch.equal(g_out, g_in)
    assert not torch.equal(g_out, g_scaled)


@pytest.mark.parametrize("layout", ["prefix", "general"])
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_loss_shifted_entry_equals_rows_entry(ops, form, layout):
    """DistillationLoss.forward (causal shift, -100 and speech mask evaluated per row by the kernel) against forward_rows
    on the rows ops.loss_rows selects: B = 2, T = 5, V = 40 008, fp32, temperature 3.  N and hits are exact and every
    valid row's gradient is bit-equal; rows at masked positions and at t = T - 1 are exactly 0.  The losses are bit-equal
    in the "prefix" layout, where the valid rows are rows 0..2 in both calls; in the "general" layout the finalize
    kernel's butterfly sum pairs the same terms differently (rows 1, 2, 3, 5, 7 against 0..4), so they agree to a few
    fp32 roundings of the sum."""
    from oracle import distill_loss as L
    from speech_distill_amd import DistillationLoss
    B, T, V, K, temp = 2, 5, P.LOSS_V, 100, 3.0
    gen = torch.Generator().manual_seed(77)
    s = torch.randn(B, T, V, generator=gen) * 3
    t = torch.randn(B, T, V, generator=gen) * 3
    labels = torch.randint(0, V, (B, T), generator=gen)
    sm = torch.ones(B, T, dtype=torch.long)
    if layout == "prefix":   # rows 0, 1, 2 valid; (0,3) masked by the speech mask; all of sequence 1 masked or ignored
        sm[0, 4] = 0
        labels[1, 1:3] = -100
        sm[1, 3:] = 0
        want_rows = [0, 1, 2]
    else:                    # row 0 ignored; (1,1) masked by the speech mask; (1,3) ignored
        labels[0, 1] = -100
        sm[1, 2] = 0
        labels[1, 4] = -100
        want_rows = [1, 2, 3, 5, 7]
    tv, ti = L.extract_topk(t, K)
    ti[0, 1, 3] = int(labels[0, 2])  # a hit in row 1
    kw_o = dict(teacher_logits=t) if form == "dense" else dict(teacher_top_k_v=tv, teacher_top_k_i=ti)
    kw = {k: to_dev(x) for k, x in kw_o.items()}
    fn = DistillationLoss(temp, P.LOSS_ALPHA)
    sd = to_dev(s).requires_grad_(True)
    out = fn(sd, to_dev(labels), speech_token_mask=to_dev(sm), **kw)
    out[0].backward()
    rows, row_labels = ops.loss_rows(to_dev(labels), to_dev(sm))
    assert rows.cpu().tolist() == want_rows
    sr = to_dev(s).reshape(-1, V)[rows].contiguous().requires_grad_(True)
    kr = {k: x.reshape(B * T, -1)[rows].contiguous() for k, x in kw.items()}
    out_r = fn.forward_rows(sr, row_labels, **kr)
    out_r[0].backward()
    got, got_r = [float(x) for x in out], [float(x) for x in out_r]
    record(f"parity_loss_shifted_{form}_{layout}", shifted=got, rows=got_r)
    if layout == "prefix":
        assert got == got_r
    else:
        assert all(abs(a - b) <= 8 * ULP32 * abs(b) for a, b in zip(got, got_r)), (got, got_r)
    g = sd.grad.reshape(B * T, V)
    assert torch.equal(g[rows], sr.grad)
    dead = torch.ones(B * T, dtype=torch.bool)
    dead[want_rows] = False
    assert float(g[to_dev(dead)].abs().max()) == 0.0 and bool(dead[T - 1]) and bool(dead[2 * T - 1])
    # and both are right: the fp64 oracle on the unshifted batch
    ref = L.distill_loss(s, labels, speech_token_mask=sm, temperature=temp, alpha=P.LOSS_ALPHA, return_grad=True, **kw_o)
    ok, why = P.loss_close(got, sd.grad.reshape(B * T, V), [float(x) for x in ref[:4]], ref[4].reshape(B * T, V), F32, form)
    assert ok, why


@pytest.mark.parametrize("dtype", [BF, F32], ids=_dt_name)
def test_celoss_rows_per_row(ops, dtype):
    """ops.celoss_rows (the Stage-1 loss) on the same eight row kinds at V = 40 008: every row on its own and the batch
    against fp64, N exact, gradient per row and per element, ignored row exactly 0."""
    s, _ = P.loss_inputs(P.LOSS_V, dtype)
    labels = P.loss_labels(P.LOSS_V, dtype)
    ref, ref_rows, n, ref_g = P.ce_ref(s, labels)
    sd = to_dev(s).requires_grad_(True)
    loss, out = ops.celoss_rows(sd, to_dev(labels))
    loss.backward()
    s_ok, _, rel = P.scalar_close([float(loss)], [ref], P.CE_SCALAR_RTOL, atol=0.0)
    v = P.rowwise_close(sd.grad, ref_g, dtype, P.CE_GRAD_FLOOR)
    rec = dict(loss=float(loss), ref=ref, scalar_rel=rel, scalar_bound=P.CE_SCALAR_RTOL, grad_worst_rel=v.worst_rel,
               grad_floor=P.CE_GRAD_FLOOR, grad_fp32_measured=P.CE_GRAD_MEASURED, scalar_fp32_measured=P.CE_SCALAR_MEASURED)
    print(rec)
    record(f"parity_celoss_{_dt_name(dtype)}", **rec)
    assert float(out[2]) == n == 7
    assert s_ok, (float(loss), ref, rel)
    assert v.ok, v
    assert float(sd.grad[7].abs().max()) == 0.0
    for r in range(7):
        with torch.no_grad():
            lr_, _ = ops.celoss_rows(to_dev(s[r:r + 1]), to_dev(labels[r:r + 1]))
        s_ok, _, rel = P.scalar_close([float(lr_)], [float(ref_rows[r])], P.CE_SCALAR_RTOL, atol=0.0)
        print("row", r, P.ROW_KINDS[r], float(lr_), float(ref_rows[r]), rel)
        assert s_ok, (r, P.ROW_KINDS[r], float(lr_), float(ref_rows[r]), rel)


# ------------------------------------------------------------------------------------------------- top-K
def _check_topk(ops, name, dtype, nt):
    c = P.TOPK_CASES[name]
    x = c["make"](dtype)
    xv = x if c["vocab"] is None else x[:, :c["vocab"]]
    v, i = ops.logsoftmax_topk(to_dev(x), c["K"], c["vocab"])
    ref_v, ref_i = P.topk_ref(xv, c["K"])
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i.numpy(), err_msg=f"{name} {dtype} NT={nt}")
    ver = P.rowwise_close(v, ref_v, torch.float16, P.TOPK_VAL_FLOOR)
    record(f"parity_topk_{name}_{_dt_name(dtype)}_nt{nt}", worst_rel=ver.worst_rel, floor=P.TOPK_VAL_FLOOR,
           fp32_measured=P.TOPK_VAL_MEASURED)
    assert ver.ok, ver


@pytest.mark.parametrize("name,dtype,nt", P.topk_case_list((512,)), ids=lambda x: x if isinstance(x, (str, int)) else _dt_name(x))
def test_topk_paths(ops, name, dtype, nt):
    """ops.logsoftmax_topk: indices exact against (logit descending, index ascending), values per element in fp16.
    (a) overflow fall-back, (b) ties carried across trips of the radix select, (c) the plain loops of rows longer than
    163 840, (d) K = 1, 513, 1024, (e) V = K = 8, (f) a vocabulary tail of +100 beyond vocab_size that must be neither
    selected nor counted, (g) rows of different paths in one launch."""
    _check_topk(ops, name, dtype, nt)


@pytest.mark.parametrize("name,dtype,nt", P.topk_case_list((256, 1024)), ids=lambda x: x if isinstance(x, (str, int)) else _dt_name(x))
def test_topk_paths_other_block_sizes(ops, name, dtype, nt):
    """(h): cases (a), (b) and (d) on the 256- and 1024-thread instantiations."""
    before = _lib.debug_get("topk.nt")
    try:
        _lib.debug_set("topk.nt", nt)
        _check_topk(ops, name, dtype, nt)
    finally:
        _lib.debug_set("topk.nt", before)


# ------------------------------------------------------------------------------------------------- AdamW
PAD = 8  # elements in front of the slice (16 bytes: the kernels' vector alignment) and at least as many behind


def _adamw_call(ops, n, set_name, clip=True):
    """One ops.adamw_ call on slices [PAD : PAD + n] of larger buffers -> (p, m, v) slices on the CPU; asserts that
    nothing outside the slices, and nothing of the gradient, changed."""
    (p, g, m, v), (ss, mx) = P.adamw_inputs(n, set_name)
    gen = torch.Generator().manual_seed(n)
    host = []
    for t in (p, g, m, v):
        buf = torch.randn(PAD + n + 24, generator=gen).bfloat16()
        buf[PAD:PAD + n] = t
        host.append(buf)
    bufs = [to_dev(b) for b in host]
    pv, gv, mv, vv = (b[PAD:PAD + n] for b in bufs)
    ss_dev = torch.tensor([ss], dtype=torch.float32, device=dev()) if (clip and ss is not None) else None
    ops.adamw_(pv, gv, mv, vv, *P.adamw_hp(set_name), ss_dev, mx if clip else 0.0)
    back = [b.cpu() for b in bufs]
    for k, h, b in zip("pgmv", host, back):
        assert torch.equal(h[:PAD], b[:PAD]) and torch.equal(h[PAD + n:], b[PAD + n:]), f"{k}: wrote outside its {n} elements"
    assert torch.equal(host[1], back[1])
    return [back[j][PAD:PAD + n] for j in (0, 2, 3)]


def _check_adamw(ops, n, set_name):
    (p, g, m, v), (ss, mx) = P.adamw_inputs(n, set_name)
    ref = P.adamw_ref64(p, g, m, v, *P.adamw_hp(set_name), sumsq=ss, max_norm=mx)
    got = _adamw_call(ops, n, set_name)
    verdicts = P.adamw_close(got, ref)
    record(f"parity_adamw_{set_name}_n{n}", floor=P.ADAMW_FLOOR, fp32_measured=P.ADAMW_MEASURED,
           **{k: x.worst_rel for k, x in verdicts.items()})
    for k, x in verdicts.items():
        assert x.ok, f"{set_name} n={n} {k}: {x}"
    if P.ADAMW_SETS[set_name]["clip"] in ("zero", "below"):  # a clip of exactly 1 is the no-clip call, bit for bit
        plain = _adamw_call(ops, n, set_name, clip=False)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), (set_name, n)


@pytest.mark.parametrize("set_name", list(P.ADAMW_SETS))
def test_adamw_small_sizes(ops, set_name):
    """n = 1, 7 (tail loop only), 8 (one vector, no tail), 9, 2055 (nine workgroups and a tail): p, m, v per element
    against fp64, every clip branch, neighbours untouched."""
    for n in P.ADAMW_SIZES[:-1]:
        _check_adamw(ops, n, set_name)


@pytest.mark.parametrize("set_name", P.ADAMW_BIG_SETS)
def test_adamw_grid_stride_wrap(ops, set_name):
    """n = 4096 * 256 * 8 + 2400 + 5: more vectors than 4096 workgroups hold, so the grid-stride loop wraps, plus a tail."""
    _check_adamw(ops, P.ADAMW_SIZES[-1], set_name)


def test_adamw_and_sumsq_refuse_a_misaligned_slice(ops):
    (p, g, m, v), _ = P.adamw_inputs(2055, "step3_none")
    bufs = [to_dev(torch.cat([t[:1], t])) for t in (p, g, m, v)]
    before = [b.clone() for b in bufs]
    with pytest.raises(_lib.SdHipError, match="SD_ERR_ALIGN"):
        ops.adamw_(*(b[1:] for b in bufs), *P.adamw_hp("step3_none"))
    out = torch.zeros(1, device=dev())
    with pytest.raises(_lib.SdHipError, match="SD_ERR_ALIGN"):
        ops.sumsq(bufs[1][1:], out)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs)) and float(out) == 0.0


@pytest.mark.parametrize("n", [1, 7, 9])
def test_sumsq_tiny(ops, n):
    """Fewer elements than one vector, and one vector plus one: at most n + 4 fp32 roundings (the squares are exact)."""
    x = torch.randn(PAD + n + 8, generator=torch.Generator().manual_seed(n)).bfloat16()
    xd = to_dev(x)
    out = torch.zeros(1, device=dev())
    ops.sumsq(xd[PAD:PAD + n], out)
    ref = float(x[PAD:PAD + n].double().pow(2).sum())
    assert abs(float(out) - ref) <= (n + 4) * ULP32 * ref, (float(out), ref)
    assert torch.equal(xd.cpu(), x)
