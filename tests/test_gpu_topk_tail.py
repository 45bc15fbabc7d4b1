"""-m gpu: sd_topk_tail (ops.topk_tail), the teacher's mass outside its top-K at a temperature, against the fp64 direct sum
of tests/gjsd_tail_ref.py (tail_direct) with the measured floor TAIL_RTOL, judged RELATIVELY: a tail of 1e-12 has to keep
its digits, which is why the kernel sums the non-members directly.

Shapes.  topk_tail_kernel streams a row with 512 threads and four 8-element chunks in flight per thread and keeps a V-bit
bitmap in LDS: V = 8 (K = 4), gjsd_ref's streaming edges 4096, 16 384, 16 392, the case table's 40 008, and once the real
159 488 (a bitmap of 19 936 bytes) and the largest supported 524 288 with two rows; K = 1, 100, 1024; T = 1, 2, 3; bf16
and fp32.
"""
import math

import pytest
import torch

import gjsd_tail_ref as R
from gpu_util import dev, record, to_dev
from parity_ref import BF, F32

pytestmark = pytest.mark.gpu

SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3
_DT = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])


@pytest.fixture(scope="module")
def ops():
    import speech_distill_amd.ops as ops_
    ops_.load_lib()
    return ops_


def _check(ops, name, dtype, temperatures=R.TAIL_TEMPERATURES):
    t, ti, V = R.tail_case(name, dtype)
    x, idx = to_dev(t), to_dev(ti)
    for T in temperatures:
        want = R.tail_direct(t.float(), ti, T, V)
        got = ops.topk_tail(x, idx, T, V)
        assert got.dtype == torch.float32 and got.shape == want.shape
        rel = ((got.double().cpu() - want).abs() / want)
        rec = dict(got=got.cpu().tolist(), want=want.tolist(), worst_rel=float(rel.max()), rtol=R.TAIL_RTOL)
        print(name, "T", T, rec)
        record(f"topk_tail_{name}_{'bf16' if dtype == BF else 'fp32'}_T{T:g}", **rec)
        assert bool(torch.isfinite(got).all()) and float(rel.max()) <= R.TAIL_RTOL, (name, T, rec)


@_DT
@pytest.mark.parametrize("name", [n for n in R.TAIL_CASES if n.startswith("randn")])
def test_tail_of_random_rows(ops, name, dtype):
    """V x K x T x dtype on random rows; at V = 159 488 the bitmap has its real size, at 524 288 (the largest V the entry
    takes) it is the whole 64 KB of LDS."""
    _check(ops, name, dtype)


@_DT
def test_tail_of_1e_minus_12_keeps_its_digits(ops, dtype):
    """One teacher logit 37 above a narrow rest: tau ~ 1.5e-12 at T = 1, where 1 - (the members' share) is 0 in fp32."""
    t, ti, V = R.tail_case("spike", dtype)
    assert 1e-13 < float(R.tail_direct(t.float(), ti, 1.0, V).max()) < 1e-11
    _check(ops, "spike", dtype)


@_DT
def test_membership_is_by_index_not_by_value(ops, dtype):
    """300 equal logits across the K-th boundary: the tied ones the top-K does not hold are tail."""
    _check(ops, "ties", dtype)


@_DT
def test_duplicated_and_out_of_range_indices(ops, dtype):
    """A duplicate sets its bit once; -1, V, 2^31 - 1 and -2^31 are ignored and never used as an address."""
    _check(ops, "bad_indices", dtype)


@_DT
def test_row_stride_beyond_v_is_never_read(ops, dtype):
    """row_stride = V + 24 with NaN and +inf behind every row: the result is that of the first V columns."""
    t, ti, V = R.tail_case("stride", dtype)
    assert t.shape[1] == V + 24 and bool(torch.isnan(t[:, V]).all()) and bool(torch.isinf(t[:, -1]).all())
    _check(ops, "stride", dtype)
    x = to_dev(t)
    assert torch.equal(ops.topk_tail(x, to_dev(ti), 2.0, V), ops.topk_tail(x[:, :V].contiguous(), to_dev(ti), 2.0))


def test_tail_goes_with_logsoftmax_topk_and_takes_leading_dimensions(ops):
    """[B, T, V] logits with the indices ops.logsoftmax_topk returned for them; 1 - tail is the sum of the stored
    probabilities at T = 1 to their fp16 precision; two calls agree bit for bit."""
    g = torch.Generator().manual_seed(9)
    x = to_dev((torch.randn(2, 3, 4096, generator=g) * 3).bfloat16())
    tv, ti = ops.logsoftmax_topk(x, 64)
    tail = ops.topk_tail(x, ti, 1.0)
    assert tail.shape == (2, 3) and torch.equal(tail, ops.topk_tail(x, ti, 1.0))
    assert float((tail - ops.tail_from_logprobs(tv)).abs().max()) <= 1e-3
    want = R.tail_direct(x.reshape(-1, 4096).float().cpu(), ti.reshape(-1, 64).cpu(), 1.0).reshape(2, 3)
    assert float(((tail.double().cpu() - want).abs() / want).max()) <= R.TAIL_RTOL


def test_guard_words_around_tail_out_and_every_error_code(ops):
    lib = ops.load_lib()
    Rn, V, K = 3, 4096, 16
    x = torch.randn(Rn, V, device=dev()).bfloat16()
    ti = torch.arange(K, dtype=torch.int32, device=dev()).repeat(Rn, 1).contiguous()
    buf = torch.full((Rn + 2,), -7.0, dtype=torch.float32, device=dev())
    stream = torch.cuda.current_stream().cuda_stream

    def call(logits=None, idx="own", out="own", rows=Rn, stride=V, v=V, k=K, T=2.0, dt=0):
        return lib.sd_topk_tail(x.data_ptr() if logits is None else logits, ti.data_ptr() if idx == "own" else idx,
                                buf[1:].data_ptr() if out == "own" else out, rows, stride, v, k, T, dt, stream)
    nan = float("nan")
    cases = [("rows 0", SHAPE, dict(rows=0)), ("V 0", SHAPE, dict(v=0)), ("K 0", SHAPE, dict(k=0)), ("K 1025", SHAPE, dict(k=1025)),
             ("K > V", SHAPE, dict(v=8, k=16)), ("stride < V", SHAPE, dict(stride=V - 8)), ("NULL logits", SHAPE, dict(logits=0)),
             ("NULL indices", SHAPE, dict(idx=None)), ("NULL out", SHAPE, dict(out=None)), ("T 0", SHAPE, dict(T=0.0)),
             ("T NaN", SHAPE, dict(T=nan)), ("T inf", SHAPE, dict(T=math.inf)), ("V 12", ALIGN, dict(v=12, k=4)),
             ("stride 4100", ALIGN, dict(stride=4100)), ("misaligned logits", ALIGN, dict(logits=x.data_ptr() + 2)),
             ("V 524296", UNSUPPORTED, dict(v=524296, stride=524296)), ("dtype 2", UNSUPPORTED, dict(dt=2))]
    for what, code, kw in cases:
        assert call(**kw) == code, what
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())                   # nothing was written by a refused call
    assert call() == 0
    torch.cuda.synchronize()
    assert float(buf[0]) == -7.0 and float(buf[Rn + 1]) == -7.0          # the guard words
    want = R.tail_direct(x.float().cpu(), ti.cpu(), 2.0)
    assert float(((buf[1:Rn + 1].double().cpu() - want).abs() / want).max()) <= R.TAIL_RTOL
