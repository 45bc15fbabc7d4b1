"""-m gpu: the loss and top-K kernels (csrc/sd_loss.hip and csrc/sd_topk.hip over the device functions of csrc/sd_rows.cuh)
write the bits they wrote when every kernel carried its own copy of the streamed row read, the online max / sum-exp step,
the block merge and the masked-row zero fill.

tests/golden/loss_rows/ holds the outputs of commit af44a8f ("Add on-policy distillation: reverse-KL / JSD loss kernels and
rollouts"), the commit before that change, on the seeded CPU inputs of tests/parity_ref.py and tests/gjsd_ref.py (written by
`SD_HIP_LIB=<that build's libsd_hip.so> python tests/test_gpu_loss_golden.py --record DIR`): whole arrays for loss_out and
for the top-K values, indices and lse (arrays.npz), SHA-256 digests of the bytes of every stats buffer and every gradient
buffer, per case and per row (digests.json; the row digests are cut to 64 bits, they only name the row), and a digest of
every case's inputs, asserted first: a mismatch there means the seeded inputs are not the recorded ones, not that a kernel
changed.

Every buffer a kernel writes is pre-filled with the NaN sentinel of tests/test_gpu_gemv.py (stats: 0xFF bytes); gradients
and top-K outputs have two guard rows above and below, and the WHOLE buffer is compared: a stray write fails like a wrong
bit.  The upstream gradient is 0.75.  Cases marked in place run the backward a second time with the gradient aliasing the
logits; that buffer must hash to the out-of-place one.

Cases (eight rows each unless the family says otherwise):
  kd    every P.LOSS_CASES and P.LOSS_EDGE_CASES entry (the 12 kd_fwd_kernel instantiations, T = 1, V = 8 / 4096 / 16384 /
        16392 / 40008), the three P.sparse_extras for both (dtype, T) pairs, and a dense and a sparse batch through the
        shifted sd_kdloss_fwd / sd_kdloss_bwd entry with a speech mask;
  ce    sd_celoss_*_rows, both dtypes, V = 40008 and the four edges, with and without a divisor;
  gjsd  the table, near and underflow families of tests/gjsd_ref.py;
  topk  P.topk_case_list((256, 512, 1024)).

The sparse families were recorded later, from commit 7b5e9af ("On-policy: roll out the accumulation window through the
engine"), the commit before gjsd_topk_bwd_kernel and gjsd_tail_bwd_kernel became wrappers of one tk_bwd_row and the
top-K forwards took their normaliser step, masked-row exit and entry epilogue from shared functions (DESIGN.md section
12e), into ONE file of their own (arrays_sparse.npz; `--record DIR sparse`), which holds the digests as well: the JSON
text of what digests.json holds for the older cases, as a byte array under the key DIGESTS_KEY:
  tk    sd_gjsd_topk_*_rows on every entry of gjsd_topk_ref.family_cases(f), f = table, peaked, underflow (V = 8 / 4096 /
        16384 / 16392 / 40008, K = 4 / 32 / 100 / 512 / 513 / 1024, duplicates, ends, no hit, dropped entries);
  tail  sd_gjsd_tail_*_rows on every entry of gjsd_tail_ref.family_cases(f) (the same, and bad tails) for each of the three
        divergences.
For each of the two backward kernels the in-place cases are one at K = 100, one at K = 1024 (two entries per thread) and
the "duplicates" extra; the tail kernel runs them in all three modes."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # first: as a script (--record) this is what puts the repository root on sys.path
import gjsd_ref as G
import gjsd_tail_ref as TL
import gjsd_topk_ref as TK
import parity_ref as P
from gpu_util import dev, to_dev
from parity_ref import BF, F32
from test_gpu_gemv import SENT

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(GOLDEN, "loss_rows")
GUARD = 2
SENT32 = 0x7FC10000   # the sentinel as an fp32 NaN
GO = 0.75             # upstream gradient
EDGE_V = (8, 4096, 16384, 16392)
MODE = {"reverse_kl": 1, "jsd": 2}


@pytest.fixture(scope="module")
def lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt_name(dt):
    return "bf16" if dt == BF else "fp32"


def _dt(dt):
    return 0 if dt == BF else 1


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------ buffers, digests
def _sentinel(rows, cols, dtype):
    """A sentinel-filled buffer [GUARD + rows + GUARD, cols] of 2- or 4-byte elements and the view of its inner rows."""
    if dtype in (torch.bfloat16, torch.float16):
        buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=torch.int16, device=dev())
    elif dtype == torch.float32:
        buf = torch.full((rows + 2 * GUARD, cols), SENT32, dtype=torch.int32, device=dev())
    else:
        buf = torch.full((rows + 2 * GUARD, cols), -1, dtype=torch.int32, device=dev())
    return buf, buf.view(dtype)[GUARD:GUARD + rows]


def _scalars(n=8):
    return torch.full((n,), SENT32, dtype=torch.int32, device=dev())


def _stats(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())


def _digest(t, rows):
    """{"all": SHA-256 of the bytes, "rows": the first 64 bits of each row's}: t is split into ``rows`` equal rows."""
    b = t.contiguous().view(torch.uint8).cpu().numpy().reshape(rows, -1)
    return {"all": hashlib.sha256(b.tobytes()).hexdigest(), "rows": [hashlib.sha256(r.tobytes()).hexdigest()[:16] for r in b]}


def _inputs_digest(tensors, params):
    h = hashlib.sha256(repr(params).encode())
    for t in tensors:
        if t is not None:
            h.update(repr((str(t.dtype), tuple(t.shape))).encode())
            h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _same(a, b, what):
    assert a == b, f"{what}: the gradient written over the logits differs from the out-of-place one in rows " \
                   f"{[i for i, (x, y) in enumerate(zip(a['rows'], b['rows'])) if x != y]} (guard rows included)"


def _backward(call, s, rows, dtype, inplace):
    """Runs call(S pointer, G pointer) into a guarded buffer -> its digest; in place as well where asked."""
    buf, g = _sentinel(rows, s.shape[-1], dtype)
    call(s.data_ptr(), g.data_ptr())
    torch.cuda.synchronize()
    d = _digest(buf, rows + 2 * GUARD)
    if inplace:
        buf2, g2 = _sentinel(rows, s.shape[-1], dtype)
        g2.copy_(s.reshape(rows, -1))
        call(g2.data_ptr(), g2.data_ptr())
        torch.cuda.synchronize()
        _same(_digest(buf2, rows + 2 * GUARD), d, "in place")
    return d


# ------------------------------------------------------------------------------------------------------ the families
# Each returns (inputs digest, {name: whole array}, {name: digest}).
def _run_kd(lib, c):
    s, labels, kw, T, dtype, mask = c["s"], c["labels"], c["kw"], c["T"], c["dtype"], c.get("mask")
    shifted = s.dim() == 3
    R, V = s.numel() // s.shape[-1], s.shape[-1]
    te, tv, ti = kw.get("teacher"), kw.get("top_v"), kw.get("top_i")
    K = 0 if tv is None else tv.shape[-1]
    ins = _inputs_digest([s, labels, te, tv, ti, mask], ("kd", T, P.LOSS_ALPHA, GO))
    sd, ld, go = to_dev(s), to_dev(labels), torch.tensor([GO], dtype=torch.float32, device=dev())
    ted = None if te is None else to_dev(te)
    tvd = None if tv is None else to_dev(tv.to(torch.float16))
    tid = None if ti is None else to_dev(ti.to(torch.int32))
    md = None if mask is None else to_dev(mask.to(torch.uint8))
    stats, out = _stats(lib.sd_kdloss_stats_bytes(R, 1)), _scalars()
    if shifted:
        B, Tl = s.shape[:2]
        rc = lib.sd_kdloss_fwd(sd.data_ptr(), _p(ted), _p(tvd), _p(tid), ld.data_ptr(), _p(md), stats.data_ptr(), out.data_ptr(),
                               B, Tl, V, K, T, P.LOSS_ALPHA, _dt(dtype), _stream())
    else:
        rc = lib.sd_kdloss_fwd_rows(sd.data_ptr(), _p(ted), _p(tvd), _p(tid), ld.data_ptr(), stats.data_ptr(), out.data_ptr(), R,
                                    V, K, T, P.LOSS_ALPHA, _dt(dtype), _stream())
    assert rc == 0, rc

    def bwd(sp, gp):
        if shifted:
            rc = lib.sd_kdloss_bwd(sp, _p(ted), _p(tvd), _p(tid), ld.data_ptr(), stats.data_ptr(), out.data_ptr(), go.data_ptr(),
                                   gp, B, Tl, V, K, T, P.LOSS_ALPHA, _dt(dtype), _stream())
        else:
            rc = lib.sd_kdloss_bwd_rows(sp, _p(ted), _p(tvd), _p(tid), ld.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                        go.data_ptr(), gp, R, V, K, T, P.LOSS_ALPHA, _dt(dtype), _stream())
        assert rc == 0, rc
    grad = _backward(bwd, sd, R, dtype, c.get("inplace", False))
    return ins, {"loss_out": out.cpu().numpy()}, {"stats": _digest(stats, R), "grad": grad}


def _run_ce(lib, c):
    s, labels, dtype, div = c["s"], c["labels"], c["dtype"], c["divisor"]
    R, V = s.shape
    ins = _inputs_digest([s, labels], ("ce", div, GO))
    sd, ld, go = to_dev(s), to_dev(labels), torch.tensor([GO], dtype=torch.float32, device=dev())
    dd = None if div is None else torch.tensor([div], dtype=torch.float32, device=dev())
    stats, out = _stats(lib.sd_celoss_stats_bytes(R)), _scalars(4)
    rc = lib.sd_celoss_fwd_rows(sd.data_ptr(), ld.data_ptr(), _p(dd), stats.data_ptr(), out.data_ptr(), R, V, _dt(dtype), _stream())
    assert rc == 0, rc

    def bwd(sp, gp):
        rc = lib.sd_celoss_bwd_rows(sp, ld.data_ptr(), stats.data_ptr(), out.data_ptr(), go.data_ptr(), gp, R, V, _dt(dtype),
                                    _stream())
        assert rc == 0, rc
    grad = _backward(bwd, sd, R, dtype, c.get("inplace", False))
    return ins, {"loss_out": out.cpu().numpy()}, {"stats": _digest(stats, R), "grad": grad}


def _run_gjsd(lib, c):
    s, t, labels, dtype, (div, beta, T) = c["s"], c["t"], c["labels"], c["dtype"], c["mode"]
    R, V = s.shape
    ins = _inputs_digest([s, t, labels], ("gjsd", div, beta, T, G.GJSD_ALPHA, GO))
    sd, td, ld = to_dev(s), to_dev(t), to_dev(labels)
    go = torch.tensor([GO], dtype=torch.float32, device=dev())
    stats, out = _stats(lib.sd_gjsd_stats_bytes(R)), _scalars()
    rc = lib.sd_gjsd_fwd_rows(sd.data_ptr(), td.data_ptr(), ld.data_ptr(), stats.data_ptr(), out.data_ptr(), R, V, T,
                              G.GJSD_ALPHA, beta, MODE[div], _dt(dtype), _stream())
    assert rc == 0, rc

    def bwd(sp, gp):
        rc = lib.sd_gjsd_bwd_rows(sp, td.data_ptr(), ld.data_ptr(), stats.data_ptr(), out.data_ptr(), go.data_ptr(), gp, R, V, T,
                                  G.GJSD_ALPHA, beta, MODE[div], _dt(dtype), _stream())
        assert rc == 0, rc
    grad = _backward(bwd, sd, R, dtype, c.get("inplace", False))
    return ins, {"loss_out": out.cpu().numpy()}, {"stats": _digest(stats, R), "grad": grad}


def _run_sparse(lib, c):
    """sd_gjsd_topk_*_rows (c["div"] None) or sd_gjsd_tail_*_rows (c["div"]: the SD_DIV_* mode, c["tau"] the tails)."""
    s, tv, ti, tau, labels, dtype, (beta, T), div = c["s"], c["tv"], c["ti"], c.get("tau"), c["labels"], c["dtype"], c["mode"], c["div"]
    R, V = s.shape
    K = tv.shape[-1]
    ins = _inputs_digest([s, tv, ti, tau, labels], ("sparse", div, beta, T, TK.ALPHA, GO))
    sd, ld = to_dev(s), to_dev(labels)
    tvd, tid = to_dev(tv.to(torch.float16)), to_dev(ti.to(torch.int32))
    go = torch.tensor([GO], dtype=torch.float32, device=dev())
    out = _scalars()
    if div is None:
        stats = _stats(lib.sd_gjsd_topk_stats_bytes(R))
        rc = lib.sd_gjsd_topk_fwd_rows(sd.data_ptr(), tvd.data_ptr(), tid.data_ptr(), ld.data_ptr(), stats.data_ptr(),
                                       out.data_ptr(), R, V, K, T, TK.ALPHA, beta, _dt(dtype), _stream())
    else:
        taud = to_dev(tau.to(torch.float32))
        stats = _stats(lib.sd_gjsd_tail_stats_bytes(R))
        rc = lib.sd_gjsd_tail_fwd_rows(sd.data_ptr(), tvd.data_ptr(), tid.data_ptr(), taud.data_ptr(), ld.data_ptr(),
                                       stats.data_ptr(), out.data_ptr(), R, V, K, T, TK.ALPHA, beta, div, _dt(dtype), _stream())
    assert rc == 0, rc

    def bwd(sp, gp):
        if div is None:
            rc = lib.sd_gjsd_topk_bwd_rows(sp, tvd.data_ptr(), tid.data_ptr(), ld.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                           go.data_ptr(), gp, R, V, K, T, TK.ALPHA, beta, _dt(dtype), _stream())
        else:
            rc = lib.sd_gjsd_tail_bwd_rows(sp, tvd.data_ptr(), tid.data_ptr(), taud.data_ptr(), ld.data_ptr(), stats.data_ptr(),
                                           out.data_ptr(), go.data_ptr(), gp, R, V, K, T, TK.ALPHA, beta, div, _dt(dtype),
                                           _stream())
        assert rc == 0, rc
    grad = _backward(bwd, sd, R, dtype, c.get("inplace", False))
    return ins, {"loss_out": out.cpu().numpy()}, {"stats": _digest(stats, R), "grad": grad}


def _run_topk(lib, c):
    from speech_distill_amd import _lib
    tc, dtype, nt = P.TOPK_CASES[c["name"]], c["dtype"], c["nt"]
    x = tc["make"](dtype)
    rows, Vt = x.shape
    V, K = Vt if tc["vocab"] is None else tc["vocab"], tc["K"]
    ins = _inputs_digest([x], ("topk", V, K, nt))
    xd = to_dev(x)
    (vb, v), (ib, i), (lb, lse) = _sentinel(rows, K, torch.float16), _sentinel(rows, K, torch.int32), _sentinel(rows, 1, F32)
    before = _lib.debug_get("topk.nt")
    try:
        _lib.debug_set("topk.nt", nt)
        rc = lib.sd_logsoftmax_topk(xd.data_ptr(), v.data_ptr(), i.data_ptr(), lse.data_ptr(), rows, Vt, V, K, _dt(dtype),
                                    _stream())
        torch.cuda.synchronize()
    finally:
        _lib.debug_set("topk.nt", before)
    assert rc == 0, rc
    return ins, {"values": vb.cpu().numpy(), "indices": ib.cpu().numpy(), "lse": lb.cpu().numpy()}, {}


# ------------------------------------------------------------------------------------------------------ the cases
# name -> (runner, function that builds the case's CPU inputs)
INPLACE = ("kd_bf16_T2_100", "kd_fp32_T3_dense", "ce_V40008_bf16_mean", "gjsd_table_V40008_bf16_jsd_b0.5_T2",
           "gjsd_table_V40008_fp32_reverse_kl_T3")


def _kd_case(V, dtype, T, te):
    return lambda: dict(s=P.loss_inputs(V, dtype)[0], labels=P.loss_labels(V, dtype), kw=P.loss_case_teacher(V, dtype, te), T=T,
                        dtype=dtype)


def _kd_extra(dtype, T, extra):
    def make():
        tv, ti, labels = P.sparse_extras(P.LOSS_V, dtype)[extra]
        return dict(s=P.loss_inputs(P.LOSS_V, dtype)[0], labels=labels, kw=dict(top_v=tv, top_i=ti), T=T, dtype=dtype)
    return make


def _kd_shifted(form, dtype, T):
    """The "general" layout of test_loss_shifted_entry_equals_rows_entry: B = 2, T = 5, rows 1, 2, 3, 5, 7 valid."""
    def make():
        from oracle import distill_loss as L
        Bn, Tl, V, K = 2, 5, P.LOSS_V, 100
        gen = torch.Generator().manual_seed(77)
        s = torch.randn(Bn, Tl, V, generator=gen) * 3
        t = torch.randn(Bn, Tl, V, generator=gen) * 3
        labels = torch.randint(0, V, (Bn, Tl), generator=gen)
        sm = torch.ones(Bn, Tl, dtype=torch.uint8)
        labels[0, 1] = -100
        sm[1, 2] = 0
        labels[1, 4] = -100
        if form == "dense":
            kw = dict(teacher=t.to(dtype))
        else:
            tv, ti = L.extract_topk(t, K)
            ti[0, 1, 3] = int(labels[0, 2])  # a hit in row 1
            kw = dict(top_v=tv, top_i=ti)
        return dict(s=s.to(dtype), labels=labels, kw=kw, T=T, dtype=dtype, mask=sm)
    return make


def _ce_case(V, dtype, div):
    return lambda: dict(s=P.loss_inputs(V, dtype)[0], labels=P.loss_labels(V, dtype), dtype=dtype, divisor=div)


def _gjsd_case(family, V, dtype, mode):
    def make():
        s, t, labels = G.FAMILIES[family](V, dtype)
        return dict(s=s, t=t, labels=labels, dtype=dtype, mode=mode)
    return make


def _cases():
    c = {}
    for name, V, dtype, T, te in P.LOSS_CASES + P.LOSS_EDGE_CASES:
        c["kd_" + name] = (_run_kd, _kd_case(V, dtype, T, te))
    for dtype, T in ((BF, 2.0), (F32, 3.0)):
        for extra in ("duplicates", "ends", "no_hit"):
            c[f"kd_{extra}_{_dt_name(dtype)}_T{T:g}"] = (_run_kd, _kd_extra(dtype, T, extra))
    c["kd_shifted_dense_bf16_T2"] = (_run_kd, _kd_shifted("dense", BF, 2.0))
    c["kd_shifted_sparse_fp32_T3"] = (_run_kd, _kd_shifted("sparse", F32, 3.0))
    for dtype in (BF, F32):
        for V in (P.LOSS_V,) + EDGE_V:
            for div, tag in ((None, "mean"), (5.0, "divisor")):
                c[f"ce_V{V}_{_dt_name(dtype)}_{tag}"] = (_run_ce, _ce_case(V, dtype, div))
    for family in ("table", "near", "underflow"):
        for V, dtype, mode in G.family_cases(family):
            c[f"gjsd_{family}_V{V}_{_dt_name(dtype)}_{G.mode_id(mode)}"] = (_run_gjsd, _gjsd_case(family, V, dtype, mode))
    for name, dtype, nt in P.topk_case_list((256, 512, 1024)):
        c[f"topk_{name}_{_dt_name(dtype)}_nt{nt}"] = (_run_topk, lambda name=name, dtype=dtype, nt=nt: dict(name=name, dtype=dtype, nt=nt))
    assert all(n in c for n in INPLACE)
    return c


def _sparse_cases():
    """-> (cases, names of the in-place ones).  The in-place inputs are picked by identity: the ref modules cache them."""
    c, inplace = {}, []
    marks = [(TK.table_inputs(TK.TABLE_V, BF), TK.MODES[0]), (TK.table_inputs(TK.TABLE_V, F32, 1024), TK.MODES[0]),
             (TK.extras_inputs(TK.TABLE_V, BF, "duplicates"), TK.MODES[0])]
    marks += [(TL.table_inputs(TL.TABLE_V, BF, TL.MODES[0][1]), TL.MODES[0]),
              (TL.table_inputs(TL.TABLE_V, F32, TL.MODES[0][1], 1024), TL.MODES[0]),
              (TL.extras_inputs(TL.TABLE_V, BF, TL.MODES[0][1], "duplicates"), TL.MODES[0])]

    def add(name, inputs, mode, case):
        c[name] = (_run_sparse, lambda: dict(case, dtype=inputs[0].dtype, mode=mode))
        if any(inputs is i and mode == m for i, m in marks):
            inplace.append(name)

    for family in ("table", "peaked", "underflow"):
        for n, (inputs, mode) in enumerate(TK.family_cases(family)):
            s, tv, ti, labels = inputs
            add(f"tk_{family}_{n:02d}_V{s.shape[1]}_K{tv.shape[1]}_{_dt_name(s.dtype)}_{TK.mode_id(mode)}", inputs, mode,
                dict(s=s, tv=tv, ti=ti, labels=labels, div=None))
        for n, (inputs, mode) in enumerate(TL.family_cases(family)):
            s, tv, ti, tau, labels = inputs
            for d, div in enumerate(TL.DIVERGENCES):   # d: SD_DIV_FORWARD_KL, SD_DIV_REVERSE_KL, SD_DIV_JSD
                add(f"tail_{family}_{n:02d}_V{s.shape[1]}_K{tv.shape[1]}_{_dt_name(s.dtype)}_{TL.case_id(div, mode)}", inputs,
                    mode, dict(s=s, tv=tv, ti=ti, tau=tau, labels=labels, div=d))
    assert len([n for n in inplace if n.startswith("tk_")]) == 3 and len([n for n in inplace if n.startswith("tail_")]) == 9
    return c, tuple(inplace)


CASES = _cases()
SPARSE_CASES, SPARSE_INPLACE = _sparse_cases()
# which recording holds which cases: suffix of digests*.json / arrays*.npz -> cases
SETS = {"": CASES, "_sparse": SPARSE_CASES}
DIGESTS_KEY = "digests.json"   # a set with a suffix keeps its digests inside its arrays*.npz, under this key
_GOLDEN = {}


def _run(lib, name):
    run, make = CASES[name] if name in CASES else SPARSE_CASES[name]
    case = make()
    case["inplace"] = name in INPLACE or name in SPARSE_INPLACE
    return run(lib, case)


def _golden(suffix=""):
    if suffix not in _GOLDEN:
        arrays = np.load(os.path.join(GOLDEN_DIR, f"arrays{suffix}.npz"), allow_pickle=False)
        if suffix:
            digests = json.loads(arrays[DIGESTS_KEY].tobytes())
        else:
            with open(os.path.join(GOLDEN_DIR, "digests.json")) as f:
                digests = json.load(f)
        _GOLDEN[suffix] = (digests, arrays)
    return _GOLDEN[suffix]


# ------------------------------------------------------------------------------------------------------ the tests
def test_the_recording_holds_exactly_these_cases():
    assert not set(CASES) & set(SPARSE_CASES)
    for suffix, cases in SETS.items():
        want, arrays = _golden(suffix)
        assert sorted(want) == sorted(cases)
        assert sorted({k.split("/")[0] for k in arrays.files} - {DIGESTS_KEY}) == sorted(cases)


@pytest.mark.parametrize("name", sorted(CASES) + sorted(SPARSE_CASES))
def test_outputs_equal_the_recorded_ones(lib, name):
    want, want_arrays = _golden("" if name in CASES else "_sparse")
    ins, arrays, digests = _run(lib, name)
    assert ins == want[name]["inputs"], f"{name}: the INPUTS differ from the recording (the seeded generators or the " \
                                        f"case tables moved): this says nothing about the kernels"
    assert sorted(k for k in want_arrays.files if k.startswith(name + "/")) == sorted(f"{name}/{k}" for k in arrays)
    assert sorted(want[name]["digests"]) == sorted(digests)
    bad = []
    for k, got in arrays.items():
        w = want_arrays[f"{name}/{k}"]
        if got.shape != w.shape or got.dtype != w.dtype:
            bad.append((k, "shape"))
        elif not np.array_equal(got, w):
            bad.append((k, "elements", np.argwhere(got != w)[:8].tolist()))
    for k, got in digests.items():
        w = want[name]["digests"][k]
        if got != w:
            bad.append((k, "rows (guard rows included where the buffer has them)",
                        [i for i, (x, y) in enumerate(zip(got["rows"], w["rows"])) if x != y]))
    assert not bad, f"{name}: the KERNEL's output differs from the recorded one (inputs equal): {bad}"


def _record(out_dir, suffix):
    import speech_distill_amd as sda
    lib = sda.load_lib()
    os.makedirs(out_dir, exist_ok=True)
    all_dig, all_arr = {}, {}
    for name in sorted(SETS[suffix]):
        ins, arrays, digests = _run(lib, name)
        all_dig[name] = {"inputs": ins, "digests": digests}
        all_arr.update({f"{name}/{k}": v for k, v in arrays.items()})
    path = os.path.join(out_dir, f"arrays{suffix}.npz")
    if suffix:
        all_arr[DIGESTS_KEY] = np.frombuffer(json.dumps(all_dig, sort_keys=True).encode(), dtype=np.uint8)
    else:
        with open(os.path.join(out_dir, "digests.json"), "w") as f:
            json.dump(all_dig, f, indent=0, sort_keys=True)
            f.write("\n")
    np.savez_compressed(path, **all_arr)
    print("recorded", len(SETS[suffix]), "cases from", sda.lib_path(), os.path.getsize(path), "bytes of arrays")


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--record" and sys.argv[3:] in ([], ["sparse"]):
        _record(sys.argv[2], "_sparse" if sys.argv[3:] else "")
    else:
        sys.exit("usage: python tests/test_gpu_loss_golden.py --record DIR [sparse]")
