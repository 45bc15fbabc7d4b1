"""fp64 references, the per-row acceptance rule and the case tables of tests/test_gpu_loss_topk_optim.py.

TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product).  tests/test_parity_ref_cpu.py shows on the CPU that
the rule rejects each named wrong formula, that it accepts the rounded exact reference, and that every case of the
tables below reaches the kernel path it is named for (``topk_path`` / ``loss_path`` restate the launchers' decisions).

The acceptance rule (``rowwise_close``), per row and per element:
        |got - ref| <= half_ulp(ref) + abs_floor * max|ref_row|
half_ulp is half an ulp of the type the result is STORED in, at the reference value; abs_floor covers the fp32 arithmetic of a correct kernel.  The
floors are not derived from the kernels: each is 4 x the worst per-row error (relative to the row maximum) of the SAME
formula evaluated in fp32 on the CPU against fp64, over the cases of its family (``measure_floors``; the factor covers
v_exp_f32 / __logf being about one ulp looser than libm).
"""
from __future__ import annotations

import collections
import functools
import math

import numpy as np
import torch

from oracle import distill_loss as L

# significand bits (hidden one included) and smallest normal exponent of the types results are stored in.  Half an ulp
# of a stored value in [2^e, 2^(e+1)) is 2^(e - bits): at most 2^-8 |ref| for bf16 and 2^-11 |ref| for fp16, and down to
# half of that at the top of the binade.  (A flat 2^-9 |ref| for bf16 is HALF of the rounding error at the bottom of a
# binade: it rejects the exactly rounded reference, see test_parity_ref_cpu.py.)  fp32 results get no such term.
SIG_BITS = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}


def half_ulp(ref64, out_dtype):
    """Half an ulp of ``out_dtype`` at each reference value: the error of one correct rounding can reach it, never pass it."""
    if out_dtype not in SIG_BITS:
        return torch.zeros_like(ref64)
    bits, emin = SIG_BITS[out_dtype]
    e = torch.frexp(ref64.abs())[1] - 1  # |ref| in [2^e, 2^(e+1))
    h = torch.ldexp(torch.ones_like(ref64), e.clamp_min(emin) - bits)
    return torch.where(ref64 == 0, torch.zeros_like(h), h)  # an exact zero stays an exact zero

# Measured by measure_floors() (fp32 evaluation on the CPU against fp64, worst row over every case of the family,
# relative to the row maximum), and the floor chosen from it (4 x, rounded up to two digits).
LOSS_GRAD_MEASURED = 1.11e-6  # d loss / d logits, oracle/distill_loss.py with acc=float32, LOSS_CASES + LOSS_EDGE_CASES
LOSS_GRAD_FLOOR = 4.5e-6
CE_GRAD_MEASURED = 1.12e-7    # cross-entropy gradient, ce_ref with acc=float32, both dtypes
CE_GRAD_FLOOR = 4.5e-7
TOPK_VAL_MEASURED = 3.56e-7   # x - lse in fp32, all TOPK_CASES (relative to the row's largest |log-prob|)
TOPK_VAL_FLOOR = 1.43e-6
ADAMW_MEASURED = 2.44e-7      # p, m, v of adamw_ref64 with acc=float32, all ADAMW_SETS (relative to the tensor maximum)
ADAMW_FLOOR = 9.8e-7
# scalar losses (total, task, distill, teacher): worst relative error of the fp32 evaluation over every single row and
# every batch of the loss cases, per teacher form (the dense KL sums V cancelling terms); the suite's existing 2e-5 is
# the ceiling.  The cross-entropy loss of ce_ref likewise.
LOSS_SCALAR_MEASURED = {"dense": 2.53e-6, "sparse": 1.47e-6}
LOSS_SCALAR_RTOL = {"dense": 1.02e-5, "sparse": 5.9e-6}
CE_SCALAR_MEASURED = 1.5e-7
CE_SCALAR_RTOL = 6.0e-7
LOSS_SCALAR_ATOL = 1e-6       # as test_loss_full_vocab_vs_oracle: for a loss that is exactly 0 in the reference (no hit)
assert max(LOSS_SCALAR_RTOL.values()) <= 2e-5 and CE_SCALAR_RTOL <= 2e-5


# ------------------------------------------------------------------------------------------------- acceptance
Verdict = collections.namedtuple("Verdict", "ok row col got ref err bound worst_rel")


def rowwise_close(got, ref64, out_dtype, abs_floor):
    """-> Verdict(ok, row, col, got, ref, err, bound, worst_rel).  ``got`` and ``ref64`` have the same shape; the last
    dimension is the row (a 1-D tensor is one row).  (row, col) is the element with the largest err / bound (the first
    non-finite one if there is any); worst_rel = max over rows of max|got - ref| / max|ref_row|."""
    g = torch.as_tensor(got).detach().double().cpu()
    r = torch.as_tensor(ref64).detach().double().cpu()
    assert g.shape == r.shape, (g.shape, r.shape)
    g = g.reshape(-1, g.shape[-1]) if g.dim() else g.reshape(1, 1)
    r = r.reshape(g.shape)
    rmax = r.abs().amax(-1, keepdim=True)
    err = (g - r).abs()
    bound = half_ulp(r, out_dtype) + abs_floor * rmax
    bad = ~(err <= bound)  # NaN compares false: a non-finite result is a failure
    ratio = torch.where(bad & ~torch.isfinite(err), torch.full_like(err, math.inf), err / bound.clamp_min(1e-300))
    flat = int(ratio.argmax())
    row, col = divmod(flat, g.shape[1])
    rel = err.amax(-1, keepdim=True) / rmax.clamp_min(1e-300)
    return Verdict(not bool(bad.any()), row, col, float(g[row, col]), float(r[row, col]), float(err[row, col]),
                   float(bound[row, col]), float(rel.max()))


def scalar_close(got, ref64, rtol, atol=LOSS_SCALAR_ATOL):
    """|got - ref| <= rtol |ref| + atol for every entry -> (ok, worst index, worst relative error)."""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    r = np.asarray(ref64, dtype=np.float64).reshape(-1)
    err = np.abs(g - r)
    ok = bool(np.all(err <= rtol * np.abs(r) + atol))  # NaN compares false
    rel = err / np.maximum(np.abs(r), 1e-300)
    rel = np.where(np.abs(r) > 0, rel, err)
    i = int(np.nanargmax(np.where(np.isfinite(rel), rel, np.inf))) if len(rel) else 0
    return ok, i, float(rel[i])


# ------------------------------------------------------------------------------------------------- AdamW
def adamw_ref64(p, g, m, v, lr, b1, b2, eps, wd, step, sumsq=None, max_norm=0.0, acc=torch.float64):
    """adam1 of sd_optim.hip plus the clip, as mathematics: decoupled weight decay, bias-corrected moments, eps outside
    the square root, the gradient scaled by min(1, max_norm / (sqrt(sumsq) + 1e-6)) when a norm is given and
    max_norm > 0.  -> (p, m, v) in ``acc`` (fp32: every scalar is taken in fp32 too, for the floor measurement)."""
    sc = (lambda x: torch.tensor(float(x), dtype=acc))
    p, g, m, v = (t.to(acc) for t in (p, g, m, v))
    clip = sc(1.0)
    if sumsq is not None and max_norm > 0:
        clip = torch.minimum(sc(1.0), sc(max_norm) / (sc(float(sumsq)).sqrt() + sc(1e-6)))
    g = g * clip
    p = p * (sc(1.0) - sc(lr) * sc(wd))
    m = sc(b1) * m + (sc(1.0) - sc(b1)) * g
    v = sc(b2) * v + (sc(1.0) - sc(b2)) * g * g
    bc1 = sc(1.0) - sc(b1) ** step
    bc2 = sc(1.0) - sc(b2) ** step
    p = p - (sc(lr) / bc1) * (m / (v.sqrt() / bc2.sqrt() + sc(eps)))
    return p, m, v


def adamw_close(got, ref64):
    """(p, m, v) as stored (bf16) against adamw_ref64's triple -> {"p" / "m" / "v": Verdict}; each tensor is one row."""
    return {k: rowwise_close(a, b, torch.bfloat16, ADAMW_FLOOR) for k, a, b in zip("pmv", got, ref64)}


def loss_close(got_losses, got_grad, ref_losses, ref_grad, grad_dtype, form):
    """The acceptance rule of one loss call: the four scalars (scalar_close at the teacher form's bound) and the
    gradient per row (rowwise_close).  -> (ok, text naming the worst scalar and the worst gradient element)."""
    s_ok, i, rel = scalar_close(got_losses, ref_losses, LOSS_SCALAR_RTOL[form])
    v = rowwise_close(got_grad, ref_grad, grad_dtype, LOSS_GRAD_FLOOR)
    return s_ok and v.ok, (f"scalars ok={s_ok} worst={('total', 'task', 'distill', 'teacher')[i % 4]} rel={rel:.3e} "
                           f"(bound {LOSS_SCALAR_RTOL[form]:.1e}); grad {v}")


# hyper-parameter sets shared by the CPU mutant tests and the GPU test.  clip: "none" (no norm given), "zero"
# (max_norm = 0), "below" (norm = max_norm / 2: the clip is exactly 1) or "above" (norm = 2 max_norm).  `kills`: the wrong
# formulas (tests/test_parity_ref_cpu.py) that the comparator must reject on this set; a mutant missing from a set's
# list is mathematically (nearly) identical there: the bias corrections at step 1000, eps = 1e-8 next to sqrt(v) ~ 0.5,
# the clip when it is 1.
_ALL = ("no_wd", "l2_wd", "no_bc1", "no_bc2", "clip_ignored", "clip_m_only", "v_frozen", "m_frozen")
ADAMW_SETS = {
    "step1_above": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=1, clip="above", g_scale=1.0, v0=False, kills=_ALL),
    "step3_above": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=3, clip="above", g_scale=1.0, v0=False, kills=_ALL),
    "step1000_above": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=1000, clip="above", g_scale=1.0, v0=False,
                           kills=("no_wd", "l2_wd", "clip_ignored", "clip_m_only", "v_frozen", "m_frozen")),
    "step3_below": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=3, clip="below", g_scale=1.0, v0=False,
                        kills=("no_wd", "l2_wd", "no_bc1", "no_bc2", "v_frozen", "m_frozen")),
    "step3_zero": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=3, clip="zero", g_scale=1.0, v0=False,
                       kills=("no_wd", "l2_wd", "no_bc1", "no_bc2", "v_frozen", "m_frozen")),
    "step3_none": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-8, step=3, clip="none", g_scale=1.0, v0=False,
                       kills=("no_wd", "l2_wd", "no_bc1", "no_bc2", "v_frozen", "m_frozen")),
    # v = 0 and |g| ~ 1e-2: sqrt(v_hat) ~ 1e-2 next to eps = 1e-2, so where eps sits decides the update
    "eps_v0": dict(lr=0.1, wd=0.5, b1=0.5, b2=0.9, eps=1e-2, step=3, clip="none", g_scale=1e-2, v0=True,
                   kills=("eps_in_sqrt", "no_wd", "l2_wd", "no_bc1", "no_bc2", "v_frozen", "m_frozen")),
}
ADAMW_SIZES = (1, 7, 8, 9, 2055, 4096 * 256 * 8 + 2400 + 5)  # the last: grid-stride wrap (4096 workgroups) plus a tail
ADAMW_BIG_SETS = ("step1_above", "step3_none")                 # the sets run at the largest size


def adamw_inputs(n, set_name):
    """-> p, g, m, v (bf16, CPU) and (sumsq fp32 scalar or None, max_norm) of one set at one size."""
    hp = ADAMW_SETS[set_name]
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    p = torch.randn(n, generator=gen).bfloat16()
    g = (torch.randn(n, generator=gen) * hp["g_scale"]).bfloat16()
    m = (torch.randn(n, generator=gen) * 0.5 * hp["g_scale"]).bfloat16()
    v = torch.zeros(n).bfloat16() if hp["v0"] else (torch.rand(n, generator=gen) * 0.5 + 0.1).bfloat16()
    ss = float(torch.tensor(float(g.double().pow(2).sum()), dtype=torch.float32))  # the fp32 value the kernel reads
    norm = math.sqrt(ss)
    sumsq, max_norm = {"none": (None, 0.0), "zero": (ss, 0.0), "below": (ss, 2.0 * norm + 1.0),
                       "above": (ss, 0.5 * norm)}[hp["clip"]]
    return (p, g, m, v), (sumsq, float(torch.tensor(max_norm, dtype=torch.float32)))


def adamw_hp(set_name):
    hp = ADAMW_SETS[set_name]
    return hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["step"]


# ------------------------------------------------------------------------------------------------- top-K
def f2key(x32):
    """Order-preserving uint32 key of fp32 values (sd_topk.hip f2key)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk_ref(x, K):
    """x [rows, V] (stored values) -> (values fp64 = x - lse, indices int64): ordered by (raw logit descending, index
    ascending) on the exact stored values."""
    x64 = x.double()
    order = torch.sort(x64, dim=-1, descending=True, stable=True).indices[..., :K]
    m = x64.amax(-1, keepdim=True)
    lse = m + (x64 - m).exp().sum(-1, keepdim=True).log()
    return x64.gather(-1, order) - lse, order


TopkPath = collections.namedtuple("TopkPath", "path trips plain_loops nc")
TOPK_CAP = 2048
_TOPK_MAXCH = {512: 40, 1024: 20, 256: 0}


def topk_path(x_row, K, NT, dtype):
    """What topk_kernel<T, NPASS, NT> does with one row: thread t owns the 8-element chunks i NT + t; t0 is the K-th
    largest thread maximum truncated to its top 16 (bf16) / 32 (fp32) key bits; nc counts the keys >= t0.
    -> path "fast", "overflow" (nc > 2048: falls back to the radix select over the whole row) or "general"
    (K > min(NT, V/8): never tries the fast path); trips of the radix select's c0 loop (0 on the fast path);
    plain_loops: the row is too long for the register-resident chunk maxima."""
    x = np.asarray(x_row.float().numpy(), dtype=np.float32)
    V = x.shape[0]
    assert V % 8 == 0
    nch = V // 8
    trips = -(-V // (NT * 8))
    plain = not (_TOPK_MAXCH[NT] > 0 and V <= _TOPK_MAXCH[NT] * NT * 8)
    if K > min(NT, nch):
        return TopkPath("general", trips, plain, None)
    keys = f2key(x)
    cmax = keys.reshape(nch, 8).max(-1)
    tk = np.zeros(NT, dtype=np.uint32)  # a thread without a chunk holds key 0
    for t in range(min(NT, nch)):
        tk[t] = cmax[t::NT].max()
    kth = np.sort(tk)[::-1][K - 1]
    t0 = kth & np.uint32(0xFFFF0000) if dtype == torch.bfloat16 else kth
    nc = int((keys >= t0).sum())
    if nc > TOPK_CAP:
        return TopkPath("overflow", trips, plain, nc)
    return TopkPath("fast", 0, plain, nc)


def _cast(x, dtype):
    return x.to(dtype)


def _topk_ties(dtype):
    """(b): x[:8150] = c - 1, x[8150:] = c, 50 larger distinct values at scattered indices: K = 128 takes those 50 and
    the 78 lowest-indexed ties 8150..8227, which straddle index 8192 (a trip boundary at every NT)."""
    c = 1.0 if dtype == torch.bfloat16 else 1.0 + 2.0 ** -20
    x = torch.full((1, 12288), c - 1.0, dtype=torch.float32)
    x[0, 8150:] = c
    pos = (torch.arange(50) * 241 + 17) % 12288
    pos = torch.where((pos >= 8150) & (pos < 8300), pos + 300, pos)
    x[0, pos] = 2.0 + 0.25 * torch.arange(50) + (0.0 if dtype == torch.bfloat16 else 2.0 ** -18)
    return _cast(x, dtype)


def _topk_randn(rows, V, seed):
    def make(dtype):
        return _cast(torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 3, dtype)
    return make


def _topk_tail(dtype):
    x = torch.randn(3, 4104, generator=torch.Generator().manual_seed(41)) * 3
    x[:, 4096:] = 100.0
    return _cast(x, dtype)


def _topk_mixed(dtype):
    """(g): rows 0 and 3 random (fast), row 1 all equal and row 2 the tie pattern of (b) cut to V = 8192 (overflow)."""
    x = torch.randn(4, 8192, generator=torch.Generator().manual_seed(43)) * 3
    x[1] = 0.5
    x[2] = 0.0
    x[2, 4000:] = 1.0
    x[2, (torch.arange(50) * 161 + 5) % 4000] = 2.0 + 0.25 * torch.arange(50)
    return _cast(x, dtype)


BF, F32 = torch.bfloat16, torch.float32
# name -> dict(make(dtype) -> logits [rows, Vt], dtypes, K, vocab (None = Vt), nt: {NT: [expected path per row]}).
# The direct "general" path is a per-launch decision (K > min(NT, V/8)), so a launch cannot mix it with "fast" rows:
# case (g) mixes fast and overflow rows, and overflow rows run the same radix select.
TOPK_CASES = {
    "a_all_equal": dict(make=lambda dt: _cast(torch.full((1, 8192), 0.25), dt), dtypes=(BF,), K=128, vocab=None,
                        nt={512: ["overflow"], 256: ["overflow"], 1024: ["overflow"]}),
    "b_ties_across_trips": dict(make=_topk_ties, dtypes=(BF, F32), K=128, vocab=None,
                                nt={512: ["overflow"], 256: ["overflow"], 1024: ["overflow"]}),
    "c_plain_loops": dict(make=_topk_randn(2, 163848, 31), dtypes=(BF, F32), K=128, vocab=None, nt={512: ["fast"] * 2}),
    "d_k1": dict(make=_topk_randn(2, 8192, 32), dtypes=(BF, F32), K=1, vocab=None,
                 nt={512: ["fast"] * 2, 256: ["fast"] * 2, 1024: ["fast"] * 2}),
    "d_k513": dict(make=_topk_randn(2, 8192, 33), dtypes=(BF, F32), K=513, vocab=None,
                   nt={512: ["general"] * 2, 256: ["general"] * 2, 1024: ["fast"] * 2}),
    "d_k1024": dict(make=_topk_randn(2, 8192, 34), dtypes=(BF, F32), K=1024, vocab=None,
                    nt={512: ["general"] * 2, 256: ["general"] * 2, 1024: ["overflow"] * 2}),
    "e_v8_k8": dict(make=_topk_randn(3, 8, 35), dtypes=(BF, F32), K=8, vocab=None, nt={512: ["general"] * 3}),
    "f_vocab_tail": dict(make=_topk_tail, dtypes=(BF, F32), K=128, vocab=4096, nt={512: ["fast"] * 3}),
    "g_mixed_rows": dict(make=_topk_mixed, dtypes=(BF, F32), K=128, vocab=None,
                         nt={512: ["fast", "overflow", "overflow", "fast"]}),
}


def topk_case_list(nts=(512,)):
    """[(name, dtype, NT)] for every case that names an expectation at one of ``nts``."""
    return [(n, dt, nt) for n, c in TOPK_CASES.items() for dt in c["dtypes"] for nt in nts if nt in c["nt"]]


# ------------------------------------------------------------------------------------------------- loss
LossPath = collections.namedtuple("LossPath", "dtype t2 nf dense chunks_per_thread")


def loss_path(V, K, dense, temperature, dtype):
    """The kd_fwd_kernel<T, T2, NF, DENSE> instantiation run_fwd launches, and the 8-element chunks per thread
    (V / 8 / NF; the streaming loop keeps four in flight, so > 4 means more than one prefetch trip)."""
    nf = 512 if (dense or K <= 512) else 1024
    return LossPath("bf16" if dtype == torch.bfloat16 else "fp32", float(temperature) == 2.0, nf, bool(dense),
                    (V / 8) / nf)


LOSS_V = 40008
LOSS_ALPHA = 0.3
ROW_KINDS = ("randn", "randn", "randn", "rising", "falling", "spike", "flat", "ignored")
# (name, V, dtype, temperature, teacher): teacher "dense" or the K of a top-K teacher
LOSS_CASES = [(f"{'bf16' if dt == BF else 'fp32'}_T{T:g}_{te}", LOSS_V, dt, T, te)
              for dt in (BF, F32) for T in (2.0, 3.0) for te in ("dense", 100, 513, 1024)]
LOSS_CASES += [("bf16_T1_dense", LOSS_V, BF, 1.0, "dense"), ("fp32_T1_100", LOSS_V, F32, 1.0, 100)]
# vocabulary edges: one chunk in all (V = 8), one chunk per thread, exactly one full prefetch trip, one chunk more
LOSS_EDGE_CASES = [(f"V{V}_{'bf16' if dt == BF else 'fp32'}_{te}", V, dt, T, (te if te == "dense" else (4 if V == 8 else te)))
                   for V in (8, 4096, 16384, 16392) for dt, T in ((BF, 2.0), (F32, 3.0)) for te in ("dense", 100)]
# the 12 instantiations, each with the LOSS_CASES entry that must reach it at more than four chunks per thread
LOSS_INSTANTIATIONS = {(d, t2, nf, dense): f"{d}_T{'2' if t2 else '3'}_{'dense' if dense else (100 if nf == 512 else 513)}"
                       for d in ("bf16", "fp32") for t2 in (True, False) for nf, dense in ((512, True), (512, False), (1024, False))}


@functools.lru_cache(maxsize=None)
def loss_inputs(V, dtype):
    """-> s, t [8, V] in ``dtype`` (CPU) of ROW_KINDS for the student (the teacher rows are random), and the teacher's
    fp32 log-softmax order used to place labels.  Row 7 is the -100 row (its label is set by loss_labels)."""
    gen = torch.Generator().manual_seed(V * 2 + (1 if dtype == BF else 0))
    s = torch.randn(8, V, generator=gen) * 3
    t = torch.randn(8, V, generator=gen) * 3
    s = s.to(dtype)
    s[3] = torch.sort(s[3].float()).values.to(dtype)
    s[4] = torch.sort(s[4].float(), descending=True).values.to(dtype)
    s[5] = (torch.randn(V, generator=gen) * 0.1).to(dtype)
    s[5, (V * 2) // 3] = 60.0
    s[6] = 1.5
    return s, t.to(dtype)


@functools.lru_cache(maxsize=None)
def loss_topk(V, dtype, K):
    """The teacher's top-K as the project extracts it (fp16 log-probs, int32 indices), from the oracle."""
    _, t = loss_inputs(V, dtype)
    return L.extract_topk(t.float(), K)


def loss_labels(V, dtype):
    """Labels that meet the teacher's ranking at both ends whatever K: row 0 the teacher's argmax (top-K position 0), row 1
    its rank min(99, V/2 - 1) (position K - 1 at K = 100, and at V = 8, K = 4), row 2 its argmin (never a hit), row 3 the
    rising row's maximum V - 1, row 4 index 0, row 5 NOT the spike, row 6 mid-row, row 7 ignored."""
    _, t = loss_inputs(V, dtype)
    order = torch.sort(t.float(), dim=-1, descending=True, stable=True).indices
    return torch.tensor([int(order[0, 0]), int(order[1, min(99, V // 2 - 1)]), int(order[2, V - 1]), V - 1, 0, 1, V // 2,
                         -100], dtype=torch.int64)


def oracle_rows(s, labels, teacher=None, top_v=None, top_i=None, temperature=2.0, alpha=0.5, acc=torch.float64):
    """oracle/distill_loss.py on rows already shifted and selected: row r becomes position 0 of a two-position sequence
    whose label sits at position 1.  -> ((total, task, distill, teacher) as floats, N, hits, grad [R, V] in acc)."""
    R, V = s.shape
    pad = (lambda x: None if x is None else torch.stack([x, torch.zeros_like(x)], 1))
    lab = torch.stack([torch.full_like(labels, -100), labels], 1)
    out = L.distill_loss(pad(s.float() if acc == torch.float32 else s.double()), lab,
                         teacher_logits=pad(None if teacher is None else (teacher.float() if acc == torch.float32 else teacher.double())),
                         teacher_top_k_v=pad(top_v), teacher_top_k_i=pad(top_i), temperature=temperature, alpha=alpha,
                         acc=acc, return_grad=True)
    valid = labels != -100
    n = int(valid.sum())
    hits = n if teacher is not None else int((top_i.long() == labels[:, None])[valid].sum())
    return tuple(float(x) for x in out[:4]), n, hits, out[4][:, 0, :]


def ce_ref(s, labels, acc=torch.float64):
    """Mean cross-entropy over the rows whose label is not -100 and its gradient (softmax - e_y) / N.
    -> (loss, per-row losses [R] (0 on ignored rows), N, grad [R, V])."""
    x = s.to(acc)
    valid = labels != -100
    n = int(valid.sum())
    m = x.amax(-1, keepdim=True)
    lse = (m + (x - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)
    y = labels.clamp_min(0)
    rows = torch.where(valid, lse - x.gather(-1, y[:, None]).squeeze(-1), torch.zeros_like(lse))
    g = (x - lse[:, None]).exp()
    g[torch.arange(len(y)), y] -= 1.0
    g = torch.where(valid[:, None], g / max(n, 1), torch.zeros_like(g))
    return float(rows.sum() / max(n, 1)), rows, n, g


def loss_case_teacher(V, dtype, teacher):
    """-> kwargs (CPU tensors) of oracle_rows / forward_rows for one teacher form."""
    if teacher == "dense":
        return dict(teacher=loss_inputs(V, dtype)[1])
    tv, ti = loss_topk(V, dtype, int(teacher))
    return dict(top_v=tv, top_i=ti)


def sparse_extras(V, dtype, K=100):
    """Top-K teachers edited by hand -> {name: (top_v, top_i, labels)}.
    duplicates: row 0 holds one index twice and its LABEL three times, row 3 holds its label twice;
    ends: the label at top-K position 0 (row 0) and K - 1 (row 1);  no_hit: no label among any row's indices."""
    tv, ti = loss_topk(V, dtype, K)
    base = loss_labels(V, dtype)
    out = {}
    i, lab = ti.clone(), base.clone()
    i[0, 6] = i[0, 5]
    i[0, 11] = i[0, 10]
    i[0, 40] = i[0, 10]
    lab[0] = int(i[0, 10])
    i[3, K - 1] = i[3, 0]
    lab[3] = int(i[3, 0])
    out["duplicates"] = (tv, i, lab)
    lab = base.clone()
    lab[0], lab[1] = int(ti[0, 0]), int(ti[1, K - 1])
    for r in range(2, 7):
        lab[r] = _not_in(ti[r], V)
    out["ends"] = (tv, ti, lab)
    lab = base.clone()
    for r in range(7):
        lab[r] = _not_in(ti[r], V)
    out["no_hit"] = (tv, ti, lab)
    return out


def _not_in(idx_row, V):
    have = set(int(x) for x in idx_row)
    return next(c for c in range(V // 3, V) if c not in have)


# ------------------------------------------------------------------------------------------------- floors
def _row_rel(a32, ref64):
    r = ref64.double().reshape(-1, ref64.shape[-1])
    e = (a32.double().reshape(r.shape) - r).abs().amax(-1)
    return float((e / r.abs().amax(-1).clamp_min(1e-300)).max())


def measure_floors(loss_cases=None, topk=True, adamw=True):
    """Worst per-row error, relative to the row maximum, of each formula evaluated in fp32 on the CPU against fp64, on
    the inputs the GPU tests use.  -> dict of the *_MEASURED quantities above."""
    out = dict(loss_grad=0.0, loss_scalar_dense=0.0, loss_scalar_sparse=0.0, ce_grad=0.0, ce_scalar=0.0, topk_val=0.0, adamw=0.0)
    for name, V, dt, T, te in (LOSS_CASES + LOSS_EDGE_CASES if loss_cases is None else loss_cases):
        s, _ = loss_inputs(V, dt)
        labels = loss_labels(V, dt)
        kw = loss_case_teacher(V, dt, te)
        l64, _, _, g64 = oracle_rows(s, labels, temperature=T, alpha=LOSS_ALPHA, **kw)
        l32, _, _, g32 = oracle_rows(s, labels, temperature=T, alpha=LOSS_ALPHA, acc=torch.float32, **kw)
        valid = labels != -100
        out["loss_grad"] = max(out["loss_grad"], _row_rel(g32[valid], g64[valid]))
        pairs = [(l32, l64)]
        for r in range(7):
            kr = {k: v[r:r + 1] for k, v in kw.items()}
            pairs.append((oracle_rows(s[r:r + 1], labels[r:r + 1], temperature=T, alpha=LOSS_ALPHA, acc=torch.float32, **kr)[0],
                          oracle_rows(s[r:r + 1], labels[r:r + 1], temperature=T, alpha=LOSS_ALPHA, **kr)[0]))
        for a, b in pairs:
            for x, y in zip(a, b):
                if y != 0.0:
                    fam = "loss_scalar_dense" if te == "dense" else "loss_scalar_sparse"
                    out[fam] = max(out[fam], abs(x - y) / abs(y))
    for dt in (BF, F32):
        s, _ = loss_inputs(LOSS_V, dt)
        labels = loss_labels(LOSS_V, dt)
        valid = labels != -100
        c32, c64 = ce_ref(s, labels, torch.float32), ce_ref(s, labels)
        out["ce_grad"] = max(out["ce_grad"], _row_rel(c32[3][valid], c64[3][valid]))
        rel = ((c32[1].double() - c64[1]).abs() / c64[1].abs().clamp_min(1e-300))[valid]
        out["ce_scalar"] = max(out["ce_scalar"], float(rel.max()), abs(c32[0] - c64[0]) / abs(c64[0]))
    if topk:
        for name, dt, _ in topk_case_list():
            c = TOPK_CASES[name]
            x = c["make"](dt)
            x = x if c["vocab"] is None else x[:, :c["vocab"]]
            v64, idx = topk_ref(x, c["K"])
            x32 = x.float()
            m = x32.amax(-1, keepdim=True)
            lse32 = m + (x32 - m).exp().sum(-1, keepdim=True).log()
            out["topk_val"] = max(out["topk_val"], _row_rel(x32.gather(-1, idx) - lse32, v64))
    if adamw:
        for sname in ADAMW_SETS:
            for n in (2055, 1 << 20):
                (p, g, m, v), (ss, mx) = adamw_inputs(n, sname)
                r64 = adamw_ref64(p, g, m, v, *adamw_hp(sname), sumsq=ss, max_norm=mx)
                r32 = adamw_ref64(p, g, m, v, *adamw_hp(sname), sumsq=ss, max_norm=mx, acc=torch.float32)
                for a, b in zip(r32, r64):
                    out["adamw"] = max(out["adamw"], _row_rel(a, b))
    return out
