"""-m gpu: the attention kernels (speech_distill_amd/csrc/sd_attn.hip) at the places where index logic goes wrong.

Every case runs the forward in both variants (classic and software-pipelined, bit-equal) and one backward through the C
ABI, into output buffers pre-filled with NaN so that a tile the kernels never store cannot pass for a zero, and compares
with tests/attn_ref.py: a plain fp64 statement of the operation and its bf16-storage emulation (the noise model).

Acceptance rule (attn_ref.judge, shown on the CPU by tests/test_attn_ref_cpu.py to reject single-entry mask errors):
  * per (token, head) row of 128, relative to the row's own norm: HIP error <= F_ROW = 2 x the worst emulated row of the
    same 64-token tile (never less than 2 x one bf16 rounding); dQ, dK, dV rows are measured against the fp64 backward
    on the o that side was handed (o is an input of sd_attn_bwd; attn_ref.judge says why);
  * the global max / rms limits of test_gpu_kernels.py::test_attention_fwd_bwd, unchanged;
  * |LSE - fp64 LSE| <= attn_ref.lse_tolerance (a few fp32 ulps of the score magnitude and of |LSE|, plus the fast log).
The ratio "worst HIP row error / (allowance / F_ROW)" of every case goes to the parity log; DESIGN.md section 5a holds
the worst per output.
"""
import pytest
import torch

import attn_ref as A
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

SCALE = 128 ** -0.5
NAN_BITS = 0x7FC1   # a quiet bf16 NaN with a payload, as int16


@pytest.fixture(scope="module")
def lib():
    from speech_distill_amd import _lib
    lib_ = _lib.load_lib()
    yield lib_
    _lib.debug_set("attn.variant", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def nan_bf16(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int16, device=dev()).view(torch.bfloat16)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def fwd_raw(lib, q, k, v, o, lse, kv_len, B, T, Hq, Hkv, scale):
    from speech_distill_amd._lib import check
    check(lib.sd_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), _p(kv_len), q.stride(0),
                          k.stride(0), v.stride(0), o.stride(0), B, T, Hq, Hkv, 128, scale, _stream()), "sd_attn_fwd")


def bwd_raw(lib, q, k, v, o, do, lse, dq, dk, dv, kv_len, B, T, Hq, Hkv, scale, side=None, two=False):
    """Returns the delta scratch: the caller holds it until it has synchronised (the kernels that use it may still be
    queued, on the side stream too)."""
    from speech_distill_amd._lib import check
    assert o.stride(0) == do.stride(0)   # the C ABI has one ldo for both
    delta = torch.full_like(lse, float("nan"))
    args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(),
            dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _p(kv_len), q.stride(0), k.stride(0), v.stride(0), do.stride(0),
            dq.stride(0), dk.stride(0), dv.stride(0), B, T, Hq, Hkv, 128, scale]
    if two:
        check(lib.sd_attn_bwd2(*args, None if side is None else side.cuda_stream, _stream()), "sd_attn_bwd2")
    else:
        check(lib.sd_attn_bwd(*args, _stream()), "sd_attn_bwd")
    return delta


def fwd_both_variants(lib, q, k, v, kv_len, B, T, Hq, Hkv, scale, make_out=None):
    """Classic (attn.variant 1) and pipelined (2) forward into NaN-filled outputs; bit-equal; returns the pipelined pair."""
    from speech_distill_amd import _lib
    outs = []
    try:
        for variant in (1, 2):
            _lib.debug_set("attn.variant", variant)
            if make_out is None:
                o, lse = nan_bf16(B * T, Hq * 128), torch.full((B, Hq, T), float("nan"), device=dev())
            else:
                o, lse = make_out()
            fwd_raw(lib, q, k, v, o, lse, kv_len, B, T, Hq, Hkv, scale)
            torch.cuda.synchronize()
            outs.append((o, lse))
    finally:
        _lib.debug_set("attn.variant", 0)
    assert same_bits(outs[0][0], outs[1][0]), "classic and pipelined forward differ in O"
    assert same_bits(outs[0][1], outs[1][1]), "classic and pipelined forward differ in LSE"
    return outs[1]


def run_hip(lib, inputs, B, T, Hq, Hkv, kv_len, scale):
    """inputs: CPU bf16 (q, k, v, do), contiguous.  -> dict of device tensors o, lse, dq, dk, dv."""
    q, k, v, do = (t.to(dev()).contiguous() for t in inputs)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev())
    o, lse = fwd_both_variants(lib, q, k, v, kl, B, T, Hq, Hkv, scale)
    dq, dk, dv = nan_bf16(B * T, Hq * 128), nan_bf16(B * T, Hkv * 128), nan_bf16(B * T, Hkv * 128)
    delta = bwd_raw(lib, q, k, v, o, do, lse, dq, dk, dv, kl, B, T, Hq, Hkv, scale)
    torch.cuda.synchronize()
    del delta
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def check_case(name, lib, inputs, B, T, Hq, Hkv, kv_len=None, scale=SCALE, per_row=("o", "dq", "dk", "dv"), rms_budget=()):
    got = run_hip(lib, inputs, B, T, Hq, Hkv, kv_len, scale)
    q, k, v, do = inputs
    ref = A.attn_ref(q, k, v, do, B, T, Hq, Hkv, kv_len, scale)
    emu = A.attn_ref(q, k, v, do, B, T, Hq, Hkv, kv_len, scale, emulate=True)
    tol = A.lse_tolerance(q, k, ref["lse"], B, T, Hq, Hkv, scale)
    # the backward is an operator on the o it is handed: per-row, each side against the reference on its own o (judge)
    ref_g = A.attn_ref(q, k, v, do, B, T, Hq, Hkv, kv_len, scale, o_given=got["o"])
    ref_e = A.attn_ref(q, k, v, do, B, T, Hq, Hkv, kv_len, scale, o_given=emu["o"])
    res = A.judge(got, ref, emu, ref_g, ref_e, B, T, tol, per_row, rms_budget)
    for n, r in res.items():
        record(f"attn_edges_{name}_{n}", **r)
        print(f"attn_edges_{name}_{n}", r)
    assert not A.rejected(res), f"{name}: {({n: res[n] for n in A.rejected(res)})}"
    if kv_len is not None:   # padded keys receive no gradient: written, and written as zeros
        pad = (torch.arange(T)[None, :] >= A.clamp_kv_len(kv_len, B, T)[:, None]).reshape(B * T).to(dev())
        assert (got["dk"][pad].float() == 0).all() and (got["dv"][pad].float() == 0).all(), f"{name}: dK / dV of padded keys"
    return got, res


# ------------------------------------------------------------------------------------------- 1. per-row parity, randn
@pytest.mark.parametrize("B,T,Hq,Hkv", [(4, 512, 16, 8), (1, 2048, 4, 2), (2, 330, 4, 2), (3, 72, 8, 8), (1, 40, 2, 1),
                                        (2, 200, 2, 1)])
def test_per_row_parity_randn(lib, B, T, Hq, Hkv):
    check_case(f"randn_B{B}T{T}H{Hq}/{Hkv}", lib, A.randn_inputs(B, T, Hq, Hkv, seed=1000 + T + Hq), B, T, Hq, Hkv)


# ---------------------------------------------------------------------------------------------------- 2. kv_len grid
KV_CASES = [(T, Hq, Hkv, i, kl) for T in (64, 65, 200, 512) for Hq, Hkv in ((4, 2), (2, 2))
            for i, kl in enumerate(A.kv_launches(T))]   # coverage of the set: test_attn_ref_cpu.py


@pytest.mark.parametrize("T,Hq,Hkv,i,kv_len", KV_CASES)
def test_kv_len_grid(lib, T, Hq, Hkv, i, kv_len):
    """Padding that covers whole K/V tiles, kv_len = 1 (waves all of whose keys are masked), kv_len on and next to the
    32- and 64-key boundaries.  Query rows >= kv_len are defined (they see the keys below kv_len) and are checked like
    any other row."""
    check_case(f"kvlen_T{T}H{Hq}/{Hkv}_{i}", lib, A.randn_inputs(8, T, Hq, Hkv, seed=2000 + T + Hq + i), 8, T, Hq, Hkv, kv_len)


# ------------------------------------------------------------------------------------------- 3. poison invariance
@pytest.mark.parametrize("B,T,Hq,Hkv,kv_len", [(8, T, Hq, Hkv, kl) for T, Hq, Hkv, i, kl in KV_CASES]
                         + [(4, 512, 16, 8, (512, 300, 64, 1))])
def test_masked_keys_have_no_influence(lib, B, T, Hq, Hkv, kv_len):
    """Bit-exact, no tolerance: O, LSE, dQ of all rows and dK, dV of the keys below kv_len do not depend on what the
    masked key rows hold (large finite values; see attn_ref.poison for why finite)."""
    q, k, v, do = A.randn_inputs(B, T, Hq, Hkv, seed=3000 + T + Hq)
    kp, vp = A.poison(k, v, B, T, kv_len)
    clean = run_hip(lib, (q, k, v, do), B, T, Hq, Hkv, kv_len, SCALE)
    dirty = run_hip(lib, (q, kp, vp, do), B, T, Hq, Hkv, kv_len, SCALE)
    live = (torch.arange(T)[None, :] < A.clamp_kv_len(kv_len, B, T)[:, None]).reshape(B * T).to(dev())
    for n in A.NAMES:
        assert torch.isfinite(dirty[n].float()).all(), n
        a, b = (clean[n], dirty[n]) if n in ("o", "lse", "dq") else (clean[n][live], dirty[n][live])
        assert same_bits(a.contiguous(), b.contiguous()), f"{n} depends on masked keys"
    assert (dirty["dk"][~live].float() == 0).all() and (dirty["dv"][~live].float() == 0).all()


# -------------------------------------------------------------------------------------------------------- 4. ramps
RAMP_CASES = [(B, T, Hq, Hkv, kl, sign, step)
              for B, T, Hq, Hkv, kl in ((1, 512, 4, 2, None), (2, 330, 4, 2, None), (2, 330, 4, 2, (330, 97)))
              for sign in (+1, -1) for step in (0.25, 1.0)] + [(1, 2048, 2, 1, None, s, 0.25) for s in (+1, -1)]


@pytest.mark.parametrize("B,T,Hq,Hkv,kv_len,sign,step", RAMP_CASES)
def test_ramps(lib, B, T, Hq, Hkv, kv_len, sign, step):
    """score(i, j) = sign * step * j nats (attn_ref.ramp_inputs): logits of tens to hundreds, a running maximum that moves
    in every tile (rising), exp2 underflow of whole tiles (falling), exp2(s*c - lse2) at |lse| of hundreds in the backward.
    Rising, any leak of a future or padded key takes the row over.  P is almost one-hot here, dQ / dK rows nearly cancel
    (the emulation's worst row is 0.1 - 0.2), so the per-row rule holds O and dV and the global rule holds dQ and dK; the
    rms limit of dQ follows the emulation where the emulation itself exceeds 6e-3, which it does on the rising ramps
    (attn_ref.judge; "rms_widened" in the parity log)."""
    name = f"ramp{'+' if sign > 0 else '-'}{step}_B{B}T{T}{'p' if kv_len else ''}"
    check_case(name, lib, A.ramp_inputs(B, T, Hq, Hkv, 4000 + T, sign, step), B, T, Hq, Hkv, kv_len,
               per_row=("o", "dv"), rms_budget=("dq",))


def test_large_scale_through_the_raw_entry(lib):
    """scale is an argument of the C ABI that ops.attn_* never varies: randn inputs with scale 0.5, scores ~ N(0, 5.7^2)."""
    B, T, Hq, Hkv = 2, 330, 4, 2
    check_case("scale0.5_B2T330", lib, A.randn_inputs(B, T, Hq, Hkv, seed=4500), B, T, Hq, Hkv, (330, 97), scale=0.5,
               per_row=("o", "dv"))


# ---------------------------------------------------------------------- 5. fused-buffer strides and unwritten output
@pytest.mark.parametrize("B,T,Hq,Hkv,kv_len", [(2, 330, 4, 2, None), (3, 72, 8, 8, (72, 41, 9)), (2, 330, 4, 2, (64, 300))])
def test_fused_buffer_strides_and_spare_memory(lib, B, T, Hq, Hkv, kv_len):
    """The runner's layout: q / k / v are column slices of one [M, (Hq+2Hkv)*128] buffer, o / do have a row stride of
    Hq*128 + 128, dq / dk / dv are column slices of one dqkv buffer with a spare 128-column block and 64 spare rows, every
    output pre-filled with a NaN pattern.  Equal to the contiguous call bit for bit; everything inside was written
    (finite); everything spare still holds the fill.  Odd pair count and a ragged last tile."""
    M, W = B * T, (Hq + 2 * Hkv) * 128
    q, k, v, do = A.randn_inputs(B, T, Hq, Hkv, seed=5000 + T)
    want = run_hip(lib, (q, k, v, do), B, T, Hq, Hkv, kv_len, SCALE)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev())
    qkv = torch.cat([q, k, v], 1).to(dev())
    qs, ks, vs = qkv[:, :Hq * 128], qkv[:, Hq * 128:(Hq + Hkv) * 128], qkv[:, (Hq + Hkv) * 128:]
    obufs = []

    def make_out():
        obuf = nan_bf16(M + 64, Hq * 128 + 128)
        lbuf = torch.full((B * Hq * T + 64,), float("nan"), device=dev())
        obufs.append((obuf, lbuf))
        return obuf[:M, :Hq * 128], lbuf[:B * Hq * T].view(B, Hq, T)

    o, lse = fwd_both_variants(lib, qs, ks, vs, kl, B, T, Hq, Hkv, SCALE, make_out)
    assert same_bits(o.contiguous(), want["o"]) and same_bits(lse, want["lse"])
    for obuf, lbuf in obufs:
        assert (bits(obuf)[M:] == NAN_BITS).all() and (bits(obuf)[:, Hq * 128:] == NAN_BITS).all(), "forward wrote outside o"
        assert torch.isnan(lbuf[B * Hq * T:]).all(), "forward wrote past lse"
        assert torch.isfinite(obuf[:M, :Hq * 128].float()).all() and torch.isfinite(lbuf[:B * Hq * T]).all()
    dobuf = nan_bf16(M + 64, Hq * 128 + 128)
    dobuf[:M, :Hq * 128] = do.to(dev())
    dqkv = nan_bf16(M + 64, W + 128)
    dq, dk, dv = dqkv[:M, :Hq * 128], dqkv[:M, Hq * 128:(Hq + Hkv) * 128], dqkv[:M, (Hq + Hkv) * 128:W]
    delta = bwd_raw(lib, qs, ks, vs, o, dobuf[:M, :Hq * 128], lse, dq, dk, dv, kl, B, T, Hq, Hkv, SCALE)
    torch.cuda.synchronize()
    del delta
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t.float()).all(), f"{n}: an element inside was never written"
        assert same_bits(t.contiguous(), want[n]), f"{n} differs from the contiguous call"
    assert (bits(dqkv)[M:] == NAN_BITS).all() and (bits(dqkv)[:, W:] == NAN_BITS).all(), "backward wrote outside dq/dk/dv"


# ------------------------------------------------------------------------------------------------- 6. side stream
@pytest.mark.parametrize("B,T,Hq,Hkv,kv_len", [(4, 512, 16, 8, None), (2, 200, 8, 4, (193, 77))])
def test_bwd2_side_stream_equals_bwd(lib, B, T, Hq, Hkv, kv_len):
    """sd_attn_bwd2 with the dQ kernel on a second stream equals sd_attn_bwd bit for bit; three repetitions as a race
    screen (the kernels share read-only inputs and the delta scratch the first one fills)."""
    inputs = A.randn_inputs(B, T, Hq, Hkv, seed=6000 + T)
    want = run_hip(lib, inputs, B, T, Hq, Hkv, kv_len, SCALE)
    q, k, v, do = (t.to(dev()) for t in inputs)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev())
    side = torch.cuda.Stream()
    for rep in range(3):
        dq, dk, dv = nan_bf16(B * T, Hq * 128), nan_bf16(B * T, Hkv * 128), nan_bf16(B * T, Hkv * 128)
        torch.cuda.synchronize()
        delta = bwd_raw(lib, q, k, v, want["o"], do, want["lse"], dq, dk, dv, kl, B, T, Hq, Hkv, SCALE, side=side, two=True)
        torch.cuda.synchronize()
        del delta
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert same_bits(t, want[n]), f"{n} differs on repetition {rep}"
