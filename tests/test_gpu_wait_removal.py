"""-m gpu: the launches and waits taken out of the backward chain change no output bit.

  * sd_attn_bwd2 as ONE launch (attn_bwd_kernel: dK/dV and dQ workgroups told apart by blockIdx.x) against the two
    launches on two streams it replaces (sd_hip_debug.h key attn.bwd_split = 1): dQ, dK, dV bit-equal, into buffers
    pre-filled with NaN, with side_stream NULL and non-NULL; and a kernel enqueued on `stream` right behind the call
    sees the final dQ / dK / dV.  The packed entry (sd_attn_bwd_varlen) goes through the same wrapper and gets the same
    comparison.
  * forward (both variants), dQ and dK/dV at T = 64, 192, 512: within the acceptance rule of tests/attn_ref.py (through
    the helpers of test_gpu_attn_edges.py) and bit-equal to tests/golden/attn_wait_removal/*.npy, the outputs of the
    commit before these changes on the same seeded inputs (written by `python tests/test_gpu_wait_removal.py --record DIR`).
"""
import os
import sys

import numpy as np
import pytest
import torch

import attn_ref as A
from conftest import GOLDEN
from gpu_util import dev
from test_gpu_attn_edges import SCALE, bits, bwd_raw, check_case, fwd_raw, nan_bf16, run_hip, same_bits

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(GOLDEN, "attn_wait_removal")
# (B, T, Hq, Hkv, seed): Hkv * B = 8 takes the per-XCD workgroup numbering (T = 64 only: the files stay small), the
# others the natural one with two query heads per kv head
GOLDEN_CASES = {64: (1, 64, 8, 8, 64001), 192: (1, 192, 2, 1, 192001), 512: (1, 512, 2, 1, 512001)}
OUT_NAMES = ("o", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def lib():
    from speech_distill_amd import _lib
    lib_ = _lib.load_lib()
    yield lib_
    _lib.debug_set("reset", 0)


# ------------------------------------------------------------------------------- 1. attention backward: one launch
def _padded(t, pad):
    """The same values in a buffer whose rows are `pad` elements longer than the packed width."""
    if not pad:
        return t.contiguous()
    wide = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _bwd_setup(lib, B, T, Hq, Hkv, kv_len, pad, seed):
    q, k, v, do = (_padded(t.to(dev()), pad) for t in A.randn_inputs(B, T, Hq, Hkv, seed))
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev())
    o = _padded(nan_bf16(B * T, Hq * 128), pad)
    lse = torch.full((B, Hq, T), float("nan"), device=dev())
    fwd_raw(lib, q, k, v, o, lse, kl, B, T, Hq, Hkv, SCALE)
    torch.cuda.synchronize()
    return q, k, v, o, do, lse, kl


def _bwd_once(lib, tensors, B, T, Hq, Hkv, pad, split, side, clone_behind=False):
    """One sd_attn_bwd2 into NaN-filled dQ, dK, dV.  clone_behind: the results are copied by kernels enqueued on the
    call's stream right behind it, with no synchronisation in between, and the copies are returned."""
    from speech_distill_amd import _lib
    q, k, v, o, do, lse, kl = tensors
    outs = [_padded(nan_bf16(B * T, h * 128), pad) for h in (Hq, Hkv, Hkv)]
    _lib.debug_set("attn.bwd_split", split)
    try:
        delta = bwd_raw(lib, q, k, v, o, do, lse, *outs, kl, B, T, Hq, Hkv, SCALE, side=side, two=True)
        if clone_behind:
            outs = [t.clone() for t in outs]
        torch.cuda.synchronize()
    finally:
        _lib.debug_set("attn.bwd_split", 0)
    del delta
    return outs


HEADS = ((2, 1), (4, 2), (3, 3))   # (3, 3): Hkv * B is no multiple of 8 -> natural numbering, padding workgroups
BWD_CASES = ([(1, T, hq, hkv, None, 0) for T in (1, 64, 65, 192, 512) for hq, hkv in HEADS] +
             [(3, 128, hq, hkv, None, 0) for hq, hkv in HEADS] +
             [(4, 512, 16, 8, None, 0),                      # the benchmark's launch: per-XCD numbering, 128 + 256 workgroups
              (3, 128, 4, 2, (128, 70, 128), 0),             # kv_len clipped on one batch row
              (3, 128, 3, 3, (128, 1, 100), 0),
              (2, 192, 4, 2, None, 64), (1, 65, 3, 3, None, 8)])   # row strides larger than the packed width


@pytest.mark.parametrize("B,T,Hq,Hkv,kv_len,pad", BWD_CASES)
def test_attn_bwd_one_launch_equals_two_launches(lib, B, T, Hq, Hkv, kv_len, pad):
    tensors = _bwd_setup(lib, B, T, Hq, Hkv, kv_len, pad, seed=7000 + 13 * T + Hq)
    side = torch.cuda.Stream()
    want = _bwd_once(lib, tensors, B, T, Hq, Hkv, pad, split=1, side=None)
    for t, n in zip(want, ("dq", "dk", "dv")):
        assert not torch.isnan(t.float()).any(), f"two launches left rows of {n} unwritten"
    for split, sd in ((1, side), (0, None), (0, side)):
        got = _bwd_once(lib, tensors, B, T, Hq, Hkv, pad, split=split, side=sd)
        for g, w, n in zip(got, want, ("dq", "dk", "dv")):
            assert not torch.isnan(g.float()).any(), f"{n}: unwritten rows (split={split}, side={sd is not None})"
            assert torch.equal(bits(g.contiguous()), bits(w.contiguous())), f"{n} differs (split={split}, side={sd is not None})"


@pytest.mark.parametrize("with_side", [False, True])
def test_attn_bwd_results_are_ordered_on_the_callers_stream(lib, with_side):
    B, T, Hq, Hkv = 4, 512, 16, 8
    tensors = _bwd_setup(lib, B, T, Hq, Hkv, None, 0, seed=7777)
    side = torch.cuda.Stream() if with_side else None
    want = _bwd_once(lib, tensors, B, T, Hq, Hkv, 0, split=0, side=side)
    got = _bwd_once(lib, tensors, B, T, Hq, Hkv, 0, split=0, side=side, clone_behind=True)
    for g, w, n in zip(got, want, ("dq", "dk", "dv")):
        assert same_bits(g, w), f"a kernel enqueued behind sd_attn_bwd2 did not see the final {n}"


@pytest.mark.parametrize("lens,Hq,Hkv", [((1, 64, 65, 192, 7), 4, 2),      # one tile, ragged, odd tile count, slots past a document
                                          ((512, 130), 3, 3),             # Hkv no multiple of 8: padding workgroups
                                          ((100,) * 5, 16, 8)])           # Hkv = 8: per-XCD numbering
def test_attn_bwd_varlen_one_launch_equals_two_launches(lib, lens, Hq, Hkv):
    """The packed entry goes through the same wrapper: dQ, dK, dV of attn.bwd_split 0 and 1 are bit-equal."""
    from speech_distill_amd import _lib, ops
    M = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev())
    q, k, v, do = (t.to(dev()) for t in A.randn_inputs(1, M, Hq, Hkv, seed=9000 + M + Hq))
    o, lse = ops.attn_fwd_varlen(q, k, v, cu, Hq, Hkv, max_seqlen=max(lens))
    outs = []
    try:
        for split in (1, 0):
            _lib.debug_set("attn.bwd_split", split)
            bufs = [nan_bf16(M, h * 128) for h in (Hq, Hkv, Hkv)]
            ops.attn_bwd_varlen(q, k, v, o, do, lse, cu, Hq, Hkv, max_seqlen=max(lens), dq=bufs[0], dk=bufs[1], dv=bufs[2])
            torch.cuda.synchronize()
            outs.append(bufs)
    finally:
        _lib.debug_set("attn.bwd_split", 0)
    for g, w, n in zip(outs[1], outs[0], ("dq", "dk", "dv")):
        assert not torch.isnan(g.float()).any(), f"{n}: unwritten rows"
        assert same_bits(g, w), f"{n} differs between one launch and two"


# -------------------------------------------------------------------- 2. attention outputs against the parent's
def _golden_inputs(T):
    B, T_, Hq, Hkv, seed = GOLDEN_CASES[T]
    return A.randn_inputs(B, T_, Hq, Hkv, seed), B, Hq, Hkv


def _as_numpy(t):
    return bits(t.contiguous()).cpu().numpy()


@pytest.mark.parametrize("T", sorted(GOLDEN_CASES))
def test_attention_outputs_equal_the_parents(lib, T):
    inputs, B, Hq, Hkv = _golden_inputs(T)
    got, _ = check_case(f"wait_removal_T{T}", lib, inputs, B, T, Hq, Hkv)   # both forward variants, one backward, attn_ref
    for n in OUT_NAMES:
        want = np.load(os.path.join(GOLDEN_DIR, f"T{T}_{n}.npy"), allow_pickle=False)
        assert np.array_equal(_as_numpy(got[n]), want), f"T={T}: {n} differs from the recorded output"


def _record(out_dir):
    from speech_distill_amd import _lib
    lib_ = _lib.load_lib()
    os.makedirs(out_dir, exist_ok=True)
    for T in sorted(GOLDEN_CASES):
        inputs, B, Hq, Hkv = _golden_inputs(T)
        got = run_hip(lib_, inputs, B, T, Hq, Hkv, None, SCALE)
        for n in OUT_NAMES:
            np.save(os.path.join(out_dir, f"T{T}_{n}.npy"), _as_numpy(got[n]))
        print("recorded T =", T)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        _record(sys.argv[2])
    else:
        sys.exit("usage: python tests/test_gpu_wait_removal.py --record DIR")
