"""CPU checks of the "wide" decode mode (sd_gemv_wide_bf16 / sd_gemv_wide_swiglu / sd_qwen3_decode_step_wide;
include/sd_hip.h "wide weight-streaming GEMV", generation.py): every error code of the three new entries is decided before
a launch, so it comes back on a machine without a GPU; the size query answers; the keyword is accepted, and refused with
MXFP8 weights before anything is allocated."""
import ctypes

import pytest
import torch

SHAPE, UNSUP, WORK = -1, -3, -5
P, BIG = 0x10000, 1 << 40


def _lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def test_wide_gemv_refusals_without_a_gpu():
    lib = _lib()

    def gemv(x=P, w=P, y=P, r=None, gain=None, M=1, N=16, K=128, ldx=None, ldw=None, ldy=None, ldr=0):
        return lib.sd_gemv_wide_bf16(x, w, y, r, gain, 1e-6, M, N, K, K if ldx is None else ldx, K if ldw is None else ldw,
                                     N if ldy is None else ldy, ldr, None)

    assert gemv(M=0) == SHAPE and gemv(M=-1) == SHAPE and gemv(N=0) == SHAPE
    assert gemv(x=None) == SHAPE and gemv(w=None) == SHAPE and gemv(y=None) == SHAPE
    assert gemv(M=65) == UNSUP and gemv(K=48) == UNSUP and gemv(K=8224) == UNSUP
    assert gemv(K=8192, gain=P) == UNSUP                                   # a norm stops at K = 4096
    assert gemv(x=P + 8) == UNSUP and gemv(w=P + 2) == UNSUP and gemv(gain=P + 4) == UNSUP   # misaligned rows
    assert gemv(ldx=132) == UNSUP and gemv(ldw=129) == UNSUP               # row strides that break the 16-byte alignment
    assert gemv(ldx=96) == UNSUP and gemv(ldy=8) == UNSUP and gemv(r=P, ldr=8) == UNSUP      # strides below the row length

    def swiglu(x=P, w=P, act=P, gain=None, M=1, I=16, K=128):
        return lib.sd_gemv_wide_swiglu(x, w, act, gain, 1e-6, M, I, K, None)

    assert swiglu(M=0) == SHAPE and swiglu(x=None) == SHAPE and swiglu(w=None) == SHAPE and swiglu(act=None) == SHAPE
    assert swiglu(M=65) == UNSUP and swiglu(K=48) == UNSUP and swiglu(K=8224) == UNSUP
    assert swiglu(K=8192, gain=P) == UNSUP and swiglu(x=P + 8) == UNSUP


def test_wide_step_refuses_before_any_launch():
    """The codes of sd_qwen3_mx_decode_step: SD_ERR_SHAPE for NULL arguments, non-positive sizes or an unknown cache kind,
    SD_ERR_WORKSPACE for short buffers, SD_ERR_UNSUPPORTED for dims the cache kernels do not take."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.Params())
    pages = L.KvPages(P, BIG, P, 8, 2)

    def ref(kind=0, cache=P, nbytes=BIG, cap=256, pg=None):
        return ctypes.byref(L.KvRef(kind, cache, nbytes, cap, ctypes.pointer(pg) if pg is not None else None))

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8):
        return lib.sd_qwen3_decode_step_wide(d, p, ids, pos, max_len, P, P, kv, acts, nb, logits, B, None)

    assert step(None) == SHAPE and step(ref(), d=None) == SHAPE and step(ref(), p=None) == SHAPE
    assert step(ref(kind=3)) == SHAPE and step(ref(kind=-1)) == SHAPE
    assert step(ref(cache=None)) == SHAPE and step(ref(cap=0)) == SHAPE
    assert step(ref(kind=1)) == SHAPE and step(ref(kind=2)) == SHAPE                   # paged kinds need the pages
    assert step(ref(), B=0) == SHAPE and step(ref(), ids=None) == SHAPE and step(ref(), pos=None) == SHAPE
    assert step(ref(), logits=None) == SHAPE and step(ref(), acts=None) == SHAPE and step(ref(), max_len=0) == SHAPE
    assert step(ref(nbytes=16)) == WORK and step(ref(), nb=16) == WORK
    assert step(ref(), B=65, nb=16) == WORK                                            # beyond the wide range: still checked
    for kind in (1, 2):
        assert step(ref(kind=kind, pg=pages), nb=16) == WORK                           # a valid pool gets as far
        assert step(ref(kind=kind, pg=L.KvPages(P, 16, P, 8, 2))) == WORK
        assert step(ref(kind=kind, pg=L.KvPages(P, BIG, None, 8, 2))) == SHAPE
    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g8 = ctypes.byref(L.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))                 # 8 query heads per kv head
    assert step(ref(), d=hd64) == UNSUP and step(ref(), d=g8) == UNSUP


def test_wide_acts_bytes_is_monotone_in_the_batch():
    from speech_distill_amd import _lib as L
    lib = _lib()
    d = ctypes.byref(L.Dims(159488, 2048, 6144, 28, 16, 8, 128, 1, 1e-6, 0))
    sizes = [lib.sd_qwen3_decode_step_wide_acts_bytes(d, B, 1024) for B in (1, 2, 16, 17, 33, 64, 65)]
    assert sizes[0] > lib.sd_attn_decode_workspace_bytes(1, 16, 1024) > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.sd_qwen3_decode_step_wide_acts_bytes(d, 0, 1024) == SHAPE
    assert lib.sd_qwen3_decode_step_wide_acts_bytes(d, 4, 0) == SHAPE
    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    assert lib.sd_qwen3_decode_step_wide_acts_bytes(hd64, 4, 256) == UNSUP


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


def test_wide_is_a_decode_kernels_value_and_refuses_mxfp8_weights():
    from speech_distill_amd import generation as G
    assert "wide" in G.DECODE_KERNELS and G.DECODE_KERNELS[:2] == ("tile", "skinny")
    G._check_decode_kernels("wide")
    G._check_decode_kernels("skinny", "mxfp8")
    with pytest.raises(ValueError, match="decode_kernels"):
        G._check_decode_kernels("fat")
    ids = torch.zeros(1, 4, dtype=torch.int64)
    m = _cpu_model().requires_grad_(False)
    for call in (lambda: m.generate(ids, max_new_tokens=2, do_sample=False, decode_kernels="wide", weight_dtype="mxfp8"),
                 lambda: m.start_session(1, capacity=256, decode_kernels="wide", weight_dtype="mxfp8"),
                 lambda: G.Decoder(m, 1, 256, decode_kernels="wide", weight_dtype="mxfp8"),
                 lambda: m.generation_engine(object(), max_batch=20, decode_kernels="wide", weight_dtype="mxfp8")):
        with pytest.raises(ValueError, match="wide"):
            call()
    # with bf16 weights the keyword passes every check and gets as far as the CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(ids, max_new_tokens=2, do_sample=False, decode_kernels="wide")
