"""CPU checks of the 64-row MXFP8 decode mode (sd_gemv_mxfp8_wide / sd_gemv_mxfp8_wide_swiglu / sd_qwen3_mx_decode_step_wide;
include/sd_hip.h "wide weight-streaming GEMV over MXFP8 weights", generation.py ``gemv_rows``): every error code of the three
entries is decided before a launch, so it comes back on a machine without a GPU; the size query answers; ``gemv_rows``
defaults to 16 everywhere, and every combination the interface refuses raises ValueError on a CPU model, before anything
is allocated (a CPU model would otherwise fail with "no CPU fallback")."""
import ctypes
import inspect

import pytest
import torch

SHAPE, UNSUP, WORK = -1, -3, -5
P, BIG = 0x10000, 1 << 40


def _lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def test_mx_wide_gemv_refusals_without_a_gpu():
    lib = _lib()

    def gemv(x=P, wq=P, ws=P, y=P, r=None, M=1, N=16, K=128, ldx=None, ldy=None, ldr=0):
        return lib.sd_gemv_mxfp8_wide(x, K if ldx is None else ldx, wq, ws, y, N if ldy is None else ldy, r, ldr, 0, 0.0, M,
                                      N, K, None)

    def swiglu(x=P, wq=P, ws=P, y=P, M=1, N=16, K=128):
        return lib.sd_gemv_mxfp8_wide_swiglu(x, wq, ws, y, 1, 1e-6, M, N, K, None)

    for call in (gemv, swiglu):
        assert call(M=0) == SHAPE and call(M=-1) == SHAPE and call(N=0) == SHAPE and call(K=0) == SHAPE
        assert call(x=None) == SHAPE and call(wq=None) == SHAPE and call(ws=None) == SHAPE and call(y=None) == SHAPE
        assert call(M=65) == UNSUP and call(K=96) == UNSUP and call(K=8320) == UNSUP
        assert call(x=P + 8) == UNSUP and call(wq=P + 4) == UNSUP and call(ws=P + 2) == UNSUP    # misaligned operands
    assert gemv(M=65, x=None) == SHAPE                                         # SHAPE is decided ahead of UNSUPPORTED
    assert gemv(ldx=132) == UNSUP and gemv(ldx=96) == UNSUP and gemv(ldy=8) == UNSUP and gemv(r=P, ldr=8) == UNSUP
    assert gemv(N=(1 << 29) + 1, ldy=(1 << 29) + 1) == UNSUP
    # the M bound is the only limit that differs from the 16-row entry
    assert lib.sd_gemv_mxfp8(P, 128, P, P, P, 16, None, 0, 0, 0.0, 17, 16, 128, None) == UNSUP
    assert lib.sd_gemv_mxfp8(P, 128, P, P, P, 16, None, 0, 0, 0.0, 0, 16, 128, None) == SHAPE


def test_mx_wide_step_refuses_before_any_launch():
    """The codes of sd_qwen3_mx_decode_step: SD_ERR_SHAPE for NULL arguments, non-positive sizes or an unknown cache kind,
    SD_ERR_WORKSPACE for short buffers, SD_ERR_UNSUPPORTED for dims outside sd_qwen3_mx_supported or the cache kernels."""
    from speech_distill_amd import _lib as L
    lib = _lib()
    d, p = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)), ctypes.byref(L.ParamsMx())
    pages = L.KvPages(P, BIG, P, 8, 2)

    def ref(kind=0, cache=P, nbytes=BIG, cap=256, pg=None):
        return ctypes.byref(L.KvRef(kind, cache, nbytes, cap, ctypes.pointer(pg) if pg is not None else None))

    def step(kv, d=d, p=p, ids=P, pos=P, acts=P, nb=BIG, logits=P, B=2, max_len=8):
        return lib.sd_qwen3_mx_decode_step_wide(d, p, ids, pos, max_len, P, P, kv, acts, nb, logits, B, None)

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
    odd = ctypes.byref(L.Dims(640, 320, 512, 1, 2, 1, 128, 1, 1e-6, 0))                # hidden no multiple of 128
    hd64 = ctypes.byref(L.Dims(640, 256, 512, 2, 4, 2, 64, 1, 1e-6, 0))
    g8 = ctypes.byref(L.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))                 # 8 query heads per kv head
    assert step(ref(), d=odd) == UNSUP and step(ref(), d=hd64) == UNSUP and step(ref(), d=g8) == UNSUP
    # the existing entry keeps its answer to an unknown flag bit
    assert lib.sd_qwen3_mx_decode_step(d, p, P, P, 8, P, P, ref(), P, BIG, P, 2, 2, None) == SHAPE
    assert lib.sd_abi_version() == 2


def test_mx_wide_acts_bytes_is_the_mx_steps_and_monotone_in_the_batch():
    from speech_distill_amd import _lib as L
    lib = _lib()
    d = ctypes.byref(L.Dims(159488, 2048, 6144, 28, 16, 8, 128, 1, 1e-6, 0))
    sizes = [lib.sd_qwen3_mx_decode_step_wide_acts_bytes(d, B, 1024) for B in (1, 2, 16, 17, 33, 64, 65)]
    assert sizes[0] > lib.sd_attn_decode_workspace_bytes(1, 16, 1024) > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes == [lib.sd_qwen3_mx_decode_step_acts_bytes(d, B, 1024) for B in (1, 2, 16, 17, 33, 64, 65)]
    assert lib.sd_qwen3_mx_decode_step_wide_acts_bytes(d, 0, 1024) == SHAPE
    assert lib.sd_qwen3_mx_decode_step_wide_acts_bytes(d, 4, 0) == SHAPE
    assert lib.sd_qwen3_mx_decode_step_wide_acts_bytes(None, 4, 256) == UNSUP
    odd = ctypes.byref(L.Dims(640, 320, 512, 1, 2, 1, 128, 1, 1e-6, 0))
    assert lib.sd_qwen3_mx_decode_step_wide_acts_bytes(odd, 4, 256) == UNSUP


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


def _entry_points(m, ids):
    """The four public places the keyword is accepted, as callables of the mode keywords."""
    from speech_distill_amd import generation as G
    return (lambda **kw: m.generate(ids, max_new_tokens=2, do_sample=False, **kw),
            lambda **kw: m.start_session(1, capacity=256, **kw),
            lambda **kw: G.Decoder(m, 1, 256, **kw),
            lambda **kw: m.generation_engine(object(), max_batch=20, **kw))


def test_gemv_rows_defaults_to_16():
    import speech_distill_amd as sda
    from speech_distill_amd import engine as E
    from speech_distill_amd import generation as G
    assert G.GEMV_ROWS == (16, 64)
    for fn in (sda.HipQwen3ForCausalLM.generate, sda.HipQwen3ForCausalLM.start_session,
               sda.HipQwen3ForCausalLM.generation_engine, G.generate, G.Decoder.__init__, G.GenerationSession.__init__,
               E.GenerationEngine.__init__, G._check_args):
        assert inspect.signature(fn).parameters["gemv_rows"].default == 16, fn
    for fn in (sda.ops.gemv_mxfp8, sda.ops.gemv_mxfp8_swiglu):
        assert inspect.signature(fn).parameters["wide"].default is False, fn
    # _check_decode_kernels keeps its signature
    assert list(inspect.signature(G._check_decode_kernels).parameters) == ["decode_kernels", "weight_dtype"]
    G._check_gemv_rows(16, "tile", "bf16", "fused", True)      # the default passes whatever the other keywords say
    G._check_gemv_rows(64, "skinny", "mxfp8")


def test_every_refused_combination_raises_before_anything_is_allocated():
    m = _cpu_model().requires_grad_(False)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    ok = dict(decode_kernels="skinny", weight_dtype="mxfp8")
    for i, call in enumerate(_entry_points(m, ids)):
        for rows in (0, 8, 32, 17, 128, "64", None, True, 64.0, 16.0):
            with pytest.raises(ValueError, match="gemv_rows"):
                call(gemv_rows=rows, **ok)
        with pytest.raises(ValueError, match='decode_kernels="wide"'):          # bf16 weights: pointed to "wide"
            call(gemv_rows=64, decode_kernels="skinny")
        for kernels in ("tile", "wide"):
            with pytest.raises(ValueError, match="gemv_rows=64"):
                call(gemv_rows=64, decode_kernels=kernels)
        with pytest.raises(ValueError, match="gemv_rows=64"):
            call(gemv_rows=64, decode_kernels="tile", weight_dtype="mxfp8")
        with pytest.raises(ValueError, match="not built"):
            call(gemv_rows=64, decode_attention="fused", **ok)
        if i in (1, 2):   # sessions and decoders take shared_kv_reads (pool: never touched, the refusal comes first)
            with pytest.raises(ValueError, match="not built"):
                call(gemv_rows=64, shared_kv_reads=True, pool=object(), **ok)
    # the accepted combination passes every check and gets as far as the CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(ids, max_new_tokens=2, do_sample=False, gemv_rows=64, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(ids, max_new_tokens=2, do_sample=False, gemv_rows=16, **ok)


def test_the_pinned_wide_mxfp8_refusal_still_raises_and_names_the_keyword():
    from speech_distill_amd import generation as G
    assert G.DECODE_KERNELS == ("tile", "skinny", "wide")
    m = _cpu_model().requires_grad_(False)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for call in _entry_points(m, ids):
        for rows in (16, 64):
            with pytest.raises(ValueError, match="wide") as e:
                call(decode_kernels="wide", weight_dtype="mxfp8", gemv_rows=rows)
            assert "gemv_rows=64" in str(e.value)
    with pytest.raises(ValueError, match="gemv_rows=64"):
        G._check_decode_kernels("wide", "mxfp8")
