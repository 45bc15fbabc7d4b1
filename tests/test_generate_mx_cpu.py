"""CPU checks of generation on MXFP8 weights (``weight_dtype``; generation.py, include/sd_hip.h "generation on MXFP8
weights"): every argument error comes before anything is allocated or launched, the default call behaves as it did before
the keyword existed, and the new entries answer their size queries and refusals without a GPU."""
import ctypes

import pytest
import torch


def _cpu_model():
    import speech_distill_amd as sda
    return sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 128, 256, 2, 2, 1), device="cpu", init_std=0)


IDS = torch.zeros(1, 4, dtype=torch.int64)


def test_unknown_weight_dtype_is_a_value_error_everywhere():
    from speech_distill_amd.generation import Decoder, GenerationSession, generate
    m = _cpu_model().requires_grad_(False)
    for call in (lambda: m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="fp8"),
                 lambda: generate(m, IDS, max_new_tokens=2, do_sample=False, weight_dtype="int8"),
                 lambda: m.start_session(1, capacity=256, weight_dtype="mx"),
                 lambda: GenerationSession(m, 1, 256, weight_dtype=None),
                 lambda: Decoder(m, 1, 256, weight_dtype="MXFP8")):
        with pytest.raises(ValueError, match="weight_dtype"):
            call()


def test_mxfp8_weights_need_a_frozen_model_without_lora_and_supported_dims():
    import speech_distill_amd as sda
    m = _cpu_model()    # trainable
    for call in (lambda: m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="mxfp8"),
                 lambda: m.start_session(1, capacity=256, weight_dtype="mxfp8")):
        with pytest.raises(ValueError, match="frozen"):
            call()
    m.requires_grad_(False)
    m._lora = object()    # what an attached adapter leaves: _check_mx looks at nothing else of it
    with pytest.raises(ValueError, match="LoRA"):
        m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="mxfp8")
    m._lora = None
    odd = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 320, 512, 1, 2, 1), device="cpu", init_std=0).requires_grad_(False)
    with pytest.raises(ValueError, match="multiples of 128"):
        odd.start_session(1, capacity=256, weight_dtype="mxfp8")
    # a frozen, supported model passes every weight_dtype check and gets as far as the CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="mxfp8")
    # ... also when its forward runs at "mxfp8": the keyword is independent of the inference precision
    m.inference_precision = "mxfp8"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="mxfp8")


def test_the_default_call_on_an_mxfp8_model_still_raises():
    from speech_distill_amd.generation import Decoder
    m = _cpu_model().requires_grad_(False)
    m.inference_precision = "mxfp8"   # what set_inference_precision("mxfp8") leaves on a model that supports it
    with pytest.raises(NotImplementedError, match="mxfp8"):
        m.generate(IDS, max_new_tokens=2, do_sample=False)
    with pytest.raises(NotImplementedError, match="mxfp8"):
        m.start_session(1, capacity=256)
    with pytest.raises(NotImplementedError, match="weight_dtype"):    # the message now names the keyword
        Decoder(m, 1, 256)
    with pytest.raises(NotImplementedError, match="mxfp8"):
        m.generate(IDS, max_new_tokens=2, do_sample=False, weight_dtype="bf16")
    # the other argument errors keep their order in front of it
    with pytest.raises(ValueError, match="top_k"):
        m.generate(IDS, max_new_tokens=2, top_k=129, weight_dtype="mxfp8")
    with pytest.raises(ValueError, match="decode_kernels"):
        m.generate(IDS, max_new_tokens=2, decode_kernels="fat", weight_dtype="mxfp8")


def test_size_queries_and_refusals_answer_without_a_gpu():
    import speech_distill_amd as sda
    from speech_distill_amd import _lib
    lib = sda.load_lib()
    d = ctypes.byref(_lib.Dims(159488, 2048, 6144, 28, 16, 8, 128, 1, 1e-6, 0))
    pre = lib.sd_qwen3_mx_prefill_acts_bytes(d, 4, 512)
    assert pre > lib.sd_qwen3_mx_acts_bytes(d, 4, 512) > 0
    assert lib.sd_qwen3_mx_extend_acts_bytes(d, 4, 512) >= pre + 2 * 4 * 512 * 128 * 2
    step = lib.sd_qwen3_mx_decode_step_acts_bytes(d, 16, 1024)
    assert step > lib.sd_attn_decode_workspace_bytes(16, 16, 1024) > 0
    assert lib.sd_qwen3_mx_decode_step_acts_bytes(d, 0, 1024) == -1 and lib.sd_qwen3_mx_decode_step_acts_bytes(d, 4, 0) == -1
    odd = ctypes.byref(_lib.Dims(640, 320, 512, 1, 2, 1, 128, 1, 1e-6, 0))
    assert lib.sd_qwen3_mx_decode_step_acts_bytes(odd, 4, 256) == -3 and lib.sd_qwen3_mx_prefill_acts_bytes(odd, 4, 8) == -3
    assert lib.sd_qwen3_mx_extend_acts_bytes(odd, 4, 8) == -3 and lib.sd_qwen3_mx_extend_acts_bytes(None, 4, 8) == -1


def test_runner_entries_refuse_before_any_launch():
    """Checks and codes of the bf16 twins: SD_ERR_SHAPE (-1) for NULL arguments, non-positive sizes, an unknown cache kind
    or flag bit; SD_ERR_WORKSPACE (-5) for short buffers; SD_ERR_UNSUPPORTED (-3) for dims the kernels do not take."""
    import speech_distill_amd as sda
    from speech_distill_amd import _lib
    lib = sda.load_lib()
    dims = _lib.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0)
    d, p = ctypes.byref(dims), ctypes.byref(_lib.ParamsMx())
    P, BIG = 0x10000, 1 << 40
    SHAPE, UNSUP, WORK = -1, -3, -5
    pages = _lib.KvPages(P, BIG, P, 8, 2)

    def ref(kind=0, cache=P, nbytes=BIG, cap=256, pg=None):
        return ctypes.byref(_lib.KvRef(kind, cache, nbytes, cap, ctypes.pointer(pg) if pg is not None else None))

    def prefill(kv, d=d, p=p, ids=P, acts=P, nb=BIG, logits=P, B=2, T=8):
        return lib.sd_qwen3_mx_prefill(d, p, ids, None, P, P, acts, nb, kv, logits, B, T, None)

    def extend(kv, d=d, p=p, ids=P, acts=P, nb=BIG, logits=P, B=2, T=8, past=P):
        return lib.sd_qwen3_mx_extend(d, p, ids, past, P, P, P, acts, nb, kv, logits, B, T, None)

    def step(kv, d=d, p=p, ids=P, acts=P, nb=BIG, logits=P, B=2, T=8, flags=0, max_len=8):
        return lib.sd_qwen3_mx_decode_step(d, p, ids, P, max_len, P, P, kv, acts, nb, logits, B, flags, None)

    for call in (prefill, extend, step):
        assert call(None) == SHAPE and call(ref(), d=None) == SHAPE and call(ref(), p=None) == SHAPE
        assert call(ref(kind=3)) == SHAPE and call(ref(kind=-1)) == SHAPE
        assert call(ref(cache=None)) == SHAPE and call(ref(cap=0)) == SHAPE
        assert call(ref(kind=1)) == SHAPE and call(ref(kind=2)) == SHAPE                  # paged kinds need the pages
        assert call(ref(), B=0) == SHAPE and call(ref(), ids=None) == SHAPE and call(ref(), logits=None) == SHAPE
        assert call(ref(), acts=None) == SHAPE
        assert call(ref(nbytes=16)) == WORK and call(ref(), nb=16) == WORK
        for kind in (1, 2):
            assert call(ref(kind=kind, pg=pages), nb=16) == WORK                          # a valid pool gets as far
            assert call(ref(kind=kind, pg=_lib.KvPages(P, 16, P, 8, 2))) == WORK
            assert call(ref(kind=kind, pg=_lib.KvPages(P, BIG, None, 8, 2))) == SHAPE
        odd = ctypes.byref(_lib.Dims(640, 320, 512, 1, 2, 1, 128, 1, 1e-6, 0))
        assert call(ref(), d=odd) == UNSUP
    assert prefill(ref(), T=0) == SHAPE and prefill(ref(cap=4)) == SHAPE and extend(ref(cap=4)) == SHAPE
    assert extend(ref(), past=None) == SHAPE
    assert step(ref(), flags=2) == SHAPE and step(ref(), flags=1, nb=16) == WORK and step(ref(), max_len=0) == SHAPE
    g8 = ctypes.byref(_lib.Dims(640, 256, 512, 2, 8, 1, 128, 1, 1e-6, 0))                 # 8 query heads per kv head
    assert extend(ref(), d=g8) == UNSUP and step(ref(), d=g8) == UNSUP


def test_gemv_refusals_without_a_gpu():
    import speech_distill_amd as sda
    lib = sda.load_lib()
    P = 0x10000

    def gemv(x=P, wq=P, ws=P, y=P, M=1, N=16, K=128):
        return lib.sd_gemv_mxfp8(x, K, wq, ws, y, N, None, 0, 0, 0.0, M, N, K, None)

    assert gemv(M=17) == -3 and gemv(K=96) == -3 and gemv(K=8320) == -3 and gemv(x=P + 8) == -3 and gemv(ws=P + 1) == -3
    assert gemv(x=None) == -1 and gemv(y=None) == -1 and gemv(M=0) == -1 and gemv(N=0) == -1
    assert lib.sd_gemv_mxfp8_swiglu(P, P, P, P, 1, 1e-6, 17, 16, 128, None) == -3
    assert lib.sd_gemv_mxfp8_swiglu(P, None, P, P, 1, 1e-6, 1, 16, 128, None) == -1
