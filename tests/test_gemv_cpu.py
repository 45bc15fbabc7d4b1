"""No GPU: sd_gemv_bf16, sd_gemv_swiglu and sd_qwen3_decode_step_flags decide their refusals before any launch, so the
codes come back on a machine without a device (the pattern of
test_cabi.py::test_runner_entries_refuse_invalid_descriptors_before_any_launch)."""
import ctypes

import pytest

SHAPE, UNSUPPORTED = -1, -3
P = 0x1000   # a 16-byte aligned address that is never dereferenced: every call below returns before a launch


@pytest.fixture(scope="module")
def lib():
    import speech_distill_amd as sda
    return sda.load_lib()


def gemv(lib, M=4, N=16, K=1024, x=P, w=P, y=P, r=None, gain=None, ldx=None, ldw=None, ldy=None, ldr=0):
    return lib.sd_gemv_bf16(x, w, y, r, gain, 1e-6, M, N, K, ldx or K, ldw or K, ldy or N, ldr, None)


def test_gemv_refusal_codes_without_a_device(lib):
    assert gemv(lib, M=17) == UNSUPPORTED                    # more rows than SD_GEMV_MAX_M
    assert gemv(lib, K=1028) == UNSUPPORTED                  # K % 8 != 0
    assert gemv(lib, K=8192, gain=P) == UNSUPPORTED          # fused norm beyond the limit of sd_rmsnorm_fwd
    assert gemv(lib, K=16384) == UNSUPPORTED
    assert gemv(lib, ldx=1016) == UNSUPPORTED and gemv(lib, ldw=1016) == UNSUPPORTED and gemv(lib, ldy=8) == UNSUPPORTED
    assert gemv(lib, r=P, ldr=8) == UNSUPPORTED
    assert gemv(lib, ldw=1028) == UNSUPPORTED and gemv(lib, x=P + 2) == UNSUPPORTED   # rows not 16-byte aligned
    assert gemv(lib, M=0) == SHAPE and gemv(lib, M=-1) == SHAPE and gemv(lib, N=0) == SHAPE
    assert gemv(lib, x=None) == SHAPE and gemv(lib, w=None) == SHAPE and gemv(lib, y=None) == SHAPE


def test_gemv_swiglu_refusal_codes_without_a_device(lib):
    def call(M=4, I=8, K=1024, x=P, gain=None):
        return lib.sd_gemv_swiglu(x, P, P, gain, 1e-6, M, I, K, None)
    assert call(M=17) == UNSUPPORTED and call(K=1028) == UNSUPPORTED and call(K=8192, gain=P) == UNSUPPORTED
    assert call(M=0) == SHAPE and call(I=0) == SHAPE and call(x=None) == SHAPE


def test_decode_step_flags_refuses_unknown_bits_without_a_device(lib):
    from speech_distill_amd import _lib
    d = ctypes.byref(_lib.Dims(640, 256, 512, 2, 4, 2, 128, 1, 1e-6, 0))
    p = ctypes.byref(_lib.Params())

    def step(flags, B=2, acts_bytes=1 << 40):
        return lib.sd_qwen3_decode_step_flags(d, p, P, P, 8, P, P, P, 1 << 40, 16, P, acts_bytes, P, B, flags, None)
    assert step(2) == SHAPE and step(3) == SHAPE and step(0x100) == SHAPE
    assert step(1, B=0) == SHAPE
    assert step(1, acts_bytes=0) == -5 and step(0, acts_bytes=0) == -5      # known flags get as far as the workspace check
