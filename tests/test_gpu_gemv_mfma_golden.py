"""-m gpu: the MFMA weight-streaming GEMVs (csrc/sd_gemv_mx.hip, csrc/sd_gemv_wide.hip over csrc/sd_gemv_mfma.cuh) write
the bits that the three kernels wrote when each carried its own work walk and its own combine.

tests/golden/gemv_mfma/ holds the outputs of the commit before that change on the seeded inputs below (written by
`SD_HIP_LIB=<that build's libsd_hip.so> python tests/test_gpu_gemv_mfma_golden.py --record DIR`): whole buffers for the
small cases, SHA-256 digests of the buffer bytes for the large-N ones.  Every output lies in a buffer pre-filled with the NaN
sentinel of tests/test_gpu_gemv.py, two guard rows above and below it and -- in the strided cases -- an ldy > N gap, and
the WHOLE buffer is compared: a stray write fails like a wrong bit.

Inputs: CPU torch.Generator, fixed seeds, randn and exact power-of-two row magnitudes only (no transcendental whose last bit
could depend on the host).  Weights are quantised as tests/test_gpu_gemv_mx.py does it (ops.mxfp8_quant of a bf16 weight).
The large weights repeat a 1024-row base under per-row magnitudes, on the device.  The grid depends on the CU count, no
output bit does, so the fixtures hold on any partition mode."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import dev, to_dev
from test_gpu_gemv import SENT
from test_gpu_gemv_mx import ops  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(GOLDEN, "gemv_mfma")
GUARD = 2
EPS = 1e-6

_DATA = {}


def _pow2_rows(rows, g):
    return 2.0 ** torch.randint(-3, 4, (rows, 1), generator=g).float()


def _data(kind, N, K):
    """x [64,K] (rows of very different magnitude), w [N,K], r [64,N], gain [K] in bf16 on the device; for kind "mx" the
    weight as (bytes, scale bytes).  Made once per (kind, N, K) and never changed."""
    key = (kind, N, K)
    if key not in _DATA:
        g = torch.Generator().manual_seed(1000003 * N + 17 * K + (kind == "mx"))
        x = (torch.randn(64, K, generator=g) * _pow2_rows(64, g)).bfloat16()
        r = torch.randn(64, N, generator=g).bfloat16()
        gain = (1 + 0.25 * torch.randn(K, generator=g)).bfloat16()
        scale = 0.05 if kind == "mx" else 1.0
        if N <= 1024:
            w = to_dev((scale * torch.randn(N, K, generator=g)).bfloat16())
        else:
            base = to_dev(torch.randn(1024, K, generator=g))
            mag = to_dev(scale * (1 + 0.5 * torch.rand(N, 1, generator=g)) * _pow2_rows(N, g))
            w = (base.repeat(-(-N // 1024), 1)[:N] * mag).bfloat16()
        if kind == "mx":
            from speech_distill_amd import ops as ops_
            w = ops_.mxfp8_quant(w)
        _DATA[key] = (to_dev(x), w, to_dev(r), to_dev(gain))
    return _DATA[key]


def _case(entry, M, N, K, norm=False, res=False, strided=False, alias=False):
    return dict(entry=entry, M=M, N=N, K=K, norm=norm, res=res, strided=strided, alias=alias)


def _name(c):
    return "{entry}_M{M}_N{N}_K{K}_n{norm:d}_r{res:d}_s{strided:d}_a{alias:d}".format(**c)


def _run(ops, c):
    """The whole output buffer [GUARD + M + GUARD, ldy] of one call, as int16 bit patterns."""
    from speech_distill_amd.ops import _stream
    entry, M, N, K = c["entry"], c["M"], c["N"], c["K"]
    mx, swiglu, wide = entry.startswith("mx"), entry.endswith("swiglu"), not entry.startswith("mx16")
    rows = 2 * N if swiglu else N                     # SwiGLU: N = I, the weight holds gate rows | up rows
    x, w, r, gain = _data("mx" if mx else "bf16", rows, K)
    x, r = x[:M], r[:M, :N]
    ldy = N + 5 if c["strided"] else N
    if c["strided"]:
        xb = torch.full((M, K + 8), float("nan"), dtype=torch.bfloat16, device=dev())
        rb = torch.full((M, N + 3), float("nan"), dtype=torch.bfloat16, device=dev())
        xb[:, :K], rb[:, :N] = x, r
        x, r = xb[:, :K], rb[:, :N]
    buf = torch.full((M + 2 * GUARD, ldy), SENT, dtype=torch.int16, device=dev())
    out = buf.view(torch.bfloat16)[GUARD:GUARD + M, :N]
    if c["alias"]:
        out.copy_(r)
        r = out
    res = r if c["res"] else None
    if swiglu:
        lib = ops.load_lib()
        if mx:
            fn = lib.sd_gemv_mxfp8_wide_swiglu if wide else lib.sd_gemv_mxfp8_swiglu
            rc = fn(x.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), 1 if c["norm"] else 0, C.c_float(EPS), M, N,
                    K, _stream())
        else:
            rc = lib.sd_gemv_wide_swiglu(x.data_ptr(), w.data_ptr(), out.data_ptr(), gain.data_ptr() if c["norm"] else None,
                                         C.c_float(EPS), M, N, K, _stream())
        assert rc == 0, (_name(c), rc)
    elif mx:
        ops.gemv_mxfp8(x, w[0], w[1], residual=res, norm=c["norm"], eps=EPS, out=out, wide=wide)
    else:
        ops.gemv_bf16(x, w, residual=res, norm_gain=gain if c["norm"] else None, eps=EPS, out=out, wide=True)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    inner = got[GUARD:GUARD + M, :N]
    assert not (inner == np.int16(SENT)).any(), f"{_name(c)}: elements of y were left unwritten"
    return got


# ------------------------------------------------------------------------------------------------------ the cases
MX16_KN = [(128, 17), (1152, 37), (2048, 600), (4224, 37), (6144, 17), (8192, 160)]


def _mx16_group(K, N):
    cs = [_case("mx16", M, N, K, norm=n, res=r) for M in (1, 5, 16) for n in (False, True) for r in (False, True)]
    if (K, N) == (1152, 37):
        cs.append(_case("mx16", 5, N, K, norm=True, res=True, strided=True))
    if (K, N) == (2048, 600):
        cs.append(_case("mx16", 16, N, K, norm=True, res=True, alias=True))
    return cs


GROUPS = {f"mx16_K{K}_N{N}": _mx16_group(K, N) for K, N in MX16_KN}
GROUPS["mx16_swiglu"] = [_case("mx16_swiglu", M, I, K, norm=n) for I, K in ((40, 512), (600, 2048), (160, 4224))
                         for M in (1, 5, 16) for n in (False, True)]
GROUPS["mxw"] = [_case("mxw", M, N, K, norm=n, res=r) for M in (17, 33, 64) for K, N in ((1152, 37), (6144, 17))
                 for n in (False, True) for r in (False, True)] + \
                [_case("mxw", 33, 37, 1152, norm=True, res=True, strided=True),
                 _case("mxw", 64, 17, 6144, norm=True, res=True, alias=True)]
GROUPS["mxw_swiglu"] = [_case("mxw_swiglu", M, 40, K, norm=n) for M in (17, 33, 64) for K in (1152, 6144)
                        for n in (False, True)]
GROUPS["bf16w"] = [_case("bf16w", M, N, K, res=r) for M in (1, 17, 64) for N, K in ((40, 128), (100, 2048), (48, 8192))
                   for r in (False, True)] + \
                  [_case("bf16w", M, N, K, norm=True) for M in (1, 17, 64) for N, K in ((40, 128), (100, 4096))] + \
                  [_case("bf16w", 17, 100, 2048, res=True, strided=True), _case("bf16w", 64, 100, 2048, res=True, alias=True)]
GROUPS["bf16w_swiglu"] = [_case("bf16w_swiglu", M, I, K, norm=n) for M in (1, 17, 64) for I, K in ((24, 2048), (256, 128))
                          for n in (False, True)]
# A workgroup owns more than one 16-row unit (more than about two units per CU) and a wave takes 2 or 4 tiles per step:
# digests.  The SwiGLU forms run on the same weight (I = N / 2).
DIGESTS = [_case("mx16", 16, N, K, norm=True, res=True) for N in (8208, 24592) for K in (1152, 6144)] + \
          [_case("mx16_swiglu", 16, N // 2, K, norm=True) for N in (8208, 24592) for K in (1152, 6144)] + \
          [_case("mxw", 64, 8208, 6144, norm=True, res=True), _case("mxw_swiglu", 64, 4104, 6144, norm=True),
           _case("bf16w", 64, 8208, 2048, res=True), _case("bf16w_swiglu", 64, 4104, 2048, norm=True)]


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_outputs_equal_the_recorded_ones(ops, group):
    want = np.load(os.path.join(GOLDEN_DIR, group + ".npz"), allow_pickle=False)
    assert sorted(want.files) == sorted(_name(c) for c in GROUPS[group])
    bad = []
    for c in GROUPS[group]:
        got, w = _run(ops, c), want[_name(c)]
        if got.shape != w.shape or not np.array_equal(got, w):
            bad.append((_name(c), int((got != w).sum()) if got.shape == w.shape else "shape"))
    assert not bad, f"buffers that differ from the recorded ones (name, elements): {bad}"


@pytest.mark.parametrize("c", DIGESTS, ids=_name)
def test_large_n_outputs_have_the_recorded_digest(ops, c):
    with open(os.path.join(GOLDEN_DIR, "digests.json")) as f:
        want = json.load(f)
    assert _digest(_run(ops, c)) == want[_name(c)], _name(c)


def _record(out_dir):
    from speech_distill_amd import ops as ops_
    ops_.load_lib()
    os.makedirs(out_dir, exist_ok=True)
    for group, cases in sorted(GROUPS.items()):
        np.savez(os.path.join(out_dir, group + ".npz"), **{_name(c): _run(ops_, c) for c in cases})
        print("recorded", group, len(cases), "cases", os.path.getsize(os.path.join(out_dir, group + ".npz")), "bytes")
    with open(os.path.join(out_dir, "digests.json"), "w") as f:
        json.dump({_name(c): _digest(_run(ops_, c)) for c in DIGESTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(DIGESTS), "digests")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        _record(sys.argv[2])
    else:
        sys.exit("usage: python tests/test_gpu_gemv_mfma_golden.py --record DIR")
