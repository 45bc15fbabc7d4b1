"""Which kernel, tile and grid the GEMM dispatch picks, checked without a GPU: `_lib.gemm_plan` (sd_debug_gemm_plan,
include/sd_hip_debug.h) runs the library's own `gemm_plan()` for 256 CUs and reports what `launch_plan()` would launch.

The expectations do not come from the code under test: profiles/gemm_plan_parent.json holds the kernel symbol every
tests/bench_tune.py call launched on an MI355X BEFORE the dispatch was rewritten into gemm_plan / launch_plan (recorded with
ops.prof_symbols), and the grid / block / group_m tables below were read off that older dispatch code by hand."""
import json
import os
import random

import pytest

import bench_tune
from speech_distill_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = json.load(open(os.path.join(ROOT, "profiles", "gemm_plan_parent.json")))
SETTINGS = {"default": {}, "no_table": {"gemm.no_table": 1}, "no_p256": {"gemm.no_p256": 1}}
# The one launch the older dispatch left without a label (pointer staging, gemm_bf16_kernel<..., false>) is recorded under
# its profiler kind; it has a label now.  Config 4's lm_head dW: K * lda * 2 bytes is past the 31-bit descriptor range.
UNLABELLED_THEN = {("c4.student.lm_head.dW", "gemm_tn"): "gemm_bf16_kernel<256, 3, true, true, 0, false>"}


@pytest.fixture(autouse=True)
def default_switches():
    _lib.debug_set("reset", 0)
    yield
    _lib.debug_set("reset", 0)


def plan_of_call(form, epi, M, N, K, **kw):
    """the plan of a tests/bench_tune.py call, dispatched the way bench_tune.py dispatches it"""
    ta, tb = form == "TN", form in ("NN", "TN")
    return _lib.gemm_plan(M, N, K, ta, tb, epi_kind=epi if epi >= 3 else 0, residual=epi == 1, split_k=epi == 2,
                          epi_I=N // 2 if epi == 3 else 0, **kw)


def test_every_recorded_call_gets_the_recorded_kernel():
    calls = [c for cfg in ("c2", "c4", "c5") for c in bench_tune.calls(cfg)]
    assert [(c["name"], c["form"], c["epi"], c["M"], c["N"], c["K"]) for c in RECORDED["calls"]] == calls
    assert RECORDED["cus"] == 256
    for setting, knobs in SETTINGS.items():
        _lib.debug_set("reset", 0)
        for k, v in knobs.items():
            _lib.debug_set(k, v)
        for c in RECORDED["calls"]:
            want = c["symbol"][setting]
            want = UNLABELLED_THEN.get((c["name"], want), want)
            got = plan_of_call(c["form"], c["epi"], c["M"], c["N"], c["K"])["symbol"]
            assert got == want, (c["name"], setting)


# config 2 (2 048 tokens, heads on 1 536 rows), default switches: symbol, grid_x, grid_y, block, group_m
C2 = {
    "c2.student.qkv": ("gemm_stag_kernel<false, false, 4>", 256, 1, 512, 4),
    "c2.student.o": ("gemm_bf16_kernel<64, 4, false, false, 1, true>", 256, 1, 256, 8),
    "c2.student.gu": ("gemm_pstag_kernel<4, false, false, 0>", 256, 1, 768, 4),
    "c2.student.down": ("gemm_bf16_kernel<64, 4, false, false, 1, true>", 256, 1, 256, 8),
    "c2.student.lm_head": ("gemm_p256_kernel<0, true>", 256, 1, 512, 6),       # 6 x 623 tiles of 256 x 256, group of 6 rows
    "c2.student.lm_head.dW": ("gemm_pstag_kernel<4, true, true, 0>", 256, 1, 768, 4),
    "c2.student.lm_head.dX": ("gemm_stag_kernel<false, true, 2>", 48, 5, 512, 4),  # 48 tiles x 5 K slices
    "c2.student.down.dX": ("gemm_bf16_kernel<128, 2, false, true, 5, true>", 384, 1, 256, 8),  # sd_gemm_table.inc
    "c2.student.gu.dX": ("gemm_stag_kernel<false, true, 2>", 64, 4, 512, 4),
    "c2.student.o.dX": ("gemm_bf16_kernel<128, 3, false, true, 6, true>", 256, 1, 256, 8),
    "c2.student.qkv.dX": ("gemm_bf16_kernel<64, 3, false, true, 0, true>", 256, 1, 256, 8),  # split-K plan of one slice
    "c2.teacher.qkv": ("gemm_stag_kernel<false, false, 4>", 256, 1, 512, 4),
    "c2.teacher.o": ("gemm_bf16_kernel<128, 3, false, false, 1, true>", 256, 1, 256, 8),
    "c2.teacher.gu": ("gemm_pstag_kernel<4, false, false, 3>", 256, 1, 768, 4),
    "c2.teacher.down": ("gemm_bf16_kernel<128, 3, false, false, 1, true>", 256, 1, 256, 8),
    "c2.teacher.lm_head": ("gemm_p256_kernel<0, true>", 256, 1, 512, 6),
}


def test_config2_grid_block_and_group_m():
    calls = bench_tune.calls("c2")
    assert sorted(C2) == sorted(c[0] for c in calls)
    for name, form, epi, M, N, K in calls:
        p = plan_of_call(form, epi, M, N, K)
        assert (p["symbol"], p["grid_x"], p["grid_y"], p["block"], p["gm"]) == C2[name], name


def grid(p):
    return p["symbol"], p["grid_x"]


def test_cu_budget_of_the_persistent_weight_gradient_launch():
    """lm_head dW at 2 048 tokens (TN, K = tokens): 3/4 of the CUs only beside the dX chain, a set budget always, -1 never"""
    sym = "gemm_pstag_kernel<4, true, true, 0>"
    for knob, want in ((0, {0: 256, 1: 192}), (192, {0: 192, 1: 192}), (-1, {0: 256, 1: 256})):
        _lib.debug_set("gemm.cu_budget", knob)
        for shared in (0, 1):
            assert grid(_lib.gemm_plan(159488, 1024, 2048, True, True, shared_gpu=shared)) == (sym, want[shared]), (knob, shared)


def test_shared_gpu_bump_of_the_student_o_projection():
    """M = 2048, N = 1024, K = 2048 with a residual: 256 tiles of 64 rows alone, 128 tiles of 128 rows beside another stream"""
    alone, bumped = ("gemm_bf16_kernel<64, 4, false, false, 1, true>", 256), ("gemm_bf16_kernel<128, 3, false, false, 1, true>", 128)
    o = dict(M=2048, N=1024, K=2048, residual=True)
    assert grid(_lib.gemm_plan(**o)) == alone and grid(_lib.gemm_plan(**o, shared_gpu=True)) == bumped
    _lib.debug_set("gemm.fwd_bump", 3)
    assert grid(_lib.gemm_plan(**o, shared_gpu=True)) == bumped and grid(_lib.gemm_plan(**o)) == bumped  # > 0: every call
    _lib.debug_set("gemm.fwd_bump", -1)
    assert grid(_lib.gemm_plan(**o, shared_gpu=True)) == alone


def test_forced_staggered_tile_without_descriptor_staging_takes_the_three_stage_ring():
    _lib.debug_set("gemm.force_bm", 256)
    _lib.debug_set("gemm.force_nst", 9)
    p = _lib.gemm_plan(520, 264, 200)  # a K-contiguous operand, K % 64 != 0: pointer staging
    assert (p["symbol"], p["grid_x"], p["block"], p["gm"]) == ("gemm_bf16_kernel<256, 3, false, false, 0, false>", 9, 512, 3)
    assert _lib.gemm_plan(520, 264, 192)["symbol"] == "gemm_stag_kernel<false, false, 0>"
    # one K-contiguous operand is enough: its rows are not zero-filled behind K (descriptor staging would multiply the gap
    # of a strided view, or the next row, by the other operand's zeros: NaN for a non-finite neighbour)
    assert _lib.gemm_plan(520, 264, 200, False, True)["symbol"] == "gemm_bf16_kernel<256, 3, false, true, 0, false>"
    assert _lib.gemm_plan(520, 264, 200, True, False)["symbol"] == "gemm_bf16_kernel<256, 3, true, false, 0, false>"
    assert _lib.gemm_plan(520, 264, 192, False, True)["symbol"] == "gemm_stag_kernel<false, true, 0>"
    assert _lib.gemm_plan(520, 264, 200, True, True)["symbol"] == "gemm_stag_kernel<true, true, 0>"  # both transposed


def test_checked_staging():
    _lib.debug_set("gemm.checked_staging", 1)
    assert grid(_lib.gemm_plan(2048, 1024, 2048)) == ("gemm_bf16_kernel<64, 4, false, false, 0, false>", 256)
    fused = [dict(M=2048, N=4096, K=1024, trans_b=epi_kind >= 5, epi_kind=epi_kind, epi_I=2048) for epi_kind in (3, 4, 5, 6)]
    for q in fused:  # the fused epilogues have no pointer-staging form
        with pytest.raises(_lib.SdHipError, match="SD_ERR_UNSUPPORTED"):
            _lib.gemm_plan(**q)
    _lib.debug_set("gemm.checked_staging", 0)
    assert [_lib.gemm_plan(**q)["symbol"] for q in fused] == [
        "gemm_stag_kernel<false, false, 3>", "gemm_stag_kernel<false, false, 4>",
        "gemm_bf16_kernel<128, 2, false, true, 5, true>", "gemm_bf16_kernel<128, 2, false, true, 6, true>"]


def test_persistent_kernel_switches():
    """M = 3584, N = 3328, K = 64: 14 x 26 = 364 tiles of 256 x 128, 14 x 13 = 182 of 256 x 256 (>= 70 % of one round of 256)"""
    s = dict(M=3584, N=3328, K=64)
    pstag, p256 = "gemm_pstag_kernel<4, false, false, 0>", "gemm_p256_kernel<0, true>"
    assert grid(_lib.gemm_plan(**s)) == (pstag, 256)
    _lib.debug_set("gemm.p256_min_tiles", 150)
    p = _lib.gemm_plan(**s)
    assert (p["symbol"], p["grid_x"], p["block"], p["gm"]) == (p256, 182, 512, 8)
    _lib.debug_set("gemm.p256_unpaired", 1)
    assert grid(_lib.gemm_plan(**s)) == ("gemm_p256_kernel<0, false>", 182)
    _lib.debug_set("gemm.p256_unpaired", 0)
    _lib.debug_set("gemm.no_p256", 1)
    assert grid(_lib.gemm_plan(**s)) == (pstag, 256)
    _lib.debug_set("gemm.p256_min_tiles", 183)
    _lib.debug_set("gemm.no_p256", 0)
    assert grid(_lib.gemm_plan(**s)) == (pstag, 256)
    _lib.debug_set("gemm.persist_balance", 1)  # 364 tiles in 2 rounds: 182 -> 184 workgroups (a multiple of 8)
    assert grid(_lib.gemm_plan(**s)) == (pstag, 184)
    _lib.debug_set("gemm.no_persist", 1)
    p = _lib.gemm_plan(**s)
    assert (p["symbol"], p["grid_x"], p["block"]) == ("gemm_stag_kernel<false, false, 0>", 364, 512)


def test_plan_properties_on_random_queries():
    rnd = random.Random(7)
    seen = set()
    for _ in range(3000):
        M, N, K = (8 * rnd.randint(1, 1500) for _ in range(3))
        if rnd.random() < 0.2:
            N, K = rnd.choice([(159488, 1024), (1024, 159488), (12288, 2048)])
        ta, tb = rnd.choice([(False, False), (False, True), (True, True), (True, False)])
        epi_kind = rnd.choice([0, 0, 0, 3, 4]) if not (ta or tb) else (rnd.choice([0, 0, 5, 6]) if not ta else 0)
        q = dict(trans_a=ta, trans_b=tb, epi_kind=epi_kind, residual=epi_kind == 0 and rnd.random() < 0.3,
                 split_k=epi_kind == 0 and rnd.random() < 0.3, epi_I=N // 2 if epi_kind == 3 else 0,
                 shared_gpu=rnd.random() < 0.3, cus=rnd.choice([256, 256, 304, 64]))
        try:
            p = _lib.gemm_plan(M, N, K, **q)
        except _lib.SdHipError:  # a fused epilogue whose operands need pointer staging (K % 64 != 0, or past 31-bit offsets)
            assert epi_kind >= 3
            continue
        assert p == _lib.gemm_plan(M, N, K, **q)
        assert p["grid_x"] * p["grid_y"] >= 1 and p["block"] in (256, 512, 768)
        kernel = p["symbol"].split("<")[0]
        seen.add(kernel)
        if kernel in ("gemm_pstag_kernel", "gemm_p256_kernel"):
            assert p["grid_x"] * p["grid_y"] <= q["cus"], (M, N, K, q, p)
        if kernel == "gemm_bf16_kernel":
            assert p["block"] == (512 if p["symbol"].startswith("gemm_bf16_kernel<256,") else 256)
        else:  # the staggered family only exists on 256-row tiles: 512 threads, 768 with the producer waves, 512 for 256 x 256
            assert p["block"] == {"gemm_stag_kernel": 512, "gemm_pstag_kernel": 768, "gemm_p256_kernel": 512}[kernel]
            assert p["grid_y"] == 1 or kernel == "gemm_stag_kernel"
            if kernel == "gemm_stag_kernel":  # one workgroup per 256 x 128 tile
                assert p["grid_x"] == -(-M // 256) * -(-N // 128)
    assert seen == {"gemm_bf16_kernel", "gemm_stag_kernel", "gemm_pstag_kernel", "gemm_p256_kernel"}
