"""-m gpu tests of the kernels of csrc/sd_lora.hip, one at a time: lora_merge_kernel, lora_db_kernel, lora_da_kernel behind
their plan, and adamw_f32_shadow_kernel.  Tables, arenas, expectations and the wrong restatements the checks are proven
against live in tests/lora_ref.py (tests/test_lora_ref_cpu.py); DESIGN.md section 5, "How the LoRA kernels are checked".

Every launch runs on packed arenas, one per buffer kind, with the targets back to back in plan order as lora.py holds
them, 64 guard rows between them: outputs start as sentinels and every guard element must keep its bits; inputs carry
zeros, +-3e4 or NaN in the gaps and the outputs must not depend on which.
"""
import ctypes as C
import functools

import pytest
import torch

import gemm_ref as G
import lora_ref as L
import parity_ref as P
from gemm_ref import LOUD, NAN, SENTINEL
from gpu_util import dev, record, to_dev
from speech_distill_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _lib.load_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _build(flats_dev, lays, shapes, r_pad):
    lib = _lib.load_lib()
    arr = L.plan_struct(_lib, L.piece_ptrs(flats_dev, lays), shapes)
    nb = lib.sd_lora_plan_bytes(len(shapes))
    host = C.create_string_buffer(nb)
    _lib.check(lib.sd_lora_plan_build(arr, len(shapes), r_pad, host, nb), "sd_lora_plan_build")
    return host, torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev())


@functools.lru_cache(maxsize=None)
def _run(family, r_pad, form, fill=L.ZERO, rep=0):
    """One sd_lora_merge + sd_lora_project over one plan form of one family -> ({kind: output arena on the CPU}, layouts,
    operand dicts in plan order).  Asserts that no input arena changed.  Cached: the tests share the runs; `rep`
    asks for another run of the same thing."""
    lib = _lib.load_lib()
    ops, _ = L.family_operands(family, r_pad)
    order = L.plan_forms()[form]
    sel, shapes = [ops[i] for i in order], [L.TARGETS[i] for i in order]
    flats, lays = L.build_arenas(sel, r_pad, fill)
    d = {k: to_dev(v) for k, v in flats.items()}
    host, devp = _build(d, lays, shapes, r_pad)
    assert L.plan_header(host) == dict(n=len(sel), r_pad=r_pad, **L.count_items(shapes))
    _lib.check(lib.sd_lora_merge(devp.data_ptr(), host, _stream()), "sd_lora_merge")
    _lib.check(lib.sd_lora_project(devp.data_ptr(), host, _stream()), "sd_lora_project")
    torch.cuda.synchronize()
    for k in L.IN_KINDS:
        assert G.first_diff(d[k], flats[k]) is None, f"{k}: an input arena changed"
    return {k: d[k].cpu() for k in L.OUT_KINDS}, lays, sel


def _accept(family, r_pad, form, **kw):
    outs, lays, sel = _run(family, r_pad, form, **kw)
    bad = L.check_outputs(outs, lays, sel, family)
    assert not bad, f"{family} r_pad={r_pad} {form}: " + "; ".join(bad[:4])
    return outs, lays, sel


# ------------------------------------------------------------------------------------------------- the three products
@pytest.mark.parametrize("form", ["forward", "reverse"])
@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_exact_family(r_pad, form):
    """Integer operands whose every reference element is an integer within 256: w_out, d_a and d_b of all six targets must
    hold the bits of the fp64 product rounded once, no tolerance; every guard keeps its bits."""
    _accept("exact", r_pad, form)


@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_random_family(r_pad):
    """The value scales of test_gpu_lora.py, per element: |got - ref64| <= half_ulp(|ref| + d) + d,
    d = 2 K 2^-24 (|X| |Y| (+ |W_res|)), K = r_pad (merge), in (dB), out (dA).  The worst err / bound goes to the record."""
    outs, lays, sel = _run("random", r_pad, "forward")
    worst = L.worst_ratios(outs, lays, sel)
    record(f"lora_kernels_random_r{r_pad}", **worst)
    _accept("random", r_pad, "forward")
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_padded_rank(r_pad):
    """r = r_pad - 8 real rows, the padding of A and B zero: the padded rows of d_a and columns of d_b are zero, the real
    part holds the bits of the full-rank run (whose operands are the same draw), w_out is within the bound."""
    r = r_pad - 8
    outs, lays, sel = _accept("padded", r_pad, "forward")
    full, _, _ = _run("random", r_pad, "forward")
    record(f"lora_kernels_padded_r{r_pad}", **L.worst_ratios(outs, lays, sel))
    for i in range(len(sel)):
        d_a, d_b = L.piece(outs["d_a"], lays["d_a"], i), L.piece(outs["d_b"], lays["d_b"], i)
        assert bool((d_a[r:] == 0).all()) and bool((d_b[:, r:] == 0).all()), f"target {i}: padding of d_a / d_b is not zero"
        at = G.first_diff(d_a[:r], L.piece(full["d_a"], lays["d_a"], i)[:r])
        assert at is None, f"target {i}: d_a differs from the full product at {at}"
        at = G.first_diff(d_b[:, :r], L.piece(full["d_b"], lays["d_b"], i)[:, :r])
        assert at is None, f"target {i}: d_b differs from the full product at {at}"


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_plan_forms_hold_the_same_bits(r_pad, family):
    """The order above, its reverse, every target alone (plan_find with lo == hi) and a second run of the first: each
    target's w_out, d_a and d_b hold the same bits in all of them ("bit-identical on every data-parallel rank"), and no
    form touches a guard."""
    base, blays, _ = _accept(family, r_pad, "forward")
    runs = [("forward", 1)] + [(f, 0) for f in L.plan_forms() if f != "forward"]
    for form, rep in runs:
        outs, lays, sel = _run(family, r_pad, form, rep=rep)
        for k in L.OUT_KINDS:
            hit = L.gaps_untouched(outs[k], lays[k])
            assert hit is None, f"{form}: {k} arena changed at element {hit[0]}, in the gap behind plan target {hit[1]}"
            for pos, i in enumerate(L.plan_forms()[form]):
                at = G.first_diff(L.piece(outs[k], lays[k], pos), L.piece(base[k], blays[k], i))
                assert at is None, f"{k} of target {L.TARGETS[i]} in plan '{form}' differs from the forward plan at {at}"


@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_nothing_outside_a_targets_operands_reaches_its_result(r_pad):
    """The gaps of the five input arenas hold zeros, then +-3e4, then NaN: the three output arenas are bit-identical.  (The
    short dB block re-reads its row 0 for the dead rows; dA reads b_scaled in 32-row tiles.)"""
    base, lays, _ = _accept("random", r_pad, "forward")
    for fill in (LOUD, NAN):
        outs, _, _ = _run("random", r_pad, "forward", fill=fill)
        for k in L.OUT_KINDS:
            at = G.first_diff(outs[k], base[k])
            assert at is None, f"{k} arena with {fill} in the input gaps differs from the run with zeros at element {at}"


def test_refusals_of_the_plan_leave_memory_alone(lib):
    """sd_lora_plan_build with a null member, a member 2 bytes off and n <= 0, on device addresses: code and every byte of
    the host buffer.  sd_lora_merge / sd_lora_project on a host header with n = 0: SD_ERR_SHAPE, every output a sentinel."""
    ops, _ = L.family_operands("random", 32)
    flats, lays = L.build_arenas(ops, 32, L.ZERO)
    d = {k: to_dev(v) for k, v in flats.items()}
    assert L.plan_build_refusals(_lib, L.piece_ptrs(d, lays), L.TARGETS) == []
    host, devp = _build(d, lays, L.TARGETS, 32)
    empty = C.create_string_buffer(b"\0\0\0\0" + host.raw[4:], len(host.raw))
    assert L.plan_header(empty)["n"] == 0 and L.plan_header(empty)["merge"] == 17
    assert lib.sd_lora_merge(devp.data_ptr(), empty, _stream()) == -1
    assert lib.sd_lora_project(devp.data_ptr(), empty, _stream()) == -1
    assert lib.sd_lora_merge(None, host, _stream()) == -1 and lib.sd_lora_project(devp.data_ptr(), None, _stream()) == -1
    torch.cuda.synchronize()
    for k in L.IN_KINDS + L.OUT_KINDS:
        assert G.first_diff(d[k], flats[k]) is None, k


# ------------------------------------------------------------------------------------------------- fp32-master AdamW
PAD = 8  # guard elements on either side of every slice (32 bytes of fp32, 16 of bf16: the slices stay aligned)


def _adamw_buffers(n, set_name):
    """-> host dict p, m, v (fp32, sentinel guards), g (bf16, +-3e4 guards), s1, s2 (bf16, all sentinel), and (ss, mx)"""
    (p, g, m, v), clip = L.adamw32_inputs(n, set_name)
    host = {}
    for k, t in (("p", p), ("m", m), ("v", v)):
        host[k] = G.filled((n + 2 * PAD,), SENTINEL, torch.float32)
        host[k][PAD:PAD + n] = t
    host["g"] = G.filled((n + 2 * PAD,), LOUD)
    host["g"][PAD:PAD + n] = g
    host["s1"], host["s2"] = G.filled((n + 2 * PAD,), SENTINEL), G.filled((n + 2 * PAD,), SENTINEL)
    return host, clip


def _adamw_call(lib, d, n, set_name, ss, mx, off=None, n_arg=None, step=None):
    """sd_adamw_f32_shadow on the slices [PAD + off[k] : ...] of the device buffers -> return code"""
    lr, b1, b2, eps, wd, st = P.adamw_hp(set_name)
    off = off or {}
    ptr = {k: d[k].data_ptr() + (PAD + off.get(k, 0)) * d[k].element_size() for k in d}
    ss_dev = None if ss is None else torch.tensor([ss], dtype=torch.float32, device=dev())
    rc = lib.sd_adamw_f32_shadow(ptr["p"], ptr["g"], ptr["m"], ptr["v"], ptr["s1"], ptr["s2"], L.ADAMW32_SCALE,
                                 n if n_arg is None else n_arg, lr, b1, b2, eps, wd, st if step is None else step,
                                 None if ss_dev is None else ss_dev.data_ptr(), mx, _stream())
    torch.cuda.synchronize()
    return rc


def _adamw_run(lib, n, set_name, clip=True):
    """-> (p, m, v, s1, s2) slices on the CPU after one call; asserts the guards of all five and the whole gradient."""
    host, (ss, mx) = _adamw_buffers(n, set_name)
    d = {k: to_dev(t) for k, t in host.items()}
    _lib.check(_adamw_call(lib, d, n, set_name, ss if clip else None, mx if clip else 0.0), "sd_adamw_f32_shadow")
    back = {k: t.cpu() for k, t in d.items()}
    for k in ("p", "m", "v", "s1", "s2"):
        for sl in (slice(0, PAD), slice(PAD + n, None)):
            assert G.first_diff(back[k][sl], host[k][sl]) is None, f"{k}: wrote outside its {n} elements"
    assert G.first_diff(back["g"], host["g"]) is None, "the gradient changed"
    return [back[k][PAD:PAD + n] for k in ("p", "m", "v", "s1", "s2")]


def _check_adamw32(lib, n, set_name):
    ref = L.adamw32_ref(n, set_name)
    p, m, v, s1, s2 = _adamw_run(lib, n, set_name)
    verdicts = L.adamw32_close((p, m, v), ref)
    record(f"lora_adamw32_{set_name}_n{n}", floor=L.ADAMW32_FLOOR, fp32_measured=L.ADAMW32_MEASURED,
           **{k: x.worst_rel for k, x in verdicts.items()})
    for k, x in verdicts.items():
        assert x.ok, f"{set_name} n={n} {k}: {x}"
    w1, w2 = L.shadows_of(p)
    at = G.first_diff(s1, w1)
    assert at is None, f"{set_name} n={n}: shadow != bf16(p) at {at}"
    at = G.first_diff(s2, w2)
    assert at is None, f"{set_name} n={n}: scaled shadow != bf16(p * {L.ADAMW32_SCALE}) at {at}"
    if P.ADAMW_SETS[set_name]["clip"] in ("zero", "below"):  # a clip of exactly 1 is the call without a norm, bit for bit
        plain = _adamw_run(lib, n, set_name, clip=False)
        assert all(G.first_diff(a, b) is None for a, b in zip((p, m, v, s1, s2), plain)), (set_name, n)


@pytest.mark.parametrize("set_name", list(P.ADAMW_SETS))
def test_adamw32_small_sizes(lib, set_name):
    """n = 4 (one vector), 8, 1020 (255 threads of one workgroup), 1028 (a second workgroup with one thread): p, m, v per
    element against fp64 at the measured fp32 floor, every clip branch, both shadows from the GPU's own p bit for bit,
    neighbours untouched."""
    for n in L.ADAMW32_SMALL:
        _check_adamw32(lib, n, set_name)


@pytest.mark.parametrize("set_name", P.ADAMW_BIG_SETS)
@pytest.mark.parametrize("n", L.ADAMW32_BIG)
def test_adamw32_grid_stride_wrap(lib, n, set_name):
    """More vectors than 4096 x 256 threads: one thread takes a second trip (n = 4 194 308); every thread two and 149 of
    them three (n = 8 389 204), as the real adapter's ~20 M elements do."""
    assert L.adamw32_trips(n)[2] >= 2
    _check_adamw32(lib, n, set_name)


ADAMW32_REFUSALS = {  # name -> (what the call changes, the code: SD_ERR_SHAPE -1, SD_ERR_ALIGN -2)
    "n_mod_4": (dict(n_arg=1026), -1), "n_zero": (dict(n_arg=0), -1), "n_negative": (dict(n_arg=-4), -1),
    "step_zero": (dict(step=0), -1), "step_negative": (dict(step=-1), -1),
    "param_plus_1_float": (dict(off={"p": 1}), -2), "exp_avg_plus_1_float": (dict(off={"m": 1}), -2),
    "exp_avg_sq_plus_1_float": (dict(off={"v": 1}), -2), "grad_plus_1_bf16": (dict(off={"g": 1}), -2),
    "shadow_plus_1_bf16": (dict(off={"s1": 1}), -2), "shadow_scaled_plus_1_bf16": (dict(off={"s2": 1}), -2),
}


@pytest.mark.parametrize("name", list(ADAMW32_REFUSALS))
def test_adamw32_refusals_leave_memory_alone(lib, name):
    """SD_ERR_SHAPE / SD_ERR_ALIGN, and p, m, v, both shadows and the gradient keep every byte."""
    kw, want = ADAMW32_REFUSALS[name]
    n = 1024
    host, (ss, mx) = _adamw_buffers(n, "step3_above")
    d = {k: to_dev(t) for k, t in host.items()}
    assert _adamw_call(lib, d, n, "step3_above", ss, mx, **kw) == want, name
    for k, t in host.items():
        assert G.first_diff(d[k], t) is None, f"{name}: {k} changed"
