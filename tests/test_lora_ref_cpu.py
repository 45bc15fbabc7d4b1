"""The tests of tests/test_gpu_lora_kernels.py's own tools (tests/lora_ref.py), on the CPU.

They show that the targets yield the item counts the tests are named for, by arithmetic of their own and by the plan
builder (host code of the library, no GPU needed); that the exact family stays within 256 everywhere; that a plain fp32
restatement of the three products passes the exact family bit for bit and the random family's derived bound; that every
wrong restatement of lora_ref.MUTANTS is rejected by the check named for it; that the packed arenas are laid out as the
GPU test needs them; and that the fp32 AdamW's floor is what the fp32 evaluation measures, with the hyper-parameter sets'
`kills` rejected at it.
"""
import ctypes as C

import pytest
import torch

import gemm_ref as G
import lora_ref as L
import parity_ref as P
from gemm_ref import BF, SENTINEL
from speech_distill_amd import _lib
from test_parity_ref_cpu import adamw_variant


# ------------------------------------------------------------------------------------------------- targets and the plan
def test_item_counts_by_own_arithmetic():
    assert L.count_items(L.TARGETS) == L.ITEMS == dict(merge=17, db=22, da=10)
    # per target, written out: (merge, dB, dA) items
    each = [L.count_items([t]) for t in L.TARGETS]
    assert [(c["merge"], c["db"], c["da"]) for c in each] == [(1, 1, 1), (1, 1, 1), (2, 2, 2), (1, 4, 1), (6, 5, 3), (6, 9, 2)]
    assert (-17) % 4 == 3                                              # waves of the last merge workgroup without an item
    assert [o % 64 for o, _ in L.TARGETS] == [32, 0, 32, 0, 32, 32]    # which targets end in a short dB block
    assert sorted({i // 128 for _, i in L.TARGETS}) == [1, 2, 3]       # K tiles of dB: none, one and two buffer swaps
    assert [-(-o // 256) for o, _ in L.TARGETS] == [1, 1, 1, 1, 2, 3]  # merge row chunks
    forms = L.plan_forms()
    assert forms["forward"] == forms["reverse"][::-1] and len(forms) == 2 + len(L.TARGETS)


@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_plan_builder_writes_the_same_counts(r_pad):
    """sd_lora_plan_build's header (five int32 at the front of the plan, as sd_lora.hip states PlanHeader) for every plan
    form, against count_items on that form's targets."""
    lib = _lib.load_lib()
    ops, _ = L.family_operands("exact", r_pad)
    for name, order in L.plan_forms().items():
        sel = [ops[i] for i in order]
        shapes = [L.TARGETS[i] for i in order]
        flats, lays = L.build_arenas(sel, r_pad, L.ZERO)
        arr = L.plan_struct(_lib, L.piece_ptrs(flats, lays), shapes)
        nb = lib.sd_lora_plan_bytes(len(sel))
        assert nb == 32 + 96 * len(sel)
        host = C.create_string_buffer(nb)
        assert lib.sd_lora_plan_build(arr, len(sel), r_pad, host, nb) == 0, name
        want = L.count_items(shapes)
        assert L.plan_header(host) == dict(n=len(sel), r_pad=r_pad, **want), name
    assert lib.sd_lora_plan_bytes(0) == 0


def test_refused_plan_builds_leave_the_buffer_alone():
    ops, _ = L.family_operands("exact", 32)
    flats, lays = L.build_arenas(ops, 32, L.ZERO)
    assert L.plan_build_refusals(_lib, L.piece_ptrs(flats, lays), L.TARGETS) == []


# ------------------------------------------------------------------------------------------------- arenas
@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_arena_layout(r_pad):
    """Pieces back to back in plan order with 64 rows of their own row length between them, in front and behind; every
    piece 16-byte aligned; the guard check names the offset and the target whose tail the gap follows."""
    for order in (L.plan_forms()["forward"], L.plan_forms()["reverse"], [2]):
        shapes = [L.TARGETS[i] for i in order]
        for kind in L.IN_KINDS + L.OUT_KINDS:
            lay = L.layout(kind, shapes, r_pad)
            assert len(lay.pieces) == len(shapes) and len(lay.gaps) == len(shapes) + 1
            end = 0
            for i, (off, rows, cols) in enumerate(lay.pieces):
                assert (rows, cols) == L.piece_shape(kind, *shapes[i], r_pad)
                start, stop, after = lay.gaps[i]
                assert start == end and stop == off and after == i - 1
                assert stop - start == 64 * lay.pieces[max(i - 1, 0)][2]  # rows of the piece in front (the first: its own)
                assert (2 * off) % 16 == 0
                end = off + rows * cols
            start, stop, after = lay.gaps[-1]
            assert start == end and stop == lay.total and stop - start == 64 * lay.pieces[-1][2] and after == len(shapes) - 1
    lay = L.layout("d_b", L.TARGETS, r_pad)
    flat = L.pack(lay, None, SENTINEL)
    assert L.gaps_untouched(flat, lay) is None
    L.piece(flat, lay, 3).fill_(1.0)                      # writing a piece is not a guard failure
    assert L.gaps_untouched(flat, lay) is None
    off, rows, cols = lay.pieces[2]
    flat[off + rows * cols + 5] = 0.0
    flat[lay.total - 1] = 0.0
    assert L.gaps_untouched(flat, lay) == (off + rows * cols + 5, 2)
    flat = L.pack(lay, None, SENTINEL)
    flat[3] = float("nan")                                # another NaN is not the sentinel
    assert L.gaps_untouched(flat, lay) == (3, -1)
    for fill in (L.ZERO, L.LOUD, L.NAN):
        x = L.fill_flat(16, fill)
        assert bool((x == 0).all()) if fill == L.ZERO else bool((x.float().abs() > 1e4).all() | x.isnan().all())


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_exact_family_is_within_256_and_exact(r_pad):
    ops, scale = L.family_operands("exact", r_pad)
    assert scale == 2.0
    for t, (out_f, in_f) in zip(ops, L.TARGETS):
        assert torch.equal(t["a_sc"].float(), 2 * t["a_sh"].float())
        for k in ("a_sh", "b_sc", "w_grad"):
            x = t[k].float()
            assert torch.equal(x, x.round()) and float(x.abs().max()) <= 3 and float(x[0].mean()) > float(x[1:].mean()) + 0.1
            assert float(x[:, 0].mean()) > float(x[:, 1:].mean())  # a column of w_grad may hold 32 thinned values only
        assert float(t["w_res"].float().abs().max()) <= 102
        for kind in L.OUT_KINDS:
            ref = L.ref64(kind, t)
            assert float(ref.abs().max()) <= L.EXACT_LIMIT, (kind, out_f, in_f, float(ref.abs().max()))
            want = L.exact_expect(kind, t)
            assert torch.equal(want.double(), ref + 0.0) and torch.equal(ref, ref.round())   # the rounding moves nothing
            assert float(ref.abs().max()) >= 3 and float((ref != 0).double().mean()) > 0.3   # and the data is not trivial
            assert tuple(ref.shape) == L.piece_shape(kind, out_f, in_f, r_pad)


@pytest.mark.parametrize("r_pad", L.R_PADS)
@pytest.mark.parametrize("form", ["forward", "reverse", "alone2"])
def test_restatement_passes_both_families(r_pad, form):
    """fp32 torch products, rounded once: bit-equal to the exact family's expectation, and within the random family's
    derived bound (worst err / bound <= 1): the bound is passable before a GPU sees it."""
    order = L.plan_forms()[form]
    for family in ("exact", "random", "padded"):
        ops, scale = L.family_operands(family, r_pad)
        sel = [ops[i] for i in order]
        flats, lays = L.emulate_plan(sel, scale, r_pad)
        assert L.check_outputs(flats, lays, sel, family) == [], (family, form)
        if family != "exact":
            worst = L.worst_ratios(flats, lays, sel)
            assert all(0 < v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("r_pad", L.R_PADS)
def test_padded_rank_operands(r_pad):
    """r = r_pad - 8: the padding of A and B is zero and everything else is the full draw, so the padded rows of d_a and
    columns of d_b are zero and the real part is the full product's, bit for bit."""
    full, scale = L.family_operands("random", r_pad)
    pad, _ = L.family_operands("padded", r_pad)
    r = r_pad - 8
    for f, p in zip(full, pad):
        assert torch.equal(p["a_sh"][:r], f["a_sh"][:r]) and float(p["a_sh"][r:].abs().max()) == 0 == float(p["a_sc"][r:].abs().max())
        assert torch.equal(p["b_sc"][:, :r], f["b_sc"][:, :r]) and float(p["b_sc"][:, r:].abs().max()) == 0
        rf, rp = L.restate(f, scale), L.restate(p, scale)
        assert G.first_diff(rp["d_a"][:r], rf["d_a"][:r]) is None and G.first_diff(rp["d_b"][:, :r], rf["d_b"][:, :r]) is None
        assert bool((rp["d_a"][r:] == 0).all()) and bool((rp["d_b"][:, r:] == 0).all())
        assert not torch.equal(rp["w_out"], rf["w_out"])


def test_the_bound_rejects_one_and_a_half_half_ulps():
    ops, scale = L.family_operands("random", 32)
    t = ops[2]
    for kind in L.OUT_KINDS:
        ref = L.ref64(kind, t)
        got = ref.clone()
        assert L.judge(kind, got.to(BF), t).ok
        got[1, 3] += 1.5 * float(P.half_ulp(ref, BF)[1, 3]) + 2 * float(L.bound(kind, t)[1, 3] - P.half_ulp(ref, BF)[1, 3])
        v = L.judge(kind, got, t)
        assert not v.ok and (v.row, v.col) == (1, 3)


# ------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("r_pad", L.R_PADS)
@pytest.mark.parametrize("mutant", list(L.MUTANTS))
def test_every_mutant_is_rejected_by_its_check(mutant, r_pad):
    """In both plan orders, by the exact family and by the random family; by the guards alone for the write-bounds
    mutant, by the values alone for every other.  neighbour_a needs a neighbour: a plan of one target computes right."""
    want = L.MUTANTS[mutant][1]
    for family in ("exact", "random"):
        ops, scale = L.family_operands(family, r_pad)
        for form in ("forward", "reverse"):
            sel = [ops[i] for i in L.plan_forms()[form]]
            bad = L.check_outputs(*L.emulate_plan(sel, scale, r_pad, mutant), sel, family)
            assert bad and all(b.startswith(want + ":") for b in bad), (mutant, family, form, bad[:2])
    if want == "guards":
        flats, lays = L.emulate_plan(ops, scale, r_pad, mutant)
        # rows 32..63 of the short block of target 0 are the first 32 rows behind its d_b
        assert L.gaps_untouched(flats["d_b"], lays["d_b"]) == (lays["d_b"].pieces[0][0] + 32 * r_pad, 0)
    if mutant == "neighbour_a":
        assert L.check_outputs(*L.emulate_plan(ops[:1], scale, r_pad, mutant), ops[:1], "random") == []


def test_mutant_table_names_what_the_issue_lists():
    assert set(L.MUTANTS) == {"merge_a_scaled", "merge_no_wres", "db_a_shadow", "da_unscaled_b", "rank_reversed",
                              "cols8_reversed", "db_short_store", "db_dead_rows_sum", "neighbour_a"}
    assert [m for m, (_, c) in L.MUTANTS.items() if c == "guards"] == ["db_short_store"]


# ------------------------------------------------------------------------------------------------- fp32-master AdamW
def test_adamw32_sizes_reach_the_trips_they_are_named_for():
    assert L.ADAMW32_SIZES == (4, 8, 1020, 1028, 4194308, 8389204)
    for n in L.ADAMW32_SIZES:
        assert n % 4 == 0 and L.adamw32_trips(n) == L.ADAMW32_TRIPS[n], n
    # by hand: 1 048 577 vectors on 1 048 576 threads, one thread goes twice; 2 097 301: threads 0..148 three times
    assert 4194308 // 4 - 4096 * 256 == 1 and 8389204 // 4 - 2 * 4096 * 256 == 149
    cases = L.adamw32_cases()
    assert len(cases) == 4 * len(P.ADAMW_SETS) + 2 * len(P.ADAMW_BIG_SETS)
    (p, g, m, v), _ = L.adamw32_inputs(1028, "step3_none")
    assert p.dtype == m.dtype == v.dtype == torch.float32 and g.dtype == BF
    assert not torch.equal(p, p.bfloat16().float()) and not torch.equal(v, v.bfloat16().float())  # the state is NOT bf16-rounded


def test_adamw32_floor_is_what_the_fp32_evaluation_measures():
    """Re-measured on every input of the GPU test (25 % slack for another libm); the floor is 4 x the measurement."""
    m = L.measure_adamw32_floor()
    assert 0 < m <= 1.25 * L.ADAMW32_MEASURED, (m, L.ADAMW32_MEASURED)
    assert 4 * L.ADAMW32_MEASURED <= L.ADAMW32_FLOOR * (1 + 1e-9) and L.ADAMW32_FLOOR <= 4.1 * L.ADAMW32_MEASURED
    assert L.ADAMW32_FLOOR <= 2e-5


@pytest.mark.parametrize("n", L.ADAMW32_SMALL)
@pytest.mark.parametrize("set_name", list(P.ADAMW_SETS))
def test_adamw32_comparator_accepts_fp32_and_rejects_the_kills(set_name, n):
    """The fp32 evaluation (what a correct kernel delivers) passes; every wrong formula the set names, delivered as fp32,
    fails.  n = 4 and 8 hold too few elements for every mistake to show in every draw: there a kill must show on at
    least the larger sizes, and the reference must still pass."""
    (p, g, m, v), (ss, mx) = L.adamw32_inputs(n, set_name)
    hp = P.adamw_hp(set_name)
    ref = L.adamw32_ref(n, set_name)
    assert all(x.ok for x in L.adamw32_close([t.float() for t in ref], ref).values())
    r32 = L.adamw32_ref(n, set_name, acc=torch.float32)
    verdicts = L.adamw32_close(r32, ref)
    assert all(x.ok for x in verdicts.values()), verdicts
    if n < 1000:
        return
    for mut in P.ADAMW_SETS[set_name]["kills"]:
        wrong = [t.float() for t in adamw_variant(mut, p, g, m, v, *hp, sumsq=ss, max_norm=mx)]
        assert not all(x.ok for x in L.adamw32_close(wrong, ref).values()), (set_name, mut, n)
    if P.ADAMW_SETS[set_name]["clip"] in ("none", "zero", "below"):
        assert all(torch.equal(a, b) for a, b in zip(P.adamw_ref64(p, g, m, v, *hp), ref))


def test_shadows_of_rounds_once_from_fp32():
    p = torch.tensor([1.0 + 2.0 ** -9, 0.3, -7.77, 1e-3])
    s1, s2 = L.shadows_of(p)
    assert torch.equal(s1, p.bfloat16()) and torch.equal(s2, (p * 11.3125).bfloat16())
    q = torch.randn(1000, generator=torch.Generator().manual_seed(5))   # the scaled shadow is taken from p, not from bf16(p)
    assert not torch.equal(L.shadows_of(q)[1], (q.bfloat16().float() * 11.3125).bfloat16())
