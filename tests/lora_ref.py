"""Targets, packed arenas, operands, expectations and wrong restatements of tests/test_gpu_lora_kernels.py: the three
MFMA kernels of csrc/sd_lora.hip (merge, dB, dA), their plan, and the fp32-master AdamW.

TEST INFRASTRUCTURE ONLY, CPU only (never imported by the product, no GPU in it; the ctypes binding is handed in by the
caller where host code of the library is called).  tests/test_lora_ref_cpu.py shows on the CPU that the item counts of
TARGETS are what the plan builder writes, that the exact family stays within EXACT_LIMIT, that a plain fp32 restatement
passes the random family's bound, that every entry of MUTANTS is rejected by the check named for it, and that the AdamW
floor is what the fp32 evaluation measures.

The three products of one target (A [r_pad, in], B [out, r_pad], W and dW [out, in]; `PRODUCTS`):
    w_out = w_res + b_sc a_sh        K = r_pad        (sd_lora_merge)
    d_b   = w_grad a_sc^T            K = in           (sd_lora_project, lora_db_kernel)
    d_a   = b_sc^T w_grad            K = out          (sd_lora_project, lora_da_kernel)
Exact family: integers chosen so that every reference element is an integer of magnitude <= 256, exact in bf16 and in the
fp32 accumulator whatever the order of the sum: the GPU result must hold the bits of gemm_ref.int_expect.  Random family:
gemm_ref.elem_bound per element, d = 2 K 2^-24 (|X| |Y| (+ |W_res|)), bound = half_ulp(|ref| + d) + d.
"""
from __future__ import annotations

import collections
import functools
import math

import torch

import gemm_ref as G
import parity_ref as P
from gemm_ref import BF, LOUD, NAN, SENTINEL
from rowk_ref import elem_close

ZERO = "zero"
R_PADS = (32, 64, 128)
# (out, in) in plan order, with what each reaches (kMergeRows = 256, kColBlock = 128, kDbRows = 64, dA walks 32 rows a step)
TARGETS = [
    (32, 128),    # one merge item; a dB block that is only the short 32 rows; dA with a single row step; one K tile
    (64, 128),    # exactly one full dB block
    (96, 256),    # dB 64 + 32 rows; two K tiles (one buffer swap); two column blocks; three dA row steps
    (256, 128),   # exactly one 256-row merge chunk
    (288, 384),   # merge chunk 256 + 32; three K tiles (the LDS buffer comes back to 0); three column blocks
    (544, 256),   # three merge chunks; eight full dB blocks and a short one
]
ITEMS = dict(merge=17, db=22, da=10)  # of TARGETS; 17 merge items: the last workgroup has three waves without one
HEADER_FIELDS = ("n", "r_pad", "merge", "db", "da")  # PlanHeader of sd_lora.hip: five int32 at byte 0, 4, 8, 12, 16
IN_KINDS = ("w_res", "w_grad", "a_sh", "a_sc", "b_sc")
OUT_KINDS = ("w_out", "d_a", "d_b")
GAP_ROWS = 64  # rows of the piece's own row length between two pieces of an arena, at its head and at its tail


def count_items(targets):
    """The work items of a plan, counted tile by tile (no ceiling division shared with the plan builder)."""
    merge = db = da = 0
    for out_f, in_f in targets:
        cols = [c for c in range(0, in_f, 128)]
        merge += sum(1 for _r in range(0, out_f, 256) for _c in cols)
        db += sum(1 for _r in range(0, out_f, 64))
        da += len(cols)
    return dict(merge=merge, db=db, da=da)


def plan_forms():
    """{name: [indices into TARGETS in plan order]}: the order above, the reverse, each target alone."""
    n = len(TARGETS)
    forms = {"forward": list(range(n)), "reverse": list(range(n - 1, -1, -1))}
    forms.update({f"alone{i}": [i] for i in range(n)})
    return forms


# ------------------------------------------------------------------------------------------------- arenas
Layout = collections.namedtuple("Layout", "kind total pieces gaps")  # pieces (off, rows, cols); gaps (start, stop, after)


def piece_shape(kind, out_f, in_f, r_pad):
    if kind in ("w_res", "w_out", "w_grad"):
        return out_f, in_f
    return (r_pad, in_f) if kind in ("a_sh", "a_sc", "d_a") else (out_f, r_pad)


def layout(kind, shapes, r_pad):
    """One arena of a buffer kind: the targets' pieces back to back in plan order, a gap of GAP_ROWS rows of the piece's
    row length after every piece and one in front of the first (after = -1).  Offsets in elements."""
    first = piece_shape(kind, *shapes[0], r_pad)[1]
    gaps, pieces, off = [(0, GAP_ROWS * first, -1)], [], GAP_ROWS * first
    for i, (out_f, in_f) in enumerate(shapes):
        rows, cols = piece_shape(kind, out_f, in_f, r_pad)
        pieces.append((off, rows, cols))
        off += rows * cols
        gaps.append((off, off + GAP_ROWS * cols, i))
        off += GAP_ROWS * cols
    return Layout(kind, off, pieces, gaps)


def fill_flat(n, fill):
    return torch.zeros(n, dtype=BF) if fill == ZERO else G.filled((n,), fill)


def pack(lay, tensors, fill):
    """-> flat bf16 arena: `fill` everywhere, then the pieces (tensors None: an output arena, all `fill`)."""
    flat = fill_flat(lay.total, fill)
    for (off, rows, cols), t in zip(lay.pieces, tensors or ()):
        assert tuple(t.shape) == (rows, cols), (lay.kind, t.shape, rows, cols)
        flat[off:off + rows * cols] = t.reshape(-1)
    return flat


def piece(flat, lay, i):
    off, rows, cols = lay.pieces[i]
    return flat[off:off + rows * cols].view(rows, cols)


def gaps_untouched(flat, lay):
    """None when every gap element of an output arena still holds the sentinel's bits, else (first changed offset, the
    plan index of the target whose tail the gap follows; -1: the gap in front of the first target)."""
    b = G.bits(flat.cpu())
    for start, stop, after in lay.gaps:
        bad = (b[start:stop] != G.SENTINEL_BITS[BF]).nonzero()
        if len(bad):
            return start + int(bad[0]), after
    return None


# ------------------------------------------------------------------------------------------------- operands
EXACT_LIMIT = 256
EXACT_SCALE = 2.0       # a_sc = 2 a_sh: taking the wrong one of the two shows
EXACT_DENSITY = dict(a=0.5, b=0.5, g=0.25)  # share of non-zeros kept, so that the raised row 0 / column 0 stay within the limit


def _seed(*key):
    s = 97
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _raised(x):
    """row 0 and column 0 one higher (gemm_ref.int_operands' asymmetry, on both axes: a transposition or a mirrored block
    shows)"""
    x[0, :] += 1.0
    x[:, 0] += 1.0
    return x


def exact_operands(out_f, in_f, r_pad, seed=0):
    """a_sh, b_sc, w_grad in {-1, 0, 1}, w_res in [-100, 100], row 0 and column 0 raised by one, then thinned (the raised
    line included: its mean stays positive), a_sc = 2 a_sh.  Every reference element of the three products stays within
    EXACT_LIMIT at the seeds the tests use (asserted on the CPU): a condition on these inputs."""
    gen = _seed(out_f, in_f, r_pad, seed)
    tri = (lambda r, c, keep: _raised(torch.randint(-1, 2, (r, c), generator=gen).float())
           * (torch.rand(r, c, generator=gen) < keep).float() + 0.0)  # + 0.0: a thinned -1 is +0, not -0
    a = tri(r_pad, in_f, EXACT_DENSITY["a"])
    b = tri(out_f, r_pad, EXACT_DENSITY["b"])
    g = tri(out_f, in_f, EXACT_DENSITY["g"])
    w = _raised(torch.randint(-100, 101, (out_f, in_f), generator=gen).float())
    return dict(w_res=w.to(BF), w_grad=g.to(BF), a_sh=a.to(BF), a_sc=(EXACT_SCALE * a).to(BF), b_sc=b.to(BF))


def lora_scale(r_pad):
    return 64 / math.sqrt(r_pad)


def random_operands(out_f, in_f, r_pad, seed=0, r=None):
    """The value scales of tests/test_gpu_lora.py: w_res 0.05, w_grad 0.01, A and B 0.05, scale = 64 / sqrt(r_pad).
    r < r_pad: rows r.. of A and columns r.. of B are zero, as lora.py holds the padding; everything else is the same
    draw as with r = None."""
    gen = _seed(out_f, in_f, r_pad, seed, 7)
    A, B = torch.randn(r_pad, in_f, generator=gen) * 0.05, torch.randn(out_f, r_pad, generator=gen) * 0.05
    w = (torch.randn(out_f, in_f, generator=gen) * 0.05).to(BF)
    g = (torch.randn(out_f, in_f, generator=gen) * 0.01).to(BF)
    if r is not None:
        A[r:] = 0.0
        B[:, r:] = 0.0
    s = lora_scale(r_pad)
    return dict(w_res=w, w_grad=g, a_sh=A.to(BF), a_sc=(A * s).to(BF), b_sc=(B * s).to(BF))


@functools.lru_cache(maxsize=None)
def family_operands(family, r_pad):
    """-> ([operand dict per entry of TARGETS], scale): "exact", "random" or "padded" (r = r_pad - 8)."""
    if family == "exact":
        return [exact_operands(o, i, r_pad) for o, i in TARGETS], EXACT_SCALE
    r = r_pad - 8 if family == "padded" else None
    return [random_operands(o, i, r_pad, r=r) for o, i in TARGETS], lora_scale(r_pad)


# ------------------------------------------------------------------------------------------------- expectations
def product_args(kind, t):
    """-> (a, b, ta, tb, r, K) of gemm_ref.ref64 / int_expect / elem_bound for one output of one target"""
    if kind == "w_out":
        return t["b_sc"], t["a_sh"], False, True, t["w_res"], t["a_sh"].shape[0]
    if kind == "d_b":
        return t["w_grad"], t["a_sc"], False, False, None, t["w_grad"].shape[1]
    return t["b_sc"], t["w_grad"], True, True, None, t["w_grad"].shape[0]


def ref64(kind, t):
    return G.ref64(*product_args(kind, t)[:5])


def exact_expect(kind, t):
    """gemm_ref.int_expect's rule: fp64 product, + 0.0, one rounding"""
    return G.int_expect(*product_args(kind, t)[:5])


def bound(kind, t):
    return G.elem_bound(*product_args(kind, t))


def judge(kind, got, t):
    """-> rowk_ref.Elem: |got - ref64| <= bound per element, .ratio the worst err / bound"""
    return elem_close(got, ref64(kind, t), bound(kind, t))


# ------------------------------------------------------------------------------------------------- restatement, mutants
# name -> (what is wrong, the check that must reject it: "values" in both families, or "guards")
MUTANTS = {
    "merge_a_scaled": ("merge takes a_scaled: the scale is applied twice.  Fails both families", "values"),
    "merge_no_wres": ("merge without W_res.  Fails both families", "values"),
    "db_a_shadow": ("dB takes a_shadow: the scale is missing.  Fails both families", "values"),
    "da_unscaled_b": ("dA takes B without its scale.  Fails both families", "values"),
    "rank_reversed": ("B A with the rank axis of A reversed.  Fails both families", "values"),
    "cols8_reversed": ("the 8 columns a lane stores in merge come out in reversed order.  Fails both families", "values"),
    "db_short_store": ("a short dB block stores its rows 32..63: they land behind the target's d_b.  Every value is right: "
                       "only the guards see it", "guards"),
    "db_dead_rows_sum": ("the dead rows of a short dB block (which re-read the block's row 0) are added to its live rows.  "
                         "Fails both families", "values"),
    "neighbour_a": ("a target is computed with the A of a plan neighbour of the same width (targets (32, 128) and "
                    "(64, 128)).  Fails both families in every plan of more than one target", "values"),
}


def _short_row0(out_f):
    """first row of the short last dB block, or None"""
    return out_f - 32 if out_f % 64 else None


def restate(t, scale, mutant=None, neighbour=None):
    """The three products of one target in plain fp32 torch, rounded once -> dict(w_out, d_a, d_b, spill): spill are rows
    a wrong kernel stores behind d_b (None for every restatement but db_short_store)."""
    f = {k: v.float() for k, v in t.items()}
    a_sh, a_sc = f["a_sh"], f["a_sc"]
    if mutant == "neighbour_a" and neighbour is not None:
        a_sh, a_sc = neighbour["a_sh"].float(), neighbour["a_sc"].float()
    a_m = a_sc if mutant == "merge_a_scaled" else a_sh
    if mutant == "rank_reversed":
        a_m = a_m.flip(0)
    w = f["b_sc"] @ a_m + (0.0 if mutant == "merge_no_wres" else f["w_res"])
    if mutant == "cols8_reversed":
        w = w.view(w.shape[0], -1, 8).flip(-1).reshape(w.shape)
    x = f["w_grad"].clone()
    row0 = _short_row0(x.shape[0])
    if mutant == "db_dead_rows_sum" and row0 is not None:
        x[row0:] += x[row0].clone()
    d_b = x @ (a_sh if mutant == "db_a_shadow" else a_sc).T
    b = (f["b_sc"] / scale).to(BF).float() if mutant == "da_unscaled_b" else f["b_sc"]
    d_a = b.T @ f["w_grad"]
    spill = None
    if mutant == "db_short_store" and row0 is not None:
        spill = (f["w_grad"][row0:row0 + 1] @ a_sc.T).expand(32, -1).to(BF)
    return dict(w_out=(w + 0.0).to(BF), d_a=(d_a + 0.0).to(BF), d_b=(d_b + 0.0).to(BF), spill=spill)


def emulate_plan(ops, scale, r_pad, mutant=None):
    """What one merge + project over the plan `ops` (operand dicts in plan order) leaves in the three output arenas,
    which start as sentinels -> ({kind: flat arena}, {kind: Layout})."""
    shapes = [tuple(t["w_res"].shape) for t in ops]
    lays = {k: layout(k, shapes, r_pad) for k in OUT_KINDS}
    flats = {k: pack(lays[k], None, SENTINEL) for k in OUT_KINDS}
    for i, t in enumerate(ops):
        nb = next((ops[j] for j in (i + 1, i - 1) if 0 <= j < len(ops) and shapes[j][1] == shapes[i][1]), None)
        res = restate(t, scale, mutant, nb)
        for k in OUT_KINDS:
            piece(flats[k], lays[k], i).copy_(res[k])
        if res["spill"] is not None:
            off, rows, cols = lays["d_b"].pieces[i]
            flats["d_b"][off + rows * cols:off + (rows + 32) * cols] = res["spill"].reshape(-1)
    return flats, lays


def check_outputs(flats, lays, ops, family):
    """The checks the GPU test applies to one run -> list of failure texts (empty: accepted).  Guards first; then the
    values: bit equality with exact_expect ("exact"), else the per-element bound."""
    bad = []
    for k in OUT_KINDS:
        hit = gaps_untouched(flats[k], lays[k])
        if hit is not None:
            bad.append(f"guards: {k} arena changed at element {hit[0]}, in the gap behind plan target {hit[1]}")
    for i, t in enumerate(ops):
        for k in OUT_KINDS:
            got = piece(flats[k], lays[k], i).cpu()
            if family == "exact":
                want = exact_expect(k, t)
                at = G.first_diff(got, want)
                if at is not None:
                    n = int((G.bits(got) != G.bits(want)).sum())
                    bad.append(f"values: {k} of plan target {i} {tuple(t['w_res'].shape)}: {n} elements differ, first at "
                               f"{at}: got {float(got[at])}, want {float(want[at])}")
            else:
                v = judge(k, got, t)
                if not v.ok:
                    bad.append(f"values: {k} of plan target {i} {tuple(t['w_res'].shape)}: {v}")
    return bad


def worst_ratios(flats, lays, ops):
    """{kind: worst err / bound over every target} of a random-family run"""
    return {k: max(judge(k, piece(flats[k], lays[k], i).cpu(), t).ratio for i, t in enumerate(ops)) for k in OUT_KINDS}


def plan_struct(_lib, ptrs, shapes):
    """ctypes array of SdLoraTarget from [{kind: address}] and [(out, in)]; `_lib` is speech_distill_amd._lib."""
    arr = (_lib.LoraTarget * len(ptrs))()
    for t, p, (out_f, in_f) in zip(arr, ptrs, shapes):
        t.w_res, t.w_out, t.w_grad = p["w_res"], p["w_out"], p["w_grad"]
        t.a_shadow, t.a_scaled, t.b_scaled = p["a_sh"], p["a_sc"], p["b_sc"]
        t.d_a, t.d_b = p["d_a"], p["d_b"]
        t.out_features, t.in_features = out_f, in_f
    return arr


def piece_ptrs(flats, lays):
    """[{kind: address of the target's piece}] in plan order, for all eight arenas (CPU or GPU tensors alike)"""
    n = len(lays["w_res"].pieces)
    return [{k: flats[k].data_ptr() + 2 * lays[k].pieces[i][0] for k in IN_KINDS + OUT_KINDS} for i in range(n)]


def build_arenas(ops, r_pad, in_fill):
    """-> ({kind: flat}, {kind: Layout}) of all eight kinds for the plan `ops`: inputs with `in_fill` in the gaps,
    outputs all sentinel"""
    shapes = [tuple(t["w_res"].shape) for t in ops]
    lays = {k: layout(k, shapes, r_pad) for k in IN_KINDS + OUT_KINDS}
    flats = {k: pack(lays[k], [t[k] for t in ops], in_fill) for k in IN_KINDS}
    flats.update({k: pack(lays[k], None, SENTINEL) for k in OUT_KINDS})
    return flats, lays


PLAN_MEMBERS = ("w_res", "w_out", "w_grad", "a_shadow", "a_scaled", "b_scaled", "d_a", "d_b")


def plan_build_refusals(_lib, ptrs, shapes, r_pad=32):
    """sd_lora_plan_build (host code: no GPU needed) on a plan whose LAST target has one null member (SD_ERR_SHAPE) or one
    member 2 bytes off (SD_ERR_ALIGN), and with n = 0 and n = -1 (SD_ERR_SHAPE), into a host buffer of 0xA5 bytes
    -> list of failure texts: a wrong code, or a buffer that did not keep every byte."""
    import ctypes as C
    lib = _lib.load_lib()
    n = len(ptrs)
    nb = lib.sd_lora_plan_bytes(n)
    cases = [(f"null {m}", m, None, n, -1) for m in PLAN_MEMBERS] + [(f"{m} + 2 bytes", m, 2, n, -2) for m in PLAN_MEMBERS]
    cases += [("n = 0", None, None, 0, -1), ("n = -1", None, None, -1, -1)]
    bad = []
    for name, member, shift, n_arg, want in cases:
        arr = plan_struct(_lib, ptrs, shapes)
        if member is not None:
            setattr(arr[n - 1], member, None if shift is None else getattr(arr[n - 1], member) + shift)
        host = C.create_string_buffer(b"\xA5" * nb, nb)
        rc = lib.sd_lora_plan_build(arr, n_arg, r_pad, host, nb)
        if rc != want:
            bad.append(f"{name}: returned {rc}, want {want}")
        if host.raw != b"\xA5" * nb:
            first = next(i for i, c in enumerate(host.raw) if c != 0xA5)
            bad.append(f"{name}: the refused build wrote the plan buffer, first at byte {first}")
    return bad


def plan_header(host):
    """{field: value} of the PlanHeader at the front of a built host plan"""
    import struct
    return dict(zip(HEADER_FIELDS, struct.unpack_from("<5i", host.raw if hasattr(host, "raw") else bytes(host), 0)))


# ------------------------------------------------------------------------------------------------- fp32-master AdamW
ADAMW32_SIZES = (4, 8, 1020, 1028, 4 * (4096 * 256) + 4, 4 * (2 * 4096 * 256 + 149))
ADAMW32_SMALL, ADAMW32_BIG = ADAMW32_SIZES[:4], ADAMW32_SIZES[4:]
ADAMW32_SCALE = 11.3125
# (workgroups, fewest trips, most trips of a thread that has work) of adamw_f32_shadow_kernel's grid-stride loop
ADAMW32_TRIPS = {4: (1, 1, 1), 8: (1, 1, 1), 1020: (1, 1, 1), 1028: (2, 1, 1), ADAMW32_SIZES[4]: (4096, 1, 2),
                 ADAMW32_SIZES[5]: (4096, 2, 3)}
# Measured by measure_adamw32_floor() (adamw_ref64 with acc=float32 against fp64 on fp32 state, worst of p, m, v over
# every set at every size it runs at, relative to the tensor maximum), and the floor: 4 x, rounded up to two digits.
ADAMW32_MEASURED = 3.0e-7
ADAMW32_FLOOR = 1.2e-6


def adamw32_trips(n):
    """The launcher's arithmetic restated: 4 elements a thread and trip, 256 threads, at most 4096 workgroups."""
    n4 = n // 4
    nb = min(-(-n4 // 256), 4096)
    threads = nb * 256
    return nb, max(1, n4 // threads), -(-n4 // threads)


def adamw32_cases():
    """[(n, set name)]: every set at the four small sizes, ADAMW_BIG_SETS at the two that wrap the grid-stride loop"""
    return [(n, s) for n in ADAMW32_SMALL for s in P.ADAMW_SETS] + [(n, s) for n in ADAMW32_BIG for s in P.ADAMW_BIG_SETS]


def adamw32_inputs(n, set_name):
    """parity_ref.adamw_inputs with fp32 state: p, m, v fp32 as drawn (not rounded to bf16), g bf16.
    -> (p, g, m, v), (sumsq as the fp32 value the kernel reads or None, max_norm)"""
    hp = P.ADAMW_SETS[set_name]
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    p = torch.randn(n, generator=gen)
    g = (torch.randn(n, generator=gen) * hp["g_scale"]).bfloat16()
    m = torch.randn(n, generator=gen) * 0.5 * hp["g_scale"]
    v = torch.zeros(n) if hp["v0"] else torch.rand(n, generator=gen) * 0.5 + 0.1
    ss = float(torch.tensor(float(g.double().pow(2).sum()), dtype=torch.float32))
    norm = math.sqrt(ss)
    sumsq, max_norm = {"none": (None, 0.0), "zero": (ss, 0.0), "below": (ss, 2.0 * norm + 1.0),
                       "above": (ss, 0.5 * norm)}[hp["clip"]]
    return (p, g, m, v), (sumsq, float(torch.tensor(max_norm, dtype=torch.float32)))


def adamw32_ref(n, set_name, acc=torch.float64):
    (p, g, m, v), (ss, mx) = adamw32_inputs(n, set_name)
    return P.adamw_ref64(p, g, m, v, *P.adamw_hp(set_name), sumsq=ss, max_norm=mx, acc=acc)


def adamw32_close(got, ref):
    """(p, m, v) fp32 against adamw_ref64's triple -> {"p" / "m" / "v": Verdict}: rowwise_close at out dtype fp32 (no
    rounding term), each tensor one row."""
    return {k: P.rowwise_close(a, b, torch.float32, ADAMW32_FLOOR) for k, a, b in zip("pmv", got, ref)}


def shadows_of(p32, scale=ADAMW32_SCALE):
    """What the kernel must leave next to its own p: bf16(p) and bf16(fp32(p) * fp32(scale))"""
    p32 = p32.float().cpu()
    return p32.to(BF), (p32 * torch.tensor(scale, dtype=torch.float32)).to(BF)


def measure_adamw32_floor(cases=None):
    worst = 0.0
    for n, s in (adamw32_cases() if cases is None else cases):
        r64, r32 = adamw32_ref(n, s), adamw32_ref(n, s, acc=torch.float32)
        for a, b in zip(r32, r64):
            worst = max(worst, float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)))
    return worst
