"""CPU checks of the MXFP8 frozen teacher: the torch statement of the number format (tests/mx_ref.py), the C ABI additions,
the command-line flag, and a static audit of the generated gfx950 ISA of sd_mx.hip."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

import mx_ref
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ["sd_mxfp8_quant", "sd_gemm_mxfp8", "sd_gemm_mxfp8_swiglu", "sd_qwen3_mx_supported", "sd_qwen3_mx_acts_bytes",
       "sd_qwen3_forward_mx"]


def test_mx_ref_follows_the_format_rule():
    """Dequantised values are bf16-exact; scale bytes follow the rule (zero block -> byte 0, exact powers of two, a block
    whose scaled maximum is just below / just above 448); small integers survive a round trip exactly."""
    g = torch.Generator().manual_seed(0)
    for x in (torch.randn(64, 2048, generator=g), 0.02 * torch.randn(64, 2048, generator=g),
              torch.randn(64, 2048, generator=g) * torch.randn(64, 2048, generator=g).exp()):
        xb = x.bfloat16().float()
        q, s = mx_ref.mx_quant(xb)
        d = mx_ref.mx_deq(q, s)
        assert torch.equal(d.bfloat16().float(), d)
        rel = float((d - xb).pow(2).mean().sqrt() / xb.pow(2).mean().sqrt())
        assert 0.02 < rel < 0.04, rel
        y = torch.ldexp(xb.view(64, -1, 32), -(s.int() - 127)[..., None])
        clamped = float((y.abs() > 448).float().mean())
        assert 0.001 < clamped < 0.02, clamped  # ordinary data exercises the clamp
    z = torch.zeros(2, 64)
    z[1, 40] = 1.0
    q, s = mx_ref.mx_quant(z)
    assert s.tolist() == [[0, 0], [0, 127 - 8]] and float(mx_ref.mx_deq(q, s)[1, 40]) == 1.0
    for p in (-20, -1, 0, 1, 7, 30):  # amax an exact power of two: e = p - 8, the maximum scales to 256
        x = torch.zeros(1, 32)
        x[0, 3] = 2.0 ** p
        q, s = mx_ref.mx_quant(x)
        assert int(s) == p - 8 + 127 and torch.equal(mx_ref.mx_deq(q, s), x)
    # scaled maximum just below 448 (447 -> RNE to 448, no clamp needed) and just above (1.75 * 256 < 450 < 512: clamped)
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1] = 446.0, -3.0   # bf16(446) = 446: e = 0
    q, s = mx_ref.mx_quant(x)
    assert int(s) == 127 and mx_ref.mx_deq(q, s)[0, :2].tolist() == [448.0, -3.0]
    x[0, 0] = 500.0                  # bf16(500) = 500, floor(log2) = 8: e = 0, 500 > 448: clamped to 448
    q, s = mx_ref.mx_quant(x)
    assert int(s) == 127 and mx_ref.mx_deq(q, s)[0, :2].tolist() == [448.0, -3.0]
    x[0, 0] = 512.0                  # next binade: e = 1, 256 and -1.5 exactly
    q, s = mx_ref.mx_quant(x)
    assert int(s) == 128 and mx_ref.mx_deq(q, s)[0, :2].tolist() == [512.0, -3.0]
    i = torch.randint(-8, 9, (4, 128), generator=g).float()
    assert torch.equal(mx_ref.mx_deq(*mx_ref.mx_quant(i)), i)
    q, s = mx_ref.mx_quant(i)
    assert torch.equal(mx_ref.mx_deq(q.view(torch.uint8), s), i)  # bytes are accepted too


def test_mx_restatement_without_quantisation_is_the_oracle_forward():
    from oracle import qwen3 as Q
    shp = Q.Qwen3Shape(512, 256, 512, 2, 2, 1)
    w = {k: v.bfloat16().float() for k, v in Q.init_weights(shp, seed=1, norm_jitter=0.1).items()}
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 512, (2, 40), generator=g)
    am = torch.ones(2, 40, dtype=torch.long)
    am[1, 30:] = 0
    m = am.bool()
    ref = Q.forward(w, shp, ids, am)[m]
    noq = mx_ref.teacher_forward_mx(w, shp, ids, am, quant=False)[m]
    rel = float((noq - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert rel < 1e-2, rel  # the rounding of the folded weights to bf16
    mx = mx_ref.teacher_forward_mx(w, shp, ids, am)[m]
    rel_q = float((mx - noq).pow(2).mean().sqrt() / noq.pow(2).mean().sqrt())
    assert 5 * rel < rel_q < 0.5, (rel, rel_q)


def test_abi_additions_are_declared_exported_and_bound():
    import speech_distill_amd as sda
    from speech_distill_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sd_hip.h")).read(), flags=re.S)
    lib = sda.load_lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "sd_qwen3_params_mx" in hdr and "sd_qwen3_layer_mx" in hdr
    assert ctypes.sizeof(_lib.LayerMx) == 10 * ctypes.sizeof(ctypes.c_void_p)
    from speech_distill_amd.qwen3 import Qwen3Dims

    def cd(d):
        return _lib.Dims(d.vocab_size, d.hidden_size, d.intermediate_size, d.num_hidden_layers, d.num_attention_heads,
                         d.num_key_value_heads, d.head_dim, int(d.tie_word_embeddings), d.rms_norm_eps, 0)
    tiny_teacher = Qwen3Dims(640, 256, 512, 2, 4, 2)
    for d in (Qwen3Dims.teacher_17b(), Qwen3Dims.student_06b(), tiny_teacher):
        assert lib.sd_qwen3_mx_supported(ctypes.byref(cd(d))) == 1
        assert lib.sd_qwen3_mx_acts_bytes(ctypes.byref(cd(d)), 4, 512) > 0
    assert lib.sd_qwen3_fold_supported(ctypes.byref(cd(tiny_teacher))) == 0  # the bf16 fold does not take the --tiny teacher
    odd = cd(Qwen3Dims(640, 320, 512, 2, 2, 1))
    assert lib.sd_qwen3_mx_supported(ctypes.byref(odd)) == 0 and lib.sd_qwen3_mx_acts_bytes(ctypes.byref(odd), 4, 512) < 0
    t = cd(Qwen3Dims.teacher_17b())
    assert lib.sd_qwen3_acts_bytes(ctypes.byref(t), 4, 512, 4) < 0  # still no fifth SD_SAVE_* mode
    assert lib.sd_abi_version() == 2


def _load_script(name):
    spec = importlib.util.spec_from_file_location("sd_cli_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag_and_refusals(monkeypatch):
    train = _load_script("train")
    monkeypatch.setattr(sys, "argv", ["train.py"])
    assert train.parse_args().teacher_precision == "bf16"
    monkeypatch.setattr(sys, "argv", ["train.py", "--teacher_precision", "mxfp8", "--load_teacher_in_8bit"])
    cfg = train.parse_args()
    assert cfg.teacher_precision == "mxfp8" and cfg.load_teacher_in_8bit and not cfg.load_teacher_in_4bit
    monkeypatch.setattr(sys, "argv", ["train.py", "--teacher_precision", "int8"])
    with pytest.raises(SystemExit):
        train.parse_args()
    ext = _load_script("extract_teacher_logits")
    base = ["--teacher_model_path", "t", "--dataset_path", "d", "--output_path", "o"]
    assert ext.parse_args(base).teacher_precision == "bf16"
    assert ext.parse_args(base + ["--teacher_precision", "mxfp8"]).teacher_precision == "mxfp8"
    with pytest.raises(SystemExit):
        ext.parse_args(base + ["--teacher_precision", "fp4"])
    import speech_distill_amd as sda
    model = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 256, 512, 1, 2, 1), device="cpu", seed=0)
    with pytest.raises(ValueError, match="frozen"):
        model.set_inference_precision("mxfp8")   # trainable parameters
    with pytest.raises(ValueError, match="bf16"):
        model.set_inference_precision("int8")
    model.requires_grad_(False)
    assert model.set_inference_precision("mxfp8").inference_precision == "mxfp8"
    assert model.set_inference_precision("bf16").inference_precision == "bf16"
    odd = sda.HipQwen3ForCausalLM(sda.Qwen3Dims(640, 320, 512, 1, 2, 1), device="cpu", seed=0).requires_grad_(False)
    with pytest.raises(ValueError, match="multiples of 128"):
        odd.set_inference_precision("mxfp8")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_isa_of_the_mx_kernels():
    """sd_mx.hip compiled for gfx950: the GEMM kernels (2 epilogues x 2 tile heights) run on
    v_mfma_scale_f32_16x16x128_f8f6f4 (16 per K-step), hold no non-scaled fp8 or bf16 MFMA, wait for their DMA ring with a
    counted vmcnt inside the K loop, no kernel of the file uses scratch or AGPR copies, and the 8-wave GEMM fits two waves
    per SIMD."""
    out = os.path.join(tempfile.mkdtemp(), "mx.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                    "--cuda-device-only", "-S", os.path.join(ROOT, "speech_distill_amd", "csrc", "sd_mx.hip"), "-o", out],
                   check=True)
    assert "sd_mx.hip" in open(os.path.join(ROOT, "speech_distill_amd", "csrc", "Makefile")).read()
    txt = open(out).read()
    kernels = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    gemms = {k: v for k, v in kernels.items() if "gemm_mx_kernel" in k}
    assert len(gemms) == 4 and any("mxfp8_quant_kernel" in k for k in kernels), list(kernels)
    for name, body in gemms.items():
        ops = [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]
        mfma = [o for o in ops if o.startswith("v_mfma")]
        assert mfma and all(o == "v_mfma_scale_f32_16x16x128_f8f6f4" for o in mfma), (name, set(mfma))
        assert len(mfma) % 16 == 0
        assert not [o for o in ops if o.startswith(("scratch_", "v_accvgpr"))], name
        loop = body[body.index("Loop Header"):]
        loop = loop[:loop.index("v_mfma_scale") + 1]
        assert re.search(r"s_waitcnt vmcnt\([1-9]\d*\)\s*\n(.*\n)?\s*s_barrier", loop), name  # counted, not vmcnt(0)
    for name in kernels:
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", txt[txt.index(".name:           " + name) - 400:
                                                                       txt.index(".name:           " + name) + 400])
        assert priv and int(priv.group(1)) == 0, name
    for name in gemms:
        at = txt.index(".name:           " + name)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", txt[at:at + 600])
        assert int(vg.group(1)) <= 256, (name, vg.group(1))


# ------------------------------------------------------------------------------------------------ edge data of the kernel tests
def test_mx_ref_equals_the_fp64_restatement_on_every_bf16_pattern():
    """mx_ref.mx_quant (torch's e4m3 cast, fp32 frexp / ldexp) against mx_ref.mx_quant_fp64 (explicit step 2^(max(floor(log2
    |y|), -6) - 3), half to even) on all 65,280 finite bf16 patterns and on the ratio sweep: scale bytes equal, every
    dequantised value equal; the patterns' scale bytes span 0..246."""
    for x in (mx_ref.all_bf16_blocks(), mx_ref.sweep_blocks()):  # [blocks, 32]: one block per row
        q, s = mx_ref.mx_quant(x.float())
        s64, v64, _ = mx_ref.mx_quant_fp64(x)
        assert torch.equal(s, s64)
        d = mx_ref.mx_deq(q, s)
        assert bool((d.double() == v64).all()), int((d.double() != v64).sum())
        assert torch.equal(d.bfloat16().float(), d)  # every MX value is a bf16 number, subnormal ones included
    assert mx_ref.all_bf16_blocks().shape == (2040, 32)
    s = mx_ref.mx_quant(mx_ref.all_bf16_blocks().float())[1]
    assert int(s.min()) == 0 and int(s.max()) == 246
    bits = mx_ref.all_bf16_blocks().view(torch.int16).to(torch.int32).flatten() & 0xFFFF
    assert torch.equal(bits, torch.cat([torch.arange(0, 0x7F80), torch.arange(0x8000, 0xFF80)]).to(torch.int32))


def test_ratio_sweep_reaches_every_code_every_tie_and_every_edge():
    """The sweep holds an element that quantises to each of the 254 finite e4m3 codes, exact ties that round up and ties that
    round down, scaled values in the saturating band (448, 512), e4m3-subnormal results, flushes to zero, blocks of the
    bf16-subnormal range (scale byte 0), of the top exponent (246) and with amax an exact power of two; edge_matrix lays
    it out with the fixed blocks in front."""
    sw = mx_ref.sweep_blocks()
    assert bool(sw.float().isfinite().all()) and torch.equal(sw[:, 0].double().unique(), mx_ref.sweep_maxima().unique())
    assert bool((sw.float().abs() <= sw[:, :1].float()).all())  # element 0 is the block's maximum
    q, s = mx_ref.mx_quant(sw.float())
    codes = set(q.view(torch.uint8).flatten().tolist())
    assert codes == set(range(256)) - {0x7F, 0xFF}
    _, _, tie = mx_ref.mx_quant_fp64(sw)
    assert int((tie > 0).sum()) > 0 and int((tie < 0).sum()) > 0
    y = torch.ldexp(sw.double(), -(s.to(torch.int32) - 127)).abs()
    assert bool(((y > 448) & (y < 512)).any())
    d = q.to(torch.float32).abs()
    assert bool(((d > 0) & (d < 2.0 ** -6)).any()) and bool(((d == 0) & (sw.float() != 0)).any())
    assert int(s.min()) == 0 and int(s.max()) == 246 and bool((s == 0).sum() > 3)
    assert {127 - 8, 127 + 100 - 8} <= set(s.flatten().tolist())
    x = mx_ref.edge_matrix(4)
    assert x.dtype == torch.bfloat16 and x.shape[1] == 512 and bool(x.float().isfinite().all())
    assert not x[0].any() and not x[3].any() and not x[1, 32:64].any() and bool(x[1, :32].any())
    assert torch.equal(x[2, 0:2].float(), torch.tensor([448.0 * 2.0 ** -15, -448.0 * 2.0 ** -15]))
    body = torch.cat([sw, mx_ref.all_bf16_blocks()])
    assert torch.equal(x[4:].reshape(-1, 32)[:body.shape[0]].view(torch.int16), body.view(torch.int16))


def test_gemm_probes_are_single_exact_products():
    """The one-hot probes of tests/test_gpu_mx_kernels.py: every output is at most one non-zero product, the stated results
    equal the fp64 matmul of the dequantised operands, and over the runs the probed A scale bytes cover 0..254 while the
    exponent sums reach both ends of [-100, 100]."""
    sas, ts = set(), set()
    probes = [mx_ref.code_table_probe(r) for r in range(mx_ref.CODE_TABLE_RUNS)]
    for p in probes:
        sas |= set(p[5].tolist())
        ts |= set(p[6].tolist())
        assert set(p[0][p[0] != 0].tolist()) == set(range(256)) - {0, 0x7F, 0xFF}  # -0 (0x80) is placed; byte 0 is the fill
        at = p[0] == 0x80
        assert int(at.sum()) == 1 and not p[1][at.any(1)].any() and not p[4][at.any(1)].any()  # its row: scale bytes 0, C == 0
    assert sas == set(range(255)) and min(ts) == -100 and max(ts) == 100
    for aq, as_, bq, bs, want in [p[:5] for p in probes] + [mx_ref.position_probe(K) for K in (128, 384)]:
        terms = (aq & 0x7F != 0).double() @ (bq & 0x7F != 0).double().T
        assert float(terms.max()) == 1
        ref = mx_ref.mx_deq(aq, as_, torch.float64) @ mx_ref.mx_deq(bq, bs, torch.float64).T
        assert bool((ref == want.double()).all())
        nz = want.float()[want != 0].abs()
        assert float(nz.min()) >= 2.0 ** -126  # normal bf16 numbers
    for aq, as_, bq, bs, want in (mx_ref.position_probe(K) for K in (128, 384)):
        for row in as_.tolist():
            assert len(set(row)) == len(row)  # a scale taken from another block of the row is another scale


def test_swiglu_probe_is_exact_and_has_its_zero_blocks():
    """act of mx_ref.swiglu_probe: both kinds of gate in every block, one all-negative-gate (zero) block in every row,
    negative up values, and an MXFP8 image with a zero scale byte and several others."""
    for M, I, K, scaled in ((1, 128, 128, False), (130, 384, 384, True)):
        aq, as_, wq, ws, rs, act = mx_ref.swiglu_probe(M, I, K, scaled)
        blk = act.view(M, I // 32, 32)
        zero = (blk == 0).all(-1)
        assert bool(zero.any(-1).all()) and bool((~zero).any(-1).all())
        assert bool((blk[~zero] != 0).any(-1).all()) and bool((blk == 0).any(-1).all())
        assert bool((act < 0).any()) and bool((act > 0).any())
        q, s = mx_ref.mx_quant(act.float())
        assert torch.equal(s == 0, zero) and s.unique().numel() >= 3
        assert (rs is None) == (not scaled)
