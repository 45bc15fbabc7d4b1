#!/usr/bin/env python3
"""bench.py -- distill-step tokens/sec (BASELINE.json metric) on N MI355X of one node.

One "step" = one Stage-2 distillation micro-step on one synthetic pre-processed batch, exactly the
body of the reference's DistillationTrainer.compute_loss + backward (train.py:43-116, HF
trainer.py:1961): student (Qwen3-0.6B shape, vocab 159 488) forward, frozen teacher (SoulX-Podcast-
1.7B shape) no-grad forward, on-the-fly log-softmax + top-128, temperature-scaled KL + CE loss,
student backward; for N > 1 plus the bucketed RCCL all-reduce (avg) of the student gradients,
overlapped with backward.  Workload = BASELINE config 2 per GPU: bf16, seq_len 512, batch 4
(config 3 = 8 ranks of it, weak scaling).  Inputs are resident in HBM before the timed region.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0: `metric` / `value` / `unit` / `ms_per_step` of the K timed steps, plus the phase split
and loss of those steps.  A plain run does nothing else.  `--full` adds what takes runs of its own after the timed
region:
  kernels, roofline -- per-kernel durations and the dominant kernel (by time) of the step, measured with HIP events
                  recorded on the launch stream around every launch in a re-run of the K steps: algorithmic FLOPs / its
                  total duration against the dense bf16 MFMA peak (2.5 PFLOP/s); `roofline.traffic` from two child
                  `rocprofv3 --pmc` runs;
  optimizer_step_ms -- the fused AdamW + clip that follows an accumulation window;
  cpu_baseline -- the CPU oracle (a port of the reference's CPU path, pinned to it by fixtures) timed
                  on this box's host cores on a bounded sample of the same workload, with `loss_match` / `grad_match`
                  of the HIP path on that very sample;
  comm, grad_sync_ok -- N > 1 (or --force-dist): per-bucket collective times and the cross-rank gradient check.

`--dump-outputs DIR` writes what the last timed step computed (its four losses and a fixed, seeded sample of the student
gradient) as DIR/*.npy; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0  # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
SPEECH_LO, VOCAB = 152927, 159488
KERNEL_NAMES = {"gemm_nt_stag": "staggered 256x128 forward GEMM family: gemm_pstag_kernel<4,false,false,EPI 0|3> (persistent: lm_heads, gate|up) + gemm_stag_kernel<false,false,EPI 4|0> (q|k|v)", "gemm_nt": "gemm_bf16_kernel<*,*,false,false,*>", "gemm_nn": "gemm_bf16_kernel<false,true,*>",
                "gemm_tn": "gemm_bf16_kernel<true,true,*>"}


def synthetic_batch(B, T, rank, device):
    """uniform ids, 25 % text prefix masked to -100, then speech_bos, then speech ids."""
    g = torch.Generator().manual_seed(1234 + rank)
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    n_text = T // 4
    ids[:, n_text] = SPEECH_LO  # speech_bos stand-in
    ids[:, n_text + 1:] = torch.randint(SPEECH_LO, VOCAB, (B, T - n_text - 1), generator=g)
    labels = ids.clone()
    labels[:, :n_text] = -100
    return {"input_ids": ids.to(device), "attention_mask": torch.ones(B, T, dtype=torch.long, device=device),
            "labels": labels.to(device), "teacher_input_ids": ids.to(device),
            "teacher_attention_mask": torch.ones(B, T, dtype=torch.long, device=device)}


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sample_T, threads, n_seq=2):
    """Oracle (port of the reference CPU path) on host cores: full-shape models, n_seq sequences.
    Weights are rounded to bf16 first (the values the HIP path holds) and returned with the batch, so that the GPU
    path can be run on the identical sample afterwards (`loss_match`)."""
    from oracle import qwen3 as Q
    from oracle import step as S
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(1234)
    sw = {}
    tw = {}
    for shape, dst, seed in ((Q.STUDENT_06B, sw, 0), (Q.TEACHER_17B, tw, 1)):
        gg = torch.Generator().manual_seed(seed)
        for name, shp in Q.param_names(shape):
            dst[name] = (torch.ones(shp) if len(shp) == 1 else
                         torch.empty(shp).normal_(0, 0.02, generator=gg).bfloat16().float())
    ids = torch.randint(0, VOCAB, (n_seq, sample_T), generator=g)
    ids[:, sample_T // 4:] = torch.randint(SPEECH_LO, VOCAB, (n_seq, sample_T - sample_T // 4), generator=g)
    labels = ids.clone()
    labels[:, : sample_T // 4] = -100
    batch = {"input_ids": ids, "attention_mask": torch.ones_like(ids), "labels": labels}
    t0 = time.time()
    out = S.distill_step(sw, Q.STUDENT_06B, tw, Q.TEACHER_17B, batch, 2.0, 0.5, top_k=128, acc=torch.float32)
    dt = time.time() - t0
    # NOT part of the timed baseline: the same step with bf16 rounding at the HIP path's storage points (oracle/qwen3.py,
    # storage="bf16") -- the noise yardstick of `grad_match`
    t0 = time.time()
    out16 = S.distill_step(sw, Q.STUDENT_06B, tw, Q.TEACHER_17B, batch, 2.0, 0.5, top_k=128, acc=torch.float32,
                           storage="bf16")
    out["bf16_storage"] = {"grads": out16["grads"], "total": float(out16["total"]), "seconds": time.time() - t0}
    res = {"value": n_seq * sample_T / dt, "unit": "tokens/s", "cores": threads, "cpu": cpu_model_name(), "kind": "port",
           "sample": f"{n_seq} sequences x {sample_T} tokens (of the 4 x 512 batch), full-shape teacher+student, fp32 "
                     f"arithmetic on bf16-rounded weights, one micro-step incl. backward, {dt:.1f} s",
           "loss": float(out["total"])}
    return res, sw, tw, batch, out


def rccl_choice(path):
    """What RCCL says it chose, parsed from its own NCCL_DEBUG=INFO log of this rank (None when the run was not started
    with NCCL_DEBUG=INFO).  TUNING lines read `<bytes> Bytes -> Algo <a> proto <p> time <t>` (algo 0 tree, 1 ring, 2/3
    collnet, proto 0 LL, 1 LL128, 2 Simple); INIT / GRAPH lines name the transport of every channel (`via P2P/...`,
    `via SHM`, `via NET`) and the ring / tree channel counts."""
    import re
    if not path or not os.path.exists(path):
        return None
    txt = open(path, errors="replace").read()
    algo_names, proto_names = {0: "tree", 1: "ring", 2: "collnet_direct", 3: "collnet_chain"}, {0: "LL", 1: "LL128", 2: "Simple"}
    picks = {}
    for m in re.finditer(r"(\d+) Bytes -> Algo (\d+) proto (\d+)", txt):
        key = (int(m.group(1)), int(m.group(2)), int(m.group(3)))
        picks[key] = picks.get(key, 0) + 1
    transports = {}
    for m in re.finditer(r"via (P2P[/\w]*|SHM[/\w]*|NET[/\w]*|direct shared memory)", txt):
        transports[m.group(1)] = transports.get(m.group(1), 0) + 1
    ch = re.search(r"(\d+) coll channels, (\d+) (?:collnet|nvls) channels.*?(\d+) p2p channels", txt)
    return {"log": path,
            "collectives": [{"bytes": b, "algo": algo_names.get(a, a), "proto": proto_names.get(pr, pr), "count": n}
                            for (b, a, pr), n in sorted(picks.items())][:40],
            "transports": transports, "rings_connected": "Connected all rings" in txt, "trees_connected": "Connected all trees" in txt,
            "channels": ch.groups() if ch else None,
            "note": "no `Bytes -> Algo` lines: this RCCL build does not print TUNING decisions, or every collective was a "
                    "one-rank shortcut" if not picks else None}


def measure_traffic(symbol, timeout_s=170):
    """`roofline.traffic`, MEASURED in this very run: two child runs of this script under
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, nothing else traced; 2 steps on one stream), the
    counter rows of the dominant kernel symbol averaged per launch.  Units / corrections per MI355X_MICROARCH.md section
    HBM: KB; FETCH_SIZE x 2 on gfx950 -- re-calibrated for the GEMMs' own load path (`buffer_load ... lds`, private and
    panel-shared streams: factor 1.9999 / 1.9986) in profiles/r04_fetch_calibration.json.  Fabric-side bytes: Infinity-
    Cache hits are counted.  On any failure (rocprofv3 absent, timeout) the value of the committed profile is reported
    and SAID to be that."""
    import shutil
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    out = {}
    try:
        from pmc_summary import per_kernel, symbol as sym_of
        if shutil.which("rocprofv3") is None:
            raise RuntimeError("rocprofv3 not on PATH")
        if any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
            raise RuntimeError("this process already runs under a profiler: no nested rocprofv3")
        got = {}
        for ctr, mul in (("FETCH_SIZE", 2048.0), ("WRITE_SIZE", 1024.0)):
            d = tempfile.mkdtemp(prefix="sd_pmc_", dir="/tmp")
            env = dict(os.environ, TMPDIR="/tmp")
            cmd = ["rocprofv3", "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
                   os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-prof",
                   "--no-overlap", "--no-traffic"]
            subprocess.run(cmd, cwd="/tmp", env=env, timeout=timeout_s, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           check=True)
            n = v = 0
            for raw, (cnt, val) in per_kernel(d, ctr).items():
                if sym_of(raw) == symbol:
                    n += cnt
                    v += val
            shutil.rmtree(d, ignore_errors=True)
            if not n:
                raise RuntimeError(f"{symbol} not in the {ctr} pass")
            got[ctr] = (v * mul / n, n)
        out["traffic"] = got["FETCH_SIZE"][0] + got["WRITE_SIZE"][0]
        out["traffic_parts"] = {"fetch_bytes_per_launch": got["FETCH_SIZE"][0], "write_bytes_per_launch": got["WRITE_SIZE"][0],
                                "launches_seen": got["FETCH_SIZE"][1]}
        out["traffic_source"] = ("measured in this run: child `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` passes of "
                                 "`bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-prof --no-overlap`; KB units, FETCH_SIZE x2 "
                                 "(gfx950; calibrated for buffer_load ... lds in profiles/r04_fetch_calibration.json); "
                                 "fabric-side bytes, Infinity-Cache hits counted")
    except Exception as e:  # noqa: BLE001
        out["traffic"] = None
        out["traffic_source"] = f"live measurement failed ({e!r})"
        for prof in ("r04_pmc_traffic.json", "r03_pmc_traffic.json"):
            pth = os.path.join(ROOT, "profiles", prof)
            if os.path.exists(pth):
                t = json.load(open(pth))
                ent = t.get("kernels", {}).get(symbol)
                if ent is not None:
                    out["traffic"] = ent["hbm_bytes_per_launch"]
                    out["traffic_source"] += f"; value REPLAYED from the committed profiles/{prof}"
                    break
    return out


DUMP_PER_TENSOR = 16384


def dump_outputs(dirname, student, losses):
    """What the last timed step hands its caller, as float .npy files: the four losses (float64) and the student
    gradient in float32 -- every element of a tensor of up to DUMP_PER_TENSOR elements, a fixed seeded sample of that
    many (sorted indices) of every larger one, tensors in the order of the flat parameter buffer (~13 MB in all)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, v in zip(("total", "task", "distill", "teacher"), losses):
        np.save(os.path.join(dirname, f"loss_{name}.npy"), np.array([v], dtype=np.float64))
    g = torch.Generator().manual_seed(4242)
    idx = []
    for off, n, _ in student._slices.values():
        if n <= DUMP_PER_TENSOR:
            idx.append(torch.arange(off, off + n))
        else:
            idx.append(off + torch.randint(0, n, (DUMP_PER_TENSOR,), generator=g).sort().values)
    idx = torch.cat(idx).to(student.flat_grad.device)
    sample = student.flat_grad.index_select(0, idx).float().cpu().numpy()
    np.save(os.path.join(dirname, "student_grad_sample.npy"), sample)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--top-k", type=int, default=128)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prof", action="store_true", help="do not record per-launch HIP events in the timed region")
    ap.add_argument("--cpu-sample-tokens", type=int, default=512)
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL over xGMI) | gloo (single-GPU rehearsal of the N>1 path)")
    ap.add_argument("--single-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the N>1 code path (process group, bucket all-reduce, embedding-row exchange) even "
                         "with one rank: a one-GPU rehearsal of the RCCL calls")
    ap.add_argument("--layers-per-bucket", type=int, default=1,
                    help="N>1: decoder layers per gradient bucket (31.5 MB each for the 0.6B student)")
    ap.add_argument("--comm-algo", default="allreduce", choices=["allreduce", "rs_ag"],
                    help="N>1: one all_reduce(AVG) per bucket | in-place reduce_scatter + all_gather (direct over all xGMI links)")
    ap.add_argument("--serial-teacher", action="store_true", help="teacher forward on the student's stream (no overlap)")
    ap.add_argument("--full-head", action="store_true",
                    help="apply lm_head / top-K / loss to all B*T rows (default: only the rows the loss reads, as "
                         "DistillationTrainer.compute_loss does on training steps)")
    ap.add_argument("--phases", action="store_true", help="print the wall time of the phases of a step (stderr)")
    ap.add_argument("--experiment-pipeline", action="store_true",
                    help="MEASUREMENT ONLY (not the reported configuration): issue the NEXT step's teacher pass under this "
                         "step's backward")
    ap.add_argument("--experiment-cached-rows", action="store_true",
                    help="MEASUREMENT ONLY (not the reported configuration): select the loss rows once instead of every "
                         "step -- an upper bound on what the per-step host read of the row count costs")
    ap.add_argument("--no-overlap", action="store_true", help="single stream everywhere (clean per-kernel profiles)")
    ap.add_argument("--no-traffic", action="store_true",
                    help="skip the live `roofline.traffic` measurement (two child runs of this script under rocprofv3 --pmc)")
    ap.add_argument("--no-shared-hint", action="store_true",
                    help="A/B: the two overlapped forwards are NOT told that they share the GPU (no SD_FWD_CONCURRENT)")
    ap.add_argument("--no-fold", action="store_true",
                    help="A/B: the frozen teacher runs its RMSNorm launches instead of folding the gains into the weights")
    ap.add_argument("--experiment-cu-hog", type=int, default=0, metavar="N",
                    help="MEASUREMENT ONLY (not the reported configuration): N idle workgroups (256 threads, 128 registers "
                         "per lane: a communication kernel's footprint) hold a CU slot each during every backward, on a "
                         "stream of their own -- how the backward reacts when RCCL's kernels take CUs (tests/csrc/cu_hog.hip)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure per-kernel times / roofline / traffic, the optimizer step, the "
                         "CPU baseline with loss and gradient match, and (N > 1) the communication report")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the losses and a seeded sample of the student gradient of the last timed step as DIR/*.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    import torch.distributed as dist
    multi = world > 1 or args.force_dist
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.single_device:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        # With NCCL_DEBUG=INFO set by whoever launches the run, keep RCCL's log in a file per rank so that rank 0 can report
        # WHICH algorithm / protocol / transport RCCL chose (`comm.rccl_choice`): the first real 8-GPU run then tells a ring
        # from a direct all-reduce without a second run.
        if args.backend == "nccl" and os.environ.get("NCCL_DEBUG", "").upper() in ("INFO", "TRACE"):
            os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,TUNING,GRAPH")
            os.environ.setdefault("NCCL_DEBUG_FILE", "/tmp/sd_rccl_rank%d.log" % rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)
    dev = torch.device("cuda", local_rank)

    import speech_distill_amd as sda
    from speech_distill_amd import ddp, ops
    sda.load_lib()  # raises if libsd_hip.so is missing: no fallback

    student = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.student_06b(), device=dev, init_std=0)
    teacher = sda.HipQwen3ForCausalLM(sda.Qwen3Dims.teacher_17b(), device=dev, init_std=0)
    for m, seed in ((student, 0), (teacher, 1)):  # HF default init N(0, 0.02), same on every rank
        gen = torch.Generator(device=dev).manual_seed(seed)
        m.flat.normal_(0.0, 0.02, generator=gen)
        for p in m._params.values():
            if p.dim() == 1:
                p.data.fill_(1.0)
    teacher.eval().requires_grad_(False)
    teacher.fold_norm_gains = not args.no_fold
    loss_fn = sda.DistillationLoss(temperature=2.0, alpha=0.5, inplace_grad=True)
    reducer = (ddp.attach(student, layers_per_bucket=args.layers_per_bucket, algo=args.comm_algo,
                          rehearse_single_rank=args.force_dist) if multi else None)
    batch = synthetic_batch(args.batch, args.seq_len, rank, dev)

    if args.no_overlap:
        args.serial_teacher = True
        student.overlap_dw = False
    side = None if args.serial_teacher else ops.concurrent_stream(dev, "teacher")  # as DistillationTrainer does

    def teacher_topk(rows, shared=False):
        t_logits = teacher(input_ids=batch["teacher_input_ids"], attention_mask=batch["teacher_attention_mask"],
                           logit_rows=rows, concurrent=shared).logits                       # train.py:60-69
        return ops.logsoftmax_topk(t_logits, args.top_k, VOCAB)                             # train.py:80-91

    phase_ev = []
    pending = []
    cached_rows = []

    def mark():  # 5 event records per step on the current stream (always on: the backward time feeds the JSON line)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        phase_ev.append(e)

    hog = None
    if args.experiment_cu_hog > 0:
        import ctypes
        hog_lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "libcu_hog.so"))
        hog_lib.cu_hog.restype, hog_lib.cu_hog.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        hog = (hog_lib, torch.cuda.Stream(device=dev))

    def step(overlap=True):
        # the same sequence as speech_distill_amd.trainer.DistillationTrainer.compute_loss on a training step
        student.zero_grad()
        mark()
        rows = row_labels = None
        if not args.full_head:  # rows whose shifted label is not -100 (distillation_loss.py:31-45); one host sync
            if args.experiment_cached_rows and cached_rows:
                rows, row_labels = cached_rows[0]  # EXPERIMENT: what the host sync costs (never the reported line)
            else:
                rows, row_labels = ops.loss_rows(batch["labels"])
                cached_rows[:] = [(rows, row_labels)]
        with torch.no_grad():
            if args.experiment_pipeline and overlap and pending:
                tv, ti = pending.pop()  # EXPERIMENT: issued on the side stream under the previous step's backward
            elif side is None or not overlap:
                tv, ti = teacher_topk(rows)
            else:  # the frozen teacher is independent of the student: run it on a second HIP stream
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    tv, ti = teacher_topk(rows, shared=not args.no_shared_hint)
        # both passes are told that they share the GPU (SD_FWD_CONCURRENT), as DistillationTrainer.compute_loss does
        shared = side is not None and overlap and not args.experiment_pipeline and not args.no_shared_hint
        logits = student(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"],
                         labels=batch["labels"], logit_rows=rows, concurrent=shared).logits  # train.py:54
        mark()
        if side is not None and overlap:
            torch.cuda.current_stream().wait_stream(side)
        mark()
        if rows is None:
            total, task, distill, teach = loss_fn(logits, batch["labels"], teacher_top_k_v=tv, teacher_top_k_i=ti)
        else:
            total, task, distill, teach = loss_fn.forward_rows(logits, row_labels, teacher_top_k_v=tv, teacher_top_k_i=ti)
        mark()
        if args.experiment_pipeline and overlap and side is not None:
            with torch.no_grad():
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    pending.append(teacher_topk(rows))
        if hog is not None:  # EXPERIMENT (also in the one-stream per-kernel pass: which kernels pay): from here for 8.5 ms (the backward takes ~8.8), then they leave
            hog[1].wait_stream(torch.cuda.current_stream())
            rc = hog[0].cu_hog(args.experiment_cu_hog, 8500, hog[1].cuda_stream)
            assert rc == 0, rc
        total.backward()                                                                    # HF trainer.py:1961
        mark()
        return total, task, distill, teach

    def barrier():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        out = step()
    barrier()
    phase_ev.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, student, [float(x.detach()) for x in out])
    n_ph = 5
    names = ["student_fwd_teacher_beside", "wait_teacher_topk", "loss_fwd", "backward"]
    phase_ms = [0.0] * 4
    for k in range(0, len(phase_ev) - n_ph + 1, n_ph):
        for j in range(4):
            phase_ms[j] += phase_ev[k + j].elapsed_time(phase_ev[k + j + 1]) / max(1, len(phase_ev) // n_ph)
    phase_ev.clear()
    if args.phases and rank == 0:
        torch.cuda.synchronize()
        t_enq = time.perf_counter()
        step()
        t_enq = time.perf_counter() - t_enq
        torch.cuda.synchronize()
        print(f"[phase] host time to enqueue one step (GPU idle at start): {t_enq * 1e3:.3f} ms", file=sys.stderr)
        for j in range(4):
            print(f"[phase] {names[j]:34s} {phase_ms[j]:7.3f} ms", file=sys.stderr)
    # Per-kernel durations: the SAME K steps again, immediately after the timed region, with HIP events
    # recorded on the launch stream around every launch.  Kept out of the timed region because ~2 000
    # event records per step stretch the step by ~20 % (measured 39.8 vs 32.9 ms) and would understate `value`.
    prof = None
    if args.full and not args.no_prof:
        student.overlap_dw = False  # one stream only, so that every event pair brackets exactly one kernel
        step(overlap=False)
        barrier()
        ops.prof_begin()
        tp = time.perf_counter()
        for _ in range(args.steps):
            step(overlap=False)
        barrier()
        prof_dt = time.perf_counter() - tp
        prof = ops.prof_end()
        syms = ops.prof_symbols()
        student.overlap_dw = not args.no_overlap
    comm = None
    if args.full and multi and reducer is not None and reducer.cuda:
        # Self-diagnosis of the N > 1 run (its first execution on real xGMI links is the driver's): the same steps again
        # with events on the communication stream around every bucket's collective and around the compute stream's final
        # wait for it (= the communication time NOT hidden under backward).  Outside the timed region.
        reducer.timing = True
        per_bucket, exposed, covered = {}, [], None
        for _ in range(max(2, min(args.steps, 5))):
            step()
            torch.cuda.synchronize()
            per, ex = reducer.timings()
            for i, (st, nbytes, ms) in enumerate(per):
                e = per_bucket.setdefault(i, {"stage": st, "MB": nbytes / 1e6, "ms": []})
                e["ms"].append(ms)
            if ex is not None:
                exposed.append(ex)
            # every element of the flat gradient must have been reduced exactly once (tied embedding: its dense part
            # as a bucket + the row exchange at the end)
            spans = sorted((a, b) for _, a, b in reducer.issued if a >= 0)
            covered = (bool(spans) and spans[0][0] == 0 and spans[-1][1] == student.numel_flat
                       and all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1)))
        reducer.timing = False
        bl = [{"stage": e["stage"], "MB": round(e["MB"], 2), "ms": round(sum(e["ms"]) / len(e["ms"]), 4)}
              for _, e in sorted(per_bucket.items())]
        try:
            rccl = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:
            rccl = repr(e)
        comm = {"rccl_version": rccl, "algo": reducer.algo, "layers_per_bucket": args.layers_per_bucket,
                "world": world, "single_rank_rehearsal": bool(args.force_dist and world == 1),
                "buckets": bl, "comm_stream_busy_ms_per_step": round(sum(b["ms"] for b in bl), 4),
                "exposed_ms_per_step": round(sum(exposed) / max(1, len(exposed)), 4) if exposed else None,
                "bytes_per_step": sum(b["MB"] for b in bl) * 1e6, "every_gradient_element_reduced_once": covered,
                "stats": dict(reducer.stats), "rccl_choice": rccl_choice(os.environ.get("NCCL_DEBUG_FILE"))}
    if multi:
        tmax = torch.tensor([dt], device=dev if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    losses = [float(x.detach()) for x in out]
    grad_sync_ok = None
    if args.full and multi:  # after the all-reduce every rank must hold the same averaged gradient
        cs = student.flat_grad.float().abs().sum().double().reshape(1)
        cs = cs if args.backend == "nccl" else cs.cpu()
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        grad_sync_ok = bool(float(hi) - float(lo) <= 1e-6 * abs(float(hi)))

    if rank == 0:
        tokens = world * args.batch * args.seq_len * args.steps
        f_student = student.dims.flops_per_token(args.seq_len)
        f_tok = 3 * f_student + teacher.dims.flops_per_token(args.seq_len)
        n_rows = args.batch * args.seq_len if args.full_head else int(ops.loss_rows(batch["labels"])[0].numel())
        skipped_rows = args.batch * args.seq_len - n_rows
        head_s, head_t = student.dims.lm_head_flops_per_row(), teacher.dims.lm_head_flops_per_row()
        step_flops_exec = f_tok * args.batch * args.seq_len - skipped_rows * (3 * head_s + head_t)
        res = {
            "metric": "distill-step tokens/sec (student seq_len=512)", "value": tokens / dt, "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"BASELINE config {2 if world == 1 else 3}: Qwen3-0.6B-shape student + SoulX-1.7B-shape "
                                   f"teacher (random init), V=159488, batch {args.batch}/GPU, seq_len {args.seq_len}, "
                                   f"top_k {args.top_k}, T=2.0 alpha=0.5, student fwd+bwd + teacher fwd + top-K + KL/CE",
                       "global_batch": world * args.batch, "seq_len": args.seq_len,
                       "parallelism": f"dp{world}" if world > 1 else "single"},
            "step_flops_per_token_algorithmic": f_tok,
            # nominal: the reference's work (lm_head on all B*T rows of both models, train.py:54-55) per wall second
            "step_mfma_frac": (tokens / dt) * f_tok / world / (MFMA_PEAK_TFLOPS * 1e12),
            # executed: what the timed step really computes -- both lm_heads, top-K and loss on the loss rows only
            "step_mfma_frac_executed": (step_flops_exec / (dt / args.steps)) / (MFMA_PEAK_TFLOPS * 1e12),
            "head_rows": {"computed": n_rows, "of": args.batch * args.seq_len},
            "phases_ms": dict(zip(names, phase_ms)),
            # north-star target (>= 0.40): student backward = 2 x student forward FLOPs over the wall time of the
            # backward phase (loss backward kernel included); "executed" counts the head on the loss rows only
            "student_bwd_mfma_frac": 2 * f_student * args.batch * args.seq_len / (phase_ms[3] * 1e-3) / (MFMA_PEAK_TFLOPS * 1e12),
            "student_bwd_mfma_frac_executed": (2 * f_student * args.batch * args.seq_len - 2 * skipped_rows * head_s)
                                              / (phase_ms[3] * 1e-3) / (MFMA_PEAK_TFLOPS * 1e12),
            "grad_sync_ok": grad_sync_ok,
            "comm": comm,
            "loss": {"total": losses[0], "task": losses[1], "distill": losses[2], "teacher": losses[3]},
        }
        if prof is not None:
            tot_ms = sum(v[0] for v in prof.values())
            kinds = {k: {"ms_per_step": v[0] / args.steps, "launches_per_step": v[2] / args.steps,
                         "avg_us": 1e3 * v[0] / max(v[2], 1),
                         ("tflops" if k.startswith(("gemm", "attn")) else "gbs"):
                             (v[1] / (v[0] * 1e-3) / (1e12 if k.startswith(("gemm", "attn")) else 1e9)) if v[0] > 0 else 0.0}
                     for k, v in prof.items() if v[2] > 0}
            res["kernels"] = kinds
            res["kernel_ms_per_step_sum"] = tot_ms / args.steps
            res["profiled_pass_ms_per_step"] = 1e3 * prof_dt / args.steps
            # ONE dominant kernel symbol (named as rocprofv3 --kernel-trace prints it, a row of
            # profiles/r03_bench_serial_kernel_stats.csv); the kind it belongs to is given beside it as `family`
            dom = max(syms, key=lambda k: syms[k][0])
            ms, work, cnt, kind = syms[dom]
            fam_ms, fam_work, fam_cnt = prof[kind]
            mfma = kind.startswith(("gemm", "attn"))
            ach = work / (ms * 1e-3) / (1e12 if mfma else 1e9)
            peak = MFMA_PEAK_TFLOPS if mfma else HBM_PEAK_GBS
            res["roofline"] = {
                "bound": "mfma" if mfma else "hbm", "achieved": ach, "peak": peak, "unit": "TFLOP/s" if mfma else "GB/s",
                "frac": ach / peak, "traffic": None, "kernel": dom, "avg_launch_us": 1e3 * ms / cnt,
                "launches_per_step": cnt / args.steps, "ms_per_step": ms / args.steps,
                ("algorithmic_flops_per_launch_avg" if mfma else "algorithmic_bytes_per_launch_avg"): work / cnt,
                "measured": "HIP events on the launch stream around every launch (sd_prof_*), the same K steps re-run "
                            "on ONE stream right after the timed region",
                "family": {"kind": kind, "kernels": KERNEL_NAMES.get(kind, kind), "ms_per_step": fam_ms / args.steps,
                           "launches_per_step": fam_cnt / args.steps,
                           "achieved": fam_work / (fam_ms * 1e-3) / (1e12 if mfma else 1e9)},
                "by_symbol_ms_per_step": {k: round(v[0] / args.steps, 4) for k, v in
                                          sorted(syms.items(), key=lambda kv: -kv[1][0])[:12]}}
            if mfma and dom.startswith(("gemm_pstag_kernel", "gemm_stag_kernel", "gemm_pgroup")):
                # What paces a 256x128x64 tile loop is the delivery of operand bytes to the CU, not the matrix pipe: every
                # 2*256*128*64 FLOP take (256+128)*64*2 B.  Ceiling of that delivery under this very access pattern with NO
                # compute: 66 GB/s per CU = 16.9 TB/s, the same through THREE load paths (LDS-DMA; coalesced global -> VGPR;
                # global -> VGPR -> ds_write: profiles/r04_fill_paths.json), and it is what the vendor's best kernel reaches
                # on the largest shapes (1.43 PFLOP/s, profiles/r04_gemm_yardstick.json).  Reported beside the MFMA fraction
                # so that the binding roofline is visible: bytes staged / launch duration.
                staged = work / (2.0 * 256 * 128 * 64) * (256 + 128) * 64 * 2
                res["roofline"]["operand_stream"] = {
                    "bound": "cu_operand_delivery", "achieved": staged / (ms * 1e-3) / 1e9, "peak": 66.0 * 256, "unit": "GB/s",
                    "frac": staged / (ms * 1e-3) / 1e9 / (66.0 * 256), "bytes_staged_per_launch_avg": staged / cnt,
                    "note": "tile 256x128x64: 11.7 B per kFLOP, so 16.9 TB/s of operand delivery caps this tile shape at "
                            "1.44 PFLOP/s whatever the loop or load path (profiles/r04_fill_paths.json: LDS-DMA 63-66, "
                            "global->VGPR 65.8, global->VGPR->LDS 66.1 GB/s per CU, fragment-layout VGPR loads 31-38; "
                            "profiles/r04_gemm_yardstick.json: hipBLASLt / rocBLAS on the same shapes)"}
        if "roofline" in res and world == 1 and not args.no_traffic:
            res["roofline"].update(measure_traffic(res["roofline"]["kernel"]))
        if args.full:
            try:
                # Not part of the metric (the distillation MICRO-step, repeated gradient_accumulation_steps times per
                # optimizer step, train.py:336): the fused AdamW + global-norm clip that follows the last micro-step
                # (HF trainer.py:1778-1796, 2539), measured on the gradients the timed steps left behind, lr = 0.
                from speech_distill_amd.optim import FlatAdamW
                opt = FlatAdamW(student, lr=0.0, weight_decay=0.01, clip=1.0)
                opt.step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    opt.step()
                e1.record()
                torch.cuda.synchronize()
                res["optimizer_step_ms"] = e0.elapsed_time(e1) / 5
                del opt
            except Exception as e:
                res["optimizer_step_ms"] = repr(e)
        if args.experiment_pipeline or args.experiment_cached_rows or args.experiment_cu_hog:
            res["experiment"] = "NOT the reported configuration: " + " ".join(
                f for f, on in (("--experiment-pipeline", args.experiment_pipeline),
                                ("--experiment-cached-rows", args.experiment_cached_rows),
                                (f"--experiment-cu-hog {args.experiment_cu_hog}", args.experiment_cu_hog)) if on)
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                cb, sw, tw, cbatch, cout = cpu_baseline(args.cpu_sample_tokens, min(os.cpu_count() or 1, 16))
                res["cpu_baseline"] = cb
                # loss match on IDENTICAL inputs: the HIP path on the very sample (weights, ids) the oracle just ran
                student.load_hf_state_dict(sw)
                teacher.load_hf_state_dict(tw)
                gb = {k: v.to(dev) for k, v in cbatch.items()}
                student.zero_grad()
                rows, row_labels = ops.loss_rows(gb["labels"])
                with torch.no_grad():
                    tv, ti = ops.logsoftmax_topk(teacher(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"],
                                                         logit_rows=rows).logits, args.top_k, VOCAB)
                got = loss_fn.forward_rows(student(input_ids=gb["input_ids"], attention_mask=gb["attention_mask"],
                                                   logit_rows=rows).logits, row_labels, teacher_top_k_v=tv,
                                           teacher_top_k_i=ti)
                g4 = [float(x.detach()) for x in got]
                w4 = [float(cout[k]) for k in ("total", "task", "distill", "teacher")]
                res["loss_match"] = {"hip_bf16": g4, "oracle_fp32": w4, "rel_err_total": abs(g4[0] - w4[0]) / abs(w4[0]),
                                     "tolerance": 2e-2, "sample": "the cpu_baseline sample: same weights (bf16-rounded), same "
                                     "ids, full-shape teacher + student", "ok": abs(g4[0] - w4[0]) <= 2e-2 * abs(w4[0])}
                # gradient match at FULL depth (28 layers) WITH an error budget: the oracle's fp32 backward of that same
                # sample against the HIP backward, per tensor, next to the same step through the oracle's bf16-storage
                # mode (oracle/qwen3.py: bf16 rounding at the HIP path's storage points, forward and backward) --
                # err = relative L2 error against the fp32 oracle; ok = err(HIP) <= 1.5 x err(bf16-storage oracle)
                got[0].backward()
                torch.cuda.synchronize()
                c16 = cout["bf16_storage"]
                names = ("model.embed_tokens.weight", "model.layers.0.self_attn.q_proj.weight",
                         "model.layers.13.mlp.gate_proj.weight", "model.layers.27.mlp.down_proj.weight",
                         "model.layers.27.input_layernorm.weight", "model.norm.weight")

                def rel_l2(g, ref):
                    ref = ref.double().reshape(-1)
                    return float((g.detach().double().cpu().reshape(-1) - ref).norm() / ref.norm())
                budget = {n: {"err_hip": rel_l2(student._params[n].grad, cout["grads"][n]),
                              "err_bf16_oracle": rel_l2(c16["grads"][n], cout["grads"][n])} for n in names}
                for b_ in budget.values():
                    b_["ratio"] = b_["err_hip"] / max(b_["err_bf16_oracle"], 1e-300)
                gm, ok_all = {}, True
                for name in names:
                    ref_g = cout["grads"][name].double().reshape(-1)
                    hip_g = student._params[name].grad.detach().double().cpu().reshape(-1)
                    rn, hn = float(ref_g.norm()), float(hip_g.norm())
                    cos = float(torch.dot(ref_g, hip_g) / max(rn * hn, 1e-300))
                    bud = budget[name]
                    ok = bud["err_hip"] <= 1.5 * bud["err_bf16_oracle"] and cos >= 0.99
                    ok_all &= ok
                    gm[name] = {"norm_hip": hn, "norm_oracle": rn, "cosine": cos, "err_hip": bud["err_hip"],
                                "err_bf16_oracle": bud["err_bf16_oracle"], "ratio": bud["ratio"], "ok": ok}
                res["grad_match"] = {"tensors": gm, "worst_ratio": max(v["ratio"] for v in gm.values()),
                                     "tolerance": {"err_hip_over_err_bf16_oracle_max": 1.5, "cosine_min": 0.99},
                                     "ok": ok_all,
                                     "bf16_oracle_loss": c16["total"],
                                     "sample": "same sample as loss_match; err = relative L2 error against the fp32 oracle "
                                               "(autograd through 28 layers); bf16 oracle = the same step with bf16 rounding "
                                               f"at the HIP path's storage points ({c16['seconds']:.1f} s of host time, not part of "
                                               "cpu_baseline)"}
                del sw, tw
            except Exception as e:  # never lose the GPU line to a host-side problem
                res.setdefault("cpu_baseline", {"value": None, "error": repr(e)})
                res["loss_match"] = {"error": repr(e)}
        print(json.dumps(res), flush=True)
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
