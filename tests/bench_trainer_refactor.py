"""Parity of ``DistillationTrainer`` between two source trees over the same compiled library (the convention of
profiles/runner_abi_parity.json): every leg is a real ``Trainer.train()`` (or ``evaluate()``) on the config-1 models and
samples of tests/golden/g4_step_c1.npz -- 13 samples, batch 2, accumulation 2, 2 epochs, seed 7 -- in a fresh process with
one tree first on ``PYTHONPATH``.  Per leg: the SHA-256 of ``student.flat``, the logged loss sequences, the launch count
per kernel symbol (``ops.prof_symbols``) and the number of ``ops.loss_rows`` + ``ops.packed_rows`` calls.

    python tests/bench_trainer_refactor.py --parent-tree DIR --parent-commit ID --out profiles/trainer_plan_parity.json

runs the parent tree twice (it must repeat) and then this tree, and compares all four per leg.  ``DIR`` is a checkout of the
parent commit (``git worktree add DIR <commit>``) outside the repository; it needs no build: ``SD_HIP_LIB`` points both trees
at this tree's library, which is the parent's as long as no kernel changed.  The profiler brackets every launch with two
events on the launch stream and orders nothing, so hashes and counts come from one run; ``--jobs`` legs run side by side.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKAHEADS = {"off": {"SD_ROWS_AHEAD": "0"}, "default": {}, "forced": {"SD_WINDOW_AHEAD": "1", "SD_TEACHER_AHEAD": "1"}}
ON_POLICY = {"max_new_tokens": 8, "temperature": 1.0, "top_k": 50, "decode_kernels": "skinny"}


def legs():
    """name -> (settings of the leg, environment)."""
    out = {}
    for layout in ("padded", "packed_cu", "packed_pos"):
        for teacher in ("topk16", "dense", "pre"):
            for look, env in LOOKAHEADS.items():
                out[f"{layout}/{teacher}/lookahead_{look}"] = (dict(layout=layout, teacher=teacher), env)
    out["padded/jsd_tail"] = (dict(layout="padded", teacher="topk16", divergence="jsd_tail"), {})
    out["padded/lmbda0.5_micro_batch"] = (dict(layout="padded", teacher="topk16", divergence="reverse_kl_tail", lmbda=0.5,
                                               rollout="micro_batch"), {})
    out["padded/lmbda0.5_window"] = (dict(layout="padded", teacher="topk16", divergence="reverse_kl_tail", lmbda=0.5,
                                          rollout="window"), {})
    out["padded/compact_head_off"] = (dict(layout="padded", teacher="topk16", compact=False), {})
    out["padded/evaluate"] = (dict(layout="padded", teacher="topk16", evaluate=True), {})
    return out


# ------------------------------------------------------------------------------------------------ one leg, in this process
def run_leg(name, prof=True):
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != os.path.dirname(os.path.abspath(__file__))
                   or p in os.environ.get("PYTHONPATH", "").split(os.pathsep)]   # the tree under test, not this script's
    import torch
    import speech_distill_amd as sda
    from transformers import TrainingArguments
    from speech_distill_amd import ops
    from speech_distill_amd.collator import ProcessedDataCollator
    from speech_distill_amd.trainer import DistillationTrainer
    from test_gpu_model import _Tok, _build, _c1
    cfg, _ = legs()[name]
    sda.load_lib()
    z, st, te, sw, tw, feats, pad, bos = _c1(sda)
    rows = [dict(f) for f in (feats * 2)[:13]]
    top_k = 0 if cfg["teacher"] == "dense" else 16
    if cfg["teacher"] == "pre":   # pre-extracted top-K: seeded stand-ins of the right shapes and dtypes, one block per sample
        for j, f in enumerate(rows):
            g = torch.Generator().manual_seed(100 + j)
            n = len(f["student_input_ids"])
            f["teacher_top_k_v"] = (-torch.rand(n, 16, generator=g) - 0.5).sort(-1, descending=True).values.half()
            f["teacher_top_k_i"] = torch.stack([torch.randperm(640, generator=g)[:16] for _ in range(n)]).int()
    collate = ProcessedDataCollator(_Tok(pad, bos), pad_token_id=pad, padding_free=cfg["layout"] != "padded")
    if cfg["layout"] == "packed_pos":   # HF's flattening without the flash-attn keys: segments by position_ids alone
        packed = collate
        collate = lambda f: {k: v for k, v in packed(f).items() if not k.startswith(("cu_seq_lens", "max_length"))}

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(rows)

        def __getitem__(self, i):
            return dict(rows[i])
    student, teacher = _build(sda, st, sw), _build(sda, te, tw)
    teacher.eval().requires_grad_(False)
    args = TrainingArguments(
        output_dir=tempfile.mkdtemp(), per_device_train_batch_size=2, per_device_eval_batch_size=2, gradient_accumulation_steps=2,
        num_train_epochs=2, learning_rate=1e-3, logging_steps=1, save_strategy="no", eval_strategy="no", report_to=[],
        remove_unused_columns=False, label_names=["labels"], seed=7, data_seed=7, lr_scheduler_type="constant", warmup_steps=0,
        max_grad_norm=1.0, dataloader_num_workers=0, bf16=True, disable_tqdm=True)
    kw = {}
    if cfg.get("lmbda"):
        kw = dict(lmbda=cfg["lmbda"], on_policy_rollout=cfg["rollout"],
                  on_policy_generate=dict(ON_POLICY, eos_token_id=pad, pad_token_id=pad))
    tr = DistillationTrainer(model=student, args=args, train_dataset=DS(), eval_dataset=DS(), data_collator=collate,
                             teacher_model=teacher, temperature=2.0, alpha=0.5, top_k=top_k,
                             divergence=cfg.get("divergence", "forward_kl"), **kw)
    tr.compact_head = cfg.get("compact", True)
    selections = []
    for fn in ("loss_rows", "packed_rows"):
        setattr(ops, fn, lambda *a, _f=getattr(ops, fn), **k: selections.append(1) or _f(*a, **k))
    if prof:
        ops.prof_begin()
    result = tr.evaluate() if cfg.get("evaluate") else tr.train()
    launches = None
    if prof:
        ops.prof_end()
        launches = {sym: v[2] for sym, v in sorted(ops.prof_symbols().items())}
    torch.cuda.synchronize()
    keys = ("loss", "student_loss", "teacher_loss", "distill_loss", "eval_loss", "on_policy_fraction")
    return {"sha256_student_flat": hashlib.sha256(student.flat.detach().cpu().view(torch.int16).numpy().tobytes()).hexdigest(),
            "logs": {k: [h[k] for h in tr.state.log_history if k in h] for k in keys},
            "eval_loss": result.get("eval_loss") if cfg.get("evaluate") else None,
            "launches": launches, "selections": len(selections), "tree": os.path.dirname(os.path.dirname(sda.__file__))}


# ------------------------------------------------------------------------------------------------------------ the driver
def spawn(tree, name, prof, seconds=240):
    """One leg in a fresh process with ``tree`` (and its tests/) first on PYTHONPATH.  -> (return code, result or None)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(tree, "tests")]),
               SD_HIP_LIB=os.path.join(ROOT, "speech_distill_amd", "libsd_hip.so"), **legs()[name][1])
    for k in ("SD_ROWS_AHEAD", "SD_WINDOW_AHEAD", "SD_TEACHER_AHEAD"):
        if k not in legs()[name][1]:
            env.pop(k, None)
    with tempfile.NamedTemporaryFile(suffix=".json") as f:
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--leg", name, "--out", f.name]
        r = subprocess.run(cmd + ([] if prof else ["--no-prof"]), cwd=tree, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"[{name} in {tree}] exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}\n")
            return r.returncode, None
        res = json.load(open(f.name))
        assert os.path.samefile(res.pop("tree"), tree), (res, tree)   # the package that ran is this tree's
        return 0, res


def run_tree(tree, names, prof, jobs):
    """Every leg of one tree, ``jobs`` at a time; nothing more is started once a leg has ended badly."""
    failed, out = [], {}

    def one(name):
        if failed:
            return
        rc, res = spawn(tree, name, prof)
        if rc != 0:
            failed.append((name, rc))
        out[name] = res
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(one, names))
    if failed:
        raise SystemExit(f"legs ended badly in {tree}: {failed}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--only", default=None, help="comma-separated substrings of leg names")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.leg:
        json.dump(run_leg(a.leg, prof=not a.no_prof), open(a.out, "w"))
        return
    names = [n for n in legs() if a.only is None or any(s in n for s in a.only.split(","))]
    parent = os.path.abspath(a.parent_tree)
    runs = {"parent_a": run_tree(parent, names, True, a.jobs), "parent_b": run_tree(parent, names, True, a.jobs),
            "child": run_tree(ROOT, names, True, a.jobs)}
    unprofiled = [n for n in names if n.endswith("topk16/lookahead_default")]
    plain = run_tree(ROOT, unprofiled, False, a.jobs)
    fields = ("sha256_student_flat", "logs", "eval_loss", "launches", "selections")
    import torch
    report = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "parent_commit": a.parent_commit,
              "device": torch.cuda.get_device_name(0),
              "profiler": {"note": "hashes and launch counts come from the same, profiled run; the legs below were run again "
                                   "on this tree without the profiler: true where hash and logs equal the profiled run's",
                           "legs": {n: all(plain[n][k] == runs["child"][n][k] for k in ("sha256_student_flat", "logs"))
                                    for n in unprofiled}},
              "legs": {}}
    for n in names:
        pa, pb, ch = (runs[t][n] for t in ("parent_a", "parent_b", "child"))
        report["legs"][n] = {"env": legs()[n][1], "parent_repeatable": {k: pa[k] == pb[k] for k in fields},
                             "child_equals_parent": {k: ch[k] == pa[k] for k in fields},
                             "parent_and_child" if all(ch[k] == pa[k] for k in fields) else "differs":
                             pa if all(ch[k] == pa[k] for k in fields) else {"parent": pa, "child": ch}}
    report["all_equal"] = (all(all(v["parent_repeatable"].values()) and all(v["child_equals_parent"].values())
                               for v in report["legs"].values()) and all(report["profiler"]["legs"].values()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(report, open(a.out, "w"), indent=1)
    print(json.dumps({"all_equal": report["all_equal"], "legs": len(names),
                      "differ": [n for n, v in report["legs"].items() if "differs" in v]}))
    sys.exit(0 if report["all_equal"] else 1)


if __name__ == "__main__":
    main()
