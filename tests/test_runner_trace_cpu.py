"""The decoder runner's exact launch sequence, checked without a GPU.

speech_distill_amd/csrc/sd_model.hip never reads device memory: it computes addresses and calls other entries.
tests/csrc/runner_trace.cpp defines every symbol the runner's object leaves undefined as a stub that logs its arguments
(streams and events as small ids, host arrays by content), drives the runner with fabricated base addresses through the
backward's schedules (side stream, overlap masks, flags, head rows, packed documents, dx0_out, callbacks, stub return
values), the forward's save modes, the block and decode entries and every refusal, and writes one trace per case.

The expectations in tests/golden/runner_trace/ were recorded from the runner BEFORE the backward was split into steps
(one 220-line function with literal event indices): every launch, record and wait, in order, with every argument.  A
wrong event, a moved wait or a changed address in the host code is a differing line here instead of a rare wrong gradient.
The program is linked against the runner's object alone -- no HIP runtime library -- so it cannot open a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "speech_distill_amd", "csrc")
WANT = os.path.join(GOLDEN, "runner_trace")
PROGRAM = os.path.join(ROOT, "tests", "csrc", "runner_trace.cpp")


def plain_stubs():
    """`int sd_x(params) { return REC(params); }` for every int-returning prototype of sd_hip.h that neither the runner nor
    the trace program defines itself (the program writes out the stubs that steer a branch or print a host array)."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sd_hip.h")).read(), flags=re.S)
    own = set(re.findall(r"^(?:int|int64_t) (sd_\w+)\(", open(PROGRAM).read(), flags=re.M))
    out = []
    for name, params in re.findall(r"\bint\s+(sd_\w+)\s*\(([^)]*)\)\s*;", header):
        if name in own or name.startswith("sd_qwen3_") or params.strip() == "void":
            continue
        params = " ".join(params.split())
        names = [re.search(r"(\w+)$", q.strip()).group(1) for q in params.split(",")]
        out.append('extern "C" int %s(%s) { return REC(%s); }\n' % (name, params, ", ".join(names)))
    return "".join(out)


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("runner_trace")
    obj, exe, out = str(tmp / "sd_model.o"), str(tmp / "runner_trace"), tmp / "out"
    out.mkdir()
    (tmp / "runner_trace_stubs.inc").write_text(plain_stubs())
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    flags = makefile.split("FLAGS  =", 1)[1].split("\nSRCS", 1)[0].replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    subprocess.run([HIPCC, *flags, "-c", os.path.join(CSRC, "sd_model.hip"), "-o", obj], check=True)
    subprocess.run([shutil.which("g++") or "c++", "-std=c++17", "-O1", "-I", str(tmp), "-o", exe, PROGRAM, obj], check=True)
    subprocess.run([exe, str(out)], check=True, timeout=60)
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


def test_same_cases_as_recorded(traces):
    assert sorted(traces) == sorted(os.listdir(WANT))
    assert len(traces) > 30


@pytest.mark.parametrize("case", sorted(os.listdir(WANT)))
def test_trace_is_byte_identical(traces, case):
    want = open(os.path.join(WANT, case), "rb").read()
    got = traces[case]
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail("%s: first difference at line %d\n  recorded: %s\n  now:      %s" % (
            case, first + 1, w[first] if first < len(w) else "<end>", g[first] if first < len(g) else "<end>"))


def test_refusals_launch_nothing():
    for line in open(os.path.join(WANT, "refusals.txt")):
        assert line.rstrip().endswith("lines=0") and " -> -" in line, line
