"""What the five host-emulation modules (tests/test_*_host_emulation.py) share: how a driver under tests/host_emu/ is built (plain, and with
ASan + UBSan), how one job is run through it as a child process, and how its result file is read.  Each module keeps its own job header, its `run_emu`,
its yardsticks and its tests; the drivers' side of the same plumbing is tests/host_emu/emu_common.h."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import N_CELLS

import ensemble_checks as ec

ROOT = Path(__file__).resolve().parent.parent
EMU = ROOT / "tests" / "host_emu"
CSRC = ROOT / "dql_multirotor_landing_amd" / "csrc"

PLAIN_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
SAN_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
# the sanitizer settings live in the child's environment only; every report is fatal (halt_on_error) and printed with its stack
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
SAN_MARKERS = ("runtime error:", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "SUMMARY: ")
NF_REAL, NF_INT = 64, 7  # dql_device.hpp


def clangxx():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    for c in (rocm / "llvm" / "bin" / "clang++", rocm / "lib" / "llvm" / "bin" / "clang++"):
        if c.exists():
            return str(c)
    c = shutil.which("clang++")
    assert c, "the host emulation needs clang++ (ROCm's llvm/bin/clang++): dql_device.hpp uses clang vector extensions"
    return c


def emu_fixture(name):
    """a module-scoped fixture: the two builds of tests/host_emu/<name>.cpp, compiled side by side: {"plain": path, "san": path}"""
    @pytest.fixture(scope="module")
    def emu(tmp_path_factory):
        out = tmp_path_factory.mktemp(name)
        cxx = clangxx()
        common = ["-I", str(EMU), "-I", str(CSRC), "-Wno-pass-failed", str(EMU / f"{name}.cpp")]
        builds = {"plain": PLAIN_FLAGS, "san": SAN_FLAGS}

        def build(kind):
            exe = out / f"{name}_{kind}"
            r = subprocess.run([cxx, *builds[kind], *common, "-o", str(exe)], capture_output=True, text=True)
            assert r.returncode == 0, f"{kind} build of {name} failed:\n{r.stderr[-4000:]}"
            return exe

        with ThreadPoolExecutor(2) as ex:
            return dict(zip(builds, ex.map(build, builds)))
    return emu


def run(exe, job_bytes, tmp, stem, sanitized=False, timeout=1800, what=""):
    """one job through the driver `exe` as a child process: status 0 and no sanitizer report, or the end of its stderr; returns the result file's bytes"""
    job, res = tmp / f"{stem}_job.bin", tmp / f"{stem}_res.bin"
    job.write_bytes(job_bytes)
    env = dict(os.environ, **SAN_ENV) if sanitized else None
    r = subprocess.run([str(exe), str(job), str(res)], capture_output=True, text=True, env=env, timeout=timeout)
    name, what = Path(exe).name.rsplit("_", 1)[0], f", {what}" if what else ""
    assert r.returncode == 0, f"{name} ({'sanitized' if sanitized else 'plain'}) failed{what}:\n{r.stderr[-6000:]}"
    assert not any(m in r.stderr for m in SAN_MARKERS), f"sanitizer report{what}:\n{r.stderr[-6000:]}"
    return res.read_bytes()


class Reader:
    """a result file, array after array in the order the driver wrote them"""

    def __init__(self, b):
        self.b, self.o = b, 0

    def take(self, dtype, shape):
        a = np.frombuffer(self.b, dtype, int(np.prod(shape)), self.o).reshape(shape)
        self.o += a.nbytes
        return a

    def done(self):
        assert self.o == len(self.b), f"{len(self.b) - self.o} bytes of the result file were not read"


def learner_result(reader, n, log_capacity, cfg):
    """what learner_emu and advance_emu both write first (emu_common.h's LearnerState::put): tables, counters, episode log, env state by field name"""
    take = reader.take
    out = {"qa": take(np.float64, (n, N_CELLS)), "qb": take(np.float64, (n, N_CELLS)), "count": take(np.float64, (n, N_CELLS)),
           "decisions": take(np.int64, (n,)), "by_code": take(np.int64, (ec.N_CODES, n)), "episodes": take(np.int32, (n,)), "successes": take(np.int32, (n,)),
           "level_episodes": take(np.int32, (n,)), "promotion_episode": take(np.int32, (n,)), "frozen": take(np.int32, (n,)), "log_n": take(np.int32, (n,)),
           "log_code": take(np.uint8, (n, log_capacity)), "log_len": take(np.uint16, (n, log_capacity))}
    reals, ints = take(np.float64, (NF_REAL, n)), take(np.int32, (NF_INT, n))
    faults = take(np.int64, (1,))
    assert faults[0] == 0, "a range check counted a fault: the bounds guard dropped an update"
    ref = ec.Reference(cfg, 1, 0)
    out.update({f: reals[k] for f, k in ref.ri.items()})
    out.update({f: ints[k] for f, k in ref.ii.items()})
    return out
