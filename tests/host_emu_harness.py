"""What the host-emulation modules (tests/test_*_host_emulation.py) share: how a driver under tests/host_emu/ is built (plain, and with ASan + UBSan; once
per test session), how one job is run through it as a child process, and how its result file is read.  For the sequential-learner family it also owns the two
job layouts (`learner_job`, `recipes_job`) and the reader of every result file of the family (`learner_result`); the drivers' side of the same layouts is
tests/host_emu/emu_learners.h.  A module keeps its `run_emu`, its yardsticks and its tests; the other modules keep their own job headers, whose drivers' side
of the plumbing is tests/host_emu/emu_common.h."""
import os
import shutil
import struct
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


_BUILDS = {}  # driver name -> {"plain": path, "san": path}: a driver is compiled once per test session, whichever modules ask for it


def emu_fixture(name):
    """a module-scoped fixture: the two builds of tests/host_emu/<name>.cpp, compiled side by side on first use: {"plain": path, "san": path}"""
    @pytest.fixture(scope="module")
    def emu(tmp_path_factory):
        if name not in _BUILDS:
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
                _BUILDS[name] = dict(zip(builds, ex.map(build, builds)))
        return _BUILDS[name]
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


def _f64(arrays):
    return b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in arrays)


def learner_job(cfg, n, seed, runs, alpha, eps, window, min_successes, max_episodes, log_capacity, tables=None, extra=()):
    """the plain layout (emu_learners.h's LearnerJob): 16 words, of which the last is extra[0] (0 / nstep / E), then extra[1:] (team_nstep_emu: nstep, rearm_after)"""
    c = bytes(cfg.to_c())
    words = [len(c), cfg.dtype, n, len(runs), *runs, *[0] * (4 - len(runs)), len(alpha), len(eps), window, min_successes, max_episodes, log_capacity, int(tables is not None),
             *(extra or (0,))]
    return struct.pack(f"<{len(words)}i", *words) + struct.pack("<q", seed) + c + _f64([alpha, eps]) + _f64(tables or ())


def recipes_header(cfg, n, seed, runs, every, log_capacity, n_recipes, has_tables, mode=0, cap=0):
    """the head of the recipe layout (emu_learners.h's RecipeJob); mode 1: recipes_emu's one call of build_worklist_recipes with `cap` slots"""
    c = bytes(cfg.to_c())
    return struct.pack("<24i", len(c), cfg.dtype, n, len(runs), *runs, *[0] * (8 - len(runs)), every, log_capacity, n_recipes, has_tables, mode, cap, *[0] * 6) + struct.pack("<q", seed) + c


def recipes_job(cfg, n, seed, runs, every, log_capacity, recipes, recipe_of, tables=None):
    """the recipe layout: the head, recipe_of, per recipe its 28 words (the recipe's nstep in word 5) and arrays, the tables"""
    job = recipes_header(cfg, n, seed, runs, every, log_capacity, len(recipes), int(tables is not None)) + np.ascontiguousarray(recipe_of, np.int32).tobytes()
    for r in recipes:
        alpha, alpha_min, ratios, lv = r.checked(cfg)
        h = [int(r.quirks), alpha.size, int(r.last_level), int(bool(r.advance_exhausted)), int(r.transfer_order), int(r.nstep), 0, 0]
        for e, w, ms, me in lv:
            h += [e.size, w, ms, me]
        job += struct.pack("<28i", *h) + struct.pack("<d", alpha_min) + ratios.tobytes() + alpha.tobytes() + b"".join(e.tobytes() for e, _, _, _ in lv)
    return job + _f64(tables or ())


def learner_result(b, n, log_capacity, cfg, n_envs=None, tail=(), periods=None):
    """a result file of the learner family, whole (emu_learners.h's write_result): tables, counters, episode log, env state by field name (n_envs envs: n, or
    n E for teams); then the tails in `tail`: "levels" (level, promoted_at, episodes_at, entered_period, and the period index reached, which must be `periods`)
    and "pending_len" (an entry per env)"""
    reader = Reader(b)
    take, m = reader.take, n if n_envs is None else n_envs
    out = {"qa": take(np.float64, (n, N_CELLS)), "qb": take(np.float64, (n, N_CELLS)), "count": take(np.float64, (n, N_CELLS)),
           "decisions": take(np.int64, (n,)), "by_code": take(np.int64, (ec.N_CODES, n)), "episodes": take(np.int32, (n,)), "successes": take(np.int32, (n,)),
           "level_episodes": take(np.int32, (n,)), "promotion_episode": take(np.int32, (n,)), "frozen": take(np.int32, (n,)), "log_n": take(np.int32, (n,)),
           "log_code": take(np.uint8, (n, log_capacity)), "log_len": take(np.uint16, (n, log_capacity))}
    reals, ints = take(np.float64, (NF_REAL, m)), take(np.int32, (NF_INT, m))
    faults = take(np.int64, (1,))
    if "levels" in tail:
        out.update({"level": take(np.int32, (n,)), "promoted_at": take(np.int32, (5, n)), "episodes_at": take(np.int32, (5, n)), "entered_period": take(np.int64, (5, n))})
        period_index = int(take(np.int64, (1,))[0])
    if "pending_len" in tail:
        out["pending_len"] = take(np.int32, (m,))
    reader.done()
    assert faults[0] == 0, "a range check counted a fault: the bounds guard dropped an update"
    assert "levels" not in tail or period_index == periods
    ref = ec.Reference(cfg, 1, 0)
    out.update({f: reals[k] for f, k in ref.ri.items()})
    out.update({f: ints[k] for f, k in ref.ii.items()})
    return out
