"""The sequential learner's per-lane body (csrc/dql_learner.hpp) run on the CPU and held `==` to the reference loop built from the oracle (CPU only, no GPU).

tests/host_emu/learner_emu.cpp compiles the real device headers as host C++ (the stand-in runtime header of step_emu.cpp) and flies every learner lane by
lane, exactly as k_learn does, in two launches of 150 + 250 periods.  The yardstick is tests/ensemble_checks.py's `Reference`: the unchanged oracle stepped
with external actions, `oracle.agent_predict` / `oracle.agent_update` on per-learner tables.  Built twice: plain, and with ASan + UBSan (any report fails)."""
import os
import shutil
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config

import ensemble_checks as ec

ROOT = Path(__file__).resolve().parent.parent
EMU = ROOT / "tests" / "host_emu"
CSRC = ROOT / "dql_multirotor_landing_amd" / "csrc"
L, SEED, RUNS, LOG_CAP = 3, 2024, (150, 250), 32

PLAIN_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
SAN_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
SAN_MARKERS = ("runtime error:", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "SUMMARY: ")


def _clangxx():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    for c in (rocm / "llvm" / "bin" / "clang++", rocm / "lib" / "llvm" / "bin" / "clang++"):
        if c.exists():
            return str(c)
    c = shutil.which("clang++")
    assert c, "the host emulation needs clang++ (ROCm's llvm/bin/clang++): dql_device.hpp uses clang vector extensions"
    return c


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = tmp_path_factory.mktemp("learner_emu")
    cxx = _clangxx()
    common = ["-I", str(EMU), "-I", str(CSRC), "-Wno-pass-failed", str(EMU / "learner_emu.cpp")]
    builds = {"plain": PLAIN_FLAGS, "san": SAN_FLAGS}

    def build(kind):
        exe = out / f"learner_emu_{kind}"
        r = subprocess.run([cxx, *builds[kind], *common, "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, f"{kind} build of learner_emu failed:\n{r.stderr[-4000:]}"
        return exe

    with ThreadPoolExecutor(2) as ex:
        return dict(zip(builds, ex.map(build, builds)))


def run_emu(exe, cfg, n, seed, runs, tmp, eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30, sanitized=False):
    c = bytes(cfg.to_c())
    alpha = cfg.alpha_table()
    r4 = list(runs) + [0] * (4 - len(runs))
    hdr = struct.pack("<16i", len(c), cfg.dtype, n, len(runs), *r4, len(alpha), len(eps), window, min_successes, max_episodes, LOG_CAP, 0, 0) + struct.pack("<q", seed)
    job, res = tmp / "learner_job.bin", tmp / "learner_res.bin"
    job.write_bytes(hdr + c + alpha.tobytes() + np.asarray(eps, np.float64).tobytes())
    env = dict(os.environ, **SAN_ENV) if sanitized else None
    r = subprocess.run([str(exe), str(job), str(res)], capture_output=True, text=True, env=env, timeout=1800)
    assert r.returncode == 0, f"learner_emu ({'sanitized' if sanitized else 'plain'}) failed:\n{r.stderr[-6000:]}"
    assert not any(m in r.stderr for m in SAN_MARKERS), f"sanitizer report:\n{r.stderr[-6000:]}"
    b = res.read_bytes()
    o = 0

    def take(dtype, shape):
        nonlocal o
        cnt = int(np.prod(shape))
        a = np.frombuffer(b, dtype, cnt, o).reshape(shape)
        o += a.nbytes
        return a

    out = {"qa": take(np.float64, (n, N_CELLS)), "qb": take(np.float64, (n, N_CELLS)), "count": take(np.float64, (n, N_CELLS)),
           "decisions": take(np.int64, (n,)), "by_code": take(np.int64, (ec.N_CODES, n)), "episodes": take(np.int32, (n,)), "successes": take(np.int32, (n,)),
           "level_episodes": take(np.int32, (n,)), "promotion_episode": take(np.int32, (n,)), "frozen": take(np.int32, (n,)), "log_n": take(np.int32, (n,)),
           "log_code": take(np.uint8, (n, LOG_CAP)), "log_len": take(np.uint16, (n, LOG_CAP))}
    reals, ints = take(np.float64, (64, n)), take(np.int32, (7, n))
    faults = take(np.int64, (1,))
    assert o == len(b)
    assert faults[0] == 0, "the bounds guard dropped an update"
    ref = ec.Reference(cfg, 1, 0)
    out.update({f: reals[k] for f, k in ref.ri.items()})
    out.update({f: ints[k] for f, k in ref.ii.items()})
    return out


@pytest.fixture(scope="module")
def reference():
    cache = {}

    def get(dtype, quirks):
        if (dtype, quirks) not in cache:
            ref = ec.Reference(training_config(0, quirks=quirks, dtype=dtype), L, SEED, log_capacity=LOG_CAP)
            ref.run(sum(RUNS))
            cache[(dtype, quirks)] = ref.result()
        return cache[(dtype, quirks)]
    return get


@pytest.mark.parametrize("quirks", [ec.Q_REFERENCE, ec.Q_BENCH, ec.Q_PAPER], ids=["quirks-0x7f", "quirks-0x60", "quirks-0x40"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_three_learners_400_periods_in_two_launches_equal_the_reference_loop(emu, reference, dtype, quirks, tmp_path):
    want = reference(dtype, quirks)
    # not vacuous: episodes ended (so the eps table moved on and envs reset), and the tables were written
    assert want["episodes"].min() >= 2 and (want["qa"] != 0).any() and want["decisions"].min() > 300
    if quirks == ec.Q_PAPER:
        assert (want["qb"] != 0).any(), "the coin never picked Q_table_b"
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    got = run_emu(emu["plain"], cfg, L, SEED, RUNS, tmp_path)
    ec.assert_equal(got, want, f"dtype {dtype} quirks {quirks:#x}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_learner_clean_under_asan_and_ubsan(emu, reference, dtype, tmp_path):
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=dtype)
    got = run_emu(emu["san"], cfg, L, SEED, RUNS, tmp_path, sanitized=True)
    ec.assert_equal(got, reference(dtype, ec.Q_PAPER), f"sanitized dtype {dtype}")
