"""The step kernel's level-0 instance against its generic twin, on the CPU (no GPU): tests/host_emu/level0_emu.cpp compiles the real device header as host
C++ (tests/host_emu_harness.py builds it plain and with ASan + UBSan, as stand-alone programs) and runs one launch of k_step through
agent_period<TICK, XMODE, LEVEL0> with LEVEL0 false — the generic body — or true — the instance the host picks for launches at level 0, in which the
working level is a compile-time constant.  On the same level-0 job the two must write identical result files, and those must be the oracle's launch; a job
at another level is refused for the level-0 form, as the host never makes that choice.  The two-axis form of the literal tick is run here too although the
library compiles level-0 instances for x-axis configs only (launch_step_t says why): its source agrees with the generic form and the oracle on the CPU.
"""
import struct
import subprocess

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, N_CELLS, Q_GOAL_COUNT_KEPT, Q_UPDATE_TABLE_A_ONLY, DqlConfig

import host_emu_harness as heh
from host_emu_harness import NF_INT, NF_REAL
from test_step_host_emulation import MODE_EXTERNAL, TICK_LIT, TICK_PACKED_LITM, X_ONLY, X_TWO, assert_launch_equal, recorded_launches

emu = heh.emu_fixture("level0_emu")

NOISY = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)
# the quirk sets of tests/test_gpu_level0_instance.py, plain and with the flagship's flags; the two-axis form of the literal tick
CONFIGS = [dict(), dict(NOISY), dict(quirks=Q_GOAL_COUNT_KEPT | Q_UPDATE_TABLE_A_ONLY), dict(quirks=0, **NOISY), dict(init_uniform=1), dict(two_axis=1), dict(two_axis=1, quirks=0, **NOISY)]


def _job_bytes(cfg, tick, xmode, level0, snap):
    c = bytes(cfg.to_c())
    n = snap["ints"].shape[1]
    hdr = struct.pack("<8i", len(c), cfg.dtype, tick, xmode, snap["mode"], snap["P"], 0, int(level0))
    hdr += struct.pack("<4q", n, 0, snap["step_index"], snap["seed"]) + struct.pack("<d", snap["eps"])
    return b"".join([hdr, c, np.ascontiguousarray(snap["reals"], np.float64).tobytes(), np.ascontiguousarray(snap["ints"], np.int32).tobytes(),
                     np.ascontiguousarray(snap["qa"], np.float64).tobytes(), np.ascontiguousarray(snap["qb"], np.float64).tobytes()])


def _run(exe, cfg, tick, xmode, level0, snap, tmp, sanitized):
    return heh.run(exe, _job_bytes(cfg, tick, xmode, level0, snap), tmp, f"l0_{tick}_{xmode}_{int(level0)}", sanitized, timeout=600,
                   what=f"tick {tick} xmode {xmode} level0 {level0} mode {snap['mode']} P {snap['P']}")


def _parsed(b, n):
    r = heh.Reader(b)
    got = r.take(np.float64, (NF_REAL, n)), r.take(np.int32, (NF_INT, n)), r.take(np.int64, (4 * N_CELLS,)), r.take(np.int64, (12,)), 0
    r.done()
    return got


def _instances(cfg):
    return [(TICK_LIT, X_TWO)] if cfg.two_axis else [(TICK_LIT, X_ONLY), (TICK_PACKED_LITM, X_ONLY)]


def _both_forms_agree(exe, kw, n, seed, periods, tmp, sanitized):
    cfg = DqlConfig(dtype=F32, t_max=2.0, **kw)  # short episodes: resets (the placement's level test) inside the launches
    snaps = [s for s in recorded_launches(cfg, n, seed=seed, periods=periods) if s["mode"] != MODE_EXTERNAL]
    assert sum(int(s["out"][3][1]) for s in snaps) > 0, "no episode ended: the case would not reach resets"
    for tick, xmode in _instances(cfg):
        for k, s in enumerate(snaps):
            what = f"{kw} tick {tick} xmode {xmode} launch {k} (mode {s['mode']}, P {s['P']})"
            generic = _run(exe, cfg, tick, xmode, False, s, tmp, sanitized)
            level0 = _run(exe, cfg, tick, xmode, True, s, tmp, sanitized)
            assert level0 == generic, f"{what}: the level-0 instance's result file differs from the generic one's"
            assert_launch_equal(_parsed(level0, n), s, what)


@pytest.mark.parametrize("kw", CONFIGS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_level0_instance_writes_the_generic_instance_s_result_file(emu, kw, tmp_path):
    _both_forms_agree(emu["plain"], kw, 96, 11, (1, 16), tmp_path, False)


@pytest.mark.parametrize("kw", [dict(NOISY), dict(two_axis=1, quirks=0, **NOISY)], ids=["noisy", "two_axis"])
def test_the_same_under_asan_and_ubsan(emu, kw, tmp_path):
    _both_forms_agree(emu["san"], kw, 24, 5, (16,), tmp_path, True)


def test_level0_form_is_refused_above_level_0(emu, tmp_path):
    cfg = DqlConfig(dtype=F32, working_curriculum_step=1)
    snap = dict(reals=np.zeros((NF_REAL, 1)), ints=np.zeros((NF_INT, 1), np.int32), qa=np.zeros(N_CELLS), qb=np.zeros(N_CELLS), mode=0, P=1, step_index=0, seed=0, eps=0.0)
    job = tmp_path / "refused.bin"
    job.write_bytes(_job_bytes(cfg, TICK_LIT, X_ONLY, True, snap))
    r = subprocess.run([str(emu["plain"]), str(job), str(tmp_path / "refused.out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "never serves level 1" in r.stderr, r.stderr[-2000:]

