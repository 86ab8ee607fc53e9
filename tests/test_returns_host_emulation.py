"""The realised-returns kernels' per-lane bodies (csrc/dql_returns.hpp on csrc/dql_model.hpp) run on the CPU and held to the oracle's stepwise loop with ==
(CPU only, no GPU).

tests/host_emu/returns_emu.cpp compiles the real device headers as host C++: the real `model_episodes` with the log sink writes every env's column of the
decision log exactly as k_returns_fly does, then the real `returns_sweep` walks every column backwards as a lane of k_returns_sweep does.  The yardstick is the
unchanged oracle stepped with external actions and a numpy float64 recursion (tests/returns_checks.py), which knows nothing of the kernels: visits, return_fx,
cut_decisions, by_code and steps_sum must be equal.  Built twice: plain, and with ASan + UBSan as a stand-alone program (any report fails).

Every row asserts on the ORACLE's result, before comparing, that the events it is there for occurred (returns_checks.yardstick).  A host wave is one lane: 64
lanes of different lengths sweeping together and the LDS staging show on the GPU only (tests/test_gpu_returns.py)."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd import ops
from dql_multirotor_landing_amd.config import N_CELLS

import host_emu_harness as heh
import model_checks as mc
import returns_checks as rck

emu = heh.emu_fixture("returns_emu")


def run_emu(exe, cfg, sets, n, seed, eps, gamma, max_steps, episodes, tmp, sanitized=False):
    """the returns of the table sets `sets` as ops.returns_map returns them"""
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = (struct.pack("<6i", len(c), cfg.dtype, K, max_steps, episodes, 0) + struct.pack("<2q", n, seed) +
           struct.pack("<3d", eps, gamma, float(ops.returns_bound_fx(cfg, gamma, max_steps))))
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + qa.tobytes() + qb.tobytes(), tmp, "returns", sanitized))
    visits, return_fx, cut = r.take(np.int64, (K, N_CELLS)), r.take(np.int64, (K, N_CELLS)), r.take(np.int64, (K,))
    by_code, steps_sum, faults = r.take(np.int64, (K, mc.N_COLS)), r.take(np.int64, (K,)), r.take(np.int64, (1,))
    r.done()
    assert faults[0] == 0, "a range check counted a fault: the guard dropped a contribution"
    return {"visits": visits, "return_fx": return_fx, "cut_decisions": cut, "by_code": by_code, "steps_sum": steps_sum}


def fly_row(exe, case_id, gamma, tmp, sanitized=False):
    cfg, tables, eps, n, max_steps, episodes = rck.case_args(case_id)
    want = rck.yardstick(case_id, gamma)
    got = run_emu(exe, cfg, [tables], n, rck.SEED, eps, gamma, max_steps, episodes, tmp, sanitized)
    rck.assert_returns_set_equal(got, 0, want, f"case {case_id}, gamma {gamma}{' (sanitized)' if sanitized else ''}")
    return got, want


@pytest.mark.parametrize("case_id,gamma", rck.ROWS, ids=rck.ROW_IDS)
def test_the_returns_of_a_row_equal_the_oracle_s_stepwise_returns(emu, case_id, gamma, tmp_path):
    got, want = fly_row(emu["plain"], case_id, gamma, tmp_path)
    # conservation: every decision the model counts is kept or cut, and the kept ones are what the yardstick kept
    if case_id in mc.CASES:
        assert int(got["visits"].sum()) + int(got["cut_decisions"][0]) == mc.yardstick(case_id)["events"]["decisions"]
    assert int(got["visits"].sum()) == want["events"]["kept"] and int(got["cut_decisions"][0]) == want["events"]["cut"]


@pytest.mark.parametrize("case_id,gamma", rck.ROWS, ids=rck.ROW_IDS)
def test_returns_clean_under_asan_and_ubsan(emu, case_id, gamma, tmp_path):
    """every row through the ASan + UBSan build: no report, and still the oracle's result"""
    fly_row(emu["san"], case_id, gamma, tmp_path, sanitized=True)


def test_gamma_zero_returns_are_the_model_s_rewards(emu, tmp_path):
    """case D (nobody cut) at gamma 0: g_t = r_t, so return_fx and visits are the transition model's reward_fx and visits of the same flights"""
    got, _ = fly_row(emu["plain"], "D", 0.0, tmp_path)
    model = mc.yardstick("D")
    assert np.array_equal(got["return_fx"][0], model["reward_fx"]) and np.array_equal(got["visits"][0], model["visits"])


def test_two_table_sets_in_one_job_equal_their_single_jobs(emu, tmp_path):
    """case A's set and the all-zero set in one job: each equals its own single job, so nothing of a set's columns lands in its neighbour's tables"""
    cfg, tables, eps, n, max_steps, episodes = rck.case_args("A")
    zeros = (np.zeros(N_CELLS), np.zeros(N_CELLS))
    both = run_emu(emu["plain"], cfg, [tables, zeros], n, rck.SEED, eps, 0.99, max_steps, episodes, tmp_path)
    rck.assert_returns_set_equal(both, 0, rck.yardstick("A", 0.99), "set 0 of two")
    alone = run_emu(emu["plain"], cfg, [zeros], n, rck.SEED, eps, 0.99, max_steps, episodes, tmp_path)
    assert alone["visits"][0].tolist() != both["visits"][0].tolist(), "the two sets fly differently"
    for f in rck.FIELDS:
        assert np.array_equal(both[f][1], alone[f][0]), f
