"""The team learner's two bodies (csrc/dql_team.hpp: team_env_period per env, team_apply per team) run on the CPU and held `==` to the reference loop built from
the oracle (CPU only, no GPU).

tests/host_emu/team_emu.cpp compiles the real device headers as host C++ and flies every team as k_learn_team's lanes do, env by env into an array of E
records and then the real team_apply on it.  The yardstick is tests/team_checks.py's `TeamReference`: the unchanged oracle stepped with external actions,
`oracle.agent_predict` before the step and `oracle.agent_update` for the envs in ascending order after it, on the learner's shared tables.  Every case first
asserts on the reference that the events it is there for occurred (team_checks.case_reference).  Built twice: plain, and with ASan + UBSan."""
import pytest

from dql_multirotor_landing_amd.config import F32, F64, training_config

import ensemble_checks as ec
import host_emu_harness as heh
import team_checks as tc
from test_learner_host_emulation import run_emu as run_learner_emu

emu = heh.emu_fixture("team_emu")
learner_emu = heh.emu_fixture("learner_emu")


def run_emu(exe, cfg, n, envs_per_learner, seed, runs, tmp, eps, window, min_successes, max_episodes, log_capacity, sanitized=False, tables=None):
    job = heh.learner_job(cfg, n, seed, runs, cfg.alpha_table(), eps, window, min_successes, max_episodes, log_capacity, tables, extra=(envs_per_learner,))
    return heh.learner_result(heh.run(exe, job, tmp, "team", sanitized), n, log_capacity, cfg, n_envs=n * envs_per_learner)


def run_case(exe, name, dtype, runs, tmp, sanitized=False, learners=None):
    c = tc.CASES[name]
    tables = tc.case_tables(name)
    n = c["L"] if learners is None else learners
    if tables is not None:
        tables = tuple(t[:n] for t in tables)
    return run_emu(exe, tc.case_config(name, dtype), n, c["E"], tc.SEED, runs, tmp, sanitized=sanitized, tables=tables, **c["sched"])


@pytest.mark.parametrize("name,dtype", tc.CASE_IDS, ids=[f"{n}-{'f64' if d == F64 else 'f32'}" for n, d in tc.CASE_IDS])
def test_case_equals_the_team_reference(emu, name, dtype, tmp_path):
    want, _ = tc.case_reference(name, dtype)  # asserts on the reference what the case is for
    got = run_case(emu["plain"], name, dtype, (tc.CASES[name]["periods"],), tmp_path)
    tc.assert_equal(got, want, f"case {name}")


@pytest.mark.parametrize("name", ["B", "C", "F"])
def test_launches_of_7_and_293_periods_equal_one_of_300(emu, name, tmp_path):
    """the launch boundary: envs, counters, ring and threshold go through memory between two launches"""
    want, ref = tc.case_reference(name, F32)
    assert tc.CASES[name]["periods"] == 300 and ref.freeze_period.max() > 7, "a team must be live across the boundary"
    got = run_case(emu["plain"], name, F32, (7, 293), tmp_path)
    tc.assert_equal(got, want, f"case {name}, 7 + 293")


@pytest.mark.parametrize("name,dtype", [("A", F32), ("B", F64), ("D", F32), ("E", F32)], ids=["A-f32", "B-f64", "D-f32", "E-f32"])
def test_clean_under_asan_and_ubsan(emu, name, dtype, tmp_path):
    """the sanitized build, two launches: the E records of a team, the per-learner arrays [L] and the per-env arrays [L * E] are exactly as long as stated"""
    want, _ = tc.case_reference(name, dtype)
    p = tc.CASES[name]["periods"]
    got = run_case(emu["san"], name, dtype, (7, p - 7), tmp_path, sanitized=True)
    tc.assert_equal(got, want, f"sanitized case {name}")


def test_independence_of_the_number_of_learners(emu, tmp_path):
    """learners [0, 3) of case B == an ensemble of 3 learners"""
    want, _ = tc.case_reference("B", F32)
    got = run_case(emu["plain"], "B", F32, (300,), tmp_path, learners=3)
    tc.assert_equal(got, want, "case B, three learners", learners=([0, 1, 2], [0, 1, 2]), envs_per_learner=tc.CASES["B"]["E"])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_one_env_per_learner_through_the_team_body_equals_learner_periods(emu, learner_emu, dtype, tmp_path):
    """E = 1: team_env_period + team_apply == learner_periods on the trained-tables case (learner_emu's result, itself held to ensemble_checks.Reference)"""
    n = 26
    cfg = training_config(4, quirks=ec.Q_PAPER, dtype=dtype)
    tables = ec.trained_tables(n)
    kw = dict(ec.TRAINED_LEARNERS_CASE, tables=tables)
    want = run_learner_emu(learner_emu["plain"], cfg, n, ec.TRAINED_LEARNERS_SEED, ec.TRAINED_LEARNERS_SPLIT, tmp_path, **kw)
    assert (want["promotion_episode"] >= 0).any() and (want["qb"] != tables[1]).any() and want["episodes"].sum() > n
    got = run_emu(emu["plain"], cfg, n, 1, ec.TRAINED_LEARNERS_SEED, ec.TRAINED_LEARNERS_SPLIT, tmp_path, tables=tables, **ec.TRAINED_LEARNERS_CASE)
    ec.assert_equal(got, want, f"E = 1 against learner_periods, dtype {dtype}")
    ref = tc.TeamReference(cfg, n, 1, ec.TRAINED_LEARNERS_SEED, tables=tables, **ec.TRAINED_LEARNERS_CASE)
    ref.run(ec.TRAINED_LEARNERS_PERIODS)
    ec.assert_equal(got, ref.result(), f"E = 1 against the team reference, dtype {dtype}")
