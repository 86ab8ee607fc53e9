"""The team n-step learner's bodies (csrc/dql_team.hpp: team_env_period per env; csrc/dql_team_nstep.hpp: team_apply_nstep per team, team_window_load /
team_window_store per env) run on the CPU and held `==` to the yardstick of tests/team_nstep_checks.py (CPU only, no GPU).

tests/host_emu/team_nstep_emu.cpp compiles the real device headers as host C++ and flies every team as k_learn_team_nstep's lanes do; the windows are reached
through checked references onto poisoned storage exactly as long as stated: the team's working copy [16][E] plus head and len [E], the persistent arrays
[16][L E] and [L E].  Built twice through tests/host_emu_harness.py: plain, and as a stand-alone ASan + UBSan program (any report fails).  The yardstick
itself is held to its two parents first: at n = 1 to `team_checks.TeamReference`, at E = 1 to `nstep_checks.NstepReference`."""
import pytest

from dql_multirotor_landing_amd.config import F32, F64, training_config

import ensemble_checks as ec
import host_emu_harness as heh
import nstep_checks as nc
import team_checks as tc
import team_nstep_checks as tn
from test_nstep_host_emulation import run_emu as run_nstep_emu
from test_team_host_emulation import run_case as run_team_case

emu = heh.emu_fixture("team_nstep_emu")
team_emu = heh.emu_fixture("team_emu")
nstep_emu = heh.emu_fixture("nstep_emu")


def run_emu(exe, cfg, n, envs_per_learner, seed, runs, nstep, tmp, eps, window, min_successes, max_episodes, log_capacity, sanitized=False, tables=None, rearm_after=-1):
    job = heh.learner_job(cfg, n, seed, runs, cfg.alpha_table(), eps, window, min_successes, max_episodes, log_capacity, tables, extra=(envs_per_learner, nstep, rearm_after))
    out = heh.learner_result(heh.run(exe, job, tmp, "team_nstep", sanitized), n, log_capacity, cfg, n_envs=n * envs_per_learner, tail=("pending_len",))
    out["team_pending_len"] = out.pop("pending_len")
    return out


def run_row(exe, name, dtype, nstep, runs, tmp, sanitized=False, learners=None, rearm_after=-1):
    c = tc.CASES[name]
    tables = tc.case_tables(name)
    n = c["L"] if learners is None else learners
    if tables is not None:
        tables = tuple(t[:n] for t in tables)
    return run_emu(exe, tc.case_config(name, dtype), n, c["E"], tc.SEED, runs, nstep, tmp, sanitized=sanitized, tables=tables, rearm_after=rearm_after, **c["sched"])


# ---- the yardstick against its parents ----
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_yardstick_at_n_1_equals_the_team_reference(name):
    want, _ = tc.case_reference(name, F32)
    ref = tn.make_reference(name, F32, 1)
    ref.run(tc.CASES[name]["periods"])
    got = ref.result()
    assert (got.pop("team_pending_len") == 0).all()
    tc.assert_equal(got, want, f"yardstick at n = 1, case {name}")


@pytest.mark.parametrize("quirks,dtype,nstep", [(ec.Q_PAPER, F32, 3), (ec.Q_BENCH, F64, 16)], ids=["quirks-0x40-f32-n3", "quirks-0x60-f64-n16"])
def test_the_yardstick_at_E_1_equals_the_nstep_reference_on_main_rows(quirks, dtype, nstep):
    want, _ = nc.main_reference(quirks, dtype, nstep, 26)
    ref = tn.TeamNstepReference(training_config(0, quirks=quirks, dtype=dtype), 26, 1, nc.MAIN_SEED, nstep, log_capacity=nc.MAIN_LOG)
    ref.run(nc.MAIN_PERIODS)
    got = ref.result()
    got["pending_len"] = got.pop("team_pending_len")
    ec.assert_equal(got, want, "yardstick at E = 1, main row")


def test_the_yardstick_at_E_1_equals_the_nstep_reference_from_trained_tables():
    level, quirks, dtype, nstep = nc.TRAINED_ROWS[0]
    want, tables, _ = nc.trained_reference(level, quirks, dtype, nstep, 26)
    assert want["frozen"].sum() >= 20
    ref = tn.TeamNstepReference(training_config(level, quirks=quirks, dtype=dtype), 26, 1, ec.TRAINED_LEARNERS_SEED, nstep, tables=tables, **ec.TRAINED_LEARNERS_CASE)
    ref.run(ec.TRAINED_LEARNERS_PERIODS)
    got = ref.result()
    got["pending_len"] = got.pop("team_pending_len")
    ec.assert_equal(got, want, "yardstick at E = 1, trained row")


# ---- the device code against the yardstick ----
@pytest.mark.parametrize("name,dtype,nstep", tn.ROWS, ids=tn.ROW_IDS)
def test_row_equals_the_yardstick(emu, name, dtype, nstep, tmp_path):
    want, _, _ = tn.row_reference(name, dtype, nstep)  # asserts on the yardstick what the row is for, and its pinned counts
    got = run_row(emu["plain"], name, dtype, nstep, (tc.CASES[name]["periods"],), tmp_path)
    tc.assert_equal(got, want, f"row {name} n {nstep}")


@pytest.mark.parametrize("name,nstep", [("A", 3), ("B", 16), ("C", 5), ("F", 8)])
def test_launches_of_7_and_the_rest_equal_one(emu, name, nstep, tmp_path):
    """the launch boundary: every env's window is open after 7 periods and goes through the persistent arrays"""
    want, ev, ref = tn.row_reference(name, F32, nstep)
    p = tc.CASES[name]["periods"]
    assert ev["open_after_7"] == tc.CASES[name]["L"] * tc.CASES[name]["E"] and ref.freeze_period.max() > tn.SPLIT
    got = run_row(emu["plain"], name, F32, nstep, (tn.SPLIT, p - tn.SPLIT), tmp_path)
    tc.assert_equal(got, want, f"row {name} n {nstep}, 7 + {p - 7}")


def test_launch_boundary_4096_plus_4(emu, tmp_path):
    """team_nstep_checks.BOUNDARY: two live teams with all 32 windows open at period 4 096 — and, under 0x7f, the only flushes with mask 1 of this file"""
    b = tn.BOUNDARY
    want, cfg = tn.boundary_reference()
    got = run_emu(emu["plain"], cfg, b["L"], b["E"], tc.SEED, (4096, 4), b["nstep"], tmp_path, max_episodes=1 << 30, **b["sched"])
    tc.assert_equal(got, want, "4096 + 4 periods")


def test_rearm_flies_on_with_the_frozen_teams_windows(emu, tmp_path):
    """A at n = 3: five frozen teams with 276 open windows; after a rearm the first period's updates come out of those carried windows"""
    ref = tn.make_reference("A", F32, 3)
    ref.run(200)
    assert ref.frozen.all() and int((ref.pending_lengths() > 0).sum()) == 276
    before = dict(ref.events)
    ref.rearm()
    ref.run(1)
    assert ref.events["full_window_updates"] - before["full_window_updates"] == 273 and ref.events["flush_entries"] - before["flush_entries"] == 9
    ref.run(29)
    assert ref.frozen.all() and int((ref.pending_lengths() > 0).sum()) == 308
    got = run_row(emu["plain"], "A", F32, 3, (200, 30), tmp_path, rearm_after=0)
    tc.assert_equal(got, ref.result(), "row A n 3, 200 periods, rearm, 30 periods")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_one_env_per_learner_equals_learner_periods_nstep(emu, nstep_emu, dtype, tmp_path):
    """E = 1: team_env_period + team_apply_nstep == learner_periods_nstep on a main row (nstep_emu's result, itself held to nstep_checks.NstepReference)"""
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=dtype)
    want = run_nstep_emu(nstep_emu["plain"], cfg, 26, nc.MAIN_SEED, nc.MAIN_SPLIT, 3, tmp_path)
    assert (want["qb"] != 0).any() and want["episodes"].sum() > 26 and (want["pending_len"] > 0).any()
    got = run_emu(emu["plain"], cfg, 26, 1, nc.MAIN_SEED, nc.MAIN_SPLIT, 3, tmp_path, eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30, log_capacity=nc.MAIN_LOG)
    got["pending_len"] = got.pop("team_pending_len")
    ec.assert_equal(got, want, f"E = 1 against learner_periods_nstep, dtype {dtype}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_n_1_equals_team_apply(emu, team_emu, name, tmp_path):
    """n = 1: team_apply_nstep == team_apply, bit for bit (team_emu's result, itself held to team_checks.TeamReference)"""
    p = tc.CASES[name]["periods"]
    want = run_team_case(team_emu["plain"], name, F32, (7, p - 7), tmp_path)
    got = run_row(emu["plain"], name, F32, 1, (7, p - 7), tmp_path)
    assert (got.pop("team_pending_len") == 0).all()
    tc.assert_equal(got, want, f"n = 1 against team_apply, case {name}")


def test_independence_of_the_number_of_learners(emu, tmp_path):
    """learners [0, 3) of row B-16 == an ensemble of 3 learners: the persistent arrays' stride is the env count, nothing else depends on it"""
    want, _, _ = tn.row_reference("B", F32, 16)
    got = run_row(emu["plain"], "B", F32, 16, (300,), tmp_path, learners=3)
    E = tc.CASES["B"]["E"]
    pend_got, pend_want = got.pop("team_pending_len"), dict(want).pop("team_pending_len")
    tc.assert_equal(got, {k: v for k, v in want.items() if k != "team_pending_len"}, "row B n 16, three learners", learners=([0, 1, 2], [0, 1, 2]), envs_per_learner=E)
    assert (pend_got == pend_want[:3 * E]).all()


@pytest.mark.parametrize("name,dtype,nstep", [("A", F32, 3), ("B", F64, 4), ("C", F32, 5), ("E", F32, 16)], ids=["A-f32-n3", "B-f64-n4", "C-f32-n5", "E-f32-n16"])
def test_clean_under_asan_and_ubsan(emu, name, dtype, nstep, tmp_path):
    """the stand-alone sanitized program, two launches: the records, the working windows [16][E] and the persistent arrays [16][L E] are exactly as long as stated"""
    want, _, _ = tn.row_reference(name, dtype, nstep)
    p = tc.CASES[name]["periods"]
    got = run_row(emu["san"], name, dtype, nstep, (tn.SPLIT, p - tn.SPLIT), tmp_path, sanitized=True)
    tc.assert_equal(got, want, f"sanitized row {name} n {nstep}")
