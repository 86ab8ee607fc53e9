"""The n-step learner's per-lane body (csrc/dql_nstep.hpp) run on the CPU and held `==` to the yardstick of tests/nstep_checks.py (CPU only, no GPU).

tests/host_emu/nstep_emu.cpp compiles the real device headers as host C++ and flies every learner lane by lane, exactly as k_learn_nstep does; the pending
windows are reached through checked references onto poisoned storage exactly as long as the library's.  Built twice through tests/host_emu_harness.py: plain,
and as a stand-alone ASan + UBSan program (any report fails)."""
import pytest

from dql_multirotor_landing_amd.config import F32, F64, training_config

import ensemble_checks as ec
import host_emu_harness as heh
import nstep_checks as nc

L = 26  # the trained rows need learner 25 (tests/test_learner_host_emulation.py TRAINED_L); the main rows use the same count

emu = heh.emu_fixture("nstep_emu")


def run_emu(exe, cfg, n, seed, runs, nstep, tmp, eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30, sanitized=False, log_capacity=nc.MAIN_LOG, tables=None):
    job = heh.learner_job(cfg, n, seed, runs, cfg.alpha_table(), eps, window, min_successes, max_episodes, log_capacity, tables, extra=(nstep,))
    return heh.learner_result(heh.run(exe, job, tmp, "nstep", sanitized), n, log_capacity, cfg, tail=("pending_len",))


def test_the_yardstick_at_n_1_equals_the_one_step_reference_loop():
    """the yardstick itself: its update at n = 1 against the unchanged oracle's agent_update, under the coin, float32"""
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    one = ec.Reference(cfg, 8, nc.MAIN_SEED, log_capacity=nc.MAIN_LOG)
    one.run(200)
    ref = nc.NstepReference(cfg, 8, nc.MAIN_SEED, 1, log_capacity=nc.MAIN_LOG)
    ref.run(200)
    want = one.result()
    assert want["episodes"].min() >= 1 and (want["qb"] != 0).any()
    got = ref.result()
    assert (got.pop("pending_len") == 0).all()
    ec.assert_equal(got, want, "yardstick at n = 1")


@pytest.mark.parametrize("quirks,dtype,nstep", nc.MAIN_ROWS, ids=nc.MAIN_IDS)
def test_main_rows_300_periods_and_7_plus_293_equal_the_yardstick(emu, quirks, dtype, nstep, tmp_path):
    want, ev = nc.main_reference(quirks, dtype, nstep, L)
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    got = run_emu(emu["plain"], cfg, L, nc.MAIN_SEED, (nc.MAIN_PERIODS,), nstep, tmp_path)
    ec.assert_equal(got, want, f"{nc.MAIN_PERIODS} periods")
    split = run_emu(emu["plain"], cfg, L, nc.MAIN_SEED, nc.MAIN_SPLIT, nstep, tmp_path)
    ec.assert_equal(split, want, "7 + 293 periods")


@pytest.mark.parametrize("quirks,dtype,nstep", [nc.MAIN_ROWS[1], nc.MAIN_ROWS[3]], ids=[nc.MAIN_IDS[1], nc.MAIN_IDS[3]])
def test_split_150_plus_250_equals_one_run_of_the_yardstick(emu, quirks, dtype, nstep, tmp_path):
    """windows open at a launch's end in the middle of learning: 150 + 250 periods against 400 of the yardstick"""
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    ref = nc.NstepReference(cfg, L, nc.MAIN_SEED, nstep, watch=(150,), log_capacity=nc.MAIN_LOG)
    ref.run(400)
    assert (ref.len_after[150] > 0).sum() >= L // 2 and ref.events["flush_entries"] >= 1 and ref.events["full_window_updates"] >= 1
    got = run_emu(emu["plain"], cfg, L, nc.MAIN_SEED, (150, 250), nstep, tmp_path)
    ec.assert_equal(got, ref.result(), "150 + 250 periods")


@pytest.mark.parametrize("level,quirks,dtype,nstep", nc.TRAINED_ROWS, ids=nc.TRAINED_IDS)
def test_trained_tables_400_periods_and_7_plus_393_equal_the_yardstick(emu, level, quirks, dtype, nstep, tmp_path):
    want, tables, ev = nc.trained_reference(level, quirks, dtype, nstep, L)
    cfg = training_config(level, quirks=quirks, dtype=dtype)
    kw = dict(ec.TRAINED_LEARNERS_CASE, tables=tables)
    got = run_emu(emu["plain"], cfg, L, ec.TRAINED_LEARNERS_SEED, (ec.TRAINED_LEARNERS_PERIODS,), nstep, tmp_path, **kw)
    ec.assert_equal(got, want, "400 periods")
    split = run_emu(emu["plain"], cfg, L, ec.TRAINED_LEARNERS_SEED, ec.TRAINED_LEARNERS_SPLIT, nstep, tmp_path, **kw)
    ec.assert_equal(split, want, "7 + 393 periods")


@pytest.mark.parametrize("quirks,dtype,nstep", [nc.MAIN_ROWS[1], nc.MAIN_ROWS[2]], ids=[nc.MAIN_IDS[1], nc.MAIN_IDS[2]])
def test_main_rows_clean_under_asan_and_ubsan(emu, quirks, dtype, nstep, tmp_path):
    want, ev = nc.main_reference(quirks, dtype, nstep, L)
    got = run_emu(emu["san"], training_config(0, quirks=quirks, dtype=dtype), L, nc.MAIN_SEED, nc.MAIN_SPLIT, nstep, tmp_path, sanitized=True)
    ec.assert_equal(got, want, "sanitized, 7 + 293 periods")


def test_trained_tables_clean_under_asan_and_ubsan(emu, tmp_path):
    level, quirks, dtype, nstep = nc.TRAINED_ROWS[0]
    want, tables, ev = nc.trained_reference(level, quirks, dtype, nstep, L)
    got = run_emu(emu["san"], training_config(level, quirks=quirks, dtype=dtype), L, ec.TRAINED_LEARNERS_SEED, ec.TRAINED_LEARNERS_SPLIT, nstep, tmp_path, sanitized=True,
                  **dict(ec.TRAINED_LEARNERS_CASE, tables=tables))
    ec.assert_equal(got, want, "sanitized, trained tables")
