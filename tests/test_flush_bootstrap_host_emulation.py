"""Flushes that bootstrap, through the real device text on the CPU (no GPU): the rows of tests/flush_bootstrap_checks.py flown by the three existing emulation
programs, unchanged — tests/host_emu/nstep_emu.cpp (learner_periods_nstep), team_nstep_emu.cpp (team_apply_nstep) and nstep_recipes_emu.cpp (the worklist by
recipe and level) — and held `==` to the yardsticks, whole and split after 7 periods.  The config's `t_max` and observation noise reach the programs in the
config's own bytes.  One plain and one team row also fly through the stand-alone ASan + UBSan builds.  """
import pytest

import ensemble_checks as ec
import flush_bootstrap_checks as fb
import host_emu_harness as heh
import nstep_recipe_checks as nr
import team_checks as tc
from test_nstep_host_emulation import run_emu as run_plain_emu
from test_nstep_recipes_host_emulation import run_emu as run_recipes_emu
from test_team_nstep_host_emulation import run_emu as run_team_emu

L = 26

plain_emu = heh.emu_fixture("nstep_emu")
team_emu = heh.emu_fixture("team_nstep_emu")
recipes_emu = heh.emu_fixture("nstep_recipes_emu")


def fly_plain(exe, row, runs, tmp, sanitized=False):
    level, quirks, dtype, nstep = row
    return run_plain_emu(exe, fb.bootstrap_config(level, quirks, dtype), L, fb.PLAIN_SEED, runs, nstep, tmp, sanitized=sanitized, log_capacity=fb.PLAIN_LOG,
                         tables=fb.plain_tables(level, L))


def fly_team(exe, row, runs, tmp, sanitized=False):
    level, quirks, L_, E, nstep, dtype = row
    return run_team_emu(exe, fb.bootstrap_config(level, quirks, dtype), L_, E, fb.TEAM_SEED, runs, nstep, tmp, sanitized=sanitized, tables=fb.plain_tables(level, L_), **fb.TEAM_SCHED)


@pytest.mark.parametrize("row", fb.PLAIN_ROWS, ids=fb.PLAIN_IDS)
def test_plain_rows_300_periods_and_7_plus_293_equal_the_yardstick(plain_emu, row, tmp_path):
    want, _ = fb.plain_reference(*row, L)  # asserts on the yardstick what the row is for, and its pinned counts
    ec.assert_equal(fly_plain(plain_emu["plain"], row, (fb.PLAIN_PERIODS,), tmp_path), want, "300 periods")
    ec.assert_equal(fly_plain(plain_emu["plain"], row, fb.PLAIN_SPLIT, tmp_path), want, "7 + 293 periods")


@pytest.mark.parametrize("row", fb.TEAM_ROWS, ids=fb.TEAM_IDS)
def test_team_rows_150_periods_and_7_plus_143_equal_the_yardstick(team_emu, row, tmp_path):
    want, _ = fb.team_reference(*row)
    tc.assert_equal(fly_team(team_emu["plain"], row, (fb.TEAM_PERIODS,), tmp_path), want, "150 periods")
    tc.assert_equal(fly_team(team_emu["plain"], row, fb.TEAM_SPLIT, tmp_path), want, "7 + 143 periods")


def test_the_recipe_case_600_periods_and_7_plus_593_equal_the_yardsticks(recipes_emu, tmp_path):
    yards = fb.recipe_reference()
    kw = dict(n=fb.RECIPE_N, recipes=fb.recipe_recipes(), recipe_of=fb.recipe_of(), cfg=fb.recipe_config())
    for runs in ((fb.RECIPE_CASE["periods"],), fb.RECIPE_SPLIT):
        got = run_recipes_emu(recipes_emu["plain"], tmp_path, runs, None, **kw)
        nr.assert_equal_by_recipe(got, yards, f"runs {runs}", recipe_of=fb.recipe_of())


def test_a_plain_row_clean_under_asan_and_ubsan(plain_emu, tmp_path):
    row = fb.PLAIN_ROWS[1]  # level 4, trained, 0x50, n = 4
    want, _ = fb.plain_reference(*row, L)
    ec.assert_equal(fly_plain(plain_emu["san"], row, fb.PLAIN_SPLIT, tmp_path, sanitized=True), want, "sanitized, 7 + 293 periods")


def test_a_team_row_clean_under_asan_and_ubsan(team_emu, tmp_path):
    row = fb.TEAM_ROWS[0]  # level 4, trained, 0x50, 3 x 16, n = 16
    want, _ = fb.team_reference(*row)
    tc.assert_equal(fly_team(team_emu["san"], row, fb.TEAM_SPLIT, tmp_path, sanitized=True), want, "sanitized, 7 + 143 periods")
