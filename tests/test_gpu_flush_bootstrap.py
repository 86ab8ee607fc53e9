"""Flushes that bootstrap, on the device: the rows of tests/flush_bootstrap_checks.py flown by k_learn_nstep, k_learn_team_nstep and
k_learn_recipes_nstep and held `==` to the unchanged yardsticks — every table, counter, log entry, state field (floats by their bits) and window length —
whole and split after 7 periods, with no index fault.  Every row first asserts ON THE YARDSTICK that its flushes with mask 1 occurred, with windows of two
entries and more, both coins and distinct bootstraps, pinned to the digit.  The one-step kernels fly the same config beside them: k_learn and k_learn_team
against the reference loops, the n-step kernels at n = 1 against those."""
import pytest

from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import advance_checks as ac
import ensemble_checks as ec
import flush_bootstrap_checks as fb
import nstep_checks as nc
import nstep_recipe_checks as nr
import team_checks as tc
import team_nstep_checks as tn

pytestmark = pytest.mark.gpu
L = 70  # a second wave of 6 lanes


def fly_plain(level, quirks, dtype, nstep, runs):
    ens = SequentialEnsemble(fb.bootstrap_config(level, quirks, dtype), L, seed=fb.PLAIN_SEED, log_capacity=fb.PLAIN_LOG, eps=ec.EPS_TABLE, max_episodes=1 << 30, nstep=nstep)
    try:
        if level >= 1:
            ens.set_tables(*ec.trained_tables(L))
        for r in runs:
            ens.run(r)
        return nc.ensemble_result(ens), ens.index_faults(), ens.period_index()
    finally:
        ens.close()


def fly_team(level, quirks, L_, E, nstep, dtype, runs):
    ens = fb.team_ensemble(level, quirks, L_, E, nstep, dtype)
    try:
        for r in runs:
            ens.run(r)
        return tn.ensemble_result(ens), ens.index_faults(), ens.period_index()
    finally:
        ens.close()


def fly_recipes(runs):
    ens = fb.recipe_ensemble()
    try:
        assert [r.nstep for r in ens.recipes()[0]] == [n for _, n in fb.RECIPE_SPECS]
        for r in runs:
            ens.run(r)
        return nr.ensemble_result(ens), ens.index_faults(), ens.period_index()
    finally:
        ens.close()


@pytest.fixture(scope="module")
def whole():
    """the device's result of a row flown in one run, per (flight, its arguments): computed once, shared"""
    cache = {}

    def get(fly, *args):
        if (fly, args) not in cache:
            cache[(fly, args)] = fly(*args)
        return cache[(fly, args)]
    return get


@pytest.mark.parametrize("level,quirks,dtype,nstep", fb.PLAIN_ROWS, ids=fb.PLAIN_IDS)
def test_plain_rows_70_learners_300_periods_and_7_plus_293(whole, level, quirks, dtype, nstep):
    want, _ = fb.plain_reference(level, quirks, dtype, nstep, L)  # asserts on the yardstick what the row is for, and its pinned counts
    got, faults, j = whole(fly_plain, level, quirks, dtype, nstep, (fb.PLAIN_PERIODS,))
    ec.assert_equal(got, want, "300 periods")
    assert faults == 0 and j == fb.PLAIN_PERIODS
    split, faults, j = fly_plain(level, quirks, dtype, nstep, fb.PLAIN_SPLIT)
    ec.assert_equal(split, want, "7 + 293 periods")
    assert faults == 0 and j == fb.PLAIN_PERIODS


@pytest.mark.parametrize("level,quirks,L_,E,nstep,dtype", fb.TEAM_ROWS, ids=fb.TEAM_IDS)
def test_team_rows_150_periods_and_7_plus_143(whole, level, quirks, L_, E, nstep, dtype):
    want, _ = fb.team_reference(level, quirks, L_, E, nstep, dtype)
    got, faults, j = whole(fly_team, level, quirks, L_, E, nstep, dtype, (fb.TEAM_PERIODS,))
    tc.assert_equal(got, want, "150 periods")
    assert faults == 0 and j == fb.TEAM_PERIODS
    split, faults, j = fly_team(level, quirks, L_, E, nstep, dtype, fb.TEAM_SPLIT)
    tc.assert_equal(split, want, "7 + 143 periods")
    assert faults == 0 and j == fb.TEAM_PERIODS


def test_the_recipe_case_600_periods_and_7_plus_593(whole):
    yards = fb.recipe_reference()  # asserts on the yardsticks what the case is for, per recipe, and the pinned counts
    periods = fb.RECIPE_CASE["periods"]
    got, faults, j = whole(fly_recipes, (periods,))
    nr.assert_equal_by_recipe(got, yards, "600 periods", recipe_of=fb.recipe_of())
    assert faults == 0 and j == periods
    split, faults, j = fly_recipes(fb.RECIPE_SPLIT)
    ac.assert_equal(split, got, "7 + 593 against one run, device against device")
    nr.assert_equal_by_recipe(split, yards, "7 + 593 periods", recipe_of=fb.recipe_of())
    assert faults == 0 and j == periods


@pytest.mark.parametrize("quirks,dtype", fb.ANCHOR_ROWS, ids=fb.ANCHOR_IDS)
def test_one_step_plain_k_learn_equals_the_reference_loop_and_n_1_equals_k_learn(whole, quirks, dtype):
    """r + gamma * (best * mask) == r + (gamma * best) * mask at terminal transitions with mask 1 and a bootstrap that is not zero"""
    want, mask_1 = fb.plain_anchor(quirks, dtype, L)  # asserts: the yardstick at n = 1 == the reference loop, >= 20 terminal transitions with mask 1
    assert mask_1 >= 20
    zero, faults0, _ = whole(fly_plain, fb.ANCHOR_LEVEL, quirks, dtype, 0, (fb.PLAIN_PERIODS,))
    assert (zero["pending_len"] == 0).all() and faults0 == 0
    ec.assert_equal(zero, want, "k_learn against the reference loop")
    one, faults1, _ = fly_plain(fb.ANCHOR_LEVEL, quirks, dtype, 1, (fb.PLAIN_PERIODS,))
    ec.assert_equal(one, zero, "k_learn_nstep at n = 1 against k_learn")
    assert faults1 == 0


@pytest.mark.parametrize("quirks,dtype", fb.ANCHOR_ROWS, ids=fb.ANCHOR_IDS)
def test_one_step_teams_k_learn_team_equals_the_team_reference_and_n_1_equals_k_learn_team(quirks, dtype):
    want, mask_1 = fb.team_anchor(quirks, dtype)
    assert mask_1 >= 20
    a = fb.ANCHOR_TEAM
    zero, faults0, _ = fly_team(fb.ANCHOR_LEVEL, quirks, a["L"], a["E"], 0, dtype, (fb.TEAM_PERIODS,))
    assert (zero["team_pending_len"] == 0).all() and faults0 == 0
    tc.assert_equal(zero, want, "k_learn_team against the team reference loop")
    one, faults1, _ = fly_team(fb.ANCHOR_LEVEL, quirks, a["L"], a["E"], 1, dtype, (fb.TEAM_PERIODS,))
    tc.assert_equal(one, zero, "k_learn_team_nstep at n = 1 against k_learn_team")
    assert faults1 == 0
