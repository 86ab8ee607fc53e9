"""Per-recipe n-step targets on the CPU: the yardstick's two anchors, and csrc/dql_recipes.hpp's worklist and advance step with
csrc/dql_nstep.hpp's learner_periods_nstep and csrc/dql_learner.hpp's learner_periods, held `==` to the yardsticks of tests/nstep_recipe_checks.py (no GPU).

tests/host_emu/nstep_recipes_emu.cpp compiles the real headers as host C++ and does what dql_ensemble_run does when a recipe has n >= 1: wave by wave, lane by
lane, the wave's n from its recipe, the working windows poisoned before every wave, the persistent ones exactly as long as the library's, both behind checked
references.  It is a stand-alone program run as its own process, built twice through tests/host_emu_harness.py: plain, and with ASan + UBSan (any report
fails).  The case is `recipe_checks.CASE` with 28 learners (20 / 4 / 4 members)."""
import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64

import advance_checks as ac
import ensemble_checks as ec
import host_emu_harness as heh
import nstep_checks as nc
import nstep_recipe_checks as nr
import recipe_checks as rc

CASE = rc.CASE
N = rc.N_SMALL

emu = heh.emu_fixture("nstep_recipes_emu")


def run_emu(exe, tmp, runs, nsteps, n=N, dtype=F32, sanitized=False, recipes=None, recipe_of=None, cfg=None):
    """cfg: the config of the starting level (default: the case's)"""
    cfg = rc.case_config(dtype) if cfg is None else cfg
    recipes = nr.case_recipes(nsteps, dtype) if recipes is None else recipes
    of = rc.case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of, np.int32)
    job = heh.recipes_job(cfg, n, CASE["seed"], runs, CASE["E"], CASE["log_capacity"], recipes, of, ec.trained_tables(n))
    return heh.learner_result(heh.run(exe, job, tmp, "nstep_recipes", sanitized), n, CASE["log_capacity"], cfg, tail=("levels", "pending_len"), periods=sum(runs))


# ---- the yardstick's anchors ----
def test_anchor_every_recipe_at_n_1_equals_the_recipe_yardstick():
    """n = 1 for every recipe: `NstepRecipeYardstick` against `RecipeYardstick` on `recipe_checks.CASE`, 28 learners, float32, all three recipes, every output"""
    got = nr.case_yardsticks(N, (1, 1, 1))
    want = rc.case_yardsticks(N)
    rc.assert_case_conditions(want)
    for r, (g, w) in enumerate(zip(got, want)):
        res = g.result()
        assert (res.pop("pending_len") == 0).all() and g.events["full_window_updates"] >= 1
        ac.assert_equal(res, w.result(), f"the yardstick at n = 1, recipe {r}")
        assert g.alpha.taken == w.alpha.taken and g.promoted_from.tolist() == w.promoted_from.tolist() and g.exhausted_from.tolist() == w.exhausted_from.tolist()


def test_anchor_one_recipe_that_stays_on_its_level_equals_the_nstep_reference():
    """one recipe, last_level = the starting level, the same schedules: `NstepRecipeYardstick` against `nstep_checks.NstepReference` (a main row's shape, level 0)"""
    from dql_multirotor_landing_amd.config import training_config
    from dql_multirotor_landing_amd.ensemble import LevelSchedule, Recipe
    n, nstep, periods = 8, 3, 200
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ref = nc.NstepReference(cfg, n, nc.MAIN_SEED, nstep, log_capacity=nc.MAIN_LOG)
    ref.run(periods)
    want = ref.result()
    assert ref.events["full_window_updates"] >= 1 and ref.events["flush_entries"] >= 1 and (want["pending_len"] > 0).any() and (want["qb"] != 0).any()
    lv = tuple(LevelSchedule(eps=tuple(ec.EPS_TABLE), window=100, min_successes=97, max_episodes=1 << 30) for _ in range(5))
    recipe = Recipe(quirks=ec.Q_PAPER, last_level=0, levels=lv, nstep=nstep)
    y = nr.NstepRecipeYardstick(cfg, n, nc.MAIN_SEED, recipe, np.ones(n, bool), 32, nstep, nc.MAIN_LOG)
    y.run(periods)
    got = y.result()
    ec.assert_equal(got, want, "one recipe on its starting level against NstepReference")
    assert (got["level"] == 0).all() and dict(y.events) == {k: v for k, v in ref.events.items() if k in y.events}


# ---- the emulation ----
@pytest.fixture(scope="module")
def main(emu, tmp_path_factory):
    return run_emu(emu["plain"], tmp_path_factory.mktemp("nstep_recipes_main"), (CASE["periods"],), nr.NSTEPS_F32)


def test_whole_run_equals_the_yardsticks_f32(main):
    nr.assert_equal_by_recipe(main, nr.case_reference(N, nr.NSTEPS_F32), "run(1024), n = (3, 16, 5), float32")


def test_7_plus_1017_equals_one_run(emu, main, tmp_path):
    """a cut that is no advance point, seven periods in: the windows open there persist outside the launch"""
    got = run_emu(emu["plain"], tmp_path, (7, CASE["periods"] - 7), nr.NSTEPS_F32)
    ac.assert_equal(got, main, "7 + 1017 against run(1024)")
    nr.assert_equal_by_recipe(got, nr.case_reference(N, nr.NSTEPS_F32), "7 + 1017, n = (3, 16, 5), float32")


def test_whole_run_equals_the_yardsticks_f64(emu, tmp_path):
    got = run_emu(emu["plain"], tmp_path, (CASE["periods"],), nr.NSTEPS_F64, dtype=F64)
    nr.assert_equal_by_recipe(got, nr.case_reference(N, nr.NSTEPS_F64, F64), "run(1024), n = (16, 4, 2), float64")


def test_a_recipe_with_n_0_beside_the_others(emu, tmp_path):
    """n = (3, 0, 16): recipe 1's learners fly learner_periods beside n-step waves and equal the one-step `RecipeYardstick`"""
    yards = nr.case_reference(N, nr.NSTEPS_WITH_ZERO)
    assert type(yards[1]) is rc.RecipeYardstick
    got = run_emu(emu["plain"], tmp_path, (CASE["periods"],), nr.NSTEPS_WITH_ZERO)
    nr.assert_equal_by_recipe(got, yards, "run(1024), n = (3, 0, 16), float32")
    assert (got["pending_len"][rc.case_recipe_of(N) == 1] == 0).all()


@pytest.mark.parametrize("nsteps,dtype", [(nr.NSTEPS_F32, F32), (nr.NSTEPS_F64, F64), (nr.NSTEPS_WITH_ZERO, F32)], ids=["n3-16-5-f32", "n16-4-2-f64", "n3-0-16-f32"])
def test_clean_under_asan_and_ubsan(emu, nsteps, dtype, tmp_path):
    """the case through the stand-alone sanitized program, in two runs"""
    got = run_emu(emu["san"], tmp_path, (7, CASE["periods"] - 7), nsteps, dtype=dtype, sanitized=True)
    nr.assert_equal_by_recipe(got, nr.case_reference(N, nsteps, dtype), f"sanitized, n = {nsteps}, dtype {dtype}")
