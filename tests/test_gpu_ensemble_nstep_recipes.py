"""Per-recipe n-step targets on the device: `Recipe.nstep`, dql_ensemble_set_recipe_nstep, k_learn_recipes_nstep over the worklist by
(recipe, level).

The yardsticks are tests/nstep_recipe_checks.py's (one per recipe over all learners, the unchanged oracle per level, the n-step update in Python floats); the
ensemble's learner l is held to the yardstick of its recipe, every comparison is `==`, floats by their bits, `pending_lengths` included.  The case's conditions
and its n-step events, pinned to the digit, are asserted on the yardsticks before an ensemble is looked at (`nstep_recipe_checks.case_reference`)."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, training_config
from dql_multirotor_landing_amd.ensemble import Recipe

import advance_checks as ac
import ensemble_checks as ec
import nstep_recipe_checks as nr
import recipe_checks as rc

pytestmark = pytest.mark.gpu
CASE = rc.CASE
N, SMALL = rc.N_BIG, rc.N_SMALL
PERIODS = CASE["periods"]


def flown(ens, *runs):
    try:
        for r in runs:
            ens.run(r)
        assert ens.index_faults() == 0
        return nr.ensemble_result(ens)
    finally:
        ens.close()


@pytest.fixture(scope="module")
def main():
    """the 112-learner ensemble with n = (3, 16, 5) after run(1024), shared"""
    ens = nr.case_ensemble(N, nr.NSTEPS_F32)
    assert [r.nstep for r in ens.recipes()[0]] == list(nr.NSTEPS_F32) and ens.nstep == 0
    return flown(ens, PERIODS)


def test_112_learners_equal_the_yardsticks_by_recipe_f32(main):
    """recipe 0's level-0 segment is two waves, the second padded (asserted on the yardsticks)"""
    yards = nr.case_reference(N, nr.NSTEPS_F32)
    nr.assert_equal_by_recipe(main, yards, "run(1024), n = (3, 16, 5), float32")
    assert (main["pending_len"] > 0).sum() == 61 + 13


def test_28_learners_equal_the_yardsticks_by_recipe_f64():
    yards = nr.case_reference(SMALL, nr.NSTEPS_F64, F64)
    nr.assert_equal_by_recipe(flown(nr.case_ensemble(SMALL, nr.NSTEPS_F64, F64), PERIODS), yards, "run(1024), n = (16, 4, 2), float64")


def test_four_runs_of_256_equal_one_run(main):
    ac.assert_equal(flown(nr.case_ensemble(N, nr.NSTEPS_F32), 256, 256, 256, 256), main, "4 x 256 against run(1024)")


def test_7_plus_1017_equal_one_run(main):
    """a cut that is no advance point, with windows open"""
    ens = nr.case_ensemble(N, nr.NSTEPS_F32)
    ens.run(7)
    assert (ens.pending_lengths() > 0).any()
    ac.assert_equal(flown(ens, PERIODS - 7), main, "7 + 1017 against run(1024)")


def test_first_28_learners_do_not_depend_on_the_other_84(main):
    first = list(range(SMALL))
    got = flown(nr.case_ensemble(SMALL, nr.NSTEPS_F32), PERIODS)
    ac.assert_equal(main, got, "L = 112 against L = 28", learners=(first, first))
    nr.assert_equal_by_recipe(got, nr.case_reference(SMALL, nr.NSTEPS_F32), "L = 28, n = (3, 16, 5), float32")


def test_relabelled_recipes_change_nothing_per_learner(main):
    """recipes 0 and 2 swapped, recipe_of mapped: other segments in another order, another wave reads another n, the same learners"""
    recipes = nr.case_recipes(nr.NSTEPS_F32)[::-1]
    got = flown(nr.case_ensemble(N, None, recipes=recipes, recipe_of=2 - rc.case_recipe_of(N)), PERIODS)
    ac.assert_equal(got, main, "recipes 0 and 2 swapped")


def test_a_recipe_with_n_0_beside_the_others_equals_the_parent_path():
    """n = (3, 0, 16): every learner `==` its yardstick, and recipe 1's learners `==` the same learners of an all-n = 0 ensemble (k_learn_recipes)"""
    yards = nr.case_reference(SMALL, nr.NSTEPS_WITH_ZERO)
    got = flown(nr.case_ensemble(SMALL, nr.NSTEPS_WITH_ZERO), PERIODS)
    nr.assert_equal_by_recipe(got, yards, "run(1024), n = (3, 0, 16), float32")
    parent = flown(rc.case_ensemble(SMALL), PERIODS)
    rows = [int(l) for l in np.nonzero(rc.case_recipe_of(SMALL) == 1)[0]]
    assert (parent["pending_len"] == 0).all() and parent["decisions"][rows].min() >= 1
    ac.assert_equal(got, parent, "recipe 1 (n = 0) beside n-step recipes against an ensemble without n-step recipes", learners=(rows, rows))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_n_1_on_the_new_kernel_equals_n_0_on_k_learn_recipes(dtype):
    n = N if dtype == F32 else SMALL
    want = flown(rc.case_ensemble(n, dtype), PERIODS)
    got = flown(nr.case_ensemble(n, (1, 1, 1), dtype), PERIODS)
    assert (got["pending_len"] == 0).all() and (want["level"] > 0).any() and (want["qb"] != ec.trained_tables(n)[1]).any()
    ac.assert_equal(got, want, f"n = (1, 1, 1) against n = (0, 0, 0), dtype {dtype}")


def test_refused_calls_say_why_change_nothing_and_a_good_run_follows():
    lib = _lib.load()
    n_out = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc_, code, *words):
        msg = lib.dql_last_error().decode()
        assert rc_ == code and all(w in msg for w in words) and "nothing was changed" in msg, (rc_, msg)

    # no recipes installed
    plain = ac.case_ensemble(**dict(ac.TRAINED_CASE, n=SMALL))
    try:
        refused(lib.dql_ensemble_set_recipe_nstep(plain._h, 0, 2), _lib.EINVAL, "dql_ensemble_set_recipe_nstep", "no recipes are installed")
        refused(lib.dql_ensemble_get_recipe_nstep(plain._h, 0, C.byref(n_out)), _lib.EINVAL, "dql_ensemble_get_recipe_nstep", "no recipes are installed")
        assert n_out.value == -7 and (plain.pending_lengths() == 0).all()
    finally:
        plain.close()
    yards = nr.case_reference(SMALL, nr.NSTEPS_F32)
    ens = nr.case_ensemble(SMALL, (0, 0, 0))
    try:
        before = nr.ensemble_result(ens)
        for r in (-1, 3):
            refused(lib.dql_ensemble_set_recipe_nstep(ens._h, r, 2), _lib.EINVAL, "the recipe must be in 0..n_recipes - 1")
            refused(lib.dql_ensemble_get_recipe_nstep(ens._h, r, C.byref(n_out)), _lib.EINVAL, "the recipe must be in 0..n_recipes - 1")
        for bad in (-1, 17):
            refused(lib.dql_ensemble_set_recipe_nstep(ens._h, 1, bad), _lib.EINVAL, "0..16")
        assert lib.dql_ensemble_get_recipe_nstep(ens._h, 0, None) == _lib.EINVAL
        # the ensemble-wide switch keeps its refusal, and `set_nstep` refuses before the library is touched
        refused(lib.dql_ensemble_set_nstep(ens._h, 2), _lib.EINVAL, "recipes installed")
        with pytest.raises(ValueError, match="plain mode"):
            ens.set_nstep(2)
        assert [r.nstep for r in ens.recipes()[0]] == [0, 0, 0] and ens.nstep == 0 and ens.period_index() == 0
        ec.assert_equal(nr.ensemble_result(ens), before, "after the refused calls")
        for r, n in enumerate(nr.NSTEPS_F32):
            assert lib.dql_ensemble_set_recipe_nstep(ens._h, r, n) == _lib.OK
            assert lib.dql_ensemble_get_recipe_nstep(ens._h, r, C.byref(n_out)) == _lib.OK and n_out.value == n
        # windows open: the n of a recipe whose member holds entries cannot change, recipes can be neither installed nor uninstalled; the state stays
        ens.run(7)
        lens, of = ens.pending_lengths(), rc.case_recipe_of(SMALL)
        assert all((lens[of == r] > 0).any() for r in range(3))
        mid = nr.ensemble_result(ens)
        for r in range(3):
            for other in (0, 1, 16 if nr.NSTEPS_F32[r] != 16 else 15):
                refused(lib.dql_ensemble_set_recipe_nstep(ens._h, r, other), _lib.ESTATE, "pending window")
            assert lib.dql_ensemble_set_recipe_nstep(ens._h, r, nr.NSTEPS_F32[r]) == _lib.OK  # no change: accepted
        refused(lib.dql_ensemble_set_recipes(ens._h, 0, None), _lib.ESTATE, "dql_ensemble_set_recipes", "pending window")
        refused(lib.dql_ensemble_set_recipes(ens._h, 3, p(of)), _lib.ESTATE, "dql_ensemble_set_recipes", "pending window")
        assert [r.nstep for r in ens.recipes()[0]] == list(nr.NSTEPS_F32) and np.array_equal(ens.recipes()[1], of)
        ec.assert_equal(nr.ensemble_result(ens), mid, "after the refused changes")
        # the good run that follows
        ens.run(PERIODS - 7)
        assert ens.index_faults() == 0
        nr.assert_equal_by_recipe(nr.ensemble_result(ens), yards, "7 + 1017 periods after the refusals")
    finally:
        ens.close()


def test_set_level_empties_the_windows_and_recipes_can_be_reinstalled_after_it():
    ens = nr.case_ensemble(SMALL, nr.NSTEPS_F32)
    try:
        ens.run(7)
        before = ens.pending_lengths()
        assert (before > 0).any()
        ens.transfer(1, 0.5); ens.rearm(); ens.set_tables(*ens.get_tables())
        assert np.array_equal(ens.pending_lengths(), before), "transfer, rearm and set_tables leave the windows alone"
        ens.set_level(0)
        assert (ens.pending_lengths() == 0).all()
        ens.set_recipes(nr.case_recipes((2, 2, 2)), rc.case_recipe_of(SMALL))  # windows empty: accepted; fresh recipes, then each n
        assert [r.nstep for r in ens.recipes()[0]] == [2, 2, 2]
        ens.run(40)
        assert (ens.pending_lengths() > 0).any() and ens.pending_lengths().max() <= 1 and ens.index_faults() == 0
    finally:
        ens.close()


def test_score_and_returns_map_read_the_resident_tables():
    ens = nr.case_ensemble(SMALL, nr.NSTEPS_F32)
    try:
        ens.run(200)
        qa, qb, _ = ens.get_tables()
        before = nr.ensemble_result(ens)
        assert (before["pending_len"] > 0).any()
        ev = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
        got, want = ens.score(ev, 64, seed=5, max_steps=120, log=True), ops.score(ev, qa, qb, 64, 5, max_steps=120, log=True)
        for k in ("by_code", "steps_sum", "ep_code", "ep_steps"):
            assert np.array_equal(got[k], want[k]), k
        assert want["by_code"].sum() > 0
        got, want = ens.returns_map(ev, 64, seed=5, eps=0.1, gamma=0.99, max_steps=120, count=16), ops.returns_map(ev, qa[:16], qb[:16], 64, 5, 0.1, 0.99, max_steps=120)
        for k in ("visits", "return_fx", "cut_decisions", "by_code", "steps_sum"):
            assert np.array_equal(got[k], want[k]), k
        assert want["visits"].sum() > 0
        ac.assert_equal(nr.ensemble_result(ens), before, "the ensemble after the operators")
    finally:
        ens.close()
