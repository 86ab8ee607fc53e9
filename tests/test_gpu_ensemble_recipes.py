"""Per-learner recipes on the device: `SequentialEnsemble.set_recipes`, k_learn_recipes over the worklist by (recipe, level),
k_ens_advance_recipes.

The yardsticks are tests/recipe_checks.py's (the unchanged oracle, one yardstick per recipe over all learners; the ensemble's learner l is held to the yardstick
of its recipe); every comparison is `==`, floats by their bits.  The case's conditions — per recipe promoted advances from two levels, exhausted advances
under recipe 0, the coin and learning rates from beyond the table under recipe 1, nobody above level 2 and a learner out of episodes for good under recipe 2,
a segment of two waves, padded segments — are asserted on the yardsticks before an ensemble is looked at."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, F64
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import advance_checks as ac
import ensemble_checks as ec
import recipe_checks as rc

pytestmark = pytest.mark.gpu
CASE = rc.CASE
N, SMALL, EVERY = rc.N_BIG, rc.N_SMALL, 256
PERIODS = CASE["periods"]


def flown(ens, *runs):
    try:
        for r in runs:
            ens.run(r)
        assert ens.index_faults() == 0
        return ac.ensemble_result(ens), ens.period_index(), ens.n_unfinished()
    finally:
        ens.close()


@pytest.fixture(scope="module")
def yards():
    """the three yardsticks over the 112 learners (about 19 s together on the CPU), checkpoints after every 256 periods, their conditions asserted"""
    ys = rc.case_yardsticks(N, checkpoint_every=EVERY)
    rc.assert_case_conditions(ys)
    return ys


@pytest.fixture(scope="module")
def main():
    """the recipe ensemble's result after run(1024), shared"""
    got, j, unfinished = flown(rc.case_ensemble(N), PERIODS)
    assert j == PERIODS
    return got, unfinished


def test_whole_run_equals_the_yardsticks_f32(yards, main):
    got, unfinished = main
    rc.assert_equal_by_recipe(got, yards, "run(1024), float32")
    assert unfinished == sum(y.n_unfinished() for y in yards) and 0 < unfinished < N


def test_whole_run_equals_the_yardsticks_f64():
    ys = rc.case_yardsticks(SMALL, F64)
    rc.assert_case_conditions(ys)
    got, j, unfinished = flown(rc.case_ensemble(SMALL, F64), PERIODS)
    rc.assert_equal_by_recipe(got, ys, "run(1024), float64")
    assert j == PERIODS and unfinished == sum(y.n_unfinished() for y in ys)


def test_recipe_0_learners_equal_curriculum_mode_without_recipes(main):
    """the parent's path: a plain curriculum-mode ensemble of 112 learners with recipe 0's config, schedules and rule (`advance_checks.TRAINED_CASE`)"""
    want, _, _ = flown(ac.case_ensemble(**dict(ac.TRAINED_CASE, n=N)), PERIODS)
    rows = [int(l) for l in np.nonzero(rc.case_recipe_of(N) == 0)[0]]
    assert len(rows) == 80
    ac.assert_equal(main[0], want, "recipe 0's learners against k_learn_levels", learners=(rows, rows))


def test_a_single_reference_order_recipe_equals_curriculum_mode_without_recipes():
    c = ac.TRAINED_CASE
    want, _, unfinished = flown(ac.case_ensemble(**c), c["periods"])
    got, j, u = flown(rc.case_ensemble(c["n"], recipes=rc.case_recipes()[:1], recipe_of=np.zeros(c["n"], np.int32)), c["periods"])
    assert j == c["periods"] and u == unfinished and (want["level"] > 0).any()
    ac.assert_equal(got, want, "one order-0 recipe for everybody against curriculum mode without recipes")


@pytest.mark.parametrize("runs", [(7, 1017), (33, 31, 960)], ids=lambda r: "+".join(map(str, r)))
def test_splits_equal_one_run(main, runs):
    """advance points depend on the period index only: cuts off the multiples of E = 32, one period after one, and on one"""
    assert sum(runs) == PERIODS and any(r % CASE["E"] for r in runs)
    got, j, _ = flown(rc.case_ensemble(N), *runs)
    assert j == PERIODS
    ac.assert_equal(got, main[0], f"runs {runs} against run(1024)")


def test_first_28_learners_do_not_depend_on_the_other_84(yards, main):
    """another worklist (one wave per segment, other lanes, other padding), the same learners"""
    first = list(range(SMALL))
    got, _, _ = flown(rc.case_ensemble(SMALL), PERIODS)
    ac.assert_equal(main[0], got, "L = 112 against L = 28", learners=(first, first))


def test_relabelled_recipes_change_nothing_per_learner(main):
    """recipes 0 and 2 swapped, recipe_of mapped: other segments in another order, the same learners"""
    got, _, _ = flown(rc.case_ensemble(N, recipes=rc.case_recipes()[::-1], recipe_of=2 - rc.case_recipe_of(N)), PERIODS)
    ac.assert_equal(got, main[0], "recipes 0 and 2 swapped")


def test_levels_unfinished_and_summary_after_every_256_periods(yards, main):
    of = rc.case_recipe_of(N)
    assert len(yards[0].checkpoints) == PERIODS // EVERY and len({sum(y.checkpoints[i][1] for y in yards) for i in range(PERIODS // EVERY)}) >= 2
    ens = rc.case_ensemble(N)
    try:
        recipes, got_of = ens.recipes()
        assert recipes == rc.case_recipes() and np.array_equal(got_of, of)
        for i in range(PERIODS // EVERY):
            ens.run(EVERY)
            got, summary = ens.levels(), ens.recipe_summary()
            j = yards[0].checkpoints[i][0]
            assert ens.period_index() == j and ens.n_unfinished() == sum(y.checkpoints[i][1] for y in yards), f"period {j}: {ens.n_unfinished()} unfinished"
            for r, y in enumerate(yards):
                m = of == r
                for k, w in y.checkpoints[i][2].items():
                    assert np.array_equal(got[k][..., m].astype(np.int64), w[..., m].astype(np.int64)), f"period {j}, recipe {r}: {k} differs"
                assert summary[r] == y.checkpoints[i][3], f"period {j}, recipe {r}: {summary[r]} vs {y.checkpoints[i][3]}"
        ac.assert_equal(ac.ensemble_result(ens), main[0], f"runs of {EVERY} against one run")
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_uninstalled_recipes_leave_no_trace():
    """install, uninstall, set_level(1), a plain run: an ensemble that never had recipes"""
    def twin():
        ens = SequentialEnsemble(rc.case_config(), SMALL, seed=CASE["seed"], **ec.TRAINED_LEARNERS_CASE)
        ens.set_tables(*ec.trained_tables(SMALL))
        return ens

    def finish(ens):
        ens.set_level(1)
        return flown(ens, 300)

    want, _, _ = finish(twin())
    assert want["decisions"].min() >= 1
    ens = twin()
    ens.set_curriculum(4, CASE["E"])
    ens.set_recipes(rc.case_recipes(), rc.case_recipe_of(SMALL))
    ens.set_recipes([], None)
    assert ens.recipes()[0] == [] and (ens.recipes()[1] == -1).all()
    ens.set_curriculum(4, 0)
    got, j, _ = finish(ens)
    assert j == 300
    ec.assert_equal(got, want, "recipes installed and uninstalled against an ensemble that never had any")


def test_refusals_change_nothing(yards):
    """every refusal returns DQL_EINVAL with a message that says nothing was changed or launched, through the C interface itself; afterwards the ensemble flies
    as its unrefused twin (the yardsticks' first 28 learners)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ratios, eps, alpha = np.array(ac.TRAINED_RATIOS), np.zeros(1), np.full(3, 0.5)
    of = rc.case_recipe_of(SMALL)

    def refused(lib, rc_, word):
        assert rc_ == _lib.EINVAL
        msg = lib.dql_last_error().decode()
        assert word in msg and ("nothing was changed" in msg or "nothing was launched" in msg), msg

    # curriculum mode off: no recipes
    ens = SequentialEnsemble(rc.case_config(), SMALL, seed=CASE["seed"], log_capacity=CASE["log_capacity"])
    lib, h = ens.lib, ens._h
    try:
        refused(lib, lib.dql_ensemble_set_recipes(h, 3, p(of)), "curriculum mode")
        refused(lib, lib.dql_ensemble_set_recipe(h, 0, 0x7F, p(alpha), 3, 0.1, p(ratios), 4, 1, 0), "no recipes are installed")
        refused(lib, lib.dql_ensemble_set_recipe_level_schedules(h, 0, 0, p(eps), 1, 4, 3, 6), "no recipes are installed")
        ens.set_curriculum(4, CASE["E"])
        refused(lib, lib.dql_ensemble_set_recipes(h, 65, p(of)), "n_recipes")
        refused(lib, lib.dql_ensemble_set_recipes(h, -1, p(of)), "n_recipes")
        refused(lib, lib.dql_ensemble_set_recipes(h, 3, None), "null")
        refused(lib, lib.dql_ensemble_set_recipes(h, 2, p(of)), "recipe_of")  # an index 2 with two recipes
        bad = of.copy(); bad[5] = -1
        refused(lib, lib.dql_ensemble_set_recipes(h, 3, p(bad)), "recipe_of")
        assert (ens.recipes()[1] == -1).all()
        # installed, nothing filled in: run is refused and flies nothing; then a rule without schedules, then schedules short of last_level
        assert lib.dql_ensemble_set_recipes(h, 3, p(of)) == _lib.OK
        refused(lib, lib.dql_ensemble_run(h, 10), "dql_ensemble_set_recipe")
        recipes = rc.case_recipes()
        checked = [r.checked(ens.cfg) for r in recipes]
        for i, (r, (a_, am, ra, lv)) in enumerate(zip(recipes, checked)):
            assert lib.dql_ensemble_set_recipe(h, i, r.quirks, p(a_), a_.size, am, p(ra), r.last_level, int(r.advance_exhausted), r.transfer_order) == _lib.OK
            refused(lib, lib.dql_ensemble_run(h, 10), "dql_ensemble_set_recipe_level_schedules")
            for k, (e, w, ms, me) in enumerate(lv):
                if k <= r.last_level and not (i == 1 and k == 3):  # recipe 1 stays without level 3 for now; recipe 2 needs none above its last level 2
                    assert lib.dql_ensemble_set_recipe_level_schedules(h, i, k, p(e), e.size, w, ms, me) == _lib.OK
        refused(lib, lib.dql_ensemble_run(h, 10), "dql_ensemble_set_recipe_level_schedules")
        assert ens.period_index() == 0 and ens.counters()["decisions"].sum() == 0
        e, w, ms, me = checked[1][3][3]
        assert lib.dql_ensemble_set_recipe_level_schedules(h, 1, 3, p(e), e.size, w, ms, me) == _lib.OK
        # every argument refusal of the two setters, on the installed and complete recipes
        a1, am1, ra1, _ = checked[1]
        set1 = lambda **kw: lib.dql_ensemble_set_recipe(h, *[{**dict(r=1, quirks=0x40, alpha=p(a1), n_alpha=a1.size, alpha_min=am1, ratios=p(ra1), last_level=4, advance_exhausted=1,
                                                                     transfer_order=1), **kw}[k] for k in ("r", "quirks", "alpha", "n_alpha", "alpha_min", "ratios", "last_level", "advance_exhausted", "transfer_order")])
        for kw, word in ((dict(r=3), "recipe must be"), (dict(r=-1), "recipe must be"), (dict(alpha=None), "null table"), (dict(n_alpha=0), "lengths"), (dict(n_alpha=(1 << 22) + 1), "lengths"),
                         (dict(alpha=p(np.array([0.5, 1.5, 0.5])), n_alpha=3), "[0, 1]"), (dict(alpha_min=np.nan), "[0, 1]"), (dict(alpha_min=1.5), "[0, 1]"), (dict(ratios=None), "ratios"),
                         (dict(ratios=p(np.array([1.0, np.nan, 1.0, 1.0, 1.0]))), "finite"), (dict(ratios=p(np.array([1.0, 1.0, 1.0, np.inf, 1.0]))), "finite"),
                         (dict(advance_exhausted=2), "advance_exhausted"), (dict(last_level=5), "last_level"), (dict(last_level=-1), "last_level"), (dict(transfer_order=2), "transfer_order"),
                         (dict(transfer_order=-1), "transfer_order")):
            refused(lib, set1(**kw), word)
        lvs = lambda **kw: lib.dql_ensemble_set_recipe_level_schedules(h, *[{**dict(r=1, level=1, eps=p(eps), n_eps=1, window=4, ms=3, me=6), **kw}[k] for k in ("r", "level", "eps", "n_eps", "window", "ms", "me")])
        for kw, word in ((dict(r=3), "recipe must be"), (dict(level=-1), "level"), (dict(level=5), "level"), (dict(eps=None), "null"), (dict(n_eps=0), "length"), (dict(window=0), "window"),
                         (dict(window=129), "window"), (dict(ms=0), "positive"), (dict(me=0), "positive"), (dict(eps=p(np.array([1.5]))), "[0, 1]")):
            refused(lib, lvs(**kw), word)
        # the mode stays on, and nobody is put above the smallest last_level of the populated recipes (recipe 2's: 2)
        refused(lib, lib.dql_ensemble_set_curriculum(h, 4, 0, None, 1), "recipes are installed")
        refused(lib, lib.dql_ensemble_set_level(h, 3), "last_level")
        assert (ens.levels()["level"] == 0).all() and ens.period_index() == 0
        # last_level below a member's level: after 256 periods learners of recipe 1 stand above level 0
        ens.set_tables(*ec.trained_tables(SMALL))
        ens.run(EVERY)
        assert ens.levels()["level"][of == 1].max() >= 1
        refused(lib, set1(last_level=0), "last_level")
        refused(lib, lib.dql_ensemble_run(h, 0), "periods")
        ens.run(PERIODS - EVERY)
        assert ens.index_faults() == 0
        first = list(range(SMALL))
        for r, y in enumerate(yards):
            rows = [l for l in first if of[l] == r]
            ac.assert_equal(ac.ensemble_result(ens), y.result(), f"after the refusals, recipe {r}", learners=(rows, rows))
    finally:
        ens.close()
