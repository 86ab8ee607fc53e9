"""Per-learner curriculum levels on the device: `SequentialEnsemble.set_curriculum`, k_learn_levels over the worklist, k_ens_advance.

The yardstick is tests/advance_checks.py (the unchanged oracle, one per level); every comparison is `==`, floats by their bits.  The case's conditions — three
levels at once, two waves of one level, padding, an empty level between populated ones, both ways of advancing, finished and unfinished learners at the end —
are asserted on the yardstick before an ensemble is looked at.  The cases from trained tables at the end of the file are there for what tables of zeros never reach:
promotions through the ring above level 0, transfers of non-zero blocks of both tables, the k = 0 wrap with a source block and a ratio that show."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import advance_checks as ac
import ensemble_checks as ec

pytestmark = pytest.mark.gpu
CASE = ac.CASE
CELLS_PER_LEVEL = N_CELLS // 5


def flown(ens, *runs):
    try:
        for r in runs:
            ens.run(r)
        assert ens.index_faults() == 0
        return ac.ensemble_result(ens), ens.period_index(), ens.n_unfinished()
    finally:
        ens.close()


@pytest.fixture(scope="module")
def yard():
    """the yardstick flown through the case once (about 6 s on the CPU), its conditions asserted"""
    y = ac.case_yardstick()
    ac.assert_case_conditions(y)
    return y, y.result()


@pytest.fixture(scope="module")
def main():
    """the ensemble's result after run(1024), shared"""
    got, j, unfinished = flown(ac.case_ensemble(), CASE["periods"])
    assert j == CASE["periods"]
    return got, unfinished


def test_whole_run_equals_the_yardstick_f32(yard, main):
    y, want = yard
    got, unfinished = main
    ac.assert_equal(got, want, "run(1024), float32")
    assert unfinished == y.n_unfinished() and 0 < unfinished < CASE["n"]


def test_whole_run_equals_the_yardstick_f64():
    """384 periods: six advance points, learners on levels 0 - 3"""
    y = ac.case_yardstick(dtype=F64, periods=384)
    want = y.result()
    assert len(set(want["level"].tolist())) >= 3 and y.advanced_promoted >= 1 and y.advanced_exhausted >= 1
    got, j, unfinished = flown(ac.case_ensemble(dtype=F64), 384)
    ac.assert_equal(got, want, "run(384), float64")
    assert unfinished == y.n_unfinished()


@pytest.mark.parametrize("runs", [(7, 1017), (7, 100, 917), (64, 1, 63, 896), (500, 524)], ids=lambda r: "+".join(map(str, r)))
def test_splits_equal_one_run(main, runs):
    """advance points depend on the period index only: cuts off the multiples of E, on them, and one period after them"""
    assert sum(runs) == CASE["periods"] and any(r % CASE["E"] for r in runs)
    got, j, _ = flown(ac.case_ensemble(), *runs)
    assert j == CASE["periods"]
    ac.assert_equal(got, main[0], f"runs {runs} against run(1024)")


def test_first_24_learners_do_not_depend_on_the_other_56(yard, main):
    """another worklist (one wave per level instead of up to two, other lanes, other padding), the same learners"""
    first = list(range(ac.SMALL))
    got, _, _ = flown(ac.case_ensemble(n=ac.SMALL), CASE["periods"])
    ac.assert_equal(main[0], got, "L = 80 against L = 24", learners=(first, first))
    ac.assert_equal(got, yard[1], "L = 24 against the yardstick", learners=(first, first))


def test_exhausted_learners_stay_where_they_froze_when_they_do_not_advance():
    """advance_exhausted = 0: promoted learners advance, a learner out of episodes keeps level, tables and env from its freeze point on; at the end everyone is
    finished, and run(3) then changes the period index and nothing else"""
    y = ac.case_yardstick(advance_exhausted=False)
    want = y.result()
    exhausted = want["frozen"] & (want["promotion_episode"] < 0)
    print("levels", np.bincount(want["level"], minlength=5).tolist(), "exhausted", int(exhausted.sum()), "advanced promoted", y.advanced_promoted)
    assert y.advanced_exhausted == 0 and y.advanced_promoted >= 1 and (exhausted & (want["level"] == 0)).any() and (want["level"] == 1).any()
    assert y.n_unfinished() == 0 and want["frozen"].all()
    ens = ac.case_ensemble(advance_exhausted=False)
    try:
        ens.run(CASE["periods"])
        got = ac.ensemble_result(ens)
        ac.assert_equal(got, want, "advance_exhausted = 0")
        assert ens.n_unfinished() == 0 and ens.n_live() == 0
        ens.run(3)
        assert ens.period_index() == CASE["periods"] + 3
        ac.assert_equal(ac.ensemble_result(ens), got, "run(3) with everyone finished")
        ens.run(200)  # crosses advance points
        assert ens.period_index() == CASE["periods"] + 203
        ac.assert_equal(ac.ensemble_result(ens), got, "run(200) with everyone finished")
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_mode_on_with_nobody_frozen_equals_the_plain_ensemble():
    """last_level = the current level, the default schedules (no freeze within 300 periods): the worklist launch against k_learn, bit for bit"""
    n, seed, periods = 70, 2024, 300
    kw = dict(eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30)
    plain = SequentialEnsemble(ac.level0(), n, seed=seed, log_capacity=32, **kw)
    want, _, _ = flown(plain, periods)
    assert not want["frozen"].any() and want["episodes"].min() >= 1
    ens = SequentialEnsemble(ac.level0(), n, seed=seed, log_capacity=32, **kw)
    ens.set_level_schedules(0, **kw)
    ens.set_curriculum(0, 64)
    got, j, unfinished = flown(ens, 7, periods - 7)
    assert j == periods and unfinished == n
    ac.assert_equal(got, want, "curriculum mode, nobody frozen, against the plain ensemble")
    # the mode switched off again: k_learn as before
    ens = SequentialEnsemble(ac.level0(), n, seed=seed, log_capacity=32, **kw)
    ens.set_level_schedules(0, **kw)
    ens.set_curriculum(0, 64)
    ens.set_curriculum(0, 0)
    got, _, _ = flown(ens, periods)
    ac.assert_equal(got, want, "curriculum mode off again")


def test_replaced_schedules_leave_no_trace():
    """`set_schedules` twice (tables of other lengths) and `set_level_schedules(0, ...)` twice (other tables), then eight periods in curriculum mode across an
    advance point: tables, counters and levels are those of an ensemble that was only ever given the final schedules, bit for bit.  One wave, float32: what is
    exercised is the host side — a replaced device table is freed when it is replaced, the last one when the ensemble is destroyed (`flown` closes it)."""
    n, seed = 64, 5
    first = dict(alpha_table=np.linspace(0.5, 0.05, 3), eps=np.full(2, 0.3), window=5, min_successes=2, max_episodes=9)
    final = dict(alpha_table=np.linspace(0.9, 0.05, 11), eps=np.linspace(0.8, 0.1, 9), window=4, min_successes=3, max_episodes=6)
    lv_first = dict(eps=np.full(3, 0.9), window=7, min_successes=2, max_episodes=4)
    lv_final = dict(eps=np.linspace(0.7, 0.2, 6), window=4, min_successes=3, max_episodes=6)

    def fly(ens):
        ens.set_level_schedules(0, **lv_final)
        ens.set_level_schedules(1, **lv_final)
        ens.set_curriculum(1, 4)
        return flown(ens, 8)

    want, j, _ = fly(SequentialEnsemble(ac.level0(), n, seed=seed, log_capacity=4, **final))
    assert j == 8 and want["decisions"].min() >= 1
    ens = SequentialEnsemble(ac.level0(), n, seed=seed, log_capacity=4, **first)
    ens.set_schedules(**final)
    ens.set_level_schedules(0, **lv_first)
    got, _, _ = fly(ens)
    ac.assert_equal(got, want, "schedules replaced before the run against the final schedules alone")


def test_last_level_2_is_never_exceeded(main):
    got, _, unfinished = flown(ac.case_ensemble(last_level=2), CASE["periods"])
    print("levels", np.bincount(got["level"], minlength=5).tolist(), "unfinished", unfinished)
    assert got["level"].max() == 2 and (got["frozen"] & (got["level"] == 2)).any()
    assert (got["entered_period"][3:] == -1).all() and (got["promoted_at"][3:] == -1).all() and (got["episodes_at"][3:] == 0).all()
    for t in ("qa", "qb", "count"):
        assert not got[t][:, 3 * CELLS_PER_LEVEL:].any(), f"{t}: cells of levels 3 and 4 were written"
    # a learner's way up to level 2 does not depend on where the curriculum ends
    want = main[0]
    assert np.array_equal(got["entered_period"][:3], want["entered_period"][:3]) and (got["entered_period"][2] >= 0).any()
    assert np.array_equal(got["promoted_at"][:2], want["promoted_at"][:2]) and np.array_equal(got["episodes_at"][:2], want["episodes_at"][:2])


def test_ring_is_cleared_on_advance():
    """`advance_checks.RING_CASE`: one success promotes above level 0, and learners arrive there with level-0 successes in their ring"""
    y = ac.case_yardstick(**ac.RING_CASE)
    want = y.result()
    ac.assert_ring_case_conditions(y, want)
    got, j, unfinished = flown(ac.case_ensemble(**ac.RING_CASE), 7, ac.RING_CASE["periods"] - 7)
    ac.assert_equal(got, want, "the ring case")
    assert j == ac.RING_CASE["periods"] and unfinished == y.n_unfinished()


def test_scoring_a_slice_between_two_runs_leaves_the_run_unchanged(main):
    ens = ac.case_ensemble()
    try:
        ens.run(500)
        r = ens.score(training_config(1, quirks=ec.Q_REFERENCE, dtype=F32), envs_per_learner=64, first=8, count=16)
        assert r["by_code"].sum() > 0
        ens.run(524)
        ac.assert_equal(ac.ensemble_result(ens), main[0], "run(500); score; run(524) against run(1024)")
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_curriculum_per_learner_runs_until_nobody_is_unfinished():
    """`ensemble.curriculum_per_learner` (one budget for all levels) against the same calls made by hand"""
    kw = dict(window=4, success_rate=0.5, max_episodes=1)
    ens = SequentialEnsemble(ac.level0(), ac.SMALL, seed=CASE["seed"], log_capacity=32)
    try:
        hist = ensemble.curriculum_per_learner(ens, advance_every=64, chunk_periods=512, max_periods=4096, **kw)
        assert ens.n_unfinished() == 0 and hist["periods"] % 512 == 0 and (hist["level"] == 4).all() and (hist["entered_period"] >= 0).all()
        assert (hist["episodes_at"] == 1).all() and (np.diff(hist["entered_period"], axis=0) > 0).all()
        got = ac.ensemble_result(ens)
        assert ens.index_faults() == 0
    finally:
        ens.close()
    by_hand = ac.case_ensemble(n=ac.SMALL, max_episodes=(1,) * 5, log_capacity=32)
    want, _, unfinished = flown(by_hand, hist["periods"])
    assert unfinished == 0
    ac.assert_equal(got, want, "curriculum_per_learner against the calls by hand")


def test_set_level_in_curriculum_mode_sets_everyone_and_clears_the_history_from_there():
    ens = ac.case_ensemble(n=ac.SMALL)
    try:
        ens.run(400)
        before = ens.levels()
        assert before["level"].max() >= 2
        ens.set_level(1)
        lv = ens.levels()
        assert (lv["level"] == 1).all() and (lv["entered_period"][1] == 400).all() and (lv["entered_period"][2:] == -1).all()
        assert (lv["promoted_at"][1:] == -1).all() and (lv["episodes_at"][1:] == 0).all()
        left0 = before["level"] > 0  # level 0's entry was recorded when the learner advanced from it (a learner still on it had no entry yet)
        assert left0.any() and np.array_equal(lv["promoted_at"][0][left0], before["promoted_at"][0][left0])
        assert np.array_equal(lv["episodes_at"][0][left0], before["episodes_at"][0][left0]) and np.array_equal(lv["entered_period"][0], before["entered_period"][0])
        c = ens.counters()
        assert not c["frozen"].any() and (c["level_episodes"] == 0).all() and (ens.state()["flags"] & 1).all()
        ens.run(200)
        assert ens.index_faults() == 0 and ens.levels()["level"].min() >= 1
    finally:
        ens.close()


def test_refusals():
    """every refusal returns DQL_EINVAL with a message, through the C interface itself"""
    ens = SequentialEnsemble(training_config(1, quirks=ec.Q_REFERENCE, dtype=F32), 8, seed=3)
    lib, h = ens.lib, ens._h
    ratios = np.array(ensemble.REFERENCE_RATIOS)
    eps = np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, word):
        assert rc == _lib.EINVAL
        msg = lib.dql_last_error().decode()
        assert word in msg, msg

    try:
        refused(lib.dql_ensemble_set_curriculum(h, 0, 64, p(ratios), 1), "last_level")  # below the current level 1
        refused(lib.dql_ensemble_set_curriculum(h, 5, 64, p(ratios), 1), "last_level")
        refused(lib.dql_ensemble_set_curriculum(h, 4, -1, p(ratios), 1), "advance_every")
        refused(lib.dql_ensemble_set_curriculum(h, 4, 4097, p(ratios), 1), "advance_every")
        for bad in (np.nan, np.inf):
            r = ratios.copy(); r[3] = bad
            refused(lib.dql_ensemble_set_curriculum(h, 4, 64, p(r), 1), "finite")
        refused(lib.dql_ensemble_set_curriculum(h, 4, 64, None, 1), "ratios")
        refused(lib.dql_ensemble_set_curriculum(h, 4, 64, p(ratios), 2), "advance_exhausted")
        for level in (-1, 5):
            refused(lib.dql_ensemble_set_level_schedules(h, level, p(eps), 1, 4, 3, 6), "level")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, None, 1, 4, 3, 6), "null")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(eps), 0, 4, 3, 6), "length")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(eps), 1, 0, 3, 6), "window")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(eps), 1, 129, 3, 6), "window")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(eps), 1, 4, 0, 6), "positive")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(eps), 1, 4, 3, 0), "positive")
        refused(lib.dql_ensemble_set_level_schedules(h, 1, p(np.array([1.5])), 1, 4, 3, 6), "[0, 1]")
        # the mode on with schedules for levels 1 and 2 only, last_level 3: run is refused and flies nothing
        ens.set_level_schedules(1, eps, 4, 3, 6); ens.set_level_schedules(2, eps, 4, 3, 6)
        ens.set_curriculum(3, 64)
        refused(lib.dql_ensemble_run(h, 10), "set_level_schedules")
        assert ens.period_index() == 0 and ens.counters()["decisions"].sum() == 0
        ens.set_level_schedules(3, eps, 4, 3, 6)
        ens.run(10)
        assert ens.period_index() == 10 and ens.index_faults() == 0
        # a level above last_level is not to be had while the mode is on ...
        refused(lib.dql_ensemble_set_level(h, 4), "last_level")
        assert (ens.levels()["level"] == 1).all()
        # ... and a level that has no schedule is never flown, whatever last_level says: schedules for levels 1 - 3, the learners put on level 4 with the
        # mode off, the mode on again with last_level 4
        ens.set_curriculum(3, 0)
        ens.set_level(4)
        ens.set_curriculum(4, 64)
        j, decisions = ens.period_index(), ens.counters()["decisions"].sum()
        refused(lib.dql_ensemble_run(h, 10), "set_level_schedules")
        assert ens.period_index() == j and ens.counters()["decisions"].sum() == decisions
        ens.set_level(2)
        ens.set_curriculum(3, 64)  # levels 2 and 3 have their schedules
        ens.run(5)
        assert ens.period_index() == j + 5 and ens.index_faults() == 0
        with pytest.raises(ValueError):
            ens.set_curriculum(4, 5000)
        with pytest.raises(ValueError):
            ens.set_level_schedules(7)
    finally:
        ens.close()


def test_the_mode_is_not_switched_off_while_learners_stand_on_different_levels():
    ens = ac.case_ensemble(n=ac.SMALL)
    try:
        ens.run(400)
        before = ac.ensemble_result(ens)
        assert len(set(before["level"].tolist())) >= 2
        rc = ens.lib.dql_ensemble_set_curriculum(ens._h, 4, 0, None, 1)
        assert rc == _lib.EINVAL and "switched off" in ens.lib.dql_last_error().decode()
        ac.assert_equal(ac.ensemble_result(ens), before, "a refused switch-off changes nothing")
        ens.set_level(1)  # everyone on the config's level again
        ens.set_curriculum(4, 0)
        ens.run(5)
        assert ens.period_index() == 405 and ens.index_faults() == 0 and (ens.levels()["level"] == 1).all()
    finally:
        ens.close()


# ---- from trained tables (advance_checks.TRAINED_CASE / TRAINED_FROM_3): promotions through the ring above level 0, transfers of non-zero blocks of both
# tables, the k = 0 wrap reading a level-4 block that is not zero with a ratio that is not 1.0 ----
TRAINED = {"0x7f": ac.TRAINED_CASE, "0x40": ac.TRAINED_CASE_PAPER, "from-3": ac.TRAINED_FROM_3}
EVERY = 256
FIRST = list(range(ac.SMALL))


@pytest.fixture(scope="module")
def trained_yard():
    """per (case, dtype, learners, overrides): the yardstick (its conditions asserted where the case is flown as it stands), its result and the case.  On the
    CPU about 12 s (0x7f) and 9 s (0x40) with 80 learners, 3 - 5 s with 24."""
    cache = {}

    def get(name, dtype=F32, n=None, **over):
        key = (name, dtype, n, tuple(sorted(over.items())))
        if key not in cache:
            c = dict(TRAINED[name], **over)
            if n is not None:
                c["n"] = n
            y = ac.case_yardstick(dtype=dtype, checkpoint_every=EVERY, **c)
            if not over:
                ac.assert_trained_case_conditions(y, c)
            cache[key] = (y, y.result(), c)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def trained_main():
    """per case: the float32 ensemble's result after ONE run of the case's periods"""
    cache = {}

    def get(name):
        if name not in cache:
            c = TRAINED[name]
            got, j, unfinished = flown(ac.case_ensemble(**c), c["periods"])
            assert j == c["periods"]
            cache[name] = (got, unfinished)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(TRAINED))
def test_trained_whole_run_equals_the_yardstick_f32(trained_yard, trained_main, name):
    """80 learners (two waves at level 0, padded segments), or the 24 created at level 3"""
    y, want, c = trained_yard(name)
    got, unfinished = trained_main(name)
    ac.assert_equal(got, want, f"trained case {name}, float32")
    assert unfinished == y.n_unfinished()


@pytest.mark.parametrize("name", list(TRAINED))
def test_trained_whole_run_equals_the_yardstick_f64(trained_yard, name):
    y, want, c = trained_yard(name, F64, ac.SMALL)
    got, j, unfinished = flown(ac.case_ensemble(dtype=F64, **c), c["periods"])
    ac.assert_equal(got, want, f"trained case {name}, float64")
    assert j == c["periods"] and unfinished == y.n_unfinished()


@pytest.mark.parametrize("runs", [(7, 1017), (33, 31, 960)], ids=lambda r: "+".join(map(str, r)))
@pytest.mark.parametrize("name", ["0x7f", "0x40"])
def test_trained_splits_equal_one_run(trained_main, name, runs):
    """cuts off the multiples of E = 32, one period after one, and on one"""
    c = TRAINED[name]
    assert sum(runs) == c["periods"] and any(r % c["E"] for r in runs)
    got, j, _ = flown(ac.case_ensemble(**c), *runs)
    assert j == c["periods"]
    ac.assert_equal(got, trained_main(name)[0], f"trained case {name}, runs {runs} against one run")


@pytest.mark.parametrize("name", ["0x7f", "0x40"])
def test_trained_first_24_learners_do_not_depend_on_the_other_56(trained_yard, trained_main, name):
    c = TRAINED[name]
    got, _, _ = flown(ac.case_ensemble(**dict(c, n=ac.SMALL)), c["periods"])
    ac.assert_equal(trained_main(name)[0], got, f"trained case {name}, L = 80 against L = 24", learners=(FIRST, FIRST))
    ac.assert_equal(got, trained_yard(name)[1], f"trained case {name}, L = 24 against the yardstick", learners=(FIRST, FIRST))


@pytest.mark.parametrize("name", list(TRAINED))
def test_trained_levels_and_unfinished_after_every_256_periods(trained_yard, trained_main, name):
    y, want, c = trained_yard(name)
    assert len(y.checkpoints) == c["periods"] // EVERY and len({u for _, u, _ in y.checkpoints}) >= 2  # the number of unfinished learners moves
    ens = ac.case_ensemble(**c)
    try:
        for j, unfinished, levels in y.checkpoints:
            ens.run(EVERY)
            got = ens.levels()
            assert ens.period_index() == j and ens.n_unfinished() == unfinished, f"period {j}: {ens.n_unfinished()} unfinished, the yardstick has {unfinished}"
            for k, w in levels.items():
                assert np.array_equal(got[k].astype(np.int64), w.astype(np.int64)), f"period {j}: {k} differs: {got[k].tolist()} vs {w.tolist()}"
        ac.assert_equal(ac.ensemble_result(ens), trained_main(name)[0], f"trained case {name}, runs of {EVERY} against one run")
        assert ens.index_faults() == 0
    finally:
        ens.close()


@pytest.mark.parametrize("name", ["0x7f", "0x40"])
def test_trained_last_level_2_is_never_exceeded(trained_yard, name):
    y, want, c = trained_yard(name, n=ac.SMALL, last_level=2)
    done = want["frozen"] & (want["level"] == 2)
    assert want["level"].max() == 2 and (done & (want["promotion_episode"] >= 0)).any(), "on the yardstick nobody finishes at level 2 by promotion"
    assert (want["entered_period"][3:] == -1).all() and y.promoted_from[1] >= 1
    got, j, unfinished = flown(ac.case_ensemble(**c), c["periods"])
    ac.assert_equal(got, want, f"trained case {name}, last_level = 2")
    assert unfinished == y.n_unfinished()
    for t, w in zip(("qa", "qb", "count"), ac.case_tables(c, c["n"])):
        assert np.array_equal(got[t][:, 3 * CELLS_PER_LEVEL:], w[:, 3 * CELLS_PER_LEVEL:]), f"{t}: cells of levels 3 and 4 were written"


def test_trained_exhausted_learners_do_not_advance(trained_yard):
    """advance_exhausted = 0 on the 0x7f case: learners that promoted above level 0 go on, the ones out of episodes stay where they froze"""
    y, want, c = trained_yard("0x7f", n=ac.SMALL, advance_exhausted=False)
    exhausted = want["frozen"] & (want["promotion_episode"] < 0)
    assert y.advanced_exhausted == 0 and (y.promoted_from[1:] > 0).sum() >= 2 and (exhausted & (want["level"] >= 1) & (want["level"] < 4)).any()
    got, j, unfinished = flown(ac.case_ensemble(**c), c["periods"])
    ac.assert_equal(got, want, "trained case 0x7f, advance_exhausted = 0")
    assert unfinished == y.n_unfinished()
