"""The ensemble of sequential learners on the device, where the headline runs go and tests/test_gpu_ensemble.py does not: both words of the promotion ring and
its wrap, calls of more than 4 096 periods (several launches, the `live == 0` shortcut, launches over frozen learners), visit counts beyond the learning-rate
table, an episode log that overflows, the as-launched parameters, and `ensemble.curriculum` through levels 0 - 4.  The yardstick is the reference loop of
tests/ensemble_checks.py; every comparison is `==`, and every case first asserts on the yardstick that the path it is for is taken."""
from types import SimpleNamespace

import numpy as np
import pytest

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, F64, as_launched_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
from dql_multirotor_landing_amd.trainer import Trainer

import ensemble_checks as ec

pytestmark = pytest.mark.gpu
LOG_CAP = 32


def level0():
    return training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)


def ring_ensemble(n=ec.RING_LEARNERS):
    return SequentialEnsemble(level0(), n, seed=ec.RING_SEED, **ec.RING_CASE)


@pytest.fixture(scope="module")
def ring():
    """(reference result, freeze periods on the reference, the ensemble's result after run(8200)): computed once, shared"""
    want, freeze_period = ec.ring_reference(level0())
    ens = ring_ensemble()
    try:
        ens.run(ec.RING_PERIODS)
        got = ec.ensemble_result(ens)
        assert ens.period_index() == ec.RING_PERIODS and ens.n_live() == 0 and ens.index_faults() == 0
    finally:
        ens.close()
    return want, freeze_period, got


def test_ring_second_word_and_wrap_in_one_call_of_three_launches(ring):
    """window 72, 28 successes, 100 episodes, run(8200) = launches of 4 096 + 4 096 + 8: learners promoted from ring word 0, from word 1, after the wrap, and
    out of episodes (asserted on the reference in ensemble_checks.ring_reference); run(5000); run(3200) puts the launch boundaries elsewhere"""
    want, _, got = ring
    ec.assert_equal(got, want, "run(8200)")
    ens = ring_ensemble()
    try:
        ens.run(5000); ens.run(3200)
        ec.assert_equal(ec.ensemble_result(ens), got, "run(5000); run(3200) against run(8200)")
        assert ens.period_index() == ec.RING_PERIODS and ens.n_live() == 0 and ens.index_faults() == 0
    finally:
        ens.close()


def test_waves_leave_at_different_periods_and_learners_do_not_depend_on_them(ring):
    """80 learners, same seed and schedules: wave 0 holds the 16 learners of the long case, which freeze between periods 3 815 and 7 583, among 64; wave 1
    has 16 lanes.  Learners 0 - 15 equal the ensemble of 16."""
    want, freeze_period, got = ring
    first = list(range(ec.RING_LEARNERS))
    ens = ring_ensemble(80)
    try:
        ens.run(ec.RING_PERIODS)
        big = ec.ensemble_result(ens)
        ec.assert_equal(big, got, "L = 80 against L = 16", learners=(first, first))
        ec.assert_equal(big, want, "L = 80 against the reference", learners=(first, first))
        assert ens.index_faults() == 0 and ens.period_index() == ec.RING_PERIODS
    finally:
        ens.close()
    # when each wave left its loop: the last freeze among its lanes (ring_reference holds `freeze period == decisions + episodes - 1` on the yardstick), or
    # the end of the call.  No reference of 80 learners is flown for this (45 s): it describes the case, the comparison is the one above.
    last = np.where(big["frozen"], big["decisions"] + big["episodes"] - 1, ec.RING_PERIODS)
    assert np.array_equal(last[first], freeze_period)
    left = int(last[:64].max()), int(last[64:].max())
    print("waves left after periods", left)
    assert left[0] != left[1] and min(left) < ec.RING_PERIODS - 8, left


def test_launches_over_frozen_learners_change_nothing_but_the_period_index(ring):
    """all 16 frozen: run(10000) is one launch in which no lane is live and then the `live == 0` shortcut for the rest; run(3) is a first launch with nobody live"""
    want, _, got = ring
    assert want["frozen"].all()
    ens = ring_ensemble()
    try:
        ens.run(ec.RING_PERIODS)
        assert ens.n_live() == 0
        ens.run(10000)
        assert ens.period_index() == ec.RING_PERIODS + 10000
        ec.assert_equal(ec.ensemble_result(ens), got, "after run(10000) on frozen learners")
        ens.run(3)
        assert ens.period_index() == ec.RING_PERIODS + 10003
        ec.assert_equal(ec.ensemble_result(ens), got, "after run(3) on frozen learners")
        assert ens.n_live() == 0 and ens.index_faults() == 0
    finally:
        ens.close()


def test_alpha_min_beyond_the_table_and_a_full_episode_log():
    """a learning-rate table of 32 entries (its last entry is not alpha_min) and a log of 8 episodes, 1 500 periods: counts pass the table's end, log_n counts on
    beyond the log, which keeps the first 8 episodes"""
    n, seed, periods, cap = 16, 11, 1500, 8
    tab = level0().alpha_table()[:32]
    assert len(tab) == 32 and tab[31] != level0().alpha_min
    ref = ec.Reference(level0(), n, seed, eps=[0.3], log_capacity=cap, alpha_tab=tab)
    ref.run(periods)
    want = ref.result()
    print("largest count", want["count"].max(), "cells beyond the table per learner", (want["count"] > 32).sum(axis=1).tolist(), "episodes", want["log_n"].tolist())
    assert want["count"].max() > 64 and ((want["count"] > 32).sum(axis=1) >= 1).all() and want["log_n"].min() > cap and not want["frozen"].any()
    assert want["log_code"].shape == (n, cap) and (want["log_len"] > 0).all()
    ens = SequentialEnsemble(level0(), n, seed=seed, eps=[0.3], log_capacity=cap, alpha_table=tab)
    try:
        ens.run(periods)
        ec.assert_equal(ec.ensemble_result(ens), want, "short alpha table, log of 8")
        assert ens.index_faults() == 0
    finally:
        ens.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_as_launched_parameters_70_learners_300_periods(dtype):
    """as_launched_config (observation noise 0.25 m / 0.1 m/s, platform at 1 m/s): what `--launched` and the G14 figures fly; also as 7 + 293 periods"""
    n, seed, periods = 70, 2024, 300
    cfg = as_launched_config(0, dtype=dtype)
    assert cfg.noise_pos_sd > 0.0 and cfg.noise_vel_sd > 0.0 and cfg.mp_t_x != training_config(0).mp_t_x and cfg.quirks == ec.Q_REFERENCE
    ref = ec.Reference(cfg, n, seed, log_capacity=LOG_CAP)
    ref.run(periods)
    want = ref.result()
    print("episodes per learner", want["episodes"].min(), "..", want["episodes"].max(), "codes", sorted(set(want["log_code"].ravel().tolist())))
    assert want["episodes"].min() >= 1 and len(set(want["log_code"][want["log_code"] > 0].tolist())) >= 2 and (want["qa"] != 0).any()
    make = lambda: SequentialEnsemble(as_launched_config(0, dtype=dtype), n, seed=seed, log_capacity=LOG_CAP, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    ens = make()
    try:
        ens.run(periods)
        got = ec.ensemble_result(ens)
        ec.assert_equal(got, want, f"as launched, dtype {dtype}")
        assert ens.index_faults() == 0 and ens.period_index() == periods
    finally:
        ens.close()
    ens = make()
    try:
        ens.run(7); ens.run(293)
        ec.assert_equal(ec.ensemble_result(ens), got, "7 + 293 periods against 300")
        assert ens.index_faults() == 0 and ens.period_index() == periods
    finally:
        ens.close()


# `ensemble.curriculum` with at most one run(P) per level.  P = 400 (from 300 .. 800): on the reference, level 0 then ends with 2 learners promoted, 17 out of
# episodes and 5 still flying, and every learner logs an episode at every level.
CURRICULUM = dict(n=24, seed=11, P=400, window=4, success_rate=0.5, max_episodes=6)


@pytest.fixture(scope="module")
def curriculum_reference():
    """the reference loop taken through the same calls by hand; -> (result after each level's run, tables after the last transfer)"""
    c = CURRICULUM
    me = SimpleNamespace(_scale_modification_value=(0.8172650252856599, 0.8211253690681617, 0.8257273369742982, 0.8311571820651724))
    min_successes = ensemble.min_successes_for(c["window"], c["success_rate"])
    assert min_successes == 3
    ref = ec.Reference(level0(), c["n"], c["seed"], log_capacity=LOG_CAP)
    levels = []
    for k in range(5):
        if k > 0:
            ref.set_level(k)
        ref.set_schedules(ensemble.exploration_rates(k), c["window"], min_successes, c["max_episodes"])
        ref.run(c["P"])
        levels.append(ref.result())
        ref.transfer(k, float(Trainer.transfer_learning_ratio(me, k)))
    promoted, frozen = levels[0]["promotion_episode"] >= 0, levels[0]["frozen"]
    print("level 0: promoted", int(promoted.sum()), "exhausted", int((frozen & ~promoted).sum()), "flying", int((~frozen).sum()))
    assert promoted.sum() >= 1 and (frozen & ~promoted).sum() >= 1 and (~frozen).sum() >= 1
    before = {"decisions": np.zeros(c["n"], np.int64), "log_n": np.zeros(c["n"], np.int32)}
    for k, w in enumerate(levels):
        assert (w["decisions"] > before["decisions"]).all() and (w["log_n"] > before["log_n"]).all(), f"level {k}"
        before = w
    assert levels[-1]["log_n"].max() <= LOG_CAP and any((w["qa"] != 0).any() for w in levels)
    return levels, (ref.qa.copy(), ref.qb.copy(), ref.cnt.copy())


def test_curriculum_levels_0_to_4_equals_the_reference_loop(curriculum_reference):
    """set_level, new schedules per level, transfer with the reference's ratios (the k = 0 wrap included), compared after every level"""
    c = CURRICULUM
    levels, tables = curriculum_reference
    seen = []

    def on_level(ens, entry):
        k = entry["level"]
        want = levels[k]
        ec.assert_equal(ec.ensemble_result(ens), want, f"after level {k}")
        assert np.array_equal(entry["promotion_episode"], want["promotion_episode"]) and np.array_equal(entry["level_episodes"], want["level_episodes"])
        assert entry["periods"] == c["P"] and ens.period_index() == (k + 1) * c["P"] and ens.cfg.working_curriculum_step == k
        seen.append(k)

    ens = SequentialEnsemble(level0(), c["n"], seed=c["seed"], log_capacity=LOG_CAP)
    try:
        history = ensemble.curriculum(ens, max_episodes=c["max_episodes"], max_periods_per_level=c["P"], window=c["window"], success_rate=c["success_rate"], on_level=on_level)
        assert seen == [0, 1, 2, 3, 4] and [h["level"] for h in history] == seen
        for g, w, name in zip(ens.get_tables(), tables, ("qa", "qb", "count")):
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), f"{name} after the last transfer"
        assert ens.index_faults() == 0
    finally:
        ens.close()
