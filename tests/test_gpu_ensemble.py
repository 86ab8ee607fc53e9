"""The ensemble of sequential learners on the device (dql_ensemble_* / k_learn) against the reference loop of tests/ensemble_checks.py — the unchanged oracle
stepped with external actions, `oracle.agent_predict` / `oracle.agent_update` on per-learner tables, freeze rules on a literal deque.  Every comparison is `==`:
all tables, counters, episode logs, promotion episodes and state fields."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import ensemble_checks as ec

pytestmark = pytest.mark.gpu
L, SEED, PERIODS, LOG_CAP = 130, 2024, 300, 32


def make(cfg, n=L, seed=SEED, eps=ec.EPS_TABLE, **kw):
    kw.setdefault("max_episodes", 1 << 30)
    return SequentialEnsemble(cfg, n, seed=seed, log_capacity=LOG_CAP, eps=eps, **kw)


@pytest.fixture(scope="module")
def main_runs():
    """(reference result, the ensemble's result after one run of 300 periods), per (dtype, quirks): computed once, shared"""
    cache = {}

    def get(dtype, quirks):
        if (dtype, quirks) not in cache:
            cfg = training_config(0, quirks=quirks, dtype=dtype)
            ref = ec.Reference(cfg, L, SEED, log_capacity=LOG_CAP)
            ref.run(PERIODS)
            ens = make(cfg)
            try:
                ens.run(PERIODS)
                cache[(dtype, quirks)] = (ref.result(), ec.ensemble_result(ens), ens.index_faults(), ens.period_index())
            finally:
                ens.close()
        return cache[(dtype, quirks)]
    return get


@pytest.mark.parametrize("quirks", [ec.Q_REFERENCE, ec.Q_BENCH], ids=["quirks-0x7f", "quirks-0x60"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_main_parity_130_learners_300_periods(main_runs, dtype, quirks):
    """three waves, the last partly empty; a second ensemble run as 7 + 293 periods equals the first"""
    want, got, faults, j = main_runs(dtype, quirks)
    assert want["episodes"].min() >= 1 and want["episodes"].max() >= 4 and (want["qa"] != 0).any() and len(set(want["log_code"][want["log_code"] > 0].tolist())) >= 2
    print("episodes per learner", want["episodes"].min(), "..", want["episodes"].max(), "codes", sorted(set(want["log_code"].ravel().tolist())))
    ec.assert_equal(got, want, f"dtype {dtype} quirks {quirks:#x}")
    assert faults == 0 and j == PERIODS
    ens = make(training_config(0, quirks=quirks, dtype=dtype))
    try:
        ens.run(7); ens.run(293)
        ec.assert_equal(ec.ensemble_result(ens), got, "7 + 293 periods against 300")
        assert ens.index_faults() == 0 and ens.period_index() == PERIODS
    finally:
        ens.close()


def test_double_q_coin_parity():
    """quirks 0x40: the coin picks the updated table, the other table values its greedy action"""
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ref = ec.Reference(cfg, 70, 5, log_capacity=LOG_CAP)
    ref.run(150)
    want = ref.result()
    assert (want["qa"] != 0).any() and (want["qb"] != 0).any()
    ens = make(cfg, 70, 5)
    try:
        ens.run(150)
        ec.assert_equal(ec.ensemble_result(ens), want, "Double Q-learning")
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_freeze_and_rearm():
    """level 0, eps = 1, window 4, 3 successes, 6 episodes, 64 learners, 350 periods: promoted, exhausted and flying learners side by side; then
    transfer(0, 1.0), set_level(1) and 100 more periods"""
    cfg = training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    kw = dict(window=4, min_successes=3, max_episodes=6)
    ref = ec.Reference(cfg, 64, 11, eps=[1.0], log_capacity=LOG_CAP, **kw)
    ref.run(350)
    want = ref.result()
    promoted, frozen = want["promotion_episode"] >= 0, want["frozen"]
    print("promoted", int(promoted.sum()), "exhausted", int((frozen & ~promoted).sum()), "flying", int((~frozen).sum()))
    assert promoted.sum() >= 1 and (frozen & ~promoted).sum() >= 1 and (~frozen).sum() >= 1  # on the reference side: the case cannot pass vacuously
    assert (want["level_episodes"][frozen & ~promoted] == 6).all() and (want["flags"][frozen] & 1).all()
    ens = make(training_config(0, quirks=ec.Q_REFERENCE, dtype=F32), 64, 11, eps=[1.0], **kw)
    try:
        ens.run(350)
        ec.assert_equal(ec.ensemble_result(ens), want, "freeze")
        assert ens.n_live() == int((~frozen).sum())
        # re-arm at the next level
        ref.transfer(0, 1.0); ref.set_level(1); ref.run(100)
        ens.transfer(0, 1.0); ens.set_level(1); ens.run(100)
        want1 = ref.result()
        assert (want1["level_episodes"] <= want1["episodes"]).all() and (want1["decisions"] > want["decisions"]).all() and not want1["frozen"].any()
        ec.assert_equal(ec.ensemble_result(ens), want1, "after transfer(0, 1.0), set_level(1) and 100 periods")
        assert ens.index_faults() == 0 and ens.period_index() == 450
    finally:
        ens.close()


def test_learner_is_independent_of_the_ensemble_size(main_runs):
    """learner 70 of the 130-learner ensemble equals learner 70 of an ensemble of 71"""
    _, got, _, _ = main_runs(F32, ec.Q_REFERENCE)
    ens = make(training_config(0, quirks=ec.Q_REFERENCE, dtype=F32), 71)
    try:
        ens.run(PERIODS)
        ec.assert_equal(ec.ensemble_result(ens), got, "L = 71 against L = 130", learners=([70], [70]))
    finally:
        ens.close()


def test_table_round_trip_with_a_slice():
    rng = np.random.default_rng(0)
    ens = make(training_config(0, dtype=F32), 5)
    try:
        qa, qb, cnt = rng.normal(size=(5, N_CELLS)), rng.normal(size=(5, N_CELLS)), rng.integers(0, 50, size=(5, N_CELLS)).astype(np.float64)
        ens.set_tables(qa, qb, cnt)
        for g, w in zip(ens.get_tables(), (qa, qb, cnt)):
            assert np.array_equal(g, w)
        new = rng.normal(size=(2, N_CELLS))
        ens.set_tables(qb=new, first=2)
        qa2, qb2, cnt2 = ens.get_tables()
        want = qb.copy(); want[2:4] = new
        assert np.array_equal(qb2, want) and np.array_equal(qa2, qa) and np.array_equal(cnt2, cnt)
        a, b, c = ens.get_tables(first=3, count=2)
        assert np.array_equal(a, qa[3:5]) and np.array_equal(b, want[3:5]) and np.array_equal(c, cnt[3:5])
        # transfer: dql_agent_transfer's arithmetic, the k = 0 wrap included
        ens.transfer(0, 0.5)
        qa3, qb3, _ = ens.get_tables()
        per = N_CELLS // 5
        assert np.array_equal(qa3[:, :per], qa[:, 4 * per:] * 0.5) and np.array_equal(qb3[:, :per], want[:, 4 * per:] * 0.5) and np.array_equal(qa3[:, per:], qa[:, per:])
    finally:
        ens.close()


def test_same_state_in_consecutive_periods_reads_the_written_row():
    """greedy on tables preset to prefer `hold` everywhere: the env dwells in a bin, the update lowers the cell the next greedy choice reads.  A stale carried
    row would keep choosing `hold` after the reference has switched."""
    cfg = training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    qa0 = np.zeros((64, N_CELLS)); qa0[:, 2::3] = 0.05
    ref = ec.Reference(cfg, 64, 3, eps=[0.0], log_capacity=LOG_CAP)
    ref.qa[:] = qa0
    ref.run(120)
    want = ref.result()
    assert ref.same_state > 64 * 20, ref.same_state  # the hazard is common in the case
    changed = (want["qa"][:, 2::3] != 0.05).sum(axis=1)
    assert (changed >= 1).all() and len(set(want["action"].tolist())) >= 2
    ens = make(cfg, 64, 3, eps=[0.0])
    try:
        ens.set_tables(qa=qa0)
        ens.run(120)
        ec.assert_equal(ec.ensemble_result(ens), want, "same-state hazard")
    finally:
        ens.close()


@pytest.mark.parametrize("quirks", [ec.Q_PAPER, ec.Q_REFERENCE], ids=["quirks-0x40", "quirks-0x7f"])
@pytest.mark.parametrize("level", [4, 2], ids=["level-4", "level-2"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_trained_tables_70_learners_400_periods(dtype, level, quirks):
    """greedy from the reference's stage-4 tables (`ensemble_checks.trained_tables`), window 4, 2 successes, 6 episodes, a second wave of 6 lanes: the coin
    picking B, argmax over non-trivial rows, alpha_min beyond the table beside table entries, promotions through the ring above level 0; then 7 + 393"""
    n = 70
    cfg = training_config(level, quirks=quirks, dtype=dtype)
    want, tables = ec.trained_reference(cfg, n)
    kw = {k: v for k, v in ec.TRAINED_LEARNERS_CASE.items() if k != "log_capacity"}
    assert ec.TRAINED_LEARNERS_CASE["log_capacity"] == LOG_CAP
    for runs in ((ec.TRAINED_LEARNERS_PERIODS,), ec.TRAINED_LEARNERS_SPLIT):
        ens = make(cfg, n, ec.TRAINED_LEARNERS_SEED, **kw)
        try:
            ens.set_tables(*tables)
            for r in runs:
                ens.run(r)
            ec.assert_equal(ec.ensemble_result(ens), want, f"trained tables, runs {runs}, level {level} dtype {dtype} quirks {quirks:#x}")
            assert ens.index_faults() == 0 and ens.period_index() == ec.TRAINED_LEARNERS_PERIODS and ens.n_live() == int((~want["frozen"]).sum())
        finally:
            ens.close()


def test_refused_calls_launch_nothing():
    lib = _lib.load()
    cfg = training_config(0, dtype=F32)
    for bad in (training_config(0, dtype=F32, two_axis=1), training_config(0, dtype=F32, trajectory=1)):
        with pytest.raises(ValueError):
            SequentialEnsemble(bad, 4)
        h = C.c_void_p()
        c = bad.to_c()
        assert lib.dql_ensemble_create(C.byref(c), 0, 4, 1, 0, C.byref(h)) == _lib.EINVAL and lib.dql_last_error() and not h.value
    c = cfg.to_c()
    h = C.c_void_p()
    assert lib.dql_ensemble_create(C.byref(c), 0, 0, 1, 0, C.byref(h)) == _lib.EINVAL
    assert lib.dql_ensemble_create(C.byref(c), 0, 4, 1, 0, None) == _lib.EINVAL
    assert lib.dql_ensemble_create(None, 0, 4, 1, 0, C.byref(h)) == _lib.EINVAL
    assert lib.dql_ensemble_run(None, 1) == _lib.EINVAL
    ens = make(cfg, 4)
    try:
        before = ec.ensemble_result(ens)
        a, e = np.array([0.1]), np.array([0.0])
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        assert lib.dql_ensemble_set_schedules(ens._h, p(a), 1, p(e), 1, 129, 3, 10) == _lib.EINVAL and b"128" in lib.dql_last_error()
        assert lib.dql_ensemble_set_schedules(ens._h, None, 1, p(e), 1, 100, 97, 10) == _lib.EINVAL
        assert lib.dql_ensemble_set_schedules(ens._h, p(a), 1, None, 1, 100, 97, 10) == _lib.EINVAL
        assert lib.dql_ensemble_set_schedules(ens._h, p(a), 1, p(e), 1, 100, 0, 10) == _lib.EINVAL
        for periods in (0, -5):
            assert lib.dql_ensemble_run(ens._h, periods) == _lib.EINVAL and b"nothing was launched" in lib.dql_last_error()
        buf = np.zeros((4, N_CELLS))
        for first, count in ((-1, 2), (3, 2), (0, 5), (4, 1), (0, 0)):
            assert lib.dql_ensemble_get_tables(ens._h, first, count, p(buf), None, None) == _lib.EINVAL
            assert lib.dql_ensemble_set_tables(ens._h, first, count, p(buf), None, None) == _lib.EINVAL
        assert lib.dql_ensemble_set_level(ens._h, 5) == _lib.EINVAL and lib.dql_ensemble_transfer(ens._h, -1, 1.0) == _lib.EINVAL
        assert lib.dql_ensemble_get_state(ens._h, None, None) == _lib.EINVAL and lib.dql_ensemble_index_faults(ens._h, None) == _lib.EINVAL
        assert lib.dql_ensemble_get_counters(ens._h, None, None, None, None, None, None, None) == _lib.EINVAL
        assert lib.dql_ensemble_get_episode_log(ens._h, None, None, LOG_CAP, None) == _lib.EINVAL
        with pytest.raises(ValueError):
            ens.run(0)
        with pytest.raises(ValueError):
            ens.get_tables(first=3, count=2)
        with pytest.raises(ValueError):
            ens.set_schedules(window=129)
        ec.assert_equal(ec.ensemble_result(ens), before, "after the refused calls")
        assert ens.period_index() == 0
    finally:
        ens.close()
