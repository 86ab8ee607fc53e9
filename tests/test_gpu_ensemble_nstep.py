"""Sequential learners with n-step Double-Q targets on the device (dql_ensemble_set_nstep / k_learn_nstep) against the yardstick of
tests/nstep_checks.py: the reference loop with literal per-learner windows and the return recursion written out.  Every comparison is `==`: all tables,
counters, episode logs, promotion episodes, state fields (floats by their bits) and the windows' lengths."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble, ops
from dql_multirotor_landing_amd.config import F32, F64, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
from dql_multirotor_landing_amd.trainer import Trainer

import ensemble_checks as ec
import nstep_checks as nc

pytestmark = pytest.mark.gpu
L, LOG_CAP = 70, nc.MAIN_LOG  # a second wave of 6 lanes


def make(cfg, n=L, seed=nc.MAIN_SEED, eps=ec.EPS_TABLE, log_capacity=LOG_CAP, **kw):
    kw.setdefault("max_episodes", 1 << 30)
    return SequentialEnsemble(cfg, n, seed=seed, log_capacity=log_capacity, eps=eps, **kw)


def fly(cfg, runs, n=L, tables=None, **kw):
    """the result of an ensemble flown through `runs`, its index faults and period index"""
    ens = make(cfg, n, **kw)
    try:
        if tables is not None:
            ens.set_tables(*tables)
        for r in runs:
            ens.run(r)
        return nc.ensemble_result(ens), ens.index_faults(), ens.period_index()
    finally:
        ens.close()


@pytest.fixture(scope="module")
def main_runs():
    """the device's result of a main row flown in one run of 300 periods, per row: computed once, shared"""
    cache = {}

    def get(quirks, dtype, nstep):
        if (quirks, dtype, nstep) not in cache:
            cache[(quirks, dtype, nstep)] = fly(training_config(0, quirks=quirks, dtype=dtype), (nc.MAIN_PERIODS,), nstep=nstep)
        return cache[(quirks, dtype, nstep)]
    return get


@pytest.mark.parametrize("quirks,dtype,nstep", nc.MAIN_ROWS, ids=nc.MAIN_IDS)
def test_main_rows_70_learners_300_periods_and_7_plus_293(main_runs, quirks, dtype, nstep):
    want, ev = nc.main_reference(quirks, dtype, nstep, L)  # asserts on the yardstick that the row's events occurred, pinned to the digit
    got, faults, j = main_runs(quirks, dtype, nstep)
    ec.assert_equal(got, want, "300 periods")
    assert faults == 0 and j == nc.MAIN_PERIODS
    split, faults, j = fly(training_config(0, quirks=quirks, dtype=dtype), nc.MAIN_SPLIT, nstep=nstep)
    ec.assert_equal(split, want, "7 + 293 periods")
    assert faults == 0 and j == nc.MAIN_PERIODS


@pytest.mark.parametrize("quirks", [ec.Q_REFERENCE, ec.Q_BENCH, ec.Q_PAPER], ids=["quirks-0x7f", "quirks-0x60", "quirks-0x40"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_n_1_on_the_new_kernel_equals_n_0_on_k_learn(dtype, quirks):
    """130 learners, 300 periods: r + gamma * (best * mask) == r + (gamma * best) * mask bit for bit, and everything else is shared"""
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    want, faults0, _ = fly(cfg, (nc.MAIN_PERIODS,), n=130)
    assert want["episodes"].min() >= 1 and (want["qa"] != 0).any() and ((want["qb"] != 0).any() or quirks != ec.Q_PAPER) and (want["pending_len"] == 0).all()
    got, faults1, _ = fly(cfg, (nc.MAIN_PERIODS,), n=130, nstep=1)
    ec.assert_equal(got, want, "n = 1 against n = 0")
    assert faults0 == 0 and faults1 == 0


def test_learner_is_independent_of_the_ensemble_size(main_runs):
    """70 learners equal the first 70 of 130"""
    quirks, dtype, nstep = nc.MAIN_ROWS[0]
    small, _, _ = main_runs(quirks, dtype, nstep)
    big, faults, _ = fly(training_config(0, quirks=quirks, dtype=dtype), (nc.MAIN_PERIODS,), n=130, nstep=nstep)
    first = list(range(L))
    ec.assert_equal(big, small, "the first 70 of 130 against 70", learners=(first, first))
    assert faults == 0


@pytest.mark.parametrize("level,quirks,dtype,nstep", nc.TRAINED_ROWS, ids=nc.TRAINED_IDS)
def test_trained_tables_70_learners_400_periods_and_7_plus_393(level, quirks, dtype, nstep):
    want, tables, ev = nc.trained_reference(level, quirks, dtype, nstep, L)
    cfg = training_config(level, quirks=quirks, dtype=dtype)
    kw = dict(ec.TRAINED_LEARNERS_CASE, seed=ec.TRAINED_LEARNERS_SEED, tables=tables, nstep=nstep)
    for runs in ((ec.TRAINED_LEARNERS_PERIODS,), ec.TRAINED_LEARNERS_SPLIT):
        got, faults, j = fly(cfg, runs, **kw)
        ec.assert_equal(got, want, f"trained tables, runs {runs}")
        assert faults == 0 and j == ec.TRAINED_LEARNERS_PERIODS


def test_launch_boundary_4096_plus_4():
    """one run of 4 100 periods (launches of 4 096 + 4) at n = 16, and again as run(4096); run(4): windows cross the boundary between launches"""
    n = 8
    want = nc.boundary_reference(n)  # asserts on the yardstick: a live learner with a non-empty window at period 4 096
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    kw = dict(nc.BOUNDARY_CASE, seed=nc.BOUNDARY_SEED, nstep=nc.BOUNDARY_N)
    for runs in ((nc.BOUNDARY_PERIODS,), (4096, 4)):
        got, faults, j = fly(cfg, runs, n=n, **kw)
        ec.assert_equal(got, want, f"runs {runs}")
        assert faults == 0 and j == nc.BOUNDARY_PERIODS


FREEZE = dict(eps=[1.0], window=4, min_successes=3, max_episodes=6)


def test_frozen_learners_have_empty_windows_and_set_level_discards_the_rest():
    """test_gpu_ensemble.py's freeze case at n = 5: level 0, eps = 1, window 4, 3 successes, 6 episodes, 64 learners, 350 periods — promoted, exhausted and
    flying learners side by side; then transfer(0, 1.0), set_level(1), which empties every window, and 100 more periods"""
    cfg, nstep = training_config(0, quirks=ec.Q_REFERENCE, dtype=F32), 5
    ref = nc.NstepReference(cfg, 64, 11, nstep, log_capacity=LOG_CAP, **FREEZE)
    ref.run(350)
    want = ref.result()
    promoted, frozen = want["promotion_episode"] >= 0, want["frozen"]
    print("promoted", int(promoted.sum()), "exhausted", int((frozen & ~promoted).sum()), "flying", int((~frozen).sum()), "windows", want["pending_len"].tolist())
    assert promoted.sum() >= 1 and (frozen & ~promoted).sum() >= 1 and (~frozen).sum() >= 1
    assert (want["pending_len"][frozen] == 0).all() and (want["pending_len"][~frozen] > 0).any()
    ens = make(training_config(0, quirks=ec.Q_REFERENCE, dtype=F32), 64, 11, nstep=nstep, **FREEZE)
    try:
        ens.run(350)
        got = nc.ensemble_result(ens)
        ec.assert_equal(got, want, "freeze")
        assert (got["pending_len"][got["frozen"]] == 0).all() and ens.nstep == nstep
        ref.transfer(0, 1.0); ref.set_level(1)
        ens.transfer(0, 1.0)
        assert (ens.pending_lengths() > 0).any(), "transfer leaves the windows alone"
        ens.set_level(1)
        assert (ens.pending_lengths() == 0).all() and (ref.pending_lengths() == 0).all()
        ref.run(100); ens.run(100)
        want1 = ref.result()
        assert (want1["decisions"] > want["decisions"]).all() and not want1["frozen"].any() and (want1["pending_len"] > 0).any()
        ec.assert_equal(nc.ensemble_result(ens), want1, "after transfer(0, 1.0), set_level(1) and 100 periods")
        assert ens.index_faults() == 0 and ens.period_index() == 450
    finally:
        ens.close()


# case (4) of DESIGN.md section 12 (tests/test_gpu_ensemble_long.py CURRICULUM) at n = 4
CURRICULUM = dict(n=24, seed=11, P=400, window=4, success_rate=0.5, max_episodes=6, nstep=4)


def test_curriculum_levels_0_to_4_with_nstep_4_equals_the_yardstick_driven_by_hand():
    c = CURRICULUM
    me = SimpleNamespace(_scale_modification_value=(0.8172650252856599, 0.8211253690681617, 0.8257273369742982, 0.8311571820651724))
    min_successes = ensemble.min_successes_for(c["window"], c["success_rate"])
    cfg = lambda: training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    ref = nc.NstepReference(cfg(), c["n"], c["seed"], c["nstep"], log_capacity=LOG_CAP)
    levels, open_at_set_level = [], 0
    for k in range(5):
        if k > 0:
            open_at_set_level += int((ref.pending_lengths() > 0).sum())
            ref.set_level(k)
        ref.set_schedules(ensemble.exploration_rates(k), c["window"], min_successes, c["max_episodes"])
        ref.run(c["P"])
        levels.append(ref.result())
        ref.transfer(k, float(Trainer.transfer_learning_ratio(me, k)))
    print("windows open when a level was left:", open_at_set_level, "events", dict(ref.events))
    assert open_at_set_level >= 1, "no window was discarded by set_level"
    assert ref.events["full_window_updates"] >= 1 and ref.events["short_flushes"] >= 1 and levels[0]["frozen"].any() and not levels[0]["frozen"].all()
    seen = []

    def on_level(ens, entry):
        k = entry["level"]
        ec.assert_equal(nc.ensemble_result(ens), levels[k], f"after level {k}")
        seen.append(k)

    ens = SequentialEnsemble(cfg(), c["n"], seed=c["seed"], log_capacity=LOG_CAP)
    try:
        ensemble.curriculum(ens, max_episodes=c["max_episodes"], max_periods_per_level=c["P"], window=c["window"], success_rate=c["success_rate"], on_level=on_level, nstep=c["nstep"])
        assert seen == [0, 1, 2, 3, 4] and ens.nstep == c["nstep"]
        for g, w, name in zip(ens.get_tables(), (ref.qa, ref.qb, ref.cnt), ("qa", "qb", "count")):
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), f"{name} after the last transfer"
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_refused_calls_say_why_change_nothing_and_a_good_call_follows():
    lib = _lib.load()
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    n_out = C.c_int32(-1)
    assert lib.dql_ensemble_set_nstep(None, 1) == _lib.EINVAL and lib.dql_ensemble_get_nstep(None, C.byref(n_out), None) == _lib.EINVAL
    want, _ = nc.main_reference(ec.Q_PAPER, F32, 3, L)
    ens = make(cfg)
    try:
        before = nc.ensemble_result(ens)
        assert ens.nstep == 0 and (ens.pending_lengths() == 0).all() and ens.pending_lengths().shape == (L,) and ens.pending_lengths().dtype == np.int32
        for bad in (-1, 17):
            assert lib.dql_ensemble_set_nstep(ens._h, bad) == _lib.EINVAL and b"0..16" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
            with pytest.raises(ValueError):
                ens.set_nstep(bad)
        assert lib.dql_ensemble_get_nstep(ens._h, None, None) == _lib.EINVAL
        # per-learner curriculum mode and n >= 1 refuse each other, in either order
        ens.set_curriculum(4, 64)
        assert lib.dql_ensemble_set_nstep(ens._h, 2) == _lib.EINVAL and b"curriculum" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        with pytest.raises(ValueError):
            ens.set_nstep(2)
        ens.set_curriculum(4, 0)
        ens.set_nstep(3)
        r = np.ascontiguousarray(ensemble.REFERENCE_RATIOS)
        assert lib.dql_ensemble_set_curriculum(ens._h, 4, 64, r.ctypes.data_as(C.c_void_p), 1) == _lib.EINVAL and b"n-step" in lib.dql_last_error()
        of = np.zeros(L, np.int32)
        assert lib.dql_ensemble_set_recipes(ens._h, 1, of.ctypes.data_as(C.c_void_p)) == _lib.EINVAL and b"n-step" in lib.dql_last_error()
        with pytest.raises(ValueError):
            ens.set_curriculum(4, 64)
        with pytest.raises(ValueError):
            ens.set_recipes([ensemble.Recipe()], of)
        assert ens.nstep == 3 and ens.period_index() == 0
        got = nc.ensemble_result(ens)
        ec.assert_equal(got, before, "after the refused calls")
        # windows open: n cannot change (DQL_ESTATE), and the state stays
        ens.run(7)
        assert (ens.pending_lengths() > 0).any()
        mid = nc.ensemble_result(ens)
        for other in (0, 1, 16):
            assert lib.dql_ensemble_set_nstep(ens._h, other) == _lib.ESTATE and b"pending window" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
            with pytest.raises(ValueError):
                ens.set_nstep(other)
        ens.set_nstep(3)  # no change: accepted
        assert ens.nstep == 3
        ec.assert_equal(nc.ensemble_result(ens), mid, "after the refused changes of n")
        # the good call that follows
        ens.run(293)
        ec.assert_equal(nc.ensemble_result(ens), want, "7 + 293 periods after the refusals")
        assert ens.index_faults() == 0
    finally:
        ens.close()
    teams = SequentialEnsemble(cfg, 8, seed=3, envs_per_learner=2)
    try:
        assert lib.dql_ensemble_set_nstep(teams._h, 2) == _lib.EINVAL and b"team" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        with pytest.raises(ValueError):
            teams.set_nstep(2)
        teams.set_nstep(0)
        assert teams.nstep == 0
    finally:
        teams.close()
    with pytest.raises(ValueError):
        SequentialEnsemble(cfg, 8, envs_per_learner=2, nstep=2)


def test_score_and_returns_map_read_the_resident_tables_of_an_nstep_ensemble():
    """the operators are unchanged: on an n-step ensemble they equal the same operators on its fetched tables (the new mode left the resident layout alone)"""
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ens = make(cfg, nstep=4)
    try:
        ens.run(nc.MAIN_PERIODS)
        qa, qb, _ = ens.get_tables()
        before = nc.ensemble_result(ens)
        assert (qa != 0).any() and (qb != 0).any() and (before["pending_len"] > 0).any()
        ev = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
        got, want = ens.score(ev, 64, seed=5, max_steps=120, log=True), ops.score(ev, qa, qb, 64, 5, max_steps=120, log=True)
        for k in ("by_code", "steps_sum", "ep_code", "ep_steps"):
            assert np.array_equal(got[k], want[k]), k
        assert want["by_code"].sum() > 0
        got, want = ens.returns_map(ev, 64, seed=5, eps=0.1, gamma=0.99, max_steps=120, count=16), ops.returns_map(ev, qa[:16], qb[:16], 64, 5, 0.1, 0.99, max_steps=120)
        for k in ("visits", "return_fx", "cut_decisions", "by_code", "steps_sum"):
            assert np.array_equal(got[k], want[k]), k
        assert want["visits"].sum() > 0
        ec.assert_equal(nc.ensemble_result(ens), before, "the ensemble after the operators")
    finally:
        ens.close()
