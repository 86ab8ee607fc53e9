"""Learners with teams of envs on the device (dql_ensemble_create_teams / k_learn_team) against the reference loop of tests/team_checks.py — the unchanged oracle
stepped with external actions, `oracle.agent_predict` before the step and `oracle.agent_update` for a learner's envs in ascending order after it, the freeze
rules on a literal deque.  Every comparison is `==`: all tables, counters, episode logs, promotion episodes and the state fields of all L * E envs.  Each case
first asserts on the reference that the events it is there for occurred (team_checks.case_reference)."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, training_config
from dql_multirotor_landing_amd.ensemble import (REFERENCE_RATIOS, Recipe, SequentialEnsemble, curriculum_per_learner, curriculum_recipes)

import ensemble_checks as ec
import team_checks as tc

pytestmark = pytest.mark.gpu


def make_case(name, dtype, learners=None):
    c = tc.CASES[name]
    n = c["L"] if learners is None else learners
    ens = SequentialEnsemble(tc.case_config(name, dtype), n, seed=tc.SEED, envs_per_learner=c["E"], **c["sched"])
    tables = tc.case_tables(name)
    if tables is not None:
        ens.set_tables(*(t[:n] for t in tables))
    return ens


@pytest.mark.parametrize("name,dtype", tc.CASE_IDS, ids=[f"{n}-{'f64' if d == F64 else 'f32'}" for n, d in tc.CASE_IDS])
def test_case_equals_the_team_reference(name, dtype):
    want, _ = tc.case_reference(name, dtype)
    c = tc.CASES[name]
    ens = make_case(name, dtype)
    try:
        assert ens.envs_per_learner == c["E"] and ens.state()["idx_x"].shape == (c["L"] * c["E"],)
        ens.run(c["periods"])
        tc.assert_equal(ec.ensemble_result(ens), want, f"case {name}")
        assert ens.index_faults() == 0 and ens.period_index() == c["periods"] and ens.n_live() == int((~want["frozen"]).sum())
    finally:
        ens.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_teams_of_one_equal_the_plain_ensemble(dtype):
    """130 learners, 300 periods (tests/test_gpu_ensemble.py's main case): k_learn_team with E = 1 == k_learn"""
    cfg = training_config(0, quirks=ec.Q_REFERENCE, dtype=dtype)
    kw = dict(seed=2024, log_capacity=32, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    plain, team = SequentialEnsemble(cfg, 130, **kw), SequentialEnsemble(cfg, 130, envs_per_learner=1, teams=True, **kw)
    try:
        v = C.c_int32(-1)
        _lib.check(team.lib.dql_ensemble_envs_per_learner(team._h, C.byref(v)))
        assert v.value == 1 and team.teams and not plain.teams
        plain.run(300); team.run(300)
        want = ec.ensemble_result(plain)
        assert want["episodes"].min() >= 1 and (want["qa"] != 0).any()
        ec.assert_equal(ec.ensemble_result(team), want, "teams of one against k_learn")
        assert team.index_faults() == 0
    finally:
        plain.close(); team.close()


def test_run_7_then_4093_equals_run_4100():
    """device against device across the launch boundary at 4 096 periods: case A with a budget that keeps learners live beyond it"""
    c = tc.CASES["A"]
    sched = dict(c["sched"], window=100, min_successes=97, max_episodes=1 << 30)
    cfg = tc.case_config("A", F32)
    a, b = (SequentialEnsemble(cfg, c["L"], seed=tc.SEED, envs_per_learner=c["E"], **sched) for _ in range(2))
    try:
        a.run(4100)
        b.run(7); b.run(4093)
        want = ec.ensemble_result(a)
        assert not want["frozen"].all() and want["episodes"].min() > 100, "learners must be live across the launch boundary"
        ec.assert_equal(ec.ensemble_result(b), want, "7 + 4093 against 4100")
        assert a.index_faults() == 0 and b.index_faults() == 0 and a.period_index() == b.period_index() == 4100
    finally:
        a.close(); b.close()


def test_learners_are_independent_of_the_ensemble_size():
    """learners [0, 3) of case B == an ensemble of 3 learners"""
    want, _ = tc.case_reference("B", F32)
    ens = make_case("B", F32, learners=3)
    try:
        ens.run(tc.CASES["B"]["periods"])
        tc.assert_equal(ec.ensemble_result(ens), want, "case B, three learners", learners=([0, 1, 2], [0, 1, 2]), envs_per_learner=tc.CASES["B"]["E"])
    finally:
        ens.close()


def test_freeze_rearm_set_level_transfer_and_a_second_level():
    """case A to its end (all five learners frozen, their 64 envs each left as they were), a re-armed second round on level 0, then transfer(0), set_level(1) and
    a level-1 round, each against the reference"""
    c = tc.CASES["A"]
    ref = tc.TeamReference(tc.case_config("A", F32), c["L"], c["E"], tc.SEED, **c["sched"])
    ens = make_case("A", F32)
    try:
        ref.run(200); ens.run(200)
        w0 = ref.result()
        assert w0["frozen"].all()
        tc.assert_equal(ec.ensemble_result(ens), w0, "level 0")
        ens.run(20)  # frozen: nothing moves
        tc.assert_equal(ec.ensemble_result(ens), w0, "20 periods with everyone frozen")
        ref.run(20)
        ref.rearm(); ens.rearm()
        ref.run(30); ens.run(30)
        w1 = ref.result()
        assert (w1["decisions"] > w0["decisions"]).all()
        tc.assert_equal(ec.ensemble_result(ens), w1, "re-armed, 30 periods")
        sched = dict(eps=[0.0], window=8, min_successes=2, max_episodes=30)
        ref.transfer(0, REFERENCE_RATIOS[0]); ref.set_level(1); ref.set_schedules(**sched)
        ens.transfer(0, REFERENCE_RATIOS[0]); ens.set_level(1); ens.set_schedules(**sched)
        ref.run(150); ens.run(150)
        w2 = ref.result()
        assert (w2["episodes"] > w1["episodes"]).all() and (w2["level_episodes"] <= w2["episodes"]).all() and ref.events["same_cell"] > 0
        tc.assert_equal(ec.ensemble_result(ens), w2, "after transfer(0), set_level(1) and 150 periods")
        assert ens.index_faults() == 0 and ens.period_index() == 400
    finally:
        ens.close()


def test_score_on_a_team_ensemble_equals_ops_score_on_its_tables():
    ens = make_case("F", F32)
    try:
        ens.run(100)
        eval_cfg = training_config(4, quirks=ec.Q_PAPER, dtype=F32)
        got = ens.score(eval_cfg, envs_per_learner=64, seed=5, max_steps=300)
        qa, qb, _ = ens.get_tables()
        want = ops.score(eval_cfg, qa, qb, envs_per_table=64, seed=5, max_steps=300)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    finally:
        ens.close()


def test_refusals_then_the_ensemble_flies_on_as_the_reference_says():
    cfg = tc.case_config("F", F32)
    c = tc.CASES["F"]
    h = C.c_void_p()
    lib = _lib.load()
    cc = cfg.to_c()
    for n, e in ((9, 3), (9, 0), (9, 128), (0, 8), ((1 << 20) // 8 + 1, 8)):
        assert lib.dql_ensemble_create_teams(C.byref(cc), 0, n, e, 1, 0, C.byref(h)) == _lib.EINVAL and not h.value, (n, e)
    c2 = training_config(4, dtype=F32, two_axis=1).to_c()
    assert lib.dql_ensemble_create_teams(C.byref(c2), 0, 9, 8, 1, 0, C.byref(h)) == _lib.EINVAL and not h.value
    ens = make_case("F", F32)
    try:
        ens.run(50)
        ratios = np.array(REFERENCE_RATIOS, np.float64)
        of = np.zeros(c["L"], np.int32)
        for refused in (lambda: lib.dql_ensemble_set_curriculum(ens._h, 4, 256, ratios.ctypes.data_as(C.c_void_p), 1), lambda: lib.dql_ensemble_set_curriculum(ens._h, 4, 0, None, 1),
                        lambda: lib.dql_ensemble_set_recipes(ens._h, 1, of.ctypes.data_as(C.c_void_p)), lambda: lib.dql_ensemble_set_recipes(ens._h, 0, None)):
            assert refused() == _lib.EINVAL and "barrier mode only" in lib.dql_last_error().decode()
        for call in (lambda: curriculum_per_learner(ens), lambda: curriculum_recipes(ens, [Recipe()], of), lambda: ens.set_curriculum(4, 256), lambda: ens.set_recipes([Recipe()], of)):
            with pytest.raises(ValueError, match="barrier mode only"):
                call()
        assert ens.n_unfinished() == ens.n_live()
        ens.run(c["periods"] - 50)
        tc.assert_equal(ec.ensemble_result(ens), tc.case_reference("F", F32)[0], "case F after the refusals")
        assert ens.index_faults() == 0
    finally:
        ens.close()
