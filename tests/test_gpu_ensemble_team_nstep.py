"""Team learners with n-step Double-Q targets on the device (dql_ensemble_set_team_nstep / k_learn_team_nstep) against the yardstick of
tests/team_nstep_checks.py: `team_checks.TeamReference` with one pending window per env as a literal Python list and the update written out in Python floats.
Every comparison is `==`: all tables, counters, episode logs, promotion episodes, the state fields of all L * E envs and `team_pending_lengths`.  Each row first
asserts on the yardstick that the events it is there for occurred, pinned to the digit (team_nstep_checks.row_reference)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble, ops
from dql_multirotor_landing_amd.config import F32, F64, training_config
from dql_multirotor_landing_amd.ensemble import REFERENCE_RATIOS, Recipe, SequentialEnsemble
from dql_multirotor_landing_amd.trainer import Trainer

import ensemble_checks as ec
import nstep_checks as nc
import team_checks as tc
import team_nstep_checks as tn

pytestmark = pytest.mark.gpu


def make_row(name, dtype, nstep, learners=None):
    c = tc.CASES[name]
    n = c["L"] if learners is None else learners
    ens = SequentialEnsemble(tc.case_config(name, dtype), n, seed=tc.SEED, envs_per_learner=c["E"], team_nstep=nstep, **c["sched"])
    tables = tc.case_tables(name)
    if tables is not None:
        ens.set_tables(*(t[:n] for t in tables))
    return ens


@pytest.mark.parametrize("name,dtype,nstep", tn.ROWS, ids=tn.ROW_IDS)
def test_row_equals_the_yardstick(name, dtype, nstep):
    want, _, _ = tn.row_reference(name, dtype, nstep)
    c = tc.CASES[name]
    ens = make_row(name, dtype, nstep)
    try:
        assert ens.team_nstep == nstep and ens.nstep == 0 and (ens.pending_lengths() == 0).all() and ens.team_pending_lengths().shape == (c["L"] * c["E"],)
        ens.run(c["periods"])
        tc.assert_equal(tn.ensemble_result(ens), want, f"row {name} n {nstep}")
        assert ens.index_faults() == 0 and ens.period_index() == c["periods"] and ens.n_live() == int((~want["frozen"]).sum())
        assert ens.nstep == 0 and (ens.pending_lengths() == 0).all(), "the plain mode's windows are not the teams'"
    finally:
        ens.close()


@pytest.mark.parametrize("name,dtype", [("A", F32), ("B", F32), ("B", F64)], ids=["A-f32", "B-f32", "B-f64"])
def test_n_1_on_the_new_kernel_equals_n_0_on_k_learn_team(name, dtype):
    c = tc.CASES[name]
    one, zero = make_row(name, dtype, 1), make_row(name, dtype, 0)
    try:
        assert one.team_nstep == 1 and zero.team_nstep == 0
        one.run(c["periods"]); zero.run(c["periods"])
        want = ec.ensemble_result(zero)
        assert want["frozen"].any() and (want["qa"] != 0).any()
        got = tn.ensemble_result(one)
        assert (got.pop("team_pending_len") == 0).all()
        tc.assert_equal(got, want, f"n = 1 against k_learn_team, case {name}")
        assert one.index_faults() == 0
    finally:
        one.close(); zero.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("quirks,nstep", [(ec.Q_PAPER, 3), (ec.Q_BENCH, 16)], ids=["quirks-0x40-n3", "quirks-0x60-n16"])
def test_teams_of_one_equal_the_plain_nstep_ensemble(quirks, nstep, dtype):
    """130 learners, 300 periods: k_learn_team_nstep with E = 1 == k_learn_nstep"""
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    kw = dict(seed=nc.MAIN_SEED, log_capacity=nc.MAIN_LOG, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    plain, team = SequentialEnsemble(cfg, 130, nstep=nstep, **kw), SequentialEnsemble(cfg, 130, envs_per_learner=1, teams=True, team_nstep=nstep, **kw)
    try:
        plain.run(300); team.run(300)
        want = nc.ensemble_result(plain)
        assert want["episodes"].min() >= 1 and (want["qa"] != 0).any() and (want["pending_len"] > 0).any()
        got = tn.ensemble_result(team)
        got["pending_len"] = got.pop("team_pending_len")
        ec.assert_equal(got, want, "teams of one against k_learn_nstep")
        assert team.index_faults() == 0
    finally:
        plain.close(); team.close()


def test_launch_boundary_4096_plus_4():
    """one run of 4 100 periods (launches of 4 096 + 4) at n = 16, and again as run(4096); run(4): the envs' windows cross the boundary between launches"""
    b = tn.BOUNDARY
    want, cfg = tn.boundary_reference()  # asserts on the yardstick: a live team with open windows at period 4 096
    kw = dict(seed=tc.SEED, envs_per_learner=b["E"], team_nstep=b["nstep"], max_episodes=1 << 30, **b["sched"])
    a, c = SequentialEnsemble(cfg, b["L"], **kw), SequentialEnsemble(cfg, b["L"], **kw)
    try:
        a.run(b["periods"])
        c.run(4096); c.run(4)
        tc.assert_equal(tn.ensemble_result(a), want, "one run of 4100")
        tc.assert_equal(tn.ensemble_result(c), want, "4096 + 4")
        assert a.launches()[0] == 2 and a.index_faults() == 0 and c.index_faults() == 0
    finally:
        a.close(); c.close()


@pytest.mark.parametrize("name,nstep", [("A", 3), ("B", 16), ("C", 5), ("F", 8)])
def test_run_7_then_the_rest_equals_one_run(name, nstep):
    want, ev, _ = tn.row_reference(name, F32, nstep)
    p = tc.CASES[name]["periods"]
    assert ev["open_after_7"] == tc.CASES[name]["L"] * tc.CASES[name]["E"]
    one, two = make_row(name, F32, nstep), make_row(name, F32, nstep)
    try:
        one.run(p)
        two.run(tn.SPLIT)
        assert (two.team_pending_lengths() > 0).all()
        two.run(p - tn.SPLIT)
        got = tn.ensemble_result(two)
        tc.assert_equal(got, tn.ensemble_result(one), "7 + rest against one run, device against device")
        tc.assert_equal(got, want, "7 + rest against the yardstick")
    finally:
        one.close(); two.close()


def test_learners_are_independent_of_the_ensemble_size():
    """learners [0, 3) of row B-16 == an ensemble of 3 learners"""
    want, _, _ = tn.row_reference("B", F32, 16)
    E = tc.CASES["B"]["E"]
    ens = make_row("B", F32, 16, learners=3)
    try:
        ens.run(tc.CASES["B"]["periods"])
        got = tn.ensemble_result(ens)
        assert (got.pop("team_pending_len") == want["team_pending_len"][:3 * E]).all()
        tc.assert_equal(got, {k: v for k, v in want.items() if k != "team_pending_len"}, "row B n 16, three learners", learners=([0, 1, 2], [0, 1, 2]), envs_per_learner=E)
    finally:
        ens.close()


def test_freeze_rearm_transfer_set_level_and_a_second_level():
    """A-3 to the freeze (276 windows stay open in the five frozen teams), 20 periods frozen, a rearm after which the envs fly on with the windows they had,
    transfer(0), which leaves them alone, set_level(1), which empties all of them, then new schedules and 150 periods: each step against the yardstick"""
    ref = tn.make_reference("A", F32, 3)
    ens = make_row("A", F32, 3)
    try:
        ref.run(200); ens.run(200)
        w0 = ref.result()
        assert w0["frozen"].all() and int((w0["team_pending_len"] > 0).sum()) == 276
        tc.assert_equal(tn.ensemble_result(ens), w0, "level 0 to the freeze")
        ens.run(20); ref.run(20)  # frozen: nothing moves, the windows' lengths included
        tc.assert_equal(tn.ensemble_result(ens), w0, "20 periods with everyone frozen")
        before = dict(ref.events)
        ref.rearm(); ens.rearm()
        tc.assert_equal(tn.ensemble_result(ens), dict(ref.result()), "right after the rearm")
        ref.run(1); ens.run(1)
        assert ref.events["full_window_updates"] - before["full_window_updates"] == 273 and ref.events["flush_entries"] - before["flush_entries"] == 9
        tc.assert_equal(tn.ensemble_result(ens), ref.result(), "the first period after the rearm: updates out of the carried windows")
        ref.run(29); ens.run(29)
        w1 = ref.result()
        assert w1["frozen"].all() and int((w1["team_pending_len"] > 0).sum()) == 308
        tc.assert_equal(tn.ensemble_result(ens), w1, "re-armed, 30 periods")
        ref.transfer(0, REFERENCE_RATIOS[0]); ens.transfer(0, REFERENCE_RATIOS[0])
        tc.assert_equal(tn.ensemble_result(ens), ref.result(), "after transfer(0): the windows as they were")
        assert (ens.team_pending_lengths() == w1["team_pending_len"]).all()
        sched = dict(eps=[0.0], window=8, min_successes=2, max_episodes=30)
        ref.set_level(1); ens.set_level(1)
        assert (ens.team_pending_lengths() == 0).all() and (ref.pending_lengths() == 0).all()
        ref.set_schedules(**sched); ens.set_schedules(**sched)
        ref.run(150); ens.run(150)
        w2 = ref.result()
        assert (w2["episodes"] > w1["episodes"]).all() and (w2["team_pending_len"] > 0).any()
        tc.assert_equal(tn.ensemble_result(ens), w2, "after set_level(1) and 150 periods")
        assert ens.index_faults() == 0 and ens.period_index() == 400
    finally:
        ens.close()


CURRICULUM = dict(L=6, E=8, seed=11, P=150, window=4, success_rate=0.5, max_episodes=12, nstep=4, levels=3, log_capacity=64)


def test_curriculum_levels_0_to_2_with_team_nstep_4_equals_the_yardstick_driven_by_hand():
    c = CURRICULUM
    me = SimpleNamespace(_scale_modification_value=(0.8172650252856599, 0.8211253690681617, 0.8257273369742982, 0.8311571820651724))
    min_successes = ensemble.min_successes_for(c["window"], c["success_rate"])
    cfg = lambda: training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    ref = tn.TeamNstepReference(cfg(), c["L"], c["E"], c["seed"], c["nstep"], log_capacity=c["log_capacity"])
    levels, open_at_set_level = [], 0
    for k in range(c["levels"]):
        if k > 0:
            open_at_set_level += int((ref.pending_lengths() > 0).sum())
            ref.set_level(k)
        ref.set_schedules(ensemble.exploration_rates(k), c["window"], min_successes, c["max_episodes"])
        ref.run(c["P"])
        levels.append(ref.result())
        ref.transfer(k, float(Trainer.transfer_learning_ratio(me, k)))
    print("windows open when a level was left:", open_at_set_level, "events", dict(ref.events))
    assert open_at_set_level >= 1 and ref.events["full_window_updates"] >= 1 and ref.events["flush_entries"] >= 1 and levels[0]["frozen"].any()
    seen = []

    def on_level(ens, entry):
        k = entry["level"]
        tc.assert_equal(tn.ensemble_result(ens), levels[k], f"after level {k}")
        seen.append(k)

    ens = SequentialEnsemble(cfg(), c["L"], seed=c["seed"], log_capacity=c["log_capacity"], envs_per_learner=c["E"])
    try:
        ensemble.curriculum(ens, levels=c["levels"], max_episodes=c["max_episodes"], max_periods_per_level=c["P"], window=c["window"], success_rate=c["success_rate"],
                            on_level=on_level, team_nstep=c["nstep"])
        assert seen == [0, 1, 2] and ens.team_nstep == c["nstep"]
        for g, w, name in zip(ens.get_tables(), (ref.qa, ref.qb, ref.cnt), ("qa", "qb", "count")):
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), f"{name} after the last transfer"
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_refused_calls_say_why_change_nothing_and_a_good_call_follows():
    lib = _lib.load()
    n_out = C.c_int32(-1)
    assert lib.dql_ensemble_set_team_nstep(None, 1) == _lib.EINVAL and b"null" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
    assert lib.dql_ensemble_get_team_nstep(None, C.byref(n_out), None) == _lib.EINVAL
    want, _, _ = tn.row_reference("A", F32, 3)
    c = tc.CASES["A"]
    ens = make_row("A", F32, 0)
    try:
        before = tn.ensemble_result(ens)
        assert ens.team_nstep == 0 and (ens.team_pending_lengths() == 0).all() and ens.team_pending_lengths().dtype == np.int32
        for bad in (-1, 17):
            assert lib.dql_ensemble_set_team_nstep(ens._h, bad) == _lib.EINVAL and b"0..16" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
            with pytest.raises(ValueError):
                ens.set_team_nstep(bad)
        assert lib.dql_ensemble_get_team_nstep(ens._h, None, None) == _lib.EINVAL
        ens.set_team_nstep(3)
        # the plain mode's switch, per-learner curriculum and recipes stay refused on the team ensemble, word for word
        assert lib.dql_ensemble_set_nstep(ens._h, 2) == _lib.EINVAL and b"a team ensemble (dql_ensemble_create_teams) has the one-step update only; nothing was changed" in lib.dql_last_error()
        ratios = np.array(REFERENCE_RATIOS, np.float64)
        of = np.zeros(c["L"], np.int32)
        assert lib.dql_ensemble_set_curriculum(ens._h, 4, 256, ratios.ctypes.data_as(C.c_void_p), 1) == _lib.EINVAL and b"barrier mode only" in lib.dql_last_error()
        assert lib.dql_ensemble_set_recipes(ens._h, 1, of.ctypes.data_as(C.c_void_p)) == _lib.EINVAL and b"barrier mode only" in lib.dql_last_error()
        for call in (lambda: ens.set_nstep(2), lambda: ens.set_curriculum(4, 256), lambda: ens.set_recipes([Recipe()], of)):
            with pytest.raises(ValueError):
                call()
        assert ens.team_nstep == 3 and ens.nstep == 0 and ens.period_index() == 0
        tc.assert_equal(tn.ensemble_result(ens), before, "after the refused calls")
        # to the freeze: every team is frozen and 276 windows are open, so n cannot change (DQL_ESTATE), and the state stays
        ens.run(c["periods"])
        assert ens.n_live() == 0 and int((ens.team_pending_lengths() > 0).sum()) == 276
        tc.assert_equal(tn.ensemble_result(ens), want, "a good run after the refusals")
        for other in (0, 1, 16):
            assert lib.dql_ensemble_set_team_nstep(ens._h, other) == _lib.ESTATE
            msg = lib.dql_last_error()
            assert b"pending window" in msg and b"frozen is not enough" in msg and b"nothing was changed" in msg
            with pytest.raises(ValueError):
                ens.set_team_nstep(other)
        ens.set_team_nstep(3)  # no change: accepted
        assert ens.team_nstep == 3
        tc.assert_equal(tn.ensemble_result(ens), want, "after the refused changes of n")
        ens.set_level(0)  # empties every window: now n may change
        ens.set_team_nstep(0)
        assert ens.team_nstep == 0 and (ens.team_pending_lengths() == 0).all() and ens.index_faults() == 0
    finally:
        ens.close()
    plain = SequentialEnsemble(training_config(0, quirks=ec.Q_PAPER, dtype=F32), 8, seed=3)
    try:
        for n in (0, 2):
            assert lib.dql_ensemble_set_team_nstep(plain._h, n) == _lib.EINVAL and b"dql_ensemble_create_teams" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        with pytest.raises(ValueError):
            plain.set_team_nstep(2)
        assert lib.dql_ensemble_get_team_nstep(plain._h, C.byref(n_out), None) == _lib.OK and n_out.value == 0
    finally:
        plain.close()


def test_teams_of_one_refuse_team_nstep_with_curriculum_mode_and_recipes_in_either_order():
    """E = 1 is the one team shape that may enter per-learner curriculum mode and take recipes; those fly the one-step learners, so they and team_nstep >= 1
    refuse each other with a sentence and nothing changed, and the ensemble then flies as the plain n-step ensemble does"""
    lib = _lib.load()
    cfg = lambda: training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    kw = dict(seed=nc.MAIN_SEED, log_capacity=nc.MAIN_LOG, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    ratios = np.array(REFERENCE_RATIOS, np.float64)
    of = np.zeros(26, np.int32)
    ens = SequentialEnsemble(cfg(), 26, envs_per_learner=1, teams=True, team_nstep=3, **kw)
    try:
        before = tn.ensemble_result(ens)
        assert lib.dql_ensemble_set_curriculum(ens._h, 4, 64, ratios.ctypes.data_as(C.c_void_p), 1) == _lib.EINVAL
        assert b"dql_ensemble_set_curriculum: team n-step targets" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        assert lib.dql_ensemble_set_recipes(ens._h, 1, of.ctypes.data_as(C.c_void_p)) == _lib.EINVAL
        assert b"dql_ensemble_set_recipes: team n-step targets" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        for call in (lambda: ens.set_curriculum(4, 64), lambda: ens.set_recipes([Recipe()], of)):
            with pytest.raises(ValueError, match="barrier mode"):
                call()
        assert ens.team_nstep == 3 and ens.n_unfinished() == ens.n_live() == 26
        tc.assert_equal(tn.ensemble_result(ens), before, "after the refused calls")
        ens.run(nc.MAIN_PERIODS)  # the barrier mode, still on k_learn_team_nstep
        want, _ = nc.main_reference(ec.Q_PAPER, F32, 3, 26)
        got = tn.ensemble_result(ens)
        got["pending_len"] = got.pop("team_pending_len")
        ec.assert_equal(got, want, "E = 1, n = 3 after the refusals")
    finally:
        ens.close()
    ens = SequentialEnsemble(cfg(), 26, envs_per_learner=1, teams=True, **kw)
    try:
        ens.set_curriculum(4, 64)  # accepted: one env per learner
        assert lib.dql_ensemble_set_team_nstep(ens._h, 2) == _lib.EINVAL and b"curriculum mode" in lib.dql_last_error() and b"nothing was changed" in lib.dql_last_error()
        with pytest.raises(ValueError, match="barrier mode"):
            ens.set_team_nstep(2)
        ens.set_team_nstep(0)  # no n-step targets: accepted
        ens.set_recipes([Recipe()], of)
        assert lib.dql_ensemble_set_team_nstep(ens._h, 2) == _lib.EINVAL and b"recipes installed" in lib.dql_last_error()
        with pytest.raises(ValueError, match="barrier mode"):
            ens.set_team_nstep(2)
        ens.set_recipes([], None); ens.set_curriculum(4, 0)
        ens.set_team_nstep(2)  # both modes off again: accepted
        assert ens.team_nstep == 2 and ens.index_faults() == 0
    finally:
        ens.close()


def test_score_and_returns_map_read_the_resident_tables_of_a_team_nstep_ensemble():
    ens = make_row("F", F32, 8)
    try:
        ens.run(100)
        qa, qb, _ = ens.get_tables()
        before = tn.ensemble_result(ens)
        assert (before["team_pending_len"] > 0).any()
        ev = training_config(4, quirks=ec.Q_PAPER, dtype=F32)
        got, want = ens.score(ev, 64, seed=5, max_steps=300, log=True), ops.score(ev, qa, qb, 64, 5, max_steps=300, log=True)
        for k in ("by_code", "steps_sum", "ep_code", "ep_steps"):
            assert np.array_equal(got[k], want[k]), k
        assert want["by_code"].sum() > 0
        got, want = ens.returns_map(ev, 64, seed=5, eps=0.1, gamma=0.99, max_steps=120), ops.returns_map(ev, qa, qb, 64, 5, 0.1, 0.99, max_steps=120)
        for k in ("visits", "return_fx", "cut_decisions", "by_code", "steps_sum"):
            assert np.array_equal(got[k], want[k]), k
        assert want["visits"].sum() > 0
        tc.assert_equal(tn.ensemble_result(ens), before, "the ensemble after the operators")
    finally:
        ens.close()
