"""Team curriculum mode on the device (dql_ensemble_set_team_curriculum / k_learn_team_levels, k_learn_team_levels_nstep, k_ens_advance_teams; DESIGN.md section
29) against the yardstick of tests/team_levels_checks.py: one oracle per level, `team_checks.TeamReference`'s period, `team_nstep_checks.TeamNstepReference`'s
literal windows, emptied when the team advances.  Every comparison is `==`: tables, counters, ring, episode log, the state fields of all L * E envs, the history
arrays, the period index and the pending lengths.  Each case first asserts on the yardstick what it is there for (team_levels_checks.case_reference).  The
shapes are the smallest at which the lane map, the padding and the advance can go wrong: sixteen teams to a wave in three waves, one team to a wave, teams of
one, four teams to a wave with windows."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, F64
from dql_multirotor_landing_amd.ensemble import Recipe, SequentialEnsemble

import advance_checks as ac
import team_levels_checks as tl

pytestmark = pytest.mark.gpu

CHUNK = 100  # not a multiple of advance_every = 64


def dtype_of(name):
    return F64 if name == "N4" else F32


def fly(ens, periods, chunk=None):
    left = periods
    while left > 0:
        k = left if chunk is None else min(chunk, left)
        ens.run(k)
        left -= k


@pytest.mark.parametrize("name", list(tl.CASES))
def test_case_equals_the_yardstick(name):
    """E = 4, L = 40 (three waves at the start, sixteen teams per wave) in both transfer orders from trained tables; E = 64, L = 5 (one team per wave); E = 1,
    L = 70 with teams=True; E = 16, L = 9 with team_nstep 3 and 16; E = 4, L = 12, team_nstep 4 in float64.  All flown in calls of 100 periods."""
    c = tl.case(name)
    want, y = tl.case_reference(name, dtype_of(name))
    ens = tl.case_ensemble(name, dtype_of(name))
    try:
        assert ens.team_nstep == c["nstep"] and ens.n_unfinished() == c["L"]
        fly(ens, c["periods"], CHUNK)
        tl.assert_equal(tl.ensemble_result(ens), want, f"case {name}")
        assert ens.index_faults() == 0 and ens.period_index() == c["periods"] == y.j and ens.n_unfinished() == y.n_unfinished()
        launches, periods, wave_periods = ens.launches()
        tpw = 64 // c["E"]
        # a launch flies the live teams of its first period, regrouped: never more waves than the advance interval began with
        assert 0 < periods <= c["periods"] and 0 < wave_periods <= sum(sum(-(-q // tpw) for q in live) * min(c["every"], c["periods"] - j) for j, live, _ in y.launches)
        assert launches >= sum(1 for _, live, _ in y.launches if sum(live))
    finally:
        ens.close()


def test_one_run_equals_the_run_in_two_calls_and_in_chunks():
    c = tl.case("N16")
    want, _ = tl.case_reference("N16")
    one, two = tl.case_ensemble("N16"), tl.case_ensemble("N16")
    try:
        one.run(c["periods"])
        two.run(7); two.run(c["periods"] - 7)
        tl.assert_equal(tl.ensemble_result(one), want, "one run")
        tl.assert_equal(tl.ensemble_result(two), want, "7 + the rest")
        assert one.index_faults() == 0 and two.index_faults() == 0
        # one call cuts its launches at the advance points: the worklist carries the live teams only, so it never flies more waves than the barrier launch would
        launches, periods, wave_periods = one.launches()
        assert launches <= c["periods"] // c["every"] and wave_periods <= periods * -(-c["L"] * c["E"] // 64)
    finally:
        one.close(); two.close()


def test_teams_of_one_equal_per_learner_curriculum_mode():
    """E = 1 through the new mode (k_learn_team_levels, advance_team) `==` the same ensemble through dql_ensemble_set_curriculum (k_learn_levels, advance_learner)"""
    c = tl.case("E1")
    team = tl.case_ensemble("E1")
    solo = SequentialEnsemble(tl.case_config(c, F32), c["L"], seed=c["seed"], log_capacity=c["log_capacity"])
    try:
        for k, s in enumerate(tl.case_schedules(c)):
            solo.set_level_schedules(k, s["eps"], s["window"], s["min_successes"], s["max_episodes"])
        solo.set_curriculum(c["last_level"], c["every"], c["ratios"], c["advance_exhausted"])
        fly(team, c["periods"], CHUNK); fly(solo, c["periods"], CHUNK)
        want = ac.ensemble_result(solo)
        assert len(set(want["level"].tolist())) >= 3 and (want["qa"] != 0).any()
        got = tl.ensemble_result(team)
        assert (got.pop("team_pending_len") == 0).all()
        ac.assert_equal(got, want, "teams of one against per-learner curriculum mode")
        assert team.index_faults() == 0 and team.launches() == solo.launches() and team.n_unfinished() == solo.n_unfinished()
    finally:
        team.close(); solo.close()


def test_first_3_teams_do_not_depend_on_the_other_37():
    c = tl.case("E4")
    want, _ = tl.case_reference("E4")
    ens = tl.case_ensemble("E4", n=3)
    try:
        fly(ens, c["periods"], CHUNK)
        first = [0, 1, 2]
        assert len(set(want["level"][:3].tolist()) | set(np.nonzero(want["promoted_at"][:, :3] >= 0)[0].tolist())) >= 2
        tl.assert_equal(tl.ensemble_result(ens), want, "L = 3 against L = 40", teams=(first, first), envs_per_team=c["E"])
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_curriculum_per_team_equals_the_same_calls_made_by_hand():
    c = tl.case("N4")
    cfg = tl.case_config(c, F32)
    kw = dict(seed=c["seed"], log_capacity=c["log_capacity"], envs_per_learner=c["E"], max_episodes=3)
    driven, by_hand = SequentialEnsemble(cfg, c["L"], **kw), SequentialEnsemble(cfg, c["L"], **kw)
    try:
        chunks = []
        out = ensemble.curriculum_per_team(driven, last_level=3, advance_every=48, ratios=ac.TRAINED_RATIOS, advance_exhausted=True, transfer_order=ensemble.ORDER_PAPER,
                                           max_episodes=None, window=4, success_rate=0.5, chunk_periods=CHUNK, max_periods=350, on_chunk=lambda e, flown: chunks.append(flown),
                                           team_nstep=4)
        by_hand.set_team_nstep(4)
        for k in range(5):
            by_hand.set_level_schedules(k, ensemble.exploration_rates(k), 4, ensemble.min_successes_for(4, 0.5), 3)
        by_hand.set_team_curriculum(3, 48, ac.TRAINED_RATIOS, True, ensemble.ORDER_PAPER)
        flown = 0
        while by_hand.n_unfinished() > 0 and flown < 350:
            k = min(CHUNK, 350 - flown)
            by_hand.run(k)
            flown += k
        want = tl.ensemble_result(by_hand)
        assert out["periods"] == flown == chunks[-1] and chunks == sorted(chunks) and want["level"].max() == 3 and (want["level"] >= 1).all()
        tl.assert_equal(tl.ensemble_result(driven), want, "curriculum_per_team against the calls by hand")
        for k in tl.HISTORY:
            assert np.array_equal(out[k], want[k]), k
        assert driven.index_faults() == 0 and driven.team_nstep == 4
    finally:
        driven.close(); by_hand.close()


# ---- the refusals of dql_ensemble_set_team_curriculum, each with its own sentence, nothing changed ----
def refused(lib, rc, *words):
    assert rc == _lib.EINVAL, rc
    msg = lib.dql_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)
    assert "nothing was" in msg
    return msg


def p(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)


def test_refusals_each_with_its_sentence():
    c = tl.case("N4")
    lib = _lib.load()
    ratios = ensemble.REFERENCE_RATIOS
    plain = SequentialEnsemble(tl.case_config(c, F32), 4, seed=1)
    team = tl.case_ensemble("N4", n=4)  # mode on: last_level 4, advance_every 64, team_nstep 4
    one = SequentialEnsemble(tl.case_config(c, F32), 4, seed=1, envs_per_learner=1, teams=True)
    try:
        call = lambda e, last=4, every=64, r=ratios, exhausted=1, order=0: lib.dql_ensemble_set_team_curriculum(e._h, last, every, None if r is None else p(r), exhausted, order)
        sentences = {
            refused(lib, lib.dql_ensemble_set_team_curriculum(None, 4, 64, p(ratios), 1, 0), "null ensemble"),
            refused(lib, call(plain), "not made by dql_ensemble_create_teams"),
            refused(lib, call(team, every=-1), "advance_every must be in 0..4096"),
            refused(lib, call(team, every=4097), "advance_every must be in 0..4096"),
            refused(lib, call(team, r=None), "null ratios"),
            refused(lib, call(team, r=[1.0, 1.0, np.nan, 1.0, 1.0]), "ratios must be finite"),
            refused(lib, call(team, r=[1.0, np.inf, 1.0, 1.0, 1.0]), "ratios must be finite"),
            refused(lib, call(team, exhausted=2), "advance_exhausted must be 0 or 1"),
            refused(lib, call(team, order=2), "transfer_order must be 0"),
            refused(lib, call(team, order=-1), "transfer_order must be 0"),
            refused(lib, call(team, last=5), "last_level must lie between"),
        }
        # while the mode is on: the level is held to last_level, the per-learner mode and recipes are refused (E = 1: E > 1 is refused already)
        assert call(one, last=2) == _lib.OK
        refused(lib, lib.dql_ensemble_set_level(one._h, 3), "in team curriculum mode the level must not exceed last_level")
        sentences.add(refused(lib, lib.dql_ensemble_set_curriculum(one._h, 4, 64, p(ratios), 1), "dql_ensemble_set_curriculum", "team curriculum mode"))
        sentences.add(refused(lib, lib.dql_ensemble_set_recipes(one._h, 1, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p)), "dql_ensemble_set_recipes", "team curriculum mode"))
        with pytest.raises(ValueError):
            one.set_level(3)
        # last_level below a team's level; switching off while teams stand on different levels; a level on a team's way up without schedules
        one.set_level(2)
        sentences.add(refused(lib, call(one, last=1), "last_level must lie between"))
        assert call(one, every=0) == _lib.OK and one.n_unfinished() == 4  # everyone on the config's level: off, and n_unfinished is n_live again
        assert call(one, last=3) == _lib.OK
        assert lib.dql_ensemble_run(one._h, 10) == _lib.EINVAL
        assert "team curriculum mode needs dql_ensemble_set_level_schedules" in lib.dql_last_error().decode() and one.period_index() == 0 and one.launches()[0] == 0
        # the per-learner mode first: the team mode is refused (E = 1 only)
        assert call(one, every=0) == _lib.OK
        one.set_curriculum(4, 64)
        sentences.add(refused(lib, call(one), "per-learner curriculum mode"))
        one.set_curriculum(4, 0)
        # teams on different levels: fly the case until they are (on the yardstick: levels 1, 2, 2, 2 after 200 periods, every window open)
        team.run(200)
        before = tl.ensemble_result(team)
        tl.assert_equal(before, tl.case_reference("N4", F32, n=4, periods=200)[0], "the four teams after 200 periods")
        assert len(set(before["level"].tolist())) >= 2
        sentences.add(refused(lib, call(team, every=0), "teams stand on different levels"))
        sentences.add(refused(lib, call(team, last=int(before["level"].max()) - 1), "last_level must lie between"))
        assert len(sentences) == 12, sorted(sentences)
        tl.assert_equal(tl.ensemble_result(team), before, "after the refusals")
        # team_nstep in either order with the mode; its own rule is unchanged: open windows refuse a change of n
        assert (before["team_pending_len"] > 0).any()
        with pytest.raises(ValueError, match="pending window holds entries"):
            team.set_team_nstep(2)
        fresh = tl.case_ensemble("E4", n=3)
        try:
            fresh.set_team_nstep(5)   # after the mode
            fresh.run(70)
            assert fresh.team_nstep == 5 and (fresh.team_pending_lengths() > 0).any() and fresh.index_faults() == 0
        finally:
            fresh.close()
        # E > 1: the per-learner calls keep refusing with the sentences they always had, mode on or off
        for e in (team, SequentialEnsemble(tl.case_config(c, F32), 3, seed=1, envs_per_learner=4)):
            try:
                msg = refused(lib, lib.dql_ensemble_set_curriculum(e._h, 4, 64, p(ratios), 1), "dql_ensemble_set_curriculum")
                assert msg.endswith("an ensemble with more than one env per learner flies the barrier mode only (teams have no per-learner curriculum and no recipes); nothing was changed and nothing was launched")
                msg = refused(lib, lib.dql_ensemble_set_recipes(e._h, 1, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p)), "dql_ensemble_set_recipes")
                assert msg.endswith("an ensemble with more than one env per learner flies the barrier mode only (teams have no per-learner curriculum and no recipes); nothing was changed and nothing was launched")
                for driver in (lambda: ensemble.curriculum_per_learner(e), lambda: ensemble.curriculum_recipes(e, [Recipe()], np.zeros(e.n, np.int32)), lambda: e.set_curriculum(4, 64),
                               lambda: e.set_recipes([Recipe()], np.zeros(e.n, np.int32))):
                    with pytest.raises(ValueError, match="barrier mode only"):
                        driver()
            finally:
                if e is not team:
                    e.close()
    finally:
        plain.close(); team.close(); one.close()
