"""Refined learners on the device (dql_ensemble_set_refinement / k_learn_refined) against the yardstick of tests/refined_checks.py — the
unchanged oracle stepped with external actions, `oracle.agent_predict` / `oracle.agent_update` on per-learner tables of 2 * N_CELLS entries, the half read from
the oracle's fields before each step — and, with cut = +-inf, against the shipped plain kernel.  Every comparison is `==`: all tables, counters, episode logs,
promotion episodes and state fields.  The reference loops are flown once per module (refined_checks caches them)."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib
from dql_multirotor_landing_amd import ensemble as ens_mod
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import ensemble_checks as ec
import refined_checks as rc

pytestmark = pytest.mark.gpu
L, SEED, PERIODS, SPLIT, LOG_CAP = 70, 2024, 300, (7, 293), rc.LOG_CAP
F = rc.F
MAIN_FEATURES = ("pitch_sp", "coin", "obs_p_x", "obs_v_x", "obs_a_x", "mp_phase", "step", "prev_action")


def make(cfg, n=L, seed=SEED, eps=ec.EPS_TABLE, refine=None, tables=None, **kw):
    kw.setdefault("max_episodes", 1 << 30)
    ens = SequentialEnsemble(cfg, n, seed=seed, log_capacity=LOG_CAP, eps=eps, **kw)
    try:
        if refine is not None:
            ens.set_refinement(*refine)
        if tables is not None:
            ens.set_refined_tables(*tables)
    except Exception:
        ens.close()
        raise
    return ens


def fly(cfg, runs, refine, n=L, seed=SEED, tables=None, **kw):
    ens = make(cfg, n, seed, refine=refine, tables=tables, **kw)
    try:
        for r in runs:
            ens.run(r)
        return rc.refined_ensemble_result(ens), ens.index_faults(), ens.period_index(), ens.n_live()
    finally:
        ens.close()


@pytest.mark.parametrize("feature", MAIN_FEATURES)
@pytest.mark.parametrize("quirks", [ec.Q_REFERENCE, ec.Q_PAPER], ids=["quirks-0x7f", "quirks-0x40"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_main_parity_70_learners_from_zeros_300_periods_and_7_plus_293(dtype, quirks, feature):
    """one full wave and a 6-lane one; level 0, the eps table; one run of 300 periods and 7 + 293"""
    f = F[feature]
    want, ref, cut = rc.zeros_reference(dtype, quirks, f, L, SEED, PERIODS, watch=(SPLIT[0],))
    rc.assert_learner_events(ref, f"zeros {feature} {quirks:#x} dtype {dtype}")
    assert want["episodes"].min() >= 1 and (want["qa"][:, 0] != 0).any() and (want["qa"][:, 1] != 0).any()
    if f in rc.OBS_FEATURES:
        rc.assert_half_one_at_the_boundary(ref, SPLIT[0], feature)
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    for runs in ((PERIODS,), SPLIT):
        got, faults, j, _ = fly(cfg, runs, (feature, cut))
        ec.assert_equal(got, want, f"zeros {feature} runs {runs} dtype {dtype} quirks {quirks:#x}")
        assert faults == 0 and j == PERIODS


@pytest.mark.parametrize("feature", rc.FEATURES)
def test_trained_tables_70_learners_400_periods_and_7_plus_393(feature):
    """from `refined_trained_tables` (the halves disagree from the first decision on) at level 4 under quirks 0x40, greedy, window 4 / 2 successes / 6 episodes"""
    f = F[feature]
    want, ref, cut, tables = rc.trained_reference(F32, f, L)
    if f in rc.OBS_FEATURES:
        rc.assert_half_one_at_the_boundary(ref, ec.TRAINED_LEARNERS_SPLIT[0], feature)
    cfg = training_config(4, quirks=ec.Q_PAPER, dtype=F32)
    kw = {k: v for k, v in ec.TRAINED_LEARNERS_CASE.items() if k != "log_capacity"}
    assert ec.TRAINED_LEARNERS_CASE["log_capacity"] == LOG_CAP
    for runs in ((ec.TRAINED_LEARNERS_PERIODS,), ec.TRAINED_LEARNERS_SPLIT):
        got, faults, j, live = fly(cfg, runs, (feature, cut), seed=ec.TRAINED_LEARNERS_SEED, tables=tables, **kw)
        ec.assert_equal(got, want, f"trained {feature} runs {runs}")
        assert faults == 0 and j == ec.TRAINED_LEARNERS_PERIODS and live == int((~want["frozen"]).sum())


def test_pitch_sp_at_the_scalar_cut_zero_where_values_sit_on_the_cut():
    f = F["pitch_sp"]
    want, ref, _ = rc.zeros_reference(F32, ec.Q_PAPER, f, L, SEED, PERIODS, cut=0.0)
    wrong, _, _ = rc.zeros_reference(F32, ec.Q_PAPER, f, L, SEED, PERIODS, cut=0.0, strict=True)
    assert ref.ev["value_on_cut"] > 0 and any(not np.array_equal(want[k], wrong[k]) for k in rc.TABLE_FIELDS), "the case cannot tell `>` from `>=`"
    got, faults, _, _ = fly(training_config(0, quirks=ec.Q_PAPER, dtype=F32), SPLIT, ("pitch_sp", 0.0))
    ec.assert_equal(got, want, "pitch_sp at cut 0.0")
    assert faults == 0


def test_a_single_learner():
    f = F["pitch_sp"]
    want, _, cut = rc.zeros_reference(F32, ec.Q_PAPER, f, 1, SEED, PERIODS)
    got, faults, _, _ = fly(training_config(0, quirks=ec.Q_PAPER, dtype=F32), SPLIT, ("pitch_sp", cut), n=1)
    ec.assert_equal(got, want, "n = 1")
    assert faults == 0


# ---- properties against the shipped plain kernel, no reference loop: 130 learners x 300 periods ----
PATTERN = 0.5 + np.arange(N_CELLS) * 1e-3


@pytest.mark.parametrize("cut,used", [(np.inf, 0), (-np.inf, 1)], ids=["cut+inf", "cut-inf"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_an_infinite_cut_is_the_plain_ensemble_in_one_half_and_leaves_the_other(dtype, cut, used):
    n = 130
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=dtype)
    plain = SequentialEnsemble(cfg, n, seed=SEED, log_capacity=LOG_CAP, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    try:
        plain.run(7); plain.run(293)
        want = ec.ensemble_result(plain)
        assert plain.index_faults() == 0
    finally:
        plain.close()
    tables = [np.zeros((n, 2, N_CELLS)) for _ in range(3)]
    for t in tables:
        t[:, 1 - used] = PATTERN
    got, faults, j, _ = fly(cfg, SPLIT, ("obs_v_x", cut), n=n, tables=tables)
    for k in rc.TABLE_FIELDS:
        assert np.array_equal(got[k][:, 1 - used], np.tile(PATTERN, (n, 1))), f"{k}: the unused half lost its planted pattern"
        got[k] = got[k][:, used]
    ec.assert_equal(got, want, f"cut {cut} dtype {dtype}")
    assert faults == 0 and j == PERIODS


# ---- curriculum: levels 0 -> 2 through set_level / run(400) / transfer by hand, and through ensemble.curriculum ----
@pytest.mark.parametrize("feature", ["pitch_sp", "coin"])
def test_levels_0_to_2_with_transfer_by_hand(feature):
    want, cut = rc.curriculum_reference(F[feature])
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ens = make(cfg, rc.CURRICULUM_L, rc.CURRICULUM_SEED, eps=rc.CURRICULUM_EPS[0], refine=(feature, cut), **rc.CURRICULUM_RULE)
    try:
        for k in range(3):
            if k:
                ens.set_level(k)
                ens.set_schedules(eps=rc.CURRICULUM_EPS[k], **rc.CURRICULUM_RULE)
            ens.run(rc.CURRICULUM_PERIODS)
            if k < 2:
                ens.transfer(k, rc.CURRICULUM_RATIOS[k])
        ec.assert_equal(rc.refined_ensemble_result(ens), want, f"curriculum {feature}")
        assert ens.index_faults() == 0 and ens.period_index() == 3 * rc.CURRICULUM_PERIODS
    finally:
        ens.close()


def test_the_level_by_level_driver_walks_a_refined_ensemble_as_it_stands():
    """`ensemble.curriculum` over levels 0 and 1 on a refined ensemble at cut = +inf equals the same call on a plain one, half 0 against the plain tables"""
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    kw = dict(levels=2, max_episodes=4, max_periods_per_level=600, window=4, success_rate=0.4)
    plain = SequentialEnsemble(training_config(0, quirks=ec.Q_PAPER, dtype=F32), 70, seed=SEED, log_capacity=LOG_CAP)
    refined = make(cfg, 70, SEED, refine=("pitch_sp", np.inf))
    try:
        start = np.random.default_rng(3).normal(scale=0.01, size=(2, 70, N_CELLS))  # (transfer(0) copies level 4's block: from zeros nothing would be left to compare)
        plain.set_tables(start[0], start[1])
        planted = np.zeros((2, 70, 2, N_CELLS)); planted[:, :, 0] = start; planted[:, :, 1] = PATTERN
        refined.set_refined_tables(planted[0], planted[1])
        hp = ens_mod.curriculum(plain, **kw)
        hr = ens_mod.curriculum(refined, **kw)
        assert [h["periods"] for h in hp] == [h["periods"] for h in hr] and hp[0]["periods"] > 0
        want, got = ec.ensemble_result(plain), rc.refined_ensemble_result(refined)
        assert (want["qa"][:, :1134] != start[0][:, :1134]).any() and (want["qa"][:, :1134] != 0).any(), "the walk left levels 0 and 1 as they were"
        for k in rc.TABLE_FIELDS:
            if k != "count":  # half 1 is never flown: it keeps its pattern but for the two transfers' arithmetic on both halves
                assert np.array_equal(got[k][:, 1, 1134:], np.tile(PATTERN[1134:], (70, 1)))
            got[k] = got[k][:, 0]
        ec.assert_equal(got, want, "ensemble.curriculum, refined at +inf against plain")
        assert refined.index_faults() == 0
    finally:
        plain.close(); refined.close()


def test_freeze_and_rearm():
    """level 0, eps = 1, window 4, 3 successes, 6 episodes, 64 learners, 350 periods: promoted, exhausted and flying learners side by side; then
    transfer(0, 1.0), set_level(1) and 100 more periods"""
    f = F["obs_v_x"]
    cfg = training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    kw = dict(window=4, min_successes=3, max_episodes=6)
    cut = rc.mean_cut("C", f)
    ref = rc.RefinedReference(cfg, 64, 11, f, cut, eps=[1.0], log_capacity=LOG_CAP, **kw)
    ref.run(350)
    want = ref.result()
    promoted, frozen = want["promotion_episode"] >= 0, want["frozen"]
    print("promoted", int(promoted.sum()), "exhausted", int((frozen & ~promoted).sum()), "flying", int((~frozen).sum()))
    assert promoted.sum() >= 1 and (frozen & ~promoted).sum() >= 1 and (~frozen).sum() >= 1  # on the reference side: the case cannot pass vacuously
    ens = make(training_config(0, quirks=ec.Q_REFERENCE, dtype=F32), 64, 11, eps=[1.0], refine=("obs_v_x", cut), **kw)
    try:
        ens.run(350)
        ec.assert_equal(rc.refined_ensemble_result(ens), want, "freeze")
        assert ens.n_live() == int((~frozen).sum())
        ref.transfer(0, 1.0); ref.set_level(1); ref.run(100)
        ens.transfer(0, 1.0); ens.set_level(1); ens.run(100)
        want1 = ref.result()
        assert (want1["decisions"] > want["decisions"]).all() and not want1["frozen"].any()
        ec.assert_equal(rc.refined_ensemble_result(ens), want1, "after transfer(0, 1.0), set_level(1) and 100 periods")
        assert ens.index_faults() == 0 and ens.period_index() == 450
        ens.rearm()
        assert ens.n_live() == 64
    finally:
        ens.close()


def test_refined_table_round_trip_with_a_slice_and_transfer_of_both_halves():
    rng = np.random.default_rng(0)
    ens = make(training_config(0, dtype=F32), 5, refine=("coin", 0.5))
    try:
        assert ens.refinement()[0] == "coin" and np.array_equal(ens.refinement()[1], np.full(945, 0.5))
        for t in ens.get_refined_tables():
            assert t.shape == (5, 2, N_CELLS) and not t.any()
        qa, qb, cnt = rng.normal(size=(5, 2, N_CELLS)), rng.normal(size=(5, 2, N_CELLS)), rng.integers(0, 50, size=(5, 2, N_CELLS)).astype(np.float64)
        ens.set_refined_tables(qa, qb, cnt)
        for g, w in zip(ens.get_refined_tables(), (qa, qb, cnt)):
            assert np.array_equal(g, w)
        new = rng.normal(size=(2, 2, N_CELLS))
        ens.set_refined_tables(qb=new, first=2)
        want = qb.copy(); want[2:4] = new
        a, b, c = ens.get_refined_tables(first=3, count=2)
        assert np.array_equal(a, qa[3:5]) and np.array_equal(b, want[3:5]) and np.array_equal(c, cnt[3:5])
        ens.transfer(0, 0.5)  # dql_agent_transfer's arithmetic on BOTH halves, the k = 0 wrap included
        qa3, qb3, cnt3 = ens.get_refined_tables()
        per = N_CELLS // 5
        assert np.array_equal(qa3[:, :, :per], qa[:, :, 4 * per:] * 0.5) and np.array_equal(qb3[:, :, :per], want[:, :, 4 * per:] * 0.5)
        assert np.array_equal(qa3[:, :, per:], qa[:, :, per:]) and np.array_equal(cnt3, cnt)
    finally:
        ens.close()


def test_refusals_name_the_call_to_use_and_touch_nothing():
    lib = _lib.load()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    cfg = training_config(0, dtype=F32)
    cut = np.full(945, 0.25)
    err = lambda: lib.dql_last_error().decode()
    # set_refinement's own refusals: nothing is installed
    plain = make(cfg, 4)
    teams = SequentialEnsemble(cfg, 4, seed=SEED, teams=True)
    try:
        before = ec.ensemble_result(plain)
        bad = cut.copy(); bad[7] = np.nan
        for args, word in (((-1, p(cut)), "feature"), ((11, p(cut)), "feature"), ((4, None), "null"), ((4, p(bad)), "NaN")):
            assert lib.dql_ensemble_set_refinement(plain._h, *args) == _lib.EINVAL and word in err() and "nothing was changed" in err()
        assert lib.dql_ensemble_set_refinement(None, 4, p(cut)) == _lib.EINVAL
        assert lib.dql_ensemble_set_refinement(teams._h, 4, p(cut)) == _lib.EINVAL and "dql_ensemble_create" in err()
        for who, call in (("dql_ensemble_get_refined_tables", lambda: lib.dql_ensemble_get_refined_tables(plain._h, 0, 4, None, None, None)),
                          ("dql_ensemble_set_refined_tables", lambda: lib.dql_ensemble_set_refined_tables(plain._h, 0, 4, None, None, None)),
                          ("dql_ensemble_score_refined", lambda: lib.dql_ensemble_score_refined(plain._h, C.byref(cfg.to_c()), 0, 4, 64, 1, 1, 50, None, None, None, None))):
            assert call() == _lib.EINVAL and who in err() and "dql_ensemble_set_refinement" in err()
        f = C.c_int32(5)
        assert lib.dql_ensemble_get_refinement(plain._h, C.byref(f), None) == 0 and f.value == -1 and plain.refinement() is None
        plain.set_nstep(2)
        assert lib.dql_ensemble_set_refinement(plain._h, 4, p(cut)) == _lib.EINVAL and "n-step" in err()
        plain.set_nstep(0)
        plain.run(1)
        assert lib.dql_ensemble_set_refinement(plain._h, 4, p(cut)) == _lib.EINVAL and "period index 0" in err()
        for bad_call in (lambda: plain.set_refinement("no_such_feature", 0.0), lambda: plain.set_refinement("coin", np.zeros(7)), lambda: plain.set_refinement(4, bad)):
            with pytest.raises(ValueError):
                bad_call()
        assert plain.refinement() is None
        del before
    finally:
        plain.close(); teams.close()
    # a refined ensemble refuses what reads or writes the plain tables or installs another mode
    ens = make(cfg, 4, refine=("pitch_sp", cut))
    try:
        ens.run(40)
        before = rc.refined_ensemble_result(ens)
        c = cfg.to_c()
        buf, i64, u8, u16 = np.full((4, N_CELLS), 7.0), np.full(4 * 16, -3, np.int64), np.full(64 * 4, 9, np.uint8), np.full(64 * 4, 9, np.uint16)
        big = np.full(8, 5, np.uint32)
        ratios = np.array(ens_mod.REFERENCE_RATIOS)
        calls = {
            "dql_ensemble_get_tables": lambda: lib.dql_ensemble_get_tables(ens._h, 0, 4, p(buf), p(buf), p(buf)),
            "dql_ensemble_set_tables": lambda: lib.dql_ensemble_set_tables(ens._h, 0, 4, p(buf), None, None),
            "dql_ensemble_score": lambda: lib.dql_ensemble_score(ens._h, C.byref(c), 0, 4, 64, 1, 1, 50, p(i64), p(i64), p(u8), p(u16)),
            "dql_ensemble_score_map": lambda: lib.dql_ensemble_score_map(ens._h, C.byref(c), 0, 4, 64, 1, 1, 50, p(i64), p(i64), p(i64), p(u8), p(u16), p(u16)),
            "dql_ensemble_model": lambda: lib.dql_ensemble_model(ens._h, C.byref(c), 0, 1, 64, 1, 1, 50, 0.1, p(big), p(i64), p(i64), p(i64), p(i64)),
            "dql_ensemble_model_split": lambda: lib.dql_ensemble_model_split(ens._h, C.byref(c), 0, 1, 64, 1, 1, 50, 0.1, 4, p(cut), p(big), p(i64), p(i64), p(i64), p(i64), p(i64)),
            "dql_ensemble_returns": lambda: lib.dql_ensemble_returns(ens._h, C.byref(c), 0, 1, 64, 1, 1, 50, 0.1, 0.99, p(i64), p(i64), p(i64), p(i64), p(i64)),
            "dql_ensemble_score_grid": lambda: lib.dql_ensemble_score_grid(ens._h, C.byref(c), 1, 0, 4, 64, 1, 1, 50, p(i64), p(i64), None, None, None),
            "dql_ensemble_set_curriculum": lambda: lib.dql_ensemble_set_curriculum(ens._h, 4, 64, p(ratios), 1),
            "dql_ensemble_set_recipes": lambda: lib.dql_ensemble_set_recipes(ens._h, 1, p(np.zeros(4, np.int32))),
            "dql_ensemble_set_recipe": lambda: lib.dql_ensemble_set_recipe(ens._h, 0, 0x40, p(ratios), 5, 0.1, p(ratios), 4, 1, 0),
            "dql_ensemble_set_recipe_level_schedules": lambda: lib.dql_ensemble_set_recipe_level_schedules(ens._h, 0, 0, p(ratios), 1, 4, 2, 6),
            "dql_ensemble_set_recipe_nstep": lambda: lib.dql_ensemble_set_recipe_nstep(ens._h, 0, 2),
            "dql_ensemble_set_nstep": lambda: lib.dql_ensemble_set_nstep(ens._h, 2),
            "dql_ensemble_set_team_nstep": lambda: lib.dql_ensemble_set_team_nstep(ens._h, 2),
            "dql_ensemble_set_team_curriculum": lambda: lib.dql_ensemble_set_team_curriculum(ens._h, 4, 64, p(ratios), 1, 0),
        }
        for who, call in calls.items():
            assert call() == _lib.EINVAL, who
            msg = err()
            assert msg.startswith(who + ":") and "dql_ensemble_set_refinement" in msg and "nothing was launched" in msg and msg.rstrip().endswith("launched"), msg
            assert any(w in msg for w in ("dql_ensemble_get_refined_tables", "dql_ensemble_set_refined_tables", "dql_ensemble_score_refined", "dql_ensemble_set_schedules")), msg
        assert (buf == 7.0).all() and (i64 == -3).all() and (big == 5).all() and (u8 == 9).all() and (u16 == 9).all(), "a refused call touched an output"
        assert lib.dql_ensemble_set_refinement(ens._h, 4, p(cut)) == _lib.EINVAL and "already" in err()
        for bad_call in (ens.get_tables, lambda: ens.set_tables(qa=buf), lambda: ens.score(cfg), lambda: ens.set_nstep(2), lambda: ens.set_curriculum(4, 64)):
            with pytest.raises(ValueError):
                bad_call()
        ec.assert_equal(rc.refined_ensemble_result(ens), before, "after the refused calls")
        assert ens.period_index() == 40
        ens.run(10)  # a good call succeeds afterwards
        assert ens.period_index() == 50 and ens.index_faults() == 0
    finally:
        ens.close()
