"""The scoring operator on the device (dql_score / dql_ensemble_score, k_score) against a real Engine driven one agent period at a time: the equality contract
of include/dql.h — the m-th time env i shows FL_DONE, its code and step count are entry (m, k * envs + i) of the log, and by_code / steps_sum are the sums of
those entries.  Every comparison is ==."""
import ctypes as C
import time

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import F32, F64, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.engine import Engine
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import rollout_checks as rc
import score_checks as sc

pytestmark = pytest.mark.gpu
SEED, MAX_STEPS, EPISODES = 123, 900, 3
CASE_IDS = ["simulation-f32", "simulation-f64", "training4-f32", "simulation-two-axis-f32", "training0-per-env-platform-noise-f32"]
N_COLS = sc.N_CODES + 1


def stacked(sets):
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])


_YARDSTICKS = {}


def engine_yardsticks(case_id, n, max_steps, episodes=EPISODES):
    """the stepwise result of each of the three table sets on a real Engine, computed once per argument set and left unchanged"""
    key = (case_id, n, max_steps, episodes)
    if key not in _YARDSTICKS:
        out = []
        for t in rc.three_table_sets():
            eng = Engine(rc.case_config(case_id), n, seed=SEED)
            try:
                out.append(sc.stepwise_episodes(eng, t, max_steps, episodes))
            finally:
                eng.close()
        _YARDSTICKS[key] = out
    return _YARDSTICKS[key]


@pytest.mark.parametrize("n", [64, 192])
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_score_equals_the_stepwise_engine(case_id, n):
    """3 table sets, 3 episodes per env; 192 envs: three waves add into one row"""
    cfg = rc.case_config(case_id)
    want = engine_yardsticks(case_id, n, MAX_STEPS)
    print(case_id, n, [w["by_code"].tolist() for w in want], [w["steps_sum"] for w in want])
    assert sum(int(w["by_code"][:sc.UNFINISHED].sum()) for w in want) >= n * EPISODES and want[0]["by_code"].tolist() != want[1]["by_code"].tolist()
    timing = {}
    got = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=EPISODES, max_steps=MAX_STEPS, log=True, timing=timing)
    assert got["by_code"].shape == (3, N_COLS) and got["ep_code"].shape == (EPISODES, 3 * n) and got["columns"] == ops.SCORE_COLUMNS
    assert timing["instance"] == f"k_score<{'float' if cfg.dtype == F32 else 'double'}, 0, {0 if cfg.two_axis else 1}>" and timing["kernel_ms"] > 0.0
    for k, w in enumerate(want):
        sc.assert_set_equal(got, k, n, w, f"{case_id} n={n} table set {k}")
    nolog = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=EPISODES, max_steps=MAX_STEPS)
    assert nolog["ep_code"] is None and nolog["ep_steps"] is None
    assert np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-f64"])
def test_cut_off_counts_unfinished_episodes_and_leaves_their_log_entries_empty(case_id):
    """max_steps = 300: first episodes of the simulation flavour end around step 200, second ones cannot"""
    cfg = rc.case_config(case_id)
    n, cut = 192, 300
    want = engine_yardsticks(case_id, n, cut)
    w = want[0]
    finished, unfinished = int(w["by_code"][:sc.UNFINISHED].sum()), int(w["by_code"][sc.UNFINISHED])
    print(case_id, "cut at", cut, w["by_code"].tolist())
    assert finished >= n // 2 and unfinished >= n and (w["ep_code"][1] == sc.NO_CODE).any(), w["by_code"].tolist()
    got = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=EPISODES, max_steps=cut, log=True)
    for k, wk in enumerate(want):
        sc.assert_set_equal(got, k, n, wk, f"{case_id} cut at {cut}, table set {k}")
    assert (got["by_code"].sum(axis=1) == n * EPISODES).all()
    assert got["by_code"][0, sc.UNFINISHED] == unfinished == int((got["ep_code"][:, :n] == sc.NO_CODE).sum())
    assert ((got["ep_code"] == sc.NO_CODE) == (got["ep_steps"] == sc.NO_STEPS)).all()


@pytest.mark.parametrize("case_id", ["simulation-f32", "training4-f32", "simulation-two-axis-f32"])
def test_one_episode_per_env_equals_the_roll_out(case_id):
    cfg = rc.case_config(case_id)
    n = 256
    sets = rc.three_table_sets()
    for max_steps in (600, 200):
        ro = ops.rollout(cfg, sets, n, SEED, max_steps=max_steps)
        got = ops.score(cfg, *stacked(sets), n, SEED, episodes=1, max_steps=max_steps, log=True)
        fin = ro["code"] >= 0
        assert fin.any() and (max_steps == 600 or not fin.all())
        assert np.array_equal(got["ep_code"][0].reshape(3, n), np.where(fin, ro["code"], sc.NO_CODE).astype(np.uint8))
        assert np.array_equal(got["ep_steps"][0].reshape(3, n), np.where(fin, ro["steps"], sc.NO_STEPS).astype(np.uint16))
        for k in range(3):
            h = rc.histogram(ro["code"][k])
            assert got["by_code"][k].tolist() == [h[name] for name in ops.SCORE_COLUMNS]
            assert int(got["steps_sum"][k]) == int(ro["steps"][k][fin[k]].sum())
    # and the rates of one episode per env are landing_scores' figures
    r = evaluation.landing_rates(*stacked(sets), n_envs=n, episodes=1)
    s = evaluation.landing_scores([(t[0], t[1]) for t in sets], n_envs=n)
    assert r["touchdown_rate"].tolist() == [x["touchdown_rate"] for x in s] and r["goal_hold_rate"].tolist() == [x["goal_hold_rate"] for x in s]


def test_three_hundred_table_sets_repeat_the_rows_of_three():
    """table indexing beyond the roll-out's 16 sets and across the grid: set k is three_table_sets()[k % 3]"""
    cfg = rc.case_config("simulation-f32")
    n, K = 64, 300
    sets = rc.three_table_sets()
    three = ops.score(cfg, *stacked(sets), n, SEED, episodes=EPISODES, max_steps=MAX_STEPS, log=True)
    assert len({tuple(r) for r in three["by_code"].tolist()}) >= 2
    big = ops.score(cfg, *stacked([sets[k % 3] for k in range(K)]), n, SEED, episodes=EPISODES, max_steps=MAX_STEPS, log=True)
    assert big["by_code"].shape == (K, N_COLS) and big["ep_code"].shape == (EPISODES, K * n)
    idx = np.arange(K) % 3
    assert np.array_equal(big["by_code"], three["by_code"][idx]) and np.array_equal(big["steps_sum"], three["steps_sum"][idx])
    assert np.array_equal(big["ep_code"].reshape(EPISODES, K, n), three["ep_code"].reshape(EPISODES, 3, n)[:, idx])
    assert np.array_equal(big["ep_steps"].reshape(EPISODES, K, n), three["ep_steps"].reshape(EPISODES, 3, n)[:, idx])


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-f64"])
def test_sixty_four_unfinished_episodes_per_lane_set_the_highest_plane_of_the_count(case_id):
    """64 episodes per env, cut at max_steps = 5: no episode ends in 6 periods, so every lane reports 64 unfinished episodes — bit 6 of the per-lane count,
    the highest of the 7 planes the wave's sum is taken over"""
    cfg = rc.case_config(case_id)
    n, episodes, cut = 64, ops.SCORE_MAX_EPISODES, 5
    want = engine_yardsticks(case_id, n, cut, episodes)
    for w in want:  # on the stepwise Engine: nothing finished
        assert w["by_code"][sc.UNFINISHED] == n * episodes and w["by_code"][:sc.UNFINISHED].sum() == 0 and w["steps_sum"] == 0
    got = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=episodes, max_steps=cut, log=True)
    for k, w in enumerate(want):
        sc.assert_set_equal(got, k, n, w, f"{case_id}, 64 unfinished episodes per lane, table set {k}")
    assert (got["by_code"][:, sc.UNFINISHED] == n * episodes).all() and (got["by_code"][:, :sc.UNFINISHED] == 0).all() and (got["steps_sum"] == 0).all()
    assert (got["ep_code"] == sc.NO_CODE).all() and (got["ep_steps"] == sc.NO_STEPS).all()
    nolog = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=episodes, max_steps=cut)
    assert np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])


def test_a_long_score_sets_every_plane_of_the_lane_sums():
    """64 episodes per env within 4 096 periods, the reference's tables, `training4-f32`: per lane 26 - 37 episodes stay unfinished and the finished ones add
    up to 3 805 - 4 070 steps, so planes 0 - 5 of `unfinished` and 0 - 11 of `lane_steps` all carry a set bit in some lane (asserted on the stepwise Engine).
    `simulation-f32`, the case of the other tests here, leaves 41 - 44 episodes unfinished per lane and never sets bit 4; plane 12 of `lane_steps` needs a sum of
    4 096 steps, which max_steps <= 4 096 with a reset period per episode cannot give."""
    case_id, n, episodes, max_steps = "training4-f32", 64, ops.SCORE_MAX_EPISODES, 4096
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    t0 = time.perf_counter()
    eng = Engine(cfg, n, seed=SEED)
    try:
        want = sc.stepwise_episodes(eng, tables, max_steps, episodes)
    finally:
        eng.close()
    print(f"stepwise Engine, {max_steps + 1} periods: {time.perf_counter() - t0:.2f} s")
    unfinished, steps = sc.lane_sums(want)
    print("unfinished per lane", int(unfinished.min()), "..", int(unfinished.max()), "steps per lane", int(steps.min()), "..", int(steps.max()), want["by_code"].tolist())
    assert int(np.bitwise_or.reduce(unfinished)) & 0x3f == 0x3f, sorted(set(unfinished.tolist()))
    assert int(np.bitwise_or.reduce(steps)) & 0xfff == 0xfff and steps.max() < 1 << 13
    got = ops.score(cfg, tables[0][None], tables[1][None], n, SEED, episodes=episodes, max_steps=max_steps, log=True)
    sc.assert_set_equal(got, 0, n, want, f"{case_id}, {episodes} episodes within {max_steps} periods")
    nolog = ops.score(cfg, tables[0][None], tables[1][None], n, SEED, episodes=episodes, max_steps=max_steps)
    assert nolog["ep_code"] is None and np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])


def ensemble_snapshot(ens):
    qa, qb, cnt = ens.get_tables()
    c = ens.counters()
    st = ens.state()
    return {"qa": qa, "qb": qb, "count": cnt, "period": np.array(ens.period_index()), **{f"c_{k}": np.asarray(v) for k, v in c.items()}, **{f"s_{k}": v for k, v in st.items()}}


def assert_snapshots_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def test_ensemble_is_scored_where_it_lives_and_left_as_it_was():
    L, n = 130, 64
    train = training_config(0, quirks=Q_PAPER, dtype=F32)
    sets = rc.three_table_sets()

    def trained(periods_a, periods_b, score_between):
        ens = SequentialEnsemble(train, L, seed=7)
        try:
            ens.run(periods_a)
            before = ensemble_snapshot(ens) if score_between else None
            if score_between:
                ens.score(simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), n, SEED, episodes=2, max_steps=500, log=True)
                assert_snapshots_equal(ensemble_snapshot(ens), before, "right after the score")
            if periods_b:
                ens.run(periods_b)
            return ensemble_snapshot(ens), ens.index_faults()
        finally:
            ens.close()

    whole, faults_w = trained(300, 0, False)
    split, faults_s = trained(150, 150, True)
    assert_snapshots_equal(split, whole, "run(150); score; run(150) against run(300)")
    assert faults_w == 0 and faults_s == 0 and int(whole["period"]) == 300 and whole["c_decisions"].sum() > 0

    ens = SequentialEnsemble(train, L, seed=7)
    try:
        ens.run(300)
        for first, t in ((0, sets[0]), (63, sets[2]), (64, sets[0]), (129, sets[2])):  # both sides of the second wave's first learner, and the last learner
            ens.set_tables(t[0], t[1], first=first)
        qa, qb, _ = ens.get_tables()
        assert np.array_equal(qa[64], sets[0][0])
        for eval_cfg in (simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), training_config(4, quirks=Q_PAPER, dtype=F64)):
            want = ops.score(eval_cfg, qa, qb, n, SEED, episodes=2, max_steps=500, log=True)
            got = ens.score(eval_cfg, n, SEED, episodes=2, max_steps=500, log=True)
            assert want["by_code"][64].tolist() != want["by_code"][65].tolist(), "neighbouring learners must fly differently for the slice to show an offset"
            for f in ("by_code", "steps_sum", "ep_code", "ep_steps"):
                assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
            part = ens.score(eval_cfg, n, SEED, episodes=2, max_steps=500, log=True, first=64, count=66)
            assert np.array_equal(part["by_code"], want["by_code"][64:130]) and np.array_equal(part["steps_sum"], want["steps_sum"][64:130])
            assert np.array_equal(part["ep_code"], want["ep_code"][:, 64 * n:130 * n]) and np.array_equal(part["ep_steps"], want["ep_steps"][:, 64 * n:130 * n])
        r = ens.landing_rates(n_envs=n, episodes=1)
        w = evaluation.landing_rates(qa, qb, n_envs=n, episodes=1)
        assert np.array_equal(r["touchdown_rate"], w["touchdown_rate"]) and np.array_equal(r["goal_hold_rate"], w["goal_hold_rate"]) and r["touchdown_rate"].shape == (L,)
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """each refusal returns DQL_EINVAL with a dql_last_error text that says nothing was launched, leaves the output arrays untouched, and the latest-kernel
    record (dql_diag_score_last) still describes the good call made before"""
    lib = _lib.load()
    cfg = rc.case_config("simulation-f32")
    n = 64
    qa, qb = (np.ascontiguousarray(t) for t in rc.stage4_tables())
    good = ops.score(cfg, qa, qb, n, SEED, episodes=2, max_steps=5, log=True, timing={})
    assert good["by_code"][0, sc.UNFINISHED] == 2 * n and (good["ep_code"] == sc.NO_CODE).all()
    ms0, inst = C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_score_last(C.byref(ms0), inst) == 0 and list(inst) == [4, 0, 1]
    c = cfg.to_c()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    by_code = np.full((2, N_COLS), sentinel, np.int64); steps_sum = np.full(2, sentinel, np.int64)
    ep_code = np.full((2, 2 * n), sentinel, np.uint8); ep_steps = np.full((2, 2 * n), sentinel, np.uint16)

    def untouched():
        return (by_code == sentinel).all() and (steps_sum == sentinel).all() and (ep_code == sentinel).all() and (ep_steps == sentinel).all()

    def call(n_tables=1, envs=n, episodes=2, max_steps=5, qa_=qa, qb_=qb, by_code_=by_code, steps_sum_=steps_sum, ep_code_=ep_code, ep_steps_=ep_steps):
        return lib.dql_score(C.byref(c), 0, n_tables, envs, episodes, SEED, max_steps, ptr(qa_), ptr(qb_), ptr(by_code_), ptr(steps_sum_), ptr(ep_code_), ptr(ep_steps_))

    refused = {
        "n_tables 0": dict(n_tables=0), "n_tables 2^20 + 1": dict(n_tables=(1 << 20) + 1),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100), "2^31 lanes": dict(n_tables=1 << 20, envs=2048),
        "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
        "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
        "log code without steps": dict(ep_steps_=None), "log steps without code": dict(ep_code_=None),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None),
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_score" in msg and "nothing was launched" in msg, f"{what}: {msg!r}"
        assert untouched(), what
        ms1 = C.c_double()
        assert lib.dql_diag_score_last(C.byref(ms1), inst) == 0 and ms1.value == ms0.value, what
    bad_cfg = rc.case_config("simulation-f32")
    bad_cfg.working_curriculum_step = 9  # check_config applies as in dql_create
    cb = bad_cfg.to_c()
    assert lib.dql_score(C.byref(cb), 0, 1, n, 2, SEED, 5, ptr(qa), ptr(qb), ptr(by_code), ptr(steps_sum), None, None) == _lib.EINVAL and untouched()
    with pytest.raises(ValueError):
        ops.score(cfg, qa, qb, 100, SEED)

    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), 130, seed=7)
    try:
        def ecall(first=0, count=2, envs=n, episodes=2, max_steps=5, cfg_=c, by_code_=by_code, steps_sum_=steps_sum, ep_code_=ep_code, ep_steps_=ep_steps):
            return lib.dql_ensemble_score(ens._h, C.byref(cfg_), first, count, envs, episodes, SEED, max_steps, ptr(by_code_), ptr(steps_sum_), ptr(ep_code_), ptr(ep_steps_))

        erefused = {
            "count 0": dict(count=0), "first -1": dict(first=-1), "slice beyond the end": dict(first=129, count=2), "first beyond the end": dict(first=131, count=1),
            "envs 0": dict(envs=0), "envs 100": dict(envs=100), "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
            "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
            "log code without steps": dict(ep_steps_=None), "log steps without code": dict(ep_code_=None),
            "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None), "bad config": dict(cfg_=cb),
        }
        for what, kw in erefused.items():
            rcode = ecall(**kw)
            msg = lib.dql_last_error().decode()
            assert rcode == _lib.EINVAL, f"ensemble, {what}: returned {rcode}"
            assert what == "bad config" or ("dql_ensemble_score" in msg and "nothing was launched" in msg), f"ensemble, {what}: {msg!r}"
            assert untouched(), what
            ms1 = C.c_double()
            assert lib.dql_diag_score_last(C.byref(ms1), inst) == 0 and ms1.value == ms0.value, what
        assert lib.dql_ensemble_score(None, C.byref(c), 0, 1, n, 2, SEED, 5, ptr(by_code), ptr(steps_sum), None, None) == _lib.EINVAL and untouched()
        with pytest.raises(ValueError):
            ens.score(cfg, n, SEED, first=129, count=2)
        assert ecall() == 0 and not untouched() and (by_code.sum(axis=1) == 2 * n).all()  # and the same arguments, well-formed, do run
    finally:
        ens.close()
    by_code[:] = sentinel
    assert call() == 0 and np.array_equal(by_code[0], good["by_code"][0]) and np.array_equal(ep_code[:, :n], good["ep_code"])
