"""The mapping scorer on the device (dql_score_map / dql_ensemble_score_map, k_score_map) against a real Engine driven one agent period at a time: the contract
of include/dql.h — an env that has episodes left adds 1 per non-reset period at the cell (index after the previous period) * 3 + action, for both axes where
there are two, and the log holds the cells of each episode's last decision.  Every comparison is ==.  The yardstick (tests/map_checks.py) also counts the events
a kernel can get wrong, and every case asserts on it first that they occurred: 64 lanes adding to one histogram at once, decisions in the flush's partial last
sweep (cells >= 2 816), unfinished episodes, lanes that stop early, reset periods, x and y cells that differ."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.engine import Engine
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import map_checks as mc
import rollout_checks as rc
import score_checks as sc

pytestmark = pytest.mark.gpu
SEED, MAX_STEPS, EPISODES = 123, 900, 3
CASE_IDS = ["simulation-f32", "training4-f64", "simulation-two-axis-f32", "training0-per-env-platform-noise-f32"]
N_COLS = sc.N_CODES + 1
SCORE_FIELDS = ("by_code", "steps_sum", "ep_code", "ep_steps")


def stacked(sets):
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])


_YARDSTICKS = {}


def engine_yardsticks(case_id, n, max_steps, episodes=EPISODES):
    """the stepwise map of each of the three table sets on a real Engine, computed once per argument set and left unchanged"""
    key = (case_id, n, max_steps, episodes)
    if key not in _YARDSTICKS:
        cfg = rc.case_config(case_id)
        out = []
        for t in rc.three_table_sets():
            eng = Engine(cfg, n, seed=SEED)
            try:
                out.append(mc.stepwise_map(eng, t, max_steps, episodes, bool(cfg.two_axis)))
            finally:
                eng.close()
        _YARDSTICKS[key] = out
    return _YARDSTICKS[key]


def score_map(case_id, n, max_steps=MAX_STEPS, episodes=EPISODES, sets=None, log=True, timing=None):
    return ops.score_map(rc.case_config(case_id), *stacked(rc.three_table_sets() if sets is None else sets), n, SEED, episodes=episodes, max_steps=max_steps, log=log, timing=timing)


def assert_all_sets_equal(got, want, n, what):
    for k, w in enumerate(want):
        mc.assert_map_set_equal(got, k, n, w, f"{what}, table set {k}")


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_score_map_equals_the_stepwise_engine_in_every_output(case_id):
    """(a) 64 envs, 3 table sets, 3 episodes, 900 steps; and the score's own outputs equal ops.score of the same arguments"""
    cfg = rc.case_config(case_id)
    n, axes = 64, 2 if cfg.two_axis else 1
    want = engine_yardsticks(case_id, n, MAX_STEPS)
    for k, w in enumerate(want):
        ev = w["events"]
        print(case_id, k, ev, int(w["visits"].sum()), w["steps_sum"], w["by_code"].tolist())
        assert ev["decisions"] == int(w["visits"].sum()) == axes * w["steps_sum"] + ev["unfinished_decisions"] and ev["ends_outside_a_decision"] == 0, ev
        assert ev["same_cell_periods"] > 0 and ev["reset_periods"] >= n and ev["early_lanes"] > 0, ev
        assert not cfg.two_axis or ev["xy_differ"] > 0, ev
    if cfg.working_curriculum_step == 4:  # the flush's partial last sweep carries counts in every level-4 case
        assert all(w["events"]["tail_decisions"] > 0 for w in want), [w["events"]["tail_decisions"] for w in want]
    assert want[0]["visits"].tolist() != want[1]["visits"].tolist()
    timing = {}
    got = score_map(case_id, n, timing=timing)
    assert got["visits"].shape == (3, N_CELLS) and got["visits"].dtype == np.int64 and got["ep_last_cell"].shape == (2, EPISODES, 3 * n) and got["columns"] == ops.SCORE_COLUMNS
    assert timing["instance"] == f"k_score_map<{'float' if cfg.dtype == F32 else 'double'}, 0, {0 if cfg.two_axis else 1}>" and timing["kernel_ms"] > 0.0
    assert_all_sets_equal(got, want, n, case_id)
    plain = ops.score(cfg, *stacked(rc.three_table_sets()), n, SEED, episodes=EPISODES, max_steps=MAX_STEPS, log=True)
    for f in SCORE_FIELDS:
        assert got[f].dtype == plain[f].dtype and np.array_equal(got[f], plain[f]), f"{case_id}: {f} differs from ops.score"
    nolog = score_map(case_id, n, log=False)
    assert nolog["ep_code"] is None and nolog["ep_steps"] is None and nolog["ep_last_cell"] is None
    for f in ("by_code", "steps_sum", "visits"):
        assert np.array_equal(nolog[f], got[f]), f


def test_three_waves_add_into_one_map_and_a_set_s_map_holds_nothing_of_its_neighbours():
    """(b) 192 envs per table set"""
    case_id, n = "simulation-f32", 192
    want = engine_yardsticks(case_id, n, MAX_STEPS)
    one_wave = engine_yardsticks(case_id, 64, MAX_STEPS)
    for k, w in enumerate(want):
        ev = w["events"]
        print(case_id, n, k, ev)
        assert ev["same_cell_periods"] > 0 and ev["tail_decisions"] > 0 and w["visits"].sum() > 2 * one_wave[k]["visits"].sum(), ev
    # cells that one set visits and its neighbour never does, in both directions: a wave that added into the wrong set's row would show
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1)):
        assert ((want[a]["visits"] > 0) & (want[b]["visits"] == 0)).any(), (a, b)
    got = score_map(case_id, n)
    assert_all_sets_equal(got, want, n, f"{case_id} n={n}")


@pytest.mark.parametrize("cut", [250, 5])
def test_cut_off_runs_count_the_decisions_of_unfinished_episodes(cut):
    """(c) training4-f32 cut at 250: finished and unfinished episodes, and lanes that already finished their three count nothing more; cut at 5: next to nothing ends"""
    case_id, n = "training4-f32", 64
    want = engine_yardsticks(case_id, n, cut)
    for k, w in enumerate(want):
        ev = w["events"]
        print(case_id, "cut at", cut, k, ev, int(w["visits"].sum()), w["steps_sum"], w["by_code"].tolist())
        assert int(w["visits"].sum()) == w["steps_sum"] + ev["unfinished_decisions"] and ev["ends_outside_a_decision"] == 0, ev
        assert ((w["ep_last_cell"][0] == mc.NO_CELL) == (w["ep_code"] == sc.NO_CODE)).all() and (w["ep_last_cell"][1] == mc.NO_CELL).all()
    w = want[0]
    assert w["events"]["unfinished_decisions"] > 0, w["events"]
    if cut == 250:
        assert w["events"]["early_lanes"] > 0 and w["by_code"][sc.UNFINISHED] >= n // 4 and w["by_code"][:sc.UNFINISHED].sum() >= n, (w["events"], w["by_code"].tolist())
    else:
        assert w["by_code"][sc.UNFINISHED] >= n * EPISODES - n // 8 and 4 * n <= w["visits"].sum() <= 5 * n
    got = score_map(case_id, n, max_steps=cut)
    assert_all_sets_equal(got, want, n, f"{case_id} cut at {cut}")


@pytest.mark.parametrize("case_id", ["training4-f32", "simulation-two-axis-f32"])
def test_one_episode_per_env_every_lane_stops_at_a_period_of_its_own(case_id):
    """(c) episodes = 1"""
    n = 64
    want = engine_yardsticks(case_id, n, MAX_STEPS, 1)
    ev = want[0]["events"]
    print(case_id, "one episode", ev)
    assert want[0]["by_code"][sc.UNFINISHED] == 0 and ev["early_lanes"] >= n // 2 and ev["reset_periods"] == n and len(set(want[0]["ep_steps"][0].tolist())) >= 8, ev
    got = score_map(case_id, n, episodes=1)
    assert_all_sets_equal(got, want, n, f"{case_id}, one episode per env")


def test_three_hundred_table_sets_repeat_the_maps_of_three():
    """(d) table indexing across the grid: set k is three_table_sets()[k % 3]"""
    case_id, n, K = "simulation-f32", 64, 300
    sets = rc.three_table_sets()
    three = score_map(case_id, n)
    assert_all_sets_equal(three, engine_yardsticks(case_id, n, MAX_STEPS), n, case_id)
    big = score_map(case_id, n, sets=[sets[k % 3] for k in range(K)])
    assert big["visits"].shape == (K, N_CELLS) and big["ep_last_cell"].shape == (2, EPISODES, K * n)
    idx = np.arange(K) % 3
    assert np.array_equal(big["visits"], three["visits"][idx]) and np.array_equal(big["by_code"], three["by_code"][idx]) and np.array_equal(big["steps_sum"], three["steps_sum"][idx])
    assert np.array_equal(big["ep_last_cell"].reshape(2, EPISODES, K, n), three["ep_last_cell"].reshape(2, EPISODES, 3, n)[:, :, idx])
    assert np.array_equal(big["ep_code"].reshape(EPISODES, K, n), three["ep_code"].reshape(EPISODES, 3, n)[:, idx])


def test_a_level_0_flight_visits_only_cells_of_level_0():
    """(e)"""
    case_id, n = "training0-per-env-platform-noise-f32", 64
    want = engine_yardsticks(case_id, n, MAX_STEPS)
    assert all(w["visits"][:mc.LEVEL0_CELLS].sum() > 0 and w["visits"][mc.LEVEL0_CELLS:].sum() == 0 for w in want)
    got = score_map(case_id, n)
    assert (got["visits"][:, mc.LEVEL0_CELLS:] == 0).all() and (got["visits"][:, :mc.LEVEL0_CELLS].sum(axis=1) > 0).all()
    cells = got["ep_last_cell"][0]
    assert (cells[cells != mc.NO_CELL] < mc.LEVEL0_CELLS).all()


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


def test_ensemble_is_mapped_where_it_lives_and_left_as_it_was():
    """(f) SequentialEnsemble.score_map whole and in slices == ops.score_map on the fetched tables; state, tables, counters and period index unchanged"""
    L, n = 130, 64
    sets = rc.three_table_sets()
    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), L, seed=7)
    try:
        ens.run(300)
        for first, t in ((0, sets[0]), (63, sets[2]), (64, sets[0]), (129, sets[2])):  # both sides of the second wave's first learner, and the last learner
            ens.set_tables(t[0], t[1], first=first)
        qa, qb, _ = ens.get_tables()
        before = ensemble_snapshot(ens)
        assert before["c_decisions"].sum() > 0 and int(before["period"]) == 300
        for eval_cfg in (simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), training_config(4, quirks=Q_PAPER, dtype=F64)):
            want = ops.score_map(eval_cfg, qa, qb, n, SEED, episodes=2, max_steps=500, log=True)
            assert want["visits"][64].tolist() != want["visits"][65].tolist(), "neighbouring learners must fly differently for the slice to show an offset"
            got = ens.score_map(eval_cfg, n, SEED, episodes=2, max_steps=500, log=True)
            for f in SCORE_FIELDS + ("visits", "ep_last_cell"):
                assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
            part = ens.score_map(eval_cfg, n, SEED, episodes=2, max_steps=500, log=True, first=64, count=66)
            assert np.array_equal(part["visits"], want["visits"][64:130]) and np.array_equal(part["by_code"], want["by_code"][64:130])
            assert np.array_equal(part["ep_last_cell"], want["ep_last_cell"][:, :, 64 * n:130 * n]) and np.array_equal(part["ep_code"], want["ep_code"][:, 64 * n:130 * n])
            assert_snapshots_equal(ensemble_snapshot(ens), before, "after score_map")
        m = ens.flight_maps(n_envs=n, episodes=1)
        w = evaluation.flight_maps(qa, qb, n_envs=n, episodes=1)
        r = ens.landing_rates(n_envs=n, episodes=1)
        for f in ("simulation_visits", "training_visits", "touchdown_rate", "goal_hold_rate"):
            assert np.array_equal(m[f], w[f]), f
        assert np.array_equal(m["touchdown_rate"], r["touchdown_rate"]) and m["simulation_visits"].shape == (L, N_CELLS) and m["simulation_log"] is None
        assert_snapshots_equal(ensemble_snapshot(ens), before, "after flight_maps")
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_greedy_actions_are_agent_predict_s():
    """(g) evaluation.greedy_actions == ops.agent_predict on every state of the three table sets and of a set with ties"""
    qa, qb = stacked(rc.three_table_sets())
    tie_a = np.tile(np.array([1.0, 1.0, 0.0, 0.0, 2.0, 2.0, 3.0, 1.0, 3.0]), N_CELLS // 9)
    qa, qb = np.vstack([qa, tie_a[None]]), np.vstack([qb, tie_a[None]])
    g = evaluation.greedy_actions(qa, qb)
    assert g.shape == (4, N_CELLS // 3)
    for k in range(4):
        assert np.array_equal(g[k], ops.agent_predict(qa[k], qb[k], np.arange(N_CELLS // 3))), k
    assert g[3][:3].tolist() == [0, 1, 0] and (g[1] == 0).all() and len(set(g[0].tolist())) == 3


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """(h) each refusal returns DQL_EINVAL with a text that says nothing was launched, leaves the output arrays untouched and the latest-kernel records as they
    were; after them a valid call still equals the yardstick"""
    lib = _lib.load()
    cfg = rc.case_config("simulation-f32")
    n = 64
    qa, qb = (np.ascontiguousarray(t) for t in rc.stage4_tables())
    ms0, ms_plain, inst = C.c_double(), C.c_double(), (C.c_int32 * 3)()
    plain = ops.score(cfg, qa, qb, n, SEED, episodes=2, max_steps=5, log=True, timing={})
    assert lib.dql_diag_score_last(C.byref(ms_plain), inst) == 0 and list(inst) == [4, 0, 1]
    good = ops.score_map(cfg, qa, qb, n, SEED, episodes=2, max_steps=5, log=True, timing={})
    assert good["by_code"][0, sc.UNFINISHED] == 2 * n and good["visits"].sum() == 5 * n and (good["ep_last_cell"] == mc.NO_CELL).all()
    assert lib.dql_diag_score_map_last(C.byref(ms0), inst) == 0 and list(inst) == [4, 0, 1]
    c = cfg.to_c()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    by_code = np.full((2, N_COLS), sentinel, np.int64); steps_sum = np.full(2, sentinel, np.int64); visits = np.full((2, N_CELLS), sentinel, np.int64)
    ep_code = np.full((2, 2 * n), sentinel, np.uint8); ep_steps = np.full((2, 2 * n), sentinel, np.uint16); ep_last = np.full((2, 2, 2 * n), sentinel, np.uint16)
    outs = (by_code, steps_sum, visits, ep_code, ep_steps, ep_last)

    def untouched():
        return all((a == sentinel).all() for a in outs)

    def records_unchanged():
        a, b = C.c_double(), C.c_double()
        return lib.dql_diag_score_map_last(C.byref(a), inst) == 0 and a.value == ms0.value and lib.dql_diag_score_last(C.byref(b), inst) == 0 and b.value == ms_plain.value

    def call(n_tables=1, envs=n, episodes=2, max_steps=5, qa_=qa, qb_=qb, by_code_=by_code, steps_sum_=steps_sum, visits_=visits, ep_code_=ep_code, ep_steps_=ep_steps, ep_last_=ep_last):
        return lib.dql_score_map(C.byref(c), 0, n_tables, envs, episodes, SEED, max_steps, ptr(qa_), ptr(qb_), ptr(by_code_), ptr(steps_sum_), ptr(visits_), ptr(ep_code_),
                                 ptr(ep_steps_), ptr(ep_last_))

    log_refusals = {
        "log without code": dict(ep_code_=None), "log without steps": dict(ep_steps_=None), "log without last cells": dict(ep_last_=None),
        "only code": dict(ep_steps_=None, ep_last_=None), "only steps": dict(ep_code_=None, ep_last_=None), "only last cells": dict(ep_code_=None, ep_steps_=None),
    }
    refused = {
        "n_tables 0": dict(n_tables=0), "n_tables 2^14 + 1": dict(n_tables=(1 << 14) + 1), "n_tables 2^20 + 1": dict(n_tables=(1 << 20) + 1),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100), "2^31 lanes": dict(n_tables=1 << 14, envs=1 << 17),
        "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65), "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None), "null visits": dict(visits_=None),
        **log_refusals,
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_score_map" in msg and "nothing was launched" in msg, f"{what}: {msg!r}"
        assert untouched() and records_unchanged(), what
    bad_cfg = rc.case_config("simulation-f32")
    bad_cfg.working_curriculum_step = 9  # check_config applies as in dql_create
    cb = bad_cfg.to_c()
    assert lib.dql_score_map(C.byref(cb), 0, 1, n, 2, SEED, 5, ptr(qa), ptr(qb), ptr(by_code), ptr(steps_sum), ptr(visits), None, None, None) == _lib.EINVAL and untouched()
    with pytest.raises(ValueError):
        ops.score_map(cfg, qa, qb, 100, SEED)

    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), 130, seed=7)
    try:
        def ecall(first=0, count=2, envs=n, episodes=2, max_steps=5, cfg_=c, by_code_=by_code, steps_sum_=steps_sum, visits_=visits, ep_code_=ep_code, ep_steps_=ep_steps, ep_last_=ep_last):
            return lib.dql_ensemble_score_map(ens._h, C.byref(cfg_), first, count, envs, episodes, SEED, max_steps, ptr(by_code_), ptr(steps_sum_), ptr(visits_), ptr(ep_code_),
                                              ptr(ep_steps_), ptr(ep_last_))

        erefused = {
            "count 0": dict(count=0), "first -1": dict(first=-1), "slice beyond the end": dict(first=129, count=2), "first beyond the end": dict(first=131, count=1),
            "count 2^14 + 1": dict(count=(1 << 14) + 1), "envs 0": dict(envs=0), "envs 100": dict(envs=100), "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
            "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
            "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None), "null visits": dict(visits_=None), "bad config": dict(cfg_=cb), **log_refusals,
        }
        for what, kw in erefused.items():
            rcode = ecall(**kw)
            msg = lib.dql_last_error().decode()
            assert rcode == _lib.EINVAL, f"ensemble, {what}: returned {rcode}"
            assert what == "bad config" or ("dql_ensemble_score_map" in msg and "nothing was launched" in msg), f"ensemble, {what}: {msg!r}"
            assert untouched() and records_unchanged(), what
        assert lib.dql_ensemble_score_map(None, C.byref(c), 0, 1, n, 2, SEED, 5, ptr(by_code), ptr(steps_sum), ptr(visits), None, None, None) == _lib.EINVAL and untouched()
        with pytest.raises(ValueError):
            ens.score_map(cfg, n, SEED, first=129, count=2)
        assert ecall() == 0 and not untouched() and (by_code.sum(axis=1) == 2 * n).all() and (visits.sum(axis=1) > 0).all()  # and the same arguments, well-formed, do run
    finally:
        ens.close()
    for a in outs:
        a[:] = sentinel
    assert call() == 0
    for f, a in zip(("by_code", "steps_sum", "visits"), outs):
        assert np.array_equal(a[0], good[f][0]), f
    # one table set: the call lays its log out as [episodes][n] and [2][episodes][n] at the head of the buffers, which were sized for two sets
    assert np.array_equal(ep_code.ravel()[:2 * n].reshape(2, n), good["ep_code"]) and np.array_equal(ep_steps.ravel()[:2 * n].reshape(2, n), good["ep_steps"])
    assert np.array_equal(ep_last.ravel()[:4 * n].reshape(2, 2, n), good["ep_last_cell"]) and np.array_equal(plain["by_code"], good["by_code"])
    assert (ep_code.ravel()[2 * n:] == sentinel).all() and (ep_last.ravel()[4 * n:] == sentinel).all(), "nothing is written beyond the one set's log"
    # and a valid call still equals the yardstick
    want = engine_yardsticks("simulation-f32", n, MAX_STEPS)
    assert_all_sets_equal(score_map("simulation-f32", n), want, n, "after the refusals")
