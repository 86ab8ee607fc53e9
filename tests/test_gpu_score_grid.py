"""The scenario-grid scorer on the device (dql_score_grid / dql_ensemble_score_grid, k_score_grid) against real Engines driven one agent period at a time: the
equality contract of include/dql.h — slice s of every output is dql_score's for scenario s alone, which is the stepwise context's, and touch_hist bins the
touchdowns by the offset the state shows after their terminal period.  The yardstick (tests/grid_checks.py) knows nothing of the kernel.  Every comparison is ==."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import DqlConfigC, F32, F64, Q_PAPER, training_config
from dql_multirotor_landing_amd.engine import Engine
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import grid_checks as gc
import rollout_checks as rc
import score_checks as sc

pytestmark = pytest.mark.gpu


def stacked(sets):
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])


_YARDSTICKS = {}


def engine_yardstick(key, cfgs, n, episodes):
    """the stepwise grid on real Engines, one per (scenario, set), computed once per key and left unchanged"""
    if key not in _YARDSTICKS:
        _YARDSTICKS[key] = gc.stepwise_grid(lambda cfg, n_, seed: Engine(cfg, n_, seed=seed), cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes)
    return _YARDSTICKS[key]


def instance_name(cfg):
    return f"k_score_grid<{'float' if cfg.dtype == F32 else 'double'}, 0, {0 if cfg.two_axis else 1}>"


@pytest.mark.parametrize("case_id", gc.CASE_IDS)
def test_every_output_of_the_grid_equals_the_stepwise_engines(case_id):
    cfgs, n, episodes = gc.case(case_id)
    want = engine_yardstick(case_id, cfgs, n, episodes)
    print(case_id, "by_code set 0:", want["by_code"][:, 0].tolist(), "touch set 0:", want["touch_hist"][:, 0].tolist())
    gc.assert_not_vacuous(case_id, want)
    qa, qb = stacked(gc.table_sets())
    timing = {}
    got = ops.score_grid(cfgs, qa, qb, n, gc.SEED, episodes=episodes, max_steps=gc.MAX_STEPS, log=True, timing=timing)
    assert timing["instance"] == instance_name(cfgs[0]) and timing["kernel_ms"] > 0.0
    assert got["columns"] == ops.SCORE_COLUMNS and got["touch_edges"].shape == (len(cfgs), 7)
    assert np.array_equal(got["touch_edges"], np.stack([gc.touch_edges(c).astype(np.float64) for c in cfgs]))
    gc.assert_grid_equal(got, want, case_id)
    again = ops.score_grid(cfgs, qa, qb, n, gc.SEED, episodes=episodes, max_steps=gc.MAX_STEPS, log=True)
    for f in gc.OUTPUTS:
        assert again[f].tobytes() == got[f].tobytes(), f"{case_id}: {f} differs between two identical calls"
    bare = ops.score_grid(cfgs, qa, qb, n, gc.SEED, episodes=episodes, max_steps=gc.MAX_STEPS, touch=False)
    assert bare["ep_code"] is None and bare["ep_steps"] is None and bare["touch_hist"] is None
    gc.assert_grid_equal(bare, want, f"{case_id} without the log and touch_hist", ("by_code", "steps_sum"))


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-f64", "training4-f32", "simulation-two-axis-f32", "training0-per-env-platform-noise-f32"])
def test_a_grid_of_one_scenario_is_the_score(case_id):
    cfg = rc.case_config(case_id)
    n, episodes, max_steps = 128, 2, 450
    qa, qb = stacked(rc.three_table_sets())
    want = ops.score(cfg, qa, qb, n, gc.SEED, episodes=episodes, max_steps=max_steps, log=True)
    assert (want["ep_code"] != sc.NO_CODE).any() and len({tuple(r) for r in want["by_code"].tolist()}) >= 2
    timing = {}
    got = ops.score_grid([cfg], qa, qb, n, gc.SEED, episodes=episodes, max_steps=max_steps, log=True, timing=timing)
    assert timing["instance"] == instance_name(cfg)
    for f in ("by_code", "steps_sum", "ep_code", "ep_steps"):
        assert got[f].shape == (1,) + want[f].shape and got[f].dtype == want[f].dtype and np.array_equal(got[f][0], want[f]), f
    assert np.array_equal(got["touch_hist"][0].sum(axis=1), want["by_code"][:, rc.CONTACT])


def test_three_waves_add_into_one_row():
    """192 envs per set on scenarios {#0, #4}: three waves per (scenario, set)"""
    g = gc.scenarios(F32)
    cfgs, n = [g[0], g[4]], 192
    want = engine_yardstick("three-waves", cfgs, n, gc.EPISODES)
    assert want["by_code"][0, 0].tolist() != want["by_code"][1, 0].tolist() and (want["touch_hist"].sum(axis=2) > 0)[:, 0].all()
    per_wave = [sc.sums_of_log(want["ep_code"][0][:, w * 64:(w + 1) * 64], want["ep_steps"][0][:, w * 64:(w + 1) * 64])["by_code"].tolist() for w in range(3)]
    assert len({tuple(r) for r in per_wave}) == 3, "the three waves of a row end differently"
    got = ops.score_grid(cfgs, *stacked(gc.table_sets()), n, gc.SEED, episodes=gc.EPISODES, max_steps=gc.MAX_STEPS, log=True)
    gc.assert_grid_equal(got, want, "192 envs per set")
    assert (got["by_code"].sum(axis=2) == n * gc.EPISODES).all()


def ensemble_snapshot(ens):
    qa, qb, cnt = ens.get_tables()
    c = ens.counters()
    st = ens.state()
    return {"qa": qa, "qb": qb, "count": cnt, "period": np.array(ens.period_index()), **{f"c_{k}": np.asarray(v) for k, v in c.items()}, **{f"s_{k}": v for k, v in st.items()}}


def test_ensemble_is_scored_over_the_grid_where_it_lives_and_left_as_it_was():
    """SequentialEnsemble.score_grid of a slice across the second wave's first learner == ops.score_grid on the fetched tables; tables and state bytes unchanged"""
    L, n, first, count = 70, 64, 62, 4
    sets = rc.three_table_sets()
    g = gc.scenarios(F32)
    cfgs = [g[0], g[1], g[5]]
    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), L, seed=7)
    try:
        ens.run(300)
        for at, t in ((62, sets[0]), (63, sets[2]), (64, sets[0])):
            ens.set_tables(t[0], t[1], first=at)
        before = ensemble_snapshot(ens)
        qa, qb = before["qa"], before["qb"]
        assert np.array_equal(qa[64].ravel(), sets[0][0]) and not np.array_equal(qa[65].ravel(), sets[0][0])
        want = ops.score_grid(cfgs, qa[first:first + count], qb[first:first + count], n, gc.SEED, episodes=2, max_steps=gc.MAX_STEPS, log=True)
        assert want["by_code"][0, 1].tolist() != want["by_code"][0, 2].tolist() and want["by_code"][0, 2].tolist() != want["by_code"][0, 3].tolist()
        assert want["touch_hist"][:2].sum() > 0
        timing = {}
        got = ens.score_grid(cfgs, n, gc.SEED, episodes=2, max_steps=gc.MAX_STEPS, log=True, first=first, count=count, timing=timing)
        assert timing["instance"] == "k_score_grid<float, 0, 1>"
        for f in gc.OUTPUTS:
            assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
        after = ensemble_snapshot(ens)
        assert before.keys() == after.keys()
        for k in before:
            x, y = np.ascontiguousarray(before[k]), np.ascontiguousarray(after[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{k} changed"
        # the slice must lie inside the ensemble
        lib = _lib.load()
        c = ops.grid_configs_to_c(cfgs)
        by_code, steps_sum, touch, _, _ = ops.grid_buffers(3, 4, n, 2, False, True)
        by_code[:] = 77
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        for bad_first, bad_count in ((-1, 4), (68, 4), (71, 1)):
            assert lib.dql_ensemble_score_grid(ens._h, c, 3, bad_first, bad_count, n, 2, gc.SEED, 50, ptr(by_code), ptr(steps_sum), ptr(touch), None, None) == _lib.EINVAL
            msg = lib.dql_last_error().decode()
            assert "dql_ensemble_score_grid" in msg and "[0, n_learners)" in msg and "nothing was launched" in msg and (by_code == 77).all()
        with pytest.raises(ValueError):
            ens.score_grid(cfgs, n, gc.SEED, first=68, count=4)
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """each refusal returns DQL_EINVAL with a whole sentence in dql_last_error that says nothing was launched (and names the scenario where there is one), leaves
    the output arrays untouched, and the latest-kernel record (dql_diag_score_grid_last) still describes the good call made before; a good call afterwards is right"""
    lib = _lib.load()
    g = gc.scenarios(F32)
    cfgs = [g[0], g[1], g[4]]
    n, S = 64, 3
    qa, qb = (np.ascontiguousarray(t) for t in rc.stage4_tables())
    good = ops.score_grid(cfgs, qa, qb, n, gc.SEED, episodes=2, max_steps=gc.MAX_STEPS, log=True, timing={})
    assert good["by_code"][0, 0, rc.CONTACT] > 0
    ms0, inst = C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_score_grid_last(C.byref(ms0), inst) == 0 and list(inst) == [4, 0, 1]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    by_code = np.full((S, 1, gc.N_COLS), sentinel, np.int64); steps_sum = np.full((S, 1), sentinel, np.int64); touch = np.full((S, 1, 8), sentinel, np.int64)
    ep_code = np.full((S, 2, n), sentinel, np.uint8); ep_steps = np.full((S, 2, n), sentinel, np.uint16)
    outputs = (by_code, steps_sum, touch, ep_code, ep_steps)

    def c_array(cs):
        return ops.grid_configs_to_c(cs)

    def call(cs=cfgs, n_scen=None, n_tables=1, envs=n, episodes=2, max_steps=5, qa_=qa, qb_=qb, by_code_=by_code, steps_sum_=steps_sum, ep_code_=ep_code, ep_steps_=ep_steps,
             null_cfgs=False):
        arr = None if null_cfgs else c_array(cs)
        return lib.dql_score_grid(arr, len(cs) if n_scen is None else n_scen, 0, n_tables, envs, episodes, gc.SEED, max_steps, ptr(qa_), ptr(qb_), ptr(by_code_), ptr(steps_sum_),
                                  ptr(touch), ptr(ep_code_), ptr(ep_steps_))

    def differs(field, value):
        return [cfgs[0], cfgs[1], dataclasses.replace(cfgs[2], **{field: value})]

    bad_level = dataclasses.replace(cfgs[1], working_curriculum_step=9)
    refused = {  # what -> (arguments, words the sentence must hold)
        "n_scenarios 0": (dict(n_scen=0), ["n_scenarios"]), "n_scenarios 1025": (dict(cs=[cfgs[0]] * 1025), ["n_scenarios", "1024"]),
        "null cfgs": (dict(null_cfgs=True), ["scenario array is null"]),
        "scenario 1 fails check_config": (dict(cs=[cfgs[0], bad_level, cfgs[2]]), ["scenario 1", "working_curriculum_step"]),
        "dtype": (dict(cs=differs("dtype", F64)), ["scenario 2", "in dtype,"]), "two_axis": (dict(cs=differs("two_axis", 1)), ["scenario 2", "in two_axis,"]),
        "f_ag": (dict(cs=differs("f_ag", 20.0)), ["scenario 2", "in f_ag,"]), "dt": (dict(cs=differs("dt", 0.001)), ["scenario 2", "in dt,"]),
        "manager_div": (dict(cs=differs("manager_div", 4)), ["scenario 2", "in manager_div,"]),
        "S K n > 2^30": (dict(n_tables=1 << 14, envs=1 << 15), ["2^30"]), "K n = 2^30, S = 3": (dict(envs=1 << 30), ["2^30"]),
        "n_tables 0": (dict(n_tables=0), []), "envs 0": (dict(envs=0), []), "envs 100": (dict(envs=100), []), "episodes 0": (dict(episodes=0), []),
        "episodes 65": (dict(episodes=65), []), "max_steps 0": (dict(max_steps=0), []), "max_steps 4097": (dict(max_steps=4097), []),
        "log code without steps": (dict(ep_steps_=None), ["both arrays or neither"]), "log steps without code": (dict(ep_code_=None), ["both arrays or neither"]),
        "null qa": (dict(qa_=None), ["null"]), "null qb": (dict(qb_=None), ["null"]), "null by_code": (dict(by_code_=None), ["null"]),
        "null steps_sum": (dict(steps_sum_=None), ["null"]),
    }
    for what, (kw, words) in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_score_grid" in msg and "nothing was launched" in msg and all(w in msg for w in words), f"{what}: {msg!r}"
        assert all((a == sentinel).all() for a in outputs), what
        ms1 = C.c_double()
        assert lib.dql_diag_score_grid_last(C.byref(ms1), inst) == 0 and ms1.value == ms0.value and list(inst) == [4, 0, 1], what
    # the Python wrapper refuses the same before the library is touched
    with pytest.raises(ValueError, match="scenario 2 differs from scenario 0 in dt"):
        ops.score_grid(differs("dt", 0.001), qa, qb, n, gc.SEED)
    # and a good call afterwards is what it was
    again = ops.score_grid(cfgs, qa, qb, n, gc.SEED, episodes=2, max_steps=gc.MAX_STEPS, log=True)
    for f in gc.OUTPUTS:
        assert again[f].tobytes() == good[f].tobytes(), f
    assert isinstance(c_array(cfgs)[0], DqlConfigC)
