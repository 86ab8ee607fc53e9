"""The transition-model operator on the device (dql_model / dql_ensemble_model, k_model) against the stepwise yardstick of tests/model_checks.py: one oracle
stepped with external actions, the eps-greedy rule spelled out with its Philox words.  Every comparison is ==.  The yardstick also counts the events a kernel
can get wrong, and every case asserts on it first that they occurred (model_checks.yardstick): the same pair added twice by one wave in one period,
transitions across levels, all three kinds of terminal, envs cut off, explored and greedy decisions, three waves adding into one set, lanes that stop at
periods of their own."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import model_checks as mc
import rollout_checks as rc

pytestmark = pytest.mark.gpu


def fly(case_id, timing=None):
    cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
    return ops.transition_model(cfg, tables[0], tables[1], n, mc.SEED, eps, episodes=episodes, max_steps=max_steps, timing=timing)


@pytest.mark.parametrize("case_id", list(mc.CASES))
def test_the_model_equals_the_stepwise_yardstick_in_every_output(case_id):
    cfg = mc.case_args(case_id)[0]
    want = mc.yardstick(case_id)
    timing = {}
    got = fly(case_id, timing)
    assert got["pairs"].shape == (1, N_CELLS, mc.N_STATES) and got["pairs"].dtype == np.uint32 and got["terminal"].shape == (1, N_CELLS, mc.N_CODES)
    assert got["reward_fx"].dtype == got["terminal"].dtype == got["visits"].dtype == np.int64 and got["columns"] == ops.SCORE_COLUMNS
    assert timing["instance"] == f"k_model<{'float' if cfg.dtype == F32 else 'double'}, 0, 1>" and timing["kernel_ms"] > 0.0
    mc.assert_model_set_equal(got, 0, want, f"case {case_id}")
    # conservation: every decision is a pair or a terminal, and the terminals are the finished episodes
    assert int(got["visits"].sum()) == want["events"]["decisions"]
    assert np.array_equal(got["terminal"][0].sum(axis=0), got["by_code"][0][:mc.N_CODES])
    again = fly(case_id)
    for f in mc.FIELDS:
        assert got[f].tobytes() == again[f].tobytes(), f"{case_id}: {f} differs between two runs"


def test_a_greedy_model_counts_what_score_map_counts():
    """case D (eps = 0): visits, by_code and steps_sum == ops.score_map's on the same arguments"""
    cfg, tables, eps, n, max_steps, episodes = mc.case_args("D")
    assert eps == 0.0
    got = fly("D")
    ref = ops.score_map(cfg, tables[0], tables[1], n, mc.SEED, episodes=episodes, max_steps=max_steps)
    for f in ("visits", "by_code", "steps_sum"):
        assert got[f].dtype == ref[f].dtype and np.array_equal(got[f], ref[f]), f


def test_three_table_sets_in_one_call_equal_three_calls():
    """and a set's tables hold nothing of its neighbours: the sets fly differently, and each equals the call that flew it alone"""
    cfg, _, eps, n, max_steps, episodes = mc.case_args("A")
    sets = rc.three_table_sets()
    qa, qb = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    got = ops.transition_model(cfg, qa, qb, n, mc.SEED, eps, episodes=episodes, max_steps=max_steps)
    assert got["pairs"].shape == (3, N_CELLS, mc.N_STATES)
    mc.assert_model_set_equal(got, 0, mc.yardstick("A"), "set 0 of three")
    for k, s in enumerate(sets):
        alone = ops.transition_model(cfg, s[0], s[1], n, mc.SEED, eps, episodes=episodes, max_steps=max_steps)
        for f in mc.FIELDS:
            assert np.array_equal(got[f][k], alone[f][0]), f"set {k}: {f}"
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1)):  # pairs that one set counts and its neighbour never does, in both directions
        assert ((got["pairs"][a] > 0) & (got["pairs"][b] == 0)).any(), (a, b)


def ensemble_snapshot(ens):
    qa, qb, cnt = ens.get_tables()
    c = ens.counters()
    st = ens.state()
    return {"qa": qa, "qb": qb, "count": cnt, "period": np.array(ens.period_index()), **{f"c_{k}": np.asarray(v) for k, v in c.items()}, **{f"s_{k}": v for k, v in st.items()}}


def test_ensemble_is_modelled_where_it_lives_and_left_as_it_was():
    """SequentialEnsemble.model of a slice == ops.transition_model on the fetched tables; state, tables, counters and period index unchanged"""
    L, n, first, count = 70, 64, 62, 4  # the slice spans the second wave's first learner
    sets = rc.three_table_sets()
    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), L, seed=7)
    try:
        ens.run(300)
        for at, t in ((62, sets[0]), (63, sets[2]), (64, sets[0])):
            ens.set_tables(t[0], t[1], first=at)
        qa, qb, _ = ens.get_tables()
        before = ensemble_snapshot(ens)
        assert before["c_decisions"].sum() > 0 and int(before["period"]) == 300
        for eval_cfg in (simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), training_config(4, quirks=Q_PAPER, dtype=F64)):
            want = ops.transition_model(eval_cfg, qa[first:first + count], qb[first:first + count], n, mc.SEED, 0.1, episodes=2, max_steps=200)
            assert want["pairs"][1].tolist() != want["pairs"][2].tolist(), "neighbouring learners must fly differently for the slice to show an offset"
            got = ens.model(eval_cfg, n, mc.SEED, 0.1, episodes=2, max_steps=200, first=first, count=count)
            for f in mc.FIELDS:
                assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
            after = ensemble_snapshot(ens)
            assert after.keys() == before.keys()
            for k in before:
                assert np.ascontiguousarray(after[k]).tobytes() == np.ascontiguousarray(before[k]).tobytes(), f"after model: {k} differs"
        with pytest.raises(ValueError):
            ens.model(simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), n, mc.SEED, 0.1, first=0, count=17)
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """each refusal returns DQL_EINVAL with a text that says nothing was launched, leaves the output arrays untouched and the latest-kernel record as it was;
    after them a valid call still equals the yardstick"""
    lib = _lib.load()
    cfg, tables, eps, n, max_steps, episodes = mc.case_args("D")
    qa, qb = (np.ascontiguousarray(t, np.float64) for t in tables)
    good = fly("D", {})
    ms0, inst = C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_model_last(C.byref(ms0), inst) == 0 and list(inst) == [4, 0, 1]
    c = cfg.to_c()
    two = simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32).to_c()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    pairs = np.full((1, N_CELLS, mc.N_STATES), sentinel, np.uint32); reward_fx = np.full((1, N_CELLS), sentinel, np.int64)
    terminal = np.full((1, N_CELLS, mc.N_CODES), sentinel, np.int64); by_code = np.full((1, mc.N_COLS), sentinel, np.int64); steps_sum = np.full(1, sentinel, np.int64)
    outs = (pairs, reward_fx, terminal, by_code, steps_sum)

    def untouched():
        return all((a == sentinel).all() for a in outs)

    def record_unchanged():
        a = C.c_double()
        return lib.dql_diag_model_last(C.byref(a), inst) == 0 and a.value == ms0.value

    def call(cfg_=c, n_tables=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, qa_=qa, qb_=qb, pairs_=pairs, reward_=reward_fx, terminal_=terminal, by_code_=by_code,
             steps_sum_=steps_sum):
        return lib.dql_model(C.byref(cfg_), 0, n_tables, envs, episodes_, mc.SEED, max_steps_, eps_, ptr(qa_), ptr(qb_), ptr(pairs_), ptr(reward_), ptr(terminal_), ptr(by_code_),
                             ptr(steps_sum_))

    refused = {
        "two axes": dict(cfg_=two), "n_tables 0": dict(n_tables=0), "n_tables 17": dict(n_tables=17), "n_tables -1": dict(n_tables=-1),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100),
        "2^20 envs x 4097 periods": dict(envs=1 << 20, max_steps_=4096), "2^20 envs x 4096 periods": dict(envs=1 << 20, max_steps_=4095),
        "episodes 0": dict(episodes_=0), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "max_steps 4097": dict(max_steps_=4097),
        "eps -0.1": dict(eps_=-0.1), "eps 1.5": dict(eps_=1.5), "eps nan": dict(eps_=float("nan")),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null pairs": dict(pairs_=None), "null reward_fx": dict(reward_=None), "null terminal": dict(terminal_=None),
        "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None),
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_model" in msg and "nothing was launched" in msg and msg.rstrip().endswith("launched"), f"{what}: {msg!r}"
        assert untouched() and record_unchanged(), what
    bad_cfg = mc.case_args("D")[0]
    bad_cfg.working_curriculum_step = 9  # check_config applies as in dql_create
    cb = bad_cfg.to_c()
    assert call(cfg_=cb) == _lib.EINVAL and untouched()
    for kw in (dict(envs_per_table=100), dict(eps=1.5), dict(episodes=0), dict(max_steps=4097)):
        args = dict(envs_per_table=n, seed=mc.SEED, eps=eps)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.transition_model(cfg, qa, qb, **args)

    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), 20, seed=7)
    try:
        def ecall(first=0, count=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, cfg_=c, pairs_=pairs, reward_=reward_fx, terminal_=terminal, by_code_=by_code,
                  steps_sum_=steps_sum):
            return lib.dql_ensemble_model(ens._h, C.byref(cfg_), first, count, envs, episodes_, mc.SEED, max_steps_, eps_, ptr(pairs_), ptr(reward_), ptr(terminal_), ptr(by_code_),
                                          ptr(steps_sum_))

        erefused = {
            "two axes": dict(cfg_=two), "count 0": dict(count=0), "count 17": dict(count=17), "first -1": dict(first=-1), "slice beyond the end": dict(first=19, count=2),
            "first beyond the end": dict(first=21), "envs 100": dict(envs=100), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "eps 2": dict(eps_=2.0),
            "null pairs": dict(pairs_=None), "null steps_sum": dict(steps_sum_=None),
        }
        for what, kw in erefused.items():
            rcode = ecall(**kw)
            msg = lib.dql_last_error().decode()
            assert rcode == _lib.EINVAL, f"ensemble, {what}: returned {rcode}"
            assert "dql_ensemble_model" in msg and "nothing was launched" in msg, f"ensemble, {what}: {msg!r}"
            assert untouched() and record_unchanged(), what
        assert lib.dql_ensemble_model(None, C.byref(c), 0, 1, n, episodes, mc.SEED, max_steps, eps, ptr(pairs), ptr(reward_fx), ptr(terminal), ptr(by_code), ptr(steps_sum)) == _lib.EINVAL
        assert untouched()
        assert ecall() == 0 and not untouched() and int(by_code.sum()) == n * episodes  # and the same arguments, well-formed, do run
    finally:
        ens.close()
    for a in outs:
        a[:] = sentinel
    assert call() == 0
    for f, a in zip(("pairs", "reward_fx", "terminal", "by_code", "steps_sum"), outs):
        assert np.array_equal(a, good[f]), f
    mc.assert_model_set_equal(fly("D"), 0, mc.yardstick("D"), "after the refusals")
