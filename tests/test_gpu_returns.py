"""The realised-returns operator on the device (dql_returns / dql_ensemble_returns: k_returns_fly, then k_returns_sweep) against the stepwise yardstick of
tests/returns_checks.py: one oracle stepped with external actions, per-env decision lists, the backward recursion in numpy float64.  Every comparison is ==.
The yardstick also counts the events a kernel can get wrong, and every row asserts on it first that they occurred (returns_checks.yardstick): envs whose
finished episode is followed by a cut-off one, envs with two finished episodes, many distinct episode lengths in one wave (64 lanes of different lengths
sweeping together), three waves adding into one set (case C: three 64-lane workgroups), four waves sharing one LDS table (case W: the 256-lane instance), an
episode that ends in period max_steps itself beside an env one period short (case F)."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import model_checks as mc
import returns_checks as rck
import rollout_checks as rc

pytestmark = pytest.mark.gpu


def fly(case_id, gamma, timing=None):
    cfg, tables, eps, n, max_steps, episodes = rck.case_args(case_id)
    return ops.returns_map(cfg, tables[0], tables[1], n, rck.SEED, eps, gamma, episodes=episodes, max_steps=max_steps, timing=timing)


def model_of(case_id):
    cfg, tables, eps, n, max_steps, episodes = rck.case_args(case_id)
    return ops.transition_model(cfg, tables[0], tables[1], n, rck.SEED, eps, episodes=episodes, max_steps=max_steps)


@pytest.mark.parametrize("case_id,gamma", rck.ROWS, ids=rck.ROW_IDS)
def test_the_returns_equal_the_stepwise_yardstick_in_every_output(case_id, gamma):
    cfg = rck.case_args(case_id)[0]
    want = rck.yardstick(case_id, gamma)
    timing = {}
    got = fly(case_id, gamma, timing)
    assert got["visits"].shape == got["return_fx"].shape == (1, N_CELLS) and got["cut_decisions"].shape == (1,) and got["columns"] == ops.SCORE_COLUMNS
    assert timing["instance"] == f"k_returns_fly<{'float' if cfg.dtype == F32 else 'double'}, 0, 1>" and timing["fly_ms"] > 0.0 and timing["sweep_ms"] > 0.0
    print("returns", case_id, gamma, "visits", int(got["visits"].sum()), "cut", int(got["cut_decisions"][0]), "return_fx", int(got["return_fx"].sum()), timing)
    rck.assert_returns_set_equal(got, 0, want, f"case {case_id}, gamma {gamma}")
    again = fly(case_id, gamma)
    for f in rck.FIELDS:
        assert got[f].tobytes() == again[f].tobytes(), f"{case_id}: {f} differs between two runs"


@pytest.mark.parametrize("case_id", ["A", "B64", "C", "F"])
def test_the_flights_are_the_transition_model_s(case_id):
    """by_code and steps_sum == ops.transition_model's for the same arguments, and every decision it counts is kept or cut"""
    got, model = fly(case_id, 0.99), model_of(case_id)
    for f in ("by_code", "steps_sum"):
        assert got[f].dtype == model[f].dtype and np.array_equal(got[f], model[f]), f
    assert int(got["visits"].sum()) + int(got["cut_decisions"].sum()) == int(model["visits"].sum())
    assert (got["visits"] <= model["visits"]).all()


def test_gamma_zero_returns_are_the_model_kernel_s_rewards():
    """case D (nobody cut) at gamma 0: return_fx and visits == ops.transition_model's reward_fx and visits — two independent kernels held to each other"""
    got, model = fly("D", 0.0), model_of("D")
    assert int(got["cut_decisions"][0]) == 0
    assert got["return_fx"].dtype == model["reward_fx"].dtype and np.array_equal(got["return_fx"], model["reward_fx"])
    assert np.array_equal(got["visits"], model["visits"])


def test_three_table_sets_in_one_call_equal_three_calls():
    """and a set's tables hold nothing of its neighbours: the sets fly differently, and each equals the call that flew it alone"""
    cfg, _, eps, n, max_steps, episodes = rck.case_args("A")
    sets = rc.three_table_sets()
    qa, qb = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    got = ops.returns_map(cfg, qa, qb, n, rck.SEED, eps, 0.99, episodes=episodes, max_steps=max_steps)
    assert got["visits"].shape == (3, N_CELLS) and got["cut_decisions"].shape == (3,)
    rck.assert_returns_set_equal(got, 0, rck.yardstick("A", 0.99), "set 0 of three")
    for k, s in enumerate(sets):
        alone = ops.returns_map(cfg, s[0], s[1], n, rck.SEED, eps, 0.99, episodes=episodes, max_steps=max_steps)
        for f in rck.FIELDS:
            assert np.array_equal(got[f][k], alone[f][0]), f"set {k}: {f}"
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1)):  # cells that one set visits and its neighbour never does, in both directions
        assert ((got["visits"][a] > 0) & (got["visits"][b] == 0)).any(), (a, b)


def ensemble_snapshot(ens):
    qa, qb, cnt = ens.get_tables()
    c = ens.counters()
    st = ens.state()
    return {"qa": qa, "qb": qb, "count": cnt, "period": np.array(ens.period_index()), **{f"c_{k}": np.asarray(v) for k, v in c.items()}, **{f"s_{k}": v for k, v in st.items()}}


def test_ensemble_returns_where_it_lives_and_is_left_as_it_was():
    """SequentialEnsemble.returns_map of a slice == ops.returns_map on the fetched tables; state, tables, counters and period index unchanged"""
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
            want = ops.returns_map(eval_cfg, qa[first:first + count], qb[first:first + count], n, rck.SEED, 0.1, 0.99, episodes=2, max_steps=200)
            assert want["visits"][1].tolist() != want["visits"][2].tolist(), "neighbouring learners must fly differently for the slice to show an offset"
            assert want["visits"].sum() > 0 and want["cut_decisions"].sum() > 0
            got = ens.returns_map(eval_cfg, n, rck.SEED, 0.1, 0.99, episodes=2, max_steps=200, first=first, count=count)
            for f in rck.FIELDS:
                assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
            after = ensemble_snapshot(ens)
            assert after.keys() == before.keys()
            for k in before:
                assert np.ascontiguousarray(after[k]).tobytes() == np.ascontiguousarray(before[k]).tobytes(), f"after returns_map: {k} differs"
        with pytest.raises(ValueError):
            ens.returns_map(simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), n, rck.SEED, 0.1, 0.99, first=60, count=11)
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """each refusal returns DQL_EINVAL with a whole sentence that says nothing was launched, leaves the output arrays untouched and the latest-kernel record as
    it was; after them a valid call still equals the yardstick"""
    lib = _lib.load()
    cfg, tables, eps, n, max_steps, episodes = rck.case_args("D")
    qa, qb = (np.ascontiguousarray(t, np.float64) for t in tables)
    good = fly("D", 0.99, {})
    fly0, sweep0, inst = C.c_double(), C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_returns_last(C.byref(fly0), C.byref(sweep0), inst) == 0 and list(inst) == [4, 0, 1]
    c = cfg.to_c()
    two = simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32).to_c()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    visits = np.full((1, N_CELLS), sentinel, np.int64); return_fx = np.full((1, N_CELLS), sentinel, np.int64); cut = np.full(1, sentinel, np.int64)
    by_code = np.full((1, mc.N_COLS), sentinel, np.int64); steps_sum = np.full(1, sentinel, np.int64)
    outs = (visits, return_fx, cut, by_code, steps_sum)

    def untouched():
        return all((a == sentinel).all() for a in outs)

    def record_unchanged():
        a, b = C.c_double(), C.c_double()
        return lib.dql_diag_returns_last(C.byref(a), C.byref(b), inst) == 0 and a.value == fly0.value and b.value == sweep0.value

    def call(cfg_=c, n_tables=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, gamma_=0.99, qa_=qa, qb_=qb, visits_=visits, return_=return_fx, cut_=cut,
             by_code_=by_code, steps_sum_=steps_sum):
        return lib.dql_returns(C.byref(cfg_), 0, n_tables, envs, episodes_, rck.SEED, max_steps_, eps_, gamma_, ptr(qa_), ptr(qb_), ptr(visits_), ptr(return_), ptr(cut_),
                               ptr(by_code_), ptr(steps_sum_))

    refused = {
        "two axes": dict(cfg_=two), "n_tables 0": dict(n_tables=0), "n_tables 2^14 + 1": dict(n_tables=(1 << 14) + 1), "n_tables -1": dict(n_tables=-1),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100),
        "episodes 0": dict(episodes_=0), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "max_steps 4097": dict(max_steps_=4097),
        "eps -0.1": dict(eps_=-0.1), "eps 1.5": dict(eps_=1.5), "eps nan": dict(eps_=float("nan")),
        "gamma -0.1": dict(gamma_=-0.1), "gamma 1.5": dict(gamma_=1.5), "gamma nan": dict(gamma_=float("nan")),
        "a log of 2^29 + 2^20 words": dict(envs=1 << 20, max_steps_=512), "131 072 envs x 601 periods at gamma 0.99": dict(envs=131072, max_steps_=600),
        "16 384 envs x 601 periods at gamma 1": dict(envs=16384, max_steps_=600, gamma_=1.0),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null visits": dict(visits_=None), "null return_fx": dict(return_=None), "null cut_decisions": dict(cut_=None),
        "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None),
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert msg.startswith("dql_returns: ") and "nothing was launched" in msg and msg.rstrip().endswith("launched"), f"{what}: {msg!r}"
        assert untouched() and record_unchanged(), what
    bad_cfg = rck.case_args("D")[0]
    bad_cfg.working_curriculum_step = 9  # check_config applies as in dql_create
    cb = bad_cfg.to_c()
    assert call(cfg_=cb) == _lib.EINVAL and untouched()
    for kw in (dict(envs_per_table=100), dict(eps=1.5), dict(gamma=1.5), dict(episodes=0), dict(max_steps=4097), dict(envs_per_table=131072, max_steps=600)):
        args = dict(envs_per_table=n, seed=rck.SEED, eps=eps, gamma=0.99)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.returns_map(cfg, qa, qb, **args)

    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), 20, seed=7)
    try:
        def ecall(first=0, count=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, gamma_=0.99, cfg_=c, visits_=visits, return_=return_fx, cut_=cut, by_code_=by_code,
                  steps_sum_=steps_sum):
            return lib.dql_ensemble_returns(ens._h, C.byref(cfg_), first, count, envs, episodes_, rck.SEED, max_steps_, eps_, gamma_, ptr(visits_), ptr(return_), ptr(cut_),
                                            ptr(by_code_), ptr(steps_sum_))

        erefused = {
            "two axes": dict(cfg_=two), "count 0": dict(count=0), "first -1": dict(first=-1), "slice beyond the end": dict(first=19, count=2),
            "first beyond the end": dict(first=21), "envs 100": dict(envs=100), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "eps 2": dict(eps_=2.0),
            "gamma 2": dict(gamma_=2.0), "null visits": dict(visits_=None), "null cut_decisions": dict(cut_=None), "null steps_sum": dict(steps_sum_=None),
        }
        for what, kw in erefused.items():
            rcode = ecall(**kw)
            msg = lib.dql_last_error().decode()
            assert rcode == _lib.EINVAL, f"ensemble, {what}: returned {rcode}"
            assert "dql_ensemble_returns" in msg and "nothing was launched" in msg, f"ensemble, {what}: {msg!r}"
            assert untouched() and record_unchanged(), what
        assert lib.dql_ensemble_returns(None, C.byref(c), 0, 1, n, episodes, rck.SEED, max_steps, eps, 0.99, ptr(visits), ptr(return_fx), ptr(cut), ptr(by_code),
                                        ptr(steps_sum)) == _lib.EINVAL
        assert untouched()
        assert ecall() == 0 and not untouched() and int(by_code.sum()) == n * episodes  # and the same arguments, well-formed, do run
    finally:
        ens.close()
    for a in outs:
        a[:] = sentinel
    assert call() == 0
    for f, a in zip(rck.FIELDS, outs):
        assert np.array_equal(a.reshape(good[f].shape), good[f]), f
    rck.assert_returns_set_equal(fly("D", 0.99), 0, rck.yardstick("D", 0.99), "after the refusals")
