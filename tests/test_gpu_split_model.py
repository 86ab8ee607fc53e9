"""The split transition-model operator on the device (dql_model_split / dql_ensemble_model_split, k_model_split) against the stepwise yardstick of
tests/split_model_checks.py: one oracle per case stepped with external actions, every feature's field read before each step.  Every comparison is ==.  The
yardstick asserts first, on its own recorded decisions, that what a kernel can get wrong occurred (split_model_checks.flight): both halves used, a value equal to
its cut, one wave holding the same (cell, s') in both halves in one period, an episode's first decision whose "before" differs from its "after"."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import model_checks as mc
import rollout_checks as rc
import split_model_checks as sc

pytestmark = pytest.mark.gpu

SHARED = ("pairs", "reward_fx", "terminal")


def fly(case_id, feature, cut, timing=None):
    cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
    return ops.split_model(cfg, tables[0], tables[1], n, sc.SEED, eps, feature, cut, episodes=episodes, max_steps=max_steps, timing=timing)


@pytest.mark.parametrize("case_id", sc.CASE_IDS)
def test_every_feature_equals_the_stepwise_yardstick_in_every_output(case_id):
    cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
    d = sc.flight(case_id)
    model = ops.transition_model(cfg, tables[0], tables[1], n, sc.SEED, eps, episodes=episodes, max_steps=max_steps)
    for f, name in enumerate(sc.FEATURES):
        cut, timing = sc.cut_of(d, f), {}
        got = fly(case_id, name, cut, timing)
        what = f"case {case_id}, {name}"
        assert got["pairs"].shape == (1, 2, N_CELLS, sc.N_STATES) and got["pairs"].dtype == np.uint32 and got["terminal"].shape == (1, 2, N_CELLS, sc.N_CODES)
        assert got["reward_fx"].dtype == got["terminal"].dtype == got["feat_sum_fx"].dtype == got["visits"].dtype == got["state_visits"].dtype == np.int64
        assert got["feature"] == name and got["columns"] == ops.SCORE_COLUMNS
        assert timing["instance"] == f"k_model_split<{'float' if cfg.dtype == F32 else 'double'}, 0, 1>" and timing["kernel_ms"] > 0.0
        sc.assert_split_set_equal(got, 0, sc.expected(d, f, cut), what)
        # the halves summed == ops.transition_model with the same arguments, in every shared output: the split changes no flight
        for field in SHARED:
            assert np.array_equal(got[field][0].astype(np.int64).sum(axis=0), model[field][0].astype(np.int64)), f"{what}: the halves of {field} do not sum to the model's"
        assert np.array_equal(got["by_code"], model["by_code"]) and np.array_equal(got["steps_sum"], model["steps_sum"]), what
        again = fly(case_id, f, cut)
        for field in sc.FIELDS:
            assert got[field].tobytes() == again[field].tobytes(), f"{what}: {field} differs between two runs"


@pytest.mark.parametrize("case_id", ["A", "B64"])
def test_a_value_equal_to_its_cut_is_in_half_one(case_id):
    d = sc.flight(case_id)
    f, cut = sc.EQUAL_TO_CUT_FEATURE, sc.equal_to_cut(d)
    got = fly(case_id, f, cut)
    sc.assert_split_set_equal(got, 0, sc.expected(d, f, cut), f"case {case_id}, crafted cut")
    assert not np.array_equal(got["visits"][0], sc.expected(d, f, cut, strict=True)["visits"]), "`>` would have given the same result"


@pytest.mark.parametrize("case_id", ["A", "B64"])
def test_infinite_cuts_send_everything_to_one_half(case_id):
    d = sc.flight(case_id)
    for cut, empty in ((np.inf, 1), (-np.inf, 0)):
        got = fly(case_id, "pitch_sp", cut)
        sc.assert_split_set_equal(got, 0, sc.expected(d, sc.FEATURES.index("pitch_sp"), cut), f"case {case_id}, cut {cut}")
        assert not got["pairs"][0, empty].any() and not got["terminal"][0, empty].any() and not got["reward_fx"][0, empty].any(), cut
        assert got["visits"][0, 1 - empty].sum() == d["env"].size
    assert np.array_equal(ops.split_cut_array(np.inf), np.full(sc.N_STATES, np.inf))


def test_three_table_sets_in_one_call_equal_three_calls():
    """and a set's tables hold nothing of its neighbours: the sets fly differently, and each equals the call that flew it alone"""
    cfg, _, eps, n, max_steps, episodes = mc.case_args("A")
    d = sc.flight("A")
    f = sc.FEATURES.index("obs_v_x")
    cut = sc.cut_of(d, f)
    sets = rc.three_table_sets()
    qa, qb = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    got = ops.split_model(cfg, qa, qb, n, sc.SEED, eps, f, cut, episodes=episodes, max_steps=max_steps)
    assert got["pairs"].shape == (3, 2, N_CELLS, sc.N_STATES) and got["feat_sum_fx"].shape == (3, sc.N_STATES)
    sc.assert_split_set_equal(got, 0, sc.expected(d, f, cut), "set 0 of three")
    for k, s in enumerate(sets):
        alone = ops.split_model(cfg, s[0], s[1], n, sc.SEED, eps, f, cut, episodes=episodes, max_steps=max_steps)
        for field in sc.FIELDS:
            assert np.array_equal(got[field][k], alone[field][0]), f"set {k}: {field}"
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1)):  # pairs that one set counts and its neighbour never does, in both directions
        assert ((got["pairs"][a] > 0) & (got["pairs"][b] == 0)).any(), (a, b)


def ensemble_snapshot(ens):
    qa, qb, cnt = ens.get_tables()
    c = ens.counters()
    st = ens.state()
    return {"qa": qa, "qb": qb, "count": cnt, "period": np.array(ens.period_index()), **{f"c_{k}": np.asarray(v) for k, v in c.items()}, **{f"s_{k}": v for k, v in st.items()}}


def test_ensemble_is_split_where_it_lives_and_left_as_it_was():
    """SequentialEnsemble.split_model of a slice == ops.split_model on the fetched tables; state, tables, counters and period index unchanged"""
    L, n, first, count = 70, 64, 62, 4  # the slice spans the second wave's first learner
    sets = rc.three_table_sets()
    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), L, seed=7)
    try:
        ens.run(300)
        for at, t in ((62, sets[0]), (63, sets[2]), (64, sets[0])):
            ens.set_tables(t[0], t[1], first=at)
        qa, qb, _ = ens.get_tables()
        before = ensemble_snapshot(ens)
        cut = np.linspace(-0.2, 0.2, sc.N_STATES)
        for eval_cfg in (simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), training_config(4, quirks=Q_PAPER, dtype=F64)):
            want = ops.split_model(eval_cfg, qa[first:first + count], qb[first:first + count], n, sc.SEED, 0.1, "pitch_sp", cut, episodes=2, max_steps=200)
            assert want["pairs"][1].tolist() != want["pairs"][2].tolist(), "neighbouring learners must fly differently for the slice to show an offset"
            assert want["visits"][:, 0].sum() > 0 and want["visits"][:, 1].sum() > 0
            got = ens.split_model(eval_cfg, "pitch_sp", cut, n, sc.SEED, 0.1, episodes=2, max_steps=200, first=first, count=count)
            for field in sc.FIELDS:
                assert got[field].dtype == want[field].dtype and np.array_equal(got[field], want[field]), field
            after = ensemble_snapshot(ens)
            assert after.keys() == before.keys()
            for k in before:
                assert np.ascontiguousarray(after[k]).tobytes() == np.ascontiguousarray(before[k]).tobytes(), f"after split_model: {k} differs"
        with pytest.raises(ValueError):
            ens.split_model(simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32), "pitch_sp", cut, n, sc.SEED, 0.1, first=0, count=9)
        assert ens.index_faults() == 0
    finally:
        ens.close()


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """each refusal returns DQL_EINVAL with a whole sentence that says nothing was launched, leaves the output arrays untouched and the latest-kernel record as it
    was; after them a valid call still equals the yardstick"""
    lib = _lib.load()
    cfg, tables, eps, n, max_steps, episodes = mc.case_args("D")
    d = sc.flight("D")
    f = sc.FEATURES.index("obs_v_x")
    cut = sc.cut_of(d, f)
    qa, qb = (np.ascontiguousarray(t, np.float64) for t in tables)
    good = fly("D", f, cut, {})
    ms0, inst = C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_model_split_last(C.byref(ms0), inst) == 0 and list(inst) == [4, 0, 1]
    c = cfg.to_c()
    two = simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32).to_c()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sentinel = 77
    pairs = np.full((1, 2, N_CELLS, sc.N_STATES), sentinel, np.uint32); reward_fx = np.full((1, 2, N_CELLS), sentinel, np.int64)
    terminal = np.full((1, 2, N_CELLS, sc.N_CODES), sentinel, np.int64); feat = np.full((1, sc.N_STATES), sentinel, np.int64)
    by_code = np.full((1, sc.N_COLS), sentinel, np.int64); steps_sum = np.full(1, sentinel, np.int64)
    outs = (pairs, reward_fx, terminal, feat, by_code, steps_sum)
    nan_cut = cut.copy(); nan_cut[944] = np.nan

    def untouched():
        return all((a == sentinel).all() for a in outs)

    def record_unchanged():
        a = C.c_double()
        return lib.dql_diag_model_split_last(C.byref(a), inst) == 0 and a.value == ms0.value

    def call(cfg_=c, n_tables=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, feature_=f, cut_=cut, qa_=qa, qb_=qb, pairs_=pairs, reward_=reward_fx,
             terminal_=terminal, feat_=feat, by_code_=by_code, steps_sum_=steps_sum):
        return lib.dql_model_split(C.byref(cfg_), 0, n_tables, envs, episodes_, sc.SEED, max_steps_, eps_, feature_, ptr(cut_), ptr(qa_), ptr(qb_), ptr(pairs_), ptr(reward_),
                                   ptr(terminal_), ptr(feat_), ptr(by_code_), ptr(steps_sum_))

    refused = {
        "two axes": dict(cfg_=two), "n_tables 0": dict(n_tables=0), "n_tables 9": dict(n_tables=9), "n_tables -1": dict(n_tables=-1),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100),
        "2^18 envs x 4096 periods": dict(envs=1 << 18, max_steps_=4095), "2^20 envs x 4096 periods": dict(envs=1 << 20, max_steps_=4095),
        "episodes 0": dict(episodes_=0), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "max_steps 4097": dict(max_steps_=4097),
        "eps -0.1": dict(eps_=-0.1), "eps 1.5": dict(eps_=1.5), "eps nan": dict(eps_=float("nan")),
        "feature -1": dict(feature_=-1), "feature 11": dict(feature_=11), "null cut": dict(cut_=None), "a NaN in cut": dict(cut_=nan_cut),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null pairs": dict(pairs_=None), "null reward_fx": dict(reward_=None), "null terminal": dict(terminal_=None),
        "null feat_sum_fx": dict(feat_=None), "null by_code": dict(by_code_=None), "null steps_sum": dict(steps_sum_=None),
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_model_split" in msg and "nothing was launched" in msg and msg.rstrip().endswith("launched"), f"{what}: {msg!r}"
        assert untouched() and record_unchanged(), what

    ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), 20, seed=7)
    try:
        def ecall(first=0, count=1, envs=n, episodes_=episodes, max_steps_=max_steps, eps_=eps, cfg_=c, feature_=f, cut_=cut, pairs_=pairs, feat_=feat, steps_sum_=steps_sum):
            return lib.dql_ensemble_model_split(ens._h, C.byref(cfg_), first, count, envs, episodes_, sc.SEED, max_steps_, eps_, feature_, ptr(cut_), ptr(pairs_), ptr(reward_fx),
                                                ptr(terminal), ptr(feat_), ptr(by_code), ptr(steps_sum_))

        erefused = {
            "two axes": dict(cfg_=two), "count 0": dict(count=0), "count 9": dict(count=9), "first -1": dict(first=-1), "slice beyond the end": dict(first=19, count=2),
            "first beyond the end": dict(first=21), "envs 100": dict(envs=100), "episodes 65": dict(episodes_=65), "max_steps 0": dict(max_steps_=0), "eps 2": dict(eps_=2.0),
            "feature 11": dict(feature_=11), "null cut": dict(cut_=None), "a NaN in cut": dict(cut_=nan_cut), "null pairs": dict(pairs_=None),
            "null feat_sum_fx": dict(feat_=None), "null steps_sum": dict(steps_sum_=None),
        }
        for what, kw in erefused.items():
            rcode = ecall(**kw)
            msg = lib.dql_last_error().decode()
            assert rcode == _lib.EINVAL, f"ensemble, {what}: returned {rcode}"
            assert "dql_ensemble_model_split" in msg and "nothing was launched" in msg, f"ensemble, {what}: {msg!r}"
            assert untouched() and record_unchanged(), what
        assert ecall() == 0 and not untouched() and int(by_code.sum()) == n * episodes  # and the same arguments, well-formed, do run
    finally:
        ens.close()
    for a in outs:
        a[:] = sentinel
    assert call() == 0
    for field, a in zip(("pairs", "reward_fx", "terminal", "feat_sum_fx", "by_code", "steps_sum"), outs):
        assert np.array_equal(a, good[field]), field
    sc.assert_split_set_equal(fly("D", f, cut), 0, sc.expected(d, f, cut), "after the refusals")
