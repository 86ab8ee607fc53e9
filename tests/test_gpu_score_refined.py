"""Greedy scoring of refined table sets on the device (dql_score_refined / dql_ensemble_score_refined / k_score_refined) against the stepwise
flight of tests/refined_checks.py — the unchanged oracle stepped with external actions, the greedy row that of half * 945 + idx_x — and against the shipped
`ops.score`.  Every comparison is `==`: by_code, steps_sum and both episode logs.  The yardsticks are flown once per module (refined_checks caches them)."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import ensemble_checks as ec
import refined_checks as rc

pytestmark = pytest.mark.gpu
F = rc.F


@pytest.mark.parametrize("feature", rc.FEATURES)
@pytest.mark.parametrize("case_id", rc.SCORE_CASES)
def test_scoring_equals_the_stepwise_flight(case_id, feature):
    f = F[feature]
    want = rc.score_yardstick(case_id, f)
    cfg, n, max_steps, episodes = rc.score_case(case_id)
    qa, qb = rc.score_tables(1)
    timing = {}
    got = ops.score_refined(cfg, qa, qb, feature, rc.score_cut(case_id, f), n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True, timing=timing)
    rc.assert_score_equal(got, 0, want, n, f"case {case_id} {feature}")
    assert timing["instance"] == "k_score_refined<float, 0, 1>" and timing["kernel_ms"] > 0.0 and got["feature"] == feature


def test_pitch_sp_at_the_scalar_cut_zero_and_in_float64():
    cfg, n, max_steps, episodes = rc.score_case("A")
    qa, qb = rc.score_tables(1)
    f = F["pitch_sp"]
    want = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, 0.0, n, rc.SCORE_SEED, max_steps, episodes)
    strict = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, 0.0, n, rc.SCORE_SEED, max_steps, episodes, strict=True)
    assert want["on_cut"] > 0 and (not np.array_equal(want["ep_steps"], strict["ep_steps"]) or not np.array_equal(want["ep_code"], strict["ep_code"]))
    got = ops.score_refined(cfg, qa, qb, "pitch_sp", 0.0, n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True)
    rc.assert_score_equal(got, 0, want, n, "pitch_sp at cut 0.0")
    cfg64 = training_config(4, dtype=F64, quirks=ec.Q_PAPER)
    want64 = rc.stepwise_refined_score(cfg64, qa[0], qb[0], f, rc.mean_cut("B64", f), 64, rc.SCORE_SEED, 200, 1)
    assert min(want64["reads"]) > 0
    timing = {}
    got64 = ops.score_refined(cfg64, qa, qb, "pitch_sp", rc.mean_cut("B64", f), 64, rc.SCORE_SEED, episodes=1, max_steps=200, log=True, timing=timing)
    rc.assert_score_equal(got64, 0, want64, 64, "float64")
    assert timing["instance"] == "k_score_refined<double, 0, 1>"


# ---- properties against the shipped kernels, no reference loop ----
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_equal_halves_are_ops_score_and_infinite_cuts_pick_a_half(dtype):
    cfg = simulation_config(working_curriculum_step=4, dtype=dtype, quirks=ec.Q_PAPER)
    n, max_steps, episodes = 128, 300, 2
    qa, qb = rc.score_tables(3)
    plain = [ops.score(cfg, qa[:, h], qb[:, h], n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True) for h in range(2)]
    assert not np.array_equal(plain[0]["ep_steps"], plain[1]["ep_steps"]), "the two halves fly alike: the case shows nothing"

    def same(got, want, what):
        for k in ("by_code", "steps_sum", "ep_code", "ep_steps"):
            assert np.array_equal(got[k], want[k]), f"{what}: {k}"

    for h in range(2):
        both = np.ascontiguousarray(np.repeat(qa[:, h:h + 1], 2, axis=1)), np.ascontiguousarray(np.repeat(qb[:, h:h + 1], 2, axis=1))
        for feature in rc.FEATURES:
            got = ops.score_refined(cfg, *both, feature, rc.mean_cut("A", F[feature]), n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True)
            same(got, plain[h], f"both halves = half {h}, {feature}")
    for cut, h in ((np.inf, 0), (-np.inf, 1)):
        got = ops.score_refined(cfg, qa, qb, "obs_a_x", cut, n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True)
        same(got, plain[h], f"cut {cut}")
    # three sets in one call == three calls
    cut = rc.mean_cut("A", F["pitch_sp"])
    three = ops.score_refined(cfg, qa, qb, "pitch_sp", cut, n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True)
    for k in range(3):
        one = ops.score_refined(cfg, qa[k], qb[k], "pitch_sp", cut, n, rc.SCORE_SEED, episodes=episodes, max_steps=max_steps, log=True)
        assert np.array_equal(three["by_code"][k], one["by_code"][0]) and three["steps_sum"][k] == one["steps_sum"][0]
        assert np.array_equal(three["ep_code"][:, k * n:(k + 1) * n], one["ep_code"]) and np.array_equal(three["ep_steps"][:, k * n:(k + 1) * n], one["ep_steps"])
    assert not np.array_equal(three["ep_steps"][:, :n], plain[0]["ep_steps"][:, :n]) and not np.array_equal(three["ep_steps"][:, :n], plain[1]["ep_steps"][:, :n]), \
        "pitch_sp at its mean cut flies like one half alone"


def test_an_ensemble_scores_its_resident_refined_tables_in_place():
    """a slice crossing a wave's first learner == ops.score_refined on the fetched tables; the ensemble's bytes are unchanged"""
    n_l = 70
    cfg = training_config(4, quirks=ec.Q_PAPER, dtype=F32)
    f = F["pitch_sp"]
    cut = rc.mean_cut("B64", f)
    ens = SequentialEnsemble(cfg, n_l, seed=5, log_capacity=8, eps=[0.0], window=4, min_successes=2, max_episodes=6)
    try:
        ens.set_refinement("pitch_sp", cut)
        ens.set_refined_tables(*rc.refined_trained_tables(n_l))
        ens.run(60)
        before = rc.refined_ensemble_result(ens)
        eval_cfg = simulation_config(working_curriculum_step=4, dtype=F32, quirks=ec.Q_PAPER)
        got = ens.score_refined(eval_cfg, 64, seed=9, episodes=2, max_steps=250, log=True, first=62, count=5)
        qa, qb, _ = ens.get_refined_tables(first=62, count=5)
        want = ops.score_refined(eval_cfg, qa, qb, "pitch_sp", cut, 64, 9, episodes=2, max_steps=250, log=True)
        for k in ("by_code", "steps_sum", "ep_code", "ep_steps"):
            assert np.array_equal(got[k], want[k]), k
        assert got["by_code"].sum() == 5 * 64 * 2 and len({tuple(r) for r in got["by_code"].tolist()}) > 1
        ec.assert_equal(rc.refined_ensemble_result(ens), before, "the ensemble after score_refined")
        assert ens.period_index() == 60 and ens.index_faults() == 0
        with pytest.raises(ValueError):
            ens.score_refined(eval_cfg, 64, first=68, count=5)
        with pytest.raises(ValueError):
            ens.score_refined(simulation_config(working_curriculum_step=4, dtype=F32, two_axis=1), 64)
    finally:
        ens.close()


def test_refused_calls_launch_nothing_and_a_good_call_succeeds_afterwards():
    lib = _lib.load()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    cfg = training_config(4, dtype=F32, quirks=ec.Q_PAPER)
    qa, qb = rc.score_tables(1)
    cut = np.full(945, 0.1)
    by_code, steps = np.full((1, 10), -3, np.int64), np.full(1, -3, np.int64)
    ep_c, ep_s = np.full((1, 64), 9, np.uint8), np.full((1, 64), 9, np.uint16)
    c = cfg.to_c()

    def call(cfg_c=c, n_tables=1, n=64, episodes=1, max_steps=50, feature=4, cut_p=p(cut), qa_p=p(qa), qb_p=p(qb), bc=p(by_code), st=p(steps), ec_=p(ep_c), es=p(ep_s)):
        return lib.dql_score_refined(C.byref(cfg_c), 0, n_tables, n, episodes, 1, max_steps, feature, cut_p, qa_p, qb_p, bc, st, ec_, es)

    bad_cut = cut.copy(); bad_cut[944] = np.nan
    two, eight = training_config(4, dtype=F32, two_axis=1).to_c(), training_config(4, dtype=F32, trajectory=1).to_c()
    for kw, word in ((dict(cfg_c=two), "two-axis"), (dict(cfg_c=eight), "figure-eight"), (dict(feature=-1), "feature"), (dict(feature=11), "feature"),
                     (dict(cut_p=None), "null"), (dict(cut_p=p(bad_cut)), "NaN"), (dict(n_tables=0), "table sets"), (dict(n_tables=4097), "DQL_SCORE_REFINED_MAX_TABLES"),
                     (dict(n=63), "multiple of 64"), (dict(episodes=0), "episodes_per_env"), (dict(episodes=65), "episodes_per_env"), (dict(max_steps=0), "max_steps"),
                     (dict(max_steps=4097), "max_steps"), (dict(qa_p=None), "null"), (dict(qb_p=None), "null"), (dict(bc=None), "null"), (dict(st=None), "null"),
                     (dict(ec_=None), "both arrays"), (dict(es=None), "both arrays")):
        assert call(**kw) == _lib.EINVAL, kw
        msg = lib.dql_last_error().decode()
        assert msg.startswith("dql_score_refined:") and word in msg and "nothing was launched" in msg, msg
    assert (by_code == -3).all() and (steps == -3).all() and (ep_c == 9).all() and (ep_s == 9).all(), "a refused call touched an output"
    for bad_call in (lambda: ops.score_refined(cfg, qa, qb, "nope", cut, 64, 1), lambda: ops.score_refined(cfg, qa, qb, 4, bad_cut, 64, 1),
                     lambda: ops.score_refined(cfg, qa[:, 0], qb[:, 0], 4, cut, 64, 1), lambda: ops.score_refined(cfg, qa, qb, 4, np.zeros(3), 64, 1),
                     lambda: ops.score_refined(training_config(4, two_axis=1), qa, qb, 4, cut, 64, 1), lambda: ops.score_refined(cfg, qa, qb, 4, cut, 63, 1)):
        with pytest.raises(ValueError):
            bad_call()
    assert call() == 0 and by_code.sum() == 64 and (ep_c != 9).any()
