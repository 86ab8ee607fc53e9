"""The roll-out operator on the device (dql_rollout / k_rollout) against a real Engine driven one agent period at a time: the equality contract of
include/dql.h — at the first period after which env i has FL_DONE, its code, step count and record fields are row (k, i) of the roll-out, bit for bit —
in float32 (4 096 envs) and float64 (512), for the six cases of tests/test_rollout_host_emulation.py, plus the harness equalities built on it."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import F32, F64, Q_PAPER
from dql_multirotor_landing_amd.engine import Engine

import rollout_checks as rc

pytestmark = pytest.mark.gpu
SEED, MAX_STEPS = 123, 600


def n_envs_of(cfg):
    return 4096 if cfg.dtype == F32 else 512


def engine_yardstick(cfg, tables, n, seed=SEED, max_steps=MAX_STEPS, trace_envs=0, block=0):
    eng = Engine(cfg, n, seed=seed)
    try:
        if block:
            eng.set_option("block", block)
        want = rc.stepwise_first_episodes(eng, tables, max_steps, trace_envs)
        want["instance"] = eng.step_instance()
        return want
    finally:
        eng.close()


@pytest.mark.parametrize("case_id", [c[0] for c in rc.CASES])
def test_rollout_equals_the_stepwise_engine_bit_for_bit(case_id):
    cfg = rc.case_config(case_id)
    n = n_envs_of(cfg)
    tables = rc.stage4_tables()
    want = engine_yardstick(cfg, tables, n)
    h = rc.histogram(want["code"])
    print(case_id, want["instance"], h, "longest episode", int(want["steps"].max()))
    assert h["unfinished"] == 0 and sum(1 for k, v in h.items() if v) >= (3 if case_id.startswith("simulation") else 2), h
    got = ops.rollout(cfg, tables, n, SEED, max_steps=MAX_STEPS)
    assert got["code"].shape == (1, n) and got["trace"] is None
    rc.assert_rows_equal(got, want, case_id, row=0)


@pytest.mark.parametrize("seed", [123, 977])
def test_rollout_outcomes_and_landing_score_equal_the_stepwise_harness(seed):
    qa, qb = rc.stage4_tables()
    tables = (qa, qb, np.zeros_like(qa))
    for flavour in ("simulation", "training"):
        a = evaluation.first_episode_outcomes(tables, 4096, 4, seed=seed, flavour=flavour, quirks=Q_PAPER)
        b = evaluation.rollout_outcomes(tables, 4096, 4, seed=seed, flavour=flavour, quirks=Q_PAPER)
        print(seed, flavour, a)
        assert a == b and a["unfinished"] == 0
    s = evaluation.landing_score(tables, seed=seed)
    assert evaluation.landing_score(tables, seed=seed, method="rollout") == s
    assert evaluation.landing_scores([tables], seed=seed) == [s]
    assert 0.5 < s["touchdown_rate"] < 1.0 and 0.5 < s["goal_hold_rate"] <= 1.0


def test_three_table_sets_equal_three_single_calls_and_sixteen_sets_run():
    cfg = rc.case_config("simulation-f32")
    n = 4096
    sets = rc.three_table_sets()
    got = ops.rollout(cfg, sets, n, SEED)
    assert got["code"].shape == (3, n)
    singles = [ops.rollout(cfg, t, n, SEED) for t in sets]
    fields = ("code", "steps") + rc.RECORD_FIELDS
    for k, s in enumerate(singles):
        rc.assert_rows_equal(got, {f: s[f][0] for f in fields}, f"table set {k} of 3 vs its single call", row=k)
    assert rc.histogram(got["code"][0]) != rc.histogram(got["code"][1])
    big = ops.rollout(cfg, [sets[k % 3] for k in range(16)], n, SEED)
    assert big["code"].shape == (16, n)
    for k in range(16):
        rc.assert_rows_equal(big, {f: singles[k % 3][f][0] for f in fields}, f"table set {k} of 16", row=k)
    scores = evaluation.landing_scores([(t[0], t[1]) for t in sets])
    assert scores[0] == evaluation.landing_score((sets[0][0], sets[0][1], None)) and len(scores) == 3


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-f64"])
def test_cut_off_at_200_steps_matches_the_unfinished_rows(case_id):
    cfg = rc.case_config(case_id)
    n = n_envs_of(cfg)
    tables = rc.stage4_tables()
    want = engine_yardstick(cfg, tables, n, max_steps=200)
    unfinished = int((want["code"] < 0).sum())
    print(case_id, "unfinished after 200 steps:", unfinished, "of", n)
    assert 0.10 * n <= unfinished <= 0.90 * n, f"{unfinished} of {n} unfinished on the stepwise yardstick"
    got = ops.rollout(cfg, tables, n, SEED, max_steps=200)
    assert int((got["code"][0] < 0).sum()) == unfinished and (got["steps"][0][got["code"][0] < 0] == 200).all()
    rc.assert_rows_equal(got, want, f"{case_id} cut at 200", row=0)


@pytest.mark.parametrize("trace_envs", [8, 64])
@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-two-axis-f32", "training4-f64"])
def test_trace_matches_get_fields_after_every_stepwise_period(case_id, trace_envs):
    cfg = rc.case_config(case_id)
    n = 512
    tables = rc.stage4_tables()
    want = engine_yardstick(cfg, tables, n, trace_envs=trace_envs)
    got = ops.rollout(cfg, tables, n, SEED, max_steps=MAX_STEPS, trace_envs=trace_envs)
    assert got["trace"].shape == (MAX_STEPS + 1, len(rc.TRACE_FIELDS), trace_envs) and got["trace_fields"] == rc.TRACE_FIELDS
    assert np.isnan(got["trace"][-1]).all() and not np.isnan(got["trace"][0]).any()
    rc.assert_trace_equal(got["trace"], want["trace"], f"{case_id} M={trace_envs}")
    rc.assert_rows_equal(got, want, case_id, row=0)


def test_the_contract_does_not_depend_on_the_yardstick_s_block_layout():
    cfg = rc.case_config("simulation-f32")
    n = 4096
    tables = rc.stage4_tables()
    got = ops.rollout(cfg, tables, n, SEED)
    seen = set()
    for block in (64, 256):
        want = engine_yardstick(cfg, tables, n, block=block)
        seen.add(want["instance"])
        rc.assert_rows_equal(got, want, f"stepwise engine forced to block {block} ({want['instance']})", row=0)
    assert len(seen) == 2, seen


def test_every_refused_call_returns_einval_and_starts_no_kernel():
    """argument checks on the host side of the ABI: each returns DQL_EINVAL with a dql_last_error text that says nothing was launched, leaves the output
    arrays untouched, and the latest-kernel record (dql_diag_rollout_last) still describes the good call made before"""
    lib = _lib.load()
    cfg = rc.case_config("simulation-f32")
    n = 64
    qa, qb = (np.ascontiguousarray(t) for t in rc.stage4_tables())
    good = ops.rollout(cfg, (qa, qb), n, SEED, max_steps=5, timing={})
    assert (good["code"] == -1).all()
    ms0, inst = C.c_double(), (C.c_int32 * 3)()
    assert lib.dql_diag_rollout_last(C.byref(ms0), inst) == 0
    c = cfg.to_c()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    sentinel = -77
    code = np.full(16 * n, sentinel, np.int32); steps = np.full(16 * n, sentinel, np.int32); rec = np.full((19, 16 * n), float(sentinel)); trace = np.full((601, 22, 64), float(sentinel))

    def call(n_tables=1, envs=n, max_steps=600, trace_envs=0, qa_=qa, qb_=qb, code_=code, steps_=steps, rec_=rec, trace_=None):
        ptr = lambda a: None if a is None else p(a)
        return lib.dql_rollout(C.byref(c), 0, n_tables, envs, SEED, max_steps, ptr(qa_), ptr(qb_), ptr(code_), ptr(steps_), ptr(rec_), trace_envs, ptr(trace_))

    refused = {
        "n_tables 0": dict(n_tables=0), "n_tables 17": dict(n_tables=17),
        "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100),
        "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
        "trace_envs -1": dict(trace_envs=-1, trace_=trace), "trace_envs 65": dict(trace_envs=65, trace_=trace),
        "trace without a buffer": dict(trace_envs=8, trace_=None),
        "null qa": dict(qa_=None), "null qb": dict(qb_=None), "null code": dict(code_=None), "null steps": dict(steps_=None), "null rec": dict(rec_=None),
    }
    for what, kw in refused.items():
        rcode = call(**kw)
        msg = lib.dql_last_error().decode()
        assert rcode == _lib.EINVAL, f"{what}: returned {rcode}"
        assert "dql_rollout" in msg and "nothing was launched" in msg, f"{what}: {msg!r}"
        assert (code == sentinel).all() and (steps == sentinel).all() and (rec == sentinel).all() and (trace == sentinel).all(), what
        ms1 = C.c_double()
        assert lib.dql_diag_rollout_last(C.byref(ms1), inst) == 0 and ms1.value == ms0.value, what
    bad_cfg = rc.case_config("simulation-f32")
    bad_cfg.working_curriculum_step = 9  # check_config applies as in dql_create
    cb = bad_cfg.to_c()
    assert lib.dql_rollout(C.byref(cb), 0, 1, n, SEED, 600, p(qa), p(qb), p(code), p(steps), p(rec), 0, None) == _lib.EINVAL
    assert (code == sentinel).all()
    assert call(max_steps=5) == 0 and np.array_equal(code[:n], good["code"][0])  # and the same arguments, well-formed, do run
