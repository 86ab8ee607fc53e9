"""The refined-state bodies (csrc/dql_refined.hpp: refined_learner_periods, score_refined_episodes) run on the CPU and held `==` to the yardsticks of
tests/refined_checks.py, which are built from the unchanged oracle (CPU only, no GPU).

tests/host_emu/refined_emu.cpp compiles the real device headers as host C++ and flies every learner (mode 0: stages of launches at a level, transfer by hand
between them) or every env of every refined table set (mode 1) lane by lane, as k_learn_refined and k_score_refined do.  Built twice through
tests/host_emu_harness.py: plain, and as a stand-alone program with ASan + UBSan (any report fails); every case goes through both builds.  The job header is
this module's own (`learner_job`, `score_job`)."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config

import ensemble_checks as ec
import host_emu_harness as heh
import refined_checks as rc

LOG_CAP = rc.LOG_CAP
BUILDS = ("plain", "san")
emu = heh.emu_fixture("refined_emu")
F = rc.F


def _head(cfg, mode, feature, w4, w5, w6, w7, n, seed, cut):
    c = bytes(cfg.to_c())
    cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cut, np.float64), (rc.N_STATES,)))
    return struct.pack("<8i", len(c), cfg.dtype, mode, feature, w4, w5, w6, w7) + struct.pack("<2q", n, seed) + c + cut.tobytes()


def learner_job(cfg, n, seed, feature, cut, stages, log_capacity=LOG_CAP, tables=None, alpha=None):
    """stages: dicts {level, runs, eps, window, min_successes, max_episodes, transfer (a ratio, or None)}"""
    alpha = cfg.alpha_table() if alpha is None else alpha
    job = _head(cfg, 0, feature, len(stages), log_capacity, int(tables is not None), len(alpha), n, seed, cut) + np.ascontiguousarray(alpha, np.float64).tobytes()
    for s in stages:
        runs, eps = list(s["runs"]), np.ascontiguousarray(s["eps"], np.float64)
        job += struct.pack("<12i", s["level"], len(runs), *runs, *[0] * (4 - len(runs)), eps.size, s["window"], s["min_successes"], s["max_episodes"],
                           int(s.get("transfer") is not None), 0)
        job += struct.pack("<d", float(s.get("transfer") or 0.0)) + eps.tobytes()
    for t in tables or ():
        job += np.ascontiguousarray(t, np.float64).tobytes()
    return job


def learner_result(b, n, log_capacity, periods):
    reader = heh.Reader(b)
    take = reader.take
    out = {"qa": take(np.float64, (n, 2, N_CELLS)), "qb": take(np.float64, (n, 2, N_CELLS)), "count": take(np.float64, (n, 2, N_CELLS)),
           "decisions": take(np.int64, (n,)), "by_code": take(np.int64, (ec.N_CODES, n)), "episodes": take(np.int32, (n,)), "successes": take(np.int32, (n,)),
           "level_episodes": take(np.int32, (n,)), "promotion_episode": take(np.int32, (n,)), "frozen": take(np.int32, (n,)), "log_n": take(np.int32, (n,)),
           "log_code": take(np.uint8, (n, log_capacity)), "log_len": take(np.uint16, (n, log_capacity))}
    reals, ints = take(np.float64, (heh.NF_REAL, n)), take(np.int32, (heh.NF_INT, n))
    faults = take(np.int64, (1,))
    half = take(np.uint8, (n,))
    j = take(np.int64, (1,))
    reader.done()
    assert faults[0] == 0, "a range check counted a fault: an update was dropped"
    assert int(j[0]) == periods and (half < 2).all()
    ref = ec.Reference(training_config(0), 1, 0)
    out.update({f: reals[k] for f, k in ref.ri.items()})
    out.update({f: ints[k] for f, k in ref.ii.items()})
    return out, half


def one_stage(cfg, runs, eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30):
    return [dict(level=cfg.working_curriculum_step, runs=runs, eps=eps, window=window, min_successes=min_successes, max_episodes=max_episodes)]


def run_learners(exe, cfg, n, seed, feature, cut, stages, tmp, sanitized, tables=None):
    periods = sum(sum(s["runs"]) for s in stages)
    return learner_result(heh.run(exe, learner_job(cfg, n, seed, feature, cut, stages, tables=tables), tmp, "refined", sanitized), n, LOG_CAP, periods)


def score_job(cfg, qa, qb, feature, cut, n, seed, max_steps, episodes, log=True):
    qa, qb = (np.ascontiguousarray(t, np.float64).reshape(-1, 2, N_CELLS) for t in (qa, qb))
    return _head(cfg, 1, feature, len(qa), int(log), max_steps, episodes, n, seed, cut) + qa.tobytes() + qb.tobytes()


def run_score(exe, cfg, qa, qb, feature, cut, n, seed, max_steps, episodes, tmp, sanitized):
    K = len(np.asarray(qa).reshape(-1, 2, N_CELLS))
    r = heh.Reader(heh.run(exe, score_job(cfg, qa, qb, feature, cut, n, seed, max_steps, episodes), tmp, "refined_score", sanitized))
    out = {"by_code": r.take(np.int64, (K, ec.N_CODES + 1)), "steps_sum": r.take(np.int64, (K,)), "ep_code": r.take(np.uint8, (episodes, K * n)),
           "ep_steps": r.take(np.uint16, (episodes, K * n))}
    faults = r.take(np.int64, (1,))
    r.done()
    assert faults[0] == 0, "the scorer counted a value out of range"
    return out


# ---- (a) 3 learners from zeros, level 0, EPS_TABLE, 150 + 250 periods ----
A_L, A_SEED, A_RUNS = 3, 2024, (150, 250)


def zeros_reference(dtype, quirks, feature, cut=None, strict=False):
    return rc.zeros_reference(dtype, quirks, feature, A_L, A_SEED, sum(A_RUNS), watch=(A_RUNS[0],), cut=cut, strict=strict)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("feature", ["pitch_sp", "coin", "obs_v_x"])
@pytest.mark.parametrize("quirks", [ec.Q_REFERENCE, ec.Q_BENCH, ec.Q_PAPER], ids=["quirks-0x7f", "quirks-0x60", "quirks-0x40"])
def test_a_three_learners_from_zeros_in_two_launches_equal_the_yardstick(emu, quirks, feature, build, tmp_path):
    f = F[feature]
    want, ref, cut = zeros_reference(F32, quirks, f)
    rc.assert_learner_events(ref, f"(a) {feature} {quirks:#x}")
    if f in rc.OBS_FEATURES:  # the launch-boundary trap: a flying learner stands in half 1 at the boundary of 150 + 250
        rc.assert_half_one_at_the_boundary(ref, A_RUNS[0], feature)
    assert want["episodes"].min() >= 2 and (want["qa"][:, 0] != 0).any() and (want["qa"][:, 1] != 0).any()
    cfg = training_config(0, quirks=quirks, dtype=F32)
    got, _ = run_learners(emu[build], cfg, A_L, A_SEED, f, cut, one_stage(cfg, A_RUNS), tmp_path, build == "san")
    ec.assert_equal(got, want, f"(a) {feature} quirks {quirks:#x} {build}")


@pytest.mark.parametrize("build", BUILDS)
def test_a_pitch_sp_cut_zero_has_values_on_the_cut_and_the_strict_rule_differs(emu, build, tmp_path):
    """reset leaves the set-point at exactly 0, so value == cut is common under the scalar cut 0.0: `>=` puts those decisions in half 1, the wrong rule `>` in half 0"""
    f = F["pitch_sp"]
    want, ref, _ = zeros_reference(F32, ec.Q_PAPER, f, cut=0.0)
    wrong, _, _ = zeros_reference(F32, ec.Q_PAPER, f, cut=0.0, strict=True)
    assert ref.ev["value_on_cut"] > 0, ref.ev
    assert any(not np.array_equal(want[k], wrong[k]) for k in rc.TABLE_FIELDS), "the rule `>` gives the same tables: the case cannot tell it from `>=`"
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    got, _ = run_learners(emu[build], cfg, A_L, A_SEED, f, 0.0, one_stage(cfg, A_RUNS), tmp_path, build == "san")
    ec.assert_equal(got, want, f"(a) pitch_sp at cut 0.0 {build}")


# ---- (b) 26 learners from trained tables, level 4, 0x40, eps 0, window 4 / 2 successes / 6 episodes, 400 periods and 7 + 393 ----
B_L = 26
B_SPLIT = ec.TRAINED_LEARNERS_SPLIT


def trained_reference(dtype, feature):
    return rc.trained_reference(dtype, feature, B_L)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("feature", rc.FEATURES)
def test_b_trained_tables_400_periods_and_7_plus_393_equal_the_yardstick(emu, feature, build, tmp_path):
    f = F[feature]
    want, ref, cut, tables = trained_reference(F32, f)
    if f in rc.OBS_FEATURES:  # the launch-boundary trap: a learner that is flying at the boundary of 7 + 393 stands in half 1
        rc.assert_half_one_at_the_boundary(ref, B_SPLIT[0], feature)
    cfg = training_config(4, quirks=ec.Q_PAPER, dtype=F32)
    kw = dict(ec.TRAINED_LEARNERS_CASE); kw.pop("log_capacity")
    for runs in ((ec.TRAINED_LEARNERS_PERIODS,), B_SPLIT):
        got, _ = run_learners(emu[build], cfg, B_L, ec.TRAINED_LEARNERS_SEED, f, cut, one_stage(cfg, runs, **kw), tmp_path, build == "san", tables=tables)
        ec.assert_equal(got, want, f"(b) {feature} runs {runs} {build}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("feature", ["pitch_sp", "coin"])
def test_b_trained_tables_in_float64(emu, feature, build, tmp_path):
    f = F[feature]
    want, _, cut, tables = trained_reference(F64, f)
    cfg = training_config(4, quirks=ec.Q_PAPER, dtype=F64)
    kw = dict(ec.TRAINED_LEARNERS_CASE); kw.pop("log_capacity")
    got, _ = run_learners(emu[build], cfg, B_L, ec.TRAINED_LEARNERS_SEED, f, cut, one_stage(cfg, B_SPLIT, **kw), tmp_path, build == "san", tables=tables)
    ec.assert_equal(got, want, f"(b) float64 {feature} {build}")


def test_same_state_transitions_change_half_and_keep_both():
    """on the yardstick's records: some transition changes half with idx' == idx (no patch of the carried row), some keeps both (patch)"""
    for feature in ("pitch_sp", "obs_v_x"):
        _, ref, _, _ = trained_reference(F32, F[feature])
        assert ref.ev["same_state_other_half"] > 0 and ref.ev["same_refined_state"] > 0, (feature, ref.ev)


# ---- (c) levels 0 -> 2 through set_level / run(400) / transfer by hand, 24 learners, window 4, 6 episodes ----
C_L, C_SEED, C_PERIODS, C_RULE = rc.CURRICULUM_L, rc.CURRICULUM_SEED, rc.CURRICULUM_PERIODS, rc.CURRICULUM_RULE


def curriculum_stages():
    return [dict(level=k, runs=(C_PERIODS,), eps=rc.CURRICULUM_EPS[k], transfer=rc.CURRICULUM_RATIOS[k] if k < 2 else None, **C_RULE) for k in range(3)]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("feature", ["pitch_sp", "coin"])
def test_c_levels_0_to_2_with_transfer_by_hand_equal_the_yardstick(emu, feature, build, tmp_path):
    f = F[feature]
    want, cut = rc.curriculum_reference(f)
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    got, _ = run_learners(emu[build], cfg, C_L, C_SEED, f, cut, curriculum_stages(), tmp_path, build == "san")
    ec.assert_equal(got, want, f"(c) {feature} {build}")


# ---- (d) scoring: cases A and D x all features ----
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("feature", rc.FEATURES)
@pytest.mark.parametrize("case_id", rc.SCORE_CASES)
def test_d_scoring_equals_the_stepwise_flight(emu, case_id, feature, build, tmp_path):
    f = F[feature]
    want = rc.score_yardstick(case_id, f)
    cfg, n, max_steps, episodes = rc.score_case(case_id)
    qa, qb = rc.score_tables(1)
    got = run_score(emu[build], cfg, qa, qb, f, rc.score_cut(case_id, f), n, rc.SCORE_SEED, max_steps, episodes, tmp_path, build == "san")
    rc.assert_score_equal(got, 0, want, n, f"(d) case {case_id} {feature} {build}")


def test_d_scoring_yardstick_tells_the_wrong_rules_apart():
    """on the yardstick: always reading half 0 changes case A's result for pitch_sp; `>` for `>=` changes it under the scalar cut 0.0"""
    cfg, n, max_steps, episodes = rc.score_case("A")
    qa, qb = rc.score_tables(1)
    f = F["pitch_sp"]
    right = rc.score_yardstick("A", f)
    half0 = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, rc.score_cut("A", f), n, rc.SCORE_SEED, max_steps, episodes, always_half0=True)
    assert not np.array_equal(right["ep_steps"], half0["ep_steps"]) or not np.array_equal(right["ep_code"], half0["ep_code"])
    at0 = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, 0.0, n, rc.SCORE_SEED, max_steps, episodes)
    strict = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, 0.0, n, rc.SCORE_SEED, max_steps, episodes, strict=True)
    assert at0["on_cut"] > 0 and (not np.array_equal(at0["ep_steps"], strict["ep_steps"]) or not np.array_equal(at0["ep_code"], strict["ep_code"]))


@pytest.mark.parametrize("build", BUILDS)
def test_d_scoring_pitch_sp_at_cut_zero(emu, build, tmp_path):
    cfg, n, max_steps, episodes = rc.score_case("A")
    qa, qb = rc.score_tables(1)
    f = F["pitch_sp"]
    want = rc.stepwise_refined_score(cfg, qa[0], qb[0], f, 0.0, n, rc.SCORE_SEED, max_steps, episodes)
    got = run_score(emu[build], cfg, qa, qb, f, 0.0, n, rc.SCORE_SEED, max_steps, episodes, tmp_path, build == "san")
    rc.assert_score_equal(got, 0, want, n, f"(d) pitch_sp at cut 0.0 {build}")


# ---- (e) the properties: against the PLAIN yardsticks, no refined reference ----
PATTERN = 0.5 + np.arange(N_CELLS) * 1e-3


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("cut,used", [(np.inf, 0), (-np.inf, 1)], ids=["cut+inf", "cut-inf"])
def test_e_infinite_cut_is_the_plain_learner_in_one_half_and_leaves_the_other(emu, cut, used, build, tmp_path):
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ref = ec.Reference(cfg, A_L, A_SEED, log_capacity=LOG_CAP)
    ref.run(sum(A_RUNS))
    want = ref.result()
    tables = [np.zeros((A_L, 2, N_CELLS)) for _ in range(3)]
    for t in tables:
        t[:, 1 - used] = PATTERN
    got, _ = run_learners(emu[build], cfg, A_L, A_SEED, F["pitch_sp"], cut, one_stage(cfg, A_RUNS), tmp_path, build == "san", tables=tables)
    for k in rc.TABLE_FIELDS:
        assert np.array_equal(got[k][:, 1 - used], np.tile(PATTERN, (A_L, 1))), f"{k}: the unused half lost its planted pattern"
        got[k] = got[k][:, used]
    ec.assert_equal(got, want, f"(e) cut {cut} {build}")


@pytest.mark.parametrize("build", BUILDS)
def test_e_scoring_properties(emu, build, tmp_path):
    """both halves equal == the plain flight of those tables; +inf / -inf pick half 0's / half 1's tables; three sets in one call == three calls"""
    cfg, n, max_steps, episodes = rc.score_case("D")
    qa, qb = rc.score_tables(3)
    f = F["obs_p_x"]
    san = build == "san"
    three = run_score(emu[build], cfg, qa, qb, f, rc.score_cut("D", f), n, rc.SCORE_SEED, max_steps, episodes, tmp_path, san)
    for k in range(3):
        one = run_score(emu[build], cfg, qa[k:k + 1], qb[k:k + 1], f, rc.score_cut("D", f), n, rc.SCORE_SEED, max_steps, episodes, tmp_path, san)
        rc.assert_score_equal(three, k, {g: (one[g][0] if g in ("by_code", "steps_sum") else one[g]) for g in one}, n, f"set {k} of three")
    for cut, h in ((np.inf, 0), (-np.inf, 1)):
        both = np.ascontiguousarray(np.repeat(qa[:1, h:h + 1], 2, axis=1)), np.ascontiguousarray(np.repeat(qb[:1, h:h + 1], 2, axis=1))
        picked = run_score(emu[build], cfg, qa[:1], qb[:1], f, cut, n, rc.SCORE_SEED, max_steps, episodes, tmp_path, san)
        same = run_score(emu[build], cfg, *both, f, rc.score_cut("D", f), n, rc.SCORE_SEED, max_steps, episodes, tmp_path, san)
        plain = rc.stepwise_refined_score(cfg, both[0][0], both[1][0], f, np.inf, n, rc.SCORE_SEED, max_steps, episodes)  # half 0 == half 1: the plain flight
        rc.assert_score_equal(picked, 0, plain, n, f"cut {cut} picks half {h}")
        rc.assert_score_equal(same, 0, plain, n, f"both halves equal, half {h}")
