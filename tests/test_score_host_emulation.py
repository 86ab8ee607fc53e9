"""The scoring kernel's per-lane body (csrc/dql_score.hpp) run on the CPU and held to the oracle's STEPWISE loop with == (CPU only, no GPU).

tests/host_emu/score_emu.cpp compiles the real device headers as host C++ and flies every env episode after episode, lane by lane, exactly as k_score
does, adding each lane's tally to its table set's row.  The yardstick is the unchanged oracle driven one period at a time (tests/score_checks.py:
`Oracle.eval_steps(1)` repeated, every FL_DONE of every env noted), which knows nothing of the scoring: the per-episode log, by_code and steps_sum must be
equal.  Built twice: plain, and with ASan + UBSan (any report fails); the builds, the child process and the result reader are tests/host_emu_harness.py's.

Every case asserts on the ORACLE's result, before comparing, that it is not vacuous."""
import struct

import numpy as np
import pytest

from oracle.oracle import Oracle

import host_emu_harness as heh
import rollout_checks as rc
import score_checks as sc

N_ENVS, SEED, EPISODES = 64, 123, 3
MAX_STEPS = 900      # three episodes of every env of every case end before it (asserted on the oracle)
CASE_IDS = ("simulation-f64", "training4-f32")
N_COLS = sc.N_CODES + 1
X_TWO, X_ONLY = 0, 1  # dql_device.hpp

emu = heh.emu_fixture("score_emu")


def run_emu(exe, cfg, sets, n, seed, max_steps, episodes, tmp, log=True, sanitized=False):
    """the score of the table sets `sets` as ops.score returns it"""
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = struct.pack("<8i", len(c), cfg.dtype, X_TWO if cfg.two_axis else X_ONLY, K, max_steps, episodes, 1 if log else 0, 0) + struct.pack("<2q", n, seed)
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + qa.tobytes() + qb.tobytes(), tmp, "score", sanitized))
    nt = K * n
    by_code, steps_sum = r.take(np.int64, (K, N_COLS)), r.take(np.int64, (K,))
    ep_code, ep_steps = (r.take(np.uint8, (episodes, nt)), r.take(np.uint16, (episodes, nt))) if log else (None, None)
    r.done()
    return {"by_code": by_code, "steps_sum": steps_sum, "ep_code": ep_code, "ep_steps": ep_steps}


_YARDSTICKS = {}


def oracle_yardsticks(case_id, max_steps):
    """the stepwise result of each of the three table sets, computed once per (case, max_steps) and left unchanged"""
    key = (case_id, max_steps)
    if key not in _YARDSTICKS:
        cfg = rc.case_config(case_id)
        _YARDSTICKS[key] = [sc.stepwise_episodes(Oracle(cfg, N_ENVS, seed=SEED), t, max_steps, EPISODES) for t in rc.three_table_sets()]
    return _YARDSTICKS[key]


def cut_for(case_id):
    """a max_steps, chosen on the oracle's full run, at which the reference's tables have finished first episodes and unfinished later ones: the median period
    at which a second episode ends (lengths + one reset period per episode)"""
    w = oracle_yardsticks(case_id, MAX_STEPS)[0]
    end_of_second = w["ep_steps"][0].astype(np.int64) + w["ep_steps"][1].astype(np.int64) + 1
    return int(np.median(end_of_second))


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_three_episodes_of_three_table_sets_equal_the_oracle_s_stepwise_loop(emu, case_id, tmp_path):
    cfg = rc.case_config(case_id)
    want = oracle_yardsticks(case_id, MAX_STEPS)
    for k, w in enumerate(want):  # not vacuous: everything finished, and the sets end differently
        assert w["by_code"][sc.UNFINISHED] == 0 and w["by_code"].sum() == N_ENVS * EPISODES, f"{case_id} set {k}: {w['by_code'].tolist()}"
        assert w["ep_steps"].min() >= 1
    assert np.count_nonzero(want[0]["by_code"]) >= 2, want[0]["by_code"].tolist()
    assert want[0]["by_code"].tolist() != want[1]["by_code"].tolist()
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, MAX_STEPS, EPISODES, tmp_path)
    assert got["by_code"].shape == (3, N_COLS) and got["ep_code"].shape == (EPISODES, 3 * N_ENVS)
    for k, w in enumerate(want):
        sc.assert_set_equal(got, k, N_ENVS, w, f"{case_id} table set {k}")
    nolog = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, MAX_STEPS, EPISODES, tmp_path, log=False)
    assert nolog["ep_code"] is None and np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_a_cut_off_run_has_finished_and_unfinished_episodes_and_counts_both(emu, case_id, tmp_path):
    cfg = rc.case_config(case_id)
    cut = cut_for(case_id)
    want = oracle_yardsticks(case_id, cut)
    w = want[0]
    finished, unfinished = int(w["by_code"][:sc.UNFINISHED].sum()), int(w["by_code"][sc.UNFINISHED])
    assert finished >= N_ENVS and unfinished >= N_ENVS // 4 and finished + unfinished == N_ENVS * EPISODES, f"cut at {cut}: {w['by_code'].tolist()}"
    assert (w["ep_code"][0] != sc.NO_CODE).any() and (w["ep_code"][EPISODES - 1] == sc.NO_CODE).any()
    assert ((w["ep_code"] == sc.NO_CODE) == (w["ep_steps"] == sc.NO_STEPS)).all()
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, EPISODES, tmp_path)
    for k, wk in enumerate(want):
        sc.assert_set_equal(got, k, N_ENVS, wk, f"{case_id} cut at {cut}, table set {k}")
    assert (got["by_code"].sum(axis=1) == N_ENVS * EPISODES).all()


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_score_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """the cut-off run (both kinds of log entry are written) through the ASan + UBSan build: no report, and still the oracle's result"""
    cfg = rc.case_config(case_id)
    cut = cut_for(case_id)
    want = oracle_yardsticks(case_id, cut)
    got = run_emu(emu["san"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, EPISODES, tmp_path, sanitized=True)
    for k, wk in enumerate(want):
        sc.assert_set_equal(got, k, N_ENVS, wk, f"sanitized {case_id} cut at {cut}, table set {k}")


# ---- the high bit planes of the lane sums (7 planes for the unfinished episodes, 13 for the steps) ----
@pytest.mark.parametrize("case_id", ("simulation-f32", "simulation-f64"))
def test_sixty_four_unfinished_episodes_per_lane_set_the_highest_plane_of_the_count(emu, case_id, tmp_path):
    """64 episodes per env, cut at max_steps = 5: no episode ends in 6 periods, so every lane reports 64 unfinished episodes, bit 6 of its count"""
    cfg = rc.case_config(case_id)
    episodes, cut = 64, 5
    want = [sc.stepwise_episodes(Oracle(cfg, N_ENVS, seed=SEED), t, cut, episodes) for t in rc.three_table_sets()]
    for w in want:  # on the oracle: nothing finished
        assert w["by_code"][sc.UNFINISHED] == N_ENVS * episodes and w["by_code"][:sc.UNFINISHED].sum() == 0 and w["steps_sum"] == 0
        assert (sc.lane_sums(w)[0] == 64).all()
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, episodes, tmp_path)
    for k, w in enumerate(want):
        sc.assert_set_equal(got, k, N_ENVS, w, f"{case_id}, 64 unfinished episodes per lane, table set {k}")
    assert (got["by_code"][:, sc.UNFINISHED] == N_ENVS * episodes).all() and (got["steps_sum"] == 0).all() and (got["ep_code"] == sc.NO_CODE).all()
    nolog = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, episodes, tmp_path, log=False)
    assert np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])


def test_a_long_score_sets_every_plane_of_the_lane_sums(emu, tmp_path):
    """64 episodes per env within 4 096 periods, the reference's tables, `training4-f32`: on the oracle the lanes leave 26 - 37 episodes unfinished and sum
    3 805 - 4 070 steps, so planes 0 - 5 of the count and 0 - 11 of the steps all carry a set bit in some lane (`simulation-f32` leaves 41 - 44 unfinished:
    bit 4 never set)"""
    case_id, episodes, max_steps = "training4-f32", 64, 4096
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    want = sc.stepwise_episodes(Oracle(cfg, N_ENVS, seed=SEED), tables, max_steps, episodes)
    unfinished, steps = sc.lane_sums(want)
    assert int(np.bitwise_or.reduce(unfinished)) & 0x3f == 0x3f, sorted(set(unfinished.tolist()))
    assert int(np.bitwise_or.reduce(steps)) & 0xfff == 0xfff and steps.max() < 1 << 13
    got = run_emu(emu["plain"], cfg, [tables], N_ENVS, SEED, max_steps, episodes, tmp_path)
    sc.assert_set_equal(got, 0, N_ENVS, want, f"{case_id}, {episodes} episodes within {max_steps} periods")
    nolog = run_emu(emu["plain"], cfg, [tables], N_ENVS, SEED, max_steps, episodes, tmp_path, log=False)
    assert nolog["ep_code"] is None and np.array_equal(nolog["by_code"], got["by_code"]) and np.array_equal(nolog["steps_sum"], got["steps_sum"])
