"""The mapping scorer's per-lane body (csrc/dql_score_map.hpp) run on the CPU and held to the oracle's STEPWISE loop with == (CPU only, no GPU).

tests/host_emu/score_map_emu.cpp compiles the real device headers as host C++ and flies every env lane by lane exactly as k_score_map does: the wave's
histogram cleared, the episodes flown, the non-zero cells and the tally added to the table set's rows.  The yardstick is the unchanged oracle driven one period
at a time (tests/map_checks.py), which knows nothing of the kernel: `visits`, `ep_last_cell`, the per-episode log, by_code and steps_sum must be equal; the
score's part of the result is also held to score_checks.stepwise_episodes, the contract score_emu is held to.  Built twice: plain, and with ASan + UBSan as a
stand-alone program (any report fails).

Every case asserts on the ORACLE's result, before comparing, that the events it is there for occurred.  A host wave is one lane: that 64 lanes share one
histogram (same-cell adds, the flush's partial last sweep) shows on the GPU only (tests/test_gpu_score_map.py)."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import N_CELLS
from oracle.oracle import Oracle

import host_emu_harness as heh
import map_checks as mc
import rollout_checks as rc
import score_checks as sc

N_ENVS, SEED, EPISODES = 64, 123, 3
MAX_STEPS = 900      # three episodes of every env of every case end before it (asserted on the oracle)
CASE_IDS = ("simulation-f64", "training4-f32", "simulation-two-axis-f32")
N_COLS = sc.N_CODES + 1
X_TWO, X_ONLY = 0, 1  # dql_device.hpp

emu = heh.emu_fixture("score_map_emu")


def run_emu(exe, cfg, sets, n, seed, max_steps, episodes, tmp, log=True, sanitized=False):
    """the score map of the table sets `sets` as ops.score_map returns it"""
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = struct.pack("<8i", len(c), cfg.dtype, X_TWO if cfg.two_axis else X_ONLY, K, max_steps, episodes, 1 if log else 0, 0) + struct.pack("<2q", n, seed)
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + qa.tobytes() + qb.tobytes(), tmp, "score_map", sanitized))
    nt = K * n
    by_code, steps_sum, visits, faults = r.take(np.int64, (K, N_COLS)), r.take(np.int64, (K,)), r.take(np.int64, (K, N_CELLS)), r.take(np.int64, (1,))
    ep_code, ep_steps, last = (r.take(np.uint8, (episodes, nt)), r.take(np.uint16, (episodes, nt)), r.take(np.uint16, (2, episodes, nt))) if log else (None, None, None)
    r.done()
    assert faults[0] == 0, "a range check counted a fault: the guard dropped a write"
    return {"by_code": by_code, "steps_sum": steps_sum, "visits": visits, "ep_code": ep_code, "ep_steps": ep_steps, "ep_last_cell": last}


_YARDSTICKS = {}


def oracle_yardsticks(case_id, max_steps, episodes=EPISODES):
    """the stepwise map of each of the three table sets, computed once per argument set and left unchanged"""
    key = (case_id, max_steps, episodes)
    if key not in _YARDSTICKS:
        cfg = rc.case_config(case_id)
        _YARDSTICKS[key] = [mc.stepwise_map(Oracle(cfg, N_ENVS, seed=SEED), t, max_steps, episodes, bool(cfg.two_axis)) for t in rc.three_table_sets()]
    return _YARDSTICKS[key]


def cut_for(case_id):
    """a max_steps, chosen on the oracle's full run, at which the reference's tables have finished first episodes and unfinished later ones: the median period
    at which a second episode ends (lengths + one reset period per episode), as tests/test_score_host_emulation.py chooses it"""
    w = oracle_yardsticks(case_id, MAX_STEPS)[0]
    end_of_second = w["ep_steps"][0].astype(np.int64) + w["ep_steps"][1].astype(np.int64) + 1
    return int(np.median(end_of_second))


def assert_all_sets_equal(got, want, what):
    for k, w in enumerate(want):
        mc.assert_map_set_equal(got, k, N_ENVS, w, f"{what}, table set {k}")


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_three_episodes_of_three_table_sets_equal_the_oracle_s_stepwise_map(emu, case_id, tmp_path):
    cfg = rc.case_config(case_id)
    axes = 2 if cfg.two_axis else 1
    want = oracle_yardsticks(case_id, MAX_STEPS)
    for k, w in enumerate(want):  # not vacuous: everything finished in a decision period, resets were met, and level 4 reaches the last cells
        ev = w["events"]
        print(case_id, k, ev, int(w["visits"].sum()), w["steps_sum"])
        assert w["by_code"][sc.UNFINISHED] == 0 and ev["unfinished_decisions"] == 0 and ev["ends_outside_a_decision"] == 0, f"{case_id} set {k}: {ev}"
        assert int(w["visits"].sum()) == axes * w["steps_sum"] == ev["decisions"]
        assert ev["reset_periods"] == N_ENVS * EPISODES and ev["early_lanes"] > 0 and ev["tail_decisions"] > 0 and ev["same_cell_periods"] > 0, f"{case_id} set {k}: {ev}"
        assert (w["ep_last_cell"][0] != mc.NO_CELL).all() and ((w["ep_last_cell"][1] != mc.NO_CELL).all() if cfg.two_axis else (w["ep_last_cell"][1] == mc.NO_CELL).all())
        assert not cfg.two_axis or ev["xy_differ"] > 0
        ref = sc.stepwise_episodes(Oracle(cfg, N_ENVS, seed=SEED), rc.three_table_sets()[k], MAX_STEPS, EPISODES)  # the contract score_emu is held to
        assert np.array_equal(ref["ep_code"], w["ep_code"]) and np.array_equal(ref["ep_steps"], w["ep_steps"]) and ref["steps_sum"] == w["steps_sum"]
    assert want[0]["visits"].tolist() != want[1]["visits"].tolist()
    levels = want[0]["visits"].reshape(5, -1).sum(axis=1)
    assert (levels > 0).all(), f"a greedy flight at level 4 visits cells of all five levels: {levels.tolist()}"
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, MAX_STEPS, EPISODES, tmp_path)
    assert got["visits"].shape == (3, N_CELLS) and got["ep_last_cell"].shape == (2, EPISODES, 3 * N_ENVS)
    assert_all_sets_equal(got, want, case_id)
    nolog = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, MAX_STEPS, EPISODES, tmp_path, log=False)
    assert nolog["ep_last_cell"] is None
    for f in ("by_code", "steps_sum", "visits"):
        assert np.array_equal(nolog[f], got[f]), f


def test_a_cut_off_run_counts_the_decisions_of_unfinished_episodes_and_nothing_of_finished_lanes(emu, tmp_path):
    case_id = "training4-f32"
    cfg = rc.case_config(case_id)
    cut = cut_for(case_id)
    want = oracle_yardsticks(case_id, cut)
    w = want[0]
    ev = w["events"]
    print(case_id, "cut at", cut, ev, int(w["visits"].sum()), w["steps_sum"], w["by_code"].tolist())
    assert ev["unfinished_decisions"] > 0 and int(w["visits"].sum()) == w["steps_sum"] + ev["unfinished_decisions"] > w["steps_sum"], ev
    assert ev["early_lanes"] > 0, "some lanes have finished their three episodes while others fly on: they must count nothing more"
    assert w["by_code"][sc.UNFINISHED] >= N_ENVS // 4 and (w["ep_last_cell"][0] == mc.NO_CELL).any() and (w["ep_last_cell"][0] != mc.NO_CELL).any()
    assert ((w["ep_last_cell"][0] == mc.NO_CELL) == (w["ep_code"] == sc.NO_CODE)).all()
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, EPISODES, tmp_path)
    assert_all_sets_equal(got, want, f"{case_id} cut at {cut}")


def test_a_run_cut_at_five_periods_counts_the_few_decisions_there_are_and_logs_next_to_nothing(emu, tmp_path):
    case_id = "training4-f32"
    cfg = rc.case_config(case_id)
    want = oracle_yardsticks(case_id, 5)
    for w in want:  # period 0 is the reset period; periods 1 .. 5 are decisions, nearly all of episodes that do not finish (a few leave the fly zone at once)
        ev = w["events"]
        print(case_id, "cut at 5", ev, w["by_code"].tolist())
        assert w["by_code"][sc.UNFINISHED] >= N_ENVS * EPISODES - N_ENVS // 8 and ev["periods"] == 6
        assert 4 * N_ENVS <= int(w["visits"].sum()) == w["steps_sum"] + ev["unfinished_decisions"] <= 5 * N_ENVS and ev["unfinished_decisions"] >= 4 * N_ENVS
        assert ((w["ep_last_cell"][0] == mc.NO_CELL) == (w["ep_code"] == sc.NO_CODE)).all() and (w["ep_last_cell"][1] == mc.NO_CELL).all()
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, 5, EPISODES, tmp_path)
    assert_all_sets_equal(got, want, f"{case_id} cut at 5")


@pytest.mark.parametrize("case_id", ("training4-f32", "simulation-two-axis-f32"))
def test_one_episode_per_env_every_lane_stops_at_a_period_of_its_own(emu, case_id, tmp_path):
    cfg = rc.case_config(case_id)
    want = oracle_yardsticks(case_id, MAX_STEPS, 1)
    w = want[0]
    ev = w["events"]
    print(case_id, "one episode", ev)
    assert w["by_code"][sc.UNFINISHED] == 0 and ev["early_lanes"] >= N_ENVS // 2 and len(set(w["ep_steps"][0].tolist())) >= 8, ev
    assert ev["reset_periods"] == N_ENVS, "a lane that finished its one episode is not flown through another reset"
    got = run_emu(emu["plain"], cfg, rc.three_table_sets(), N_ENVS, SEED, MAX_STEPS, 1, tmp_path)
    assert_all_sets_equal(got, want, f"{case_id}, one episode per env")


@pytest.mark.parametrize("case_id", ("training4-f32", "simulation-two-axis-f32"))
def test_score_map_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """the cut-off run (finished and unfinished log entries, lanes that stop early) through the ASan + UBSan build: no report, and still the oracle's result"""
    cfg = rc.case_config(case_id)
    cut = cut_for(case_id)
    want = oracle_yardsticks(case_id, cut)
    got = run_emu(emu["san"], cfg, rc.three_table_sets(), N_ENVS, SEED, cut, EPISODES, tmp_path, sanitized=True)
    assert_all_sets_equal(got, want, f"sanitized {case_id} cut at {cut}")
