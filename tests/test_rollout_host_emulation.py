"""The roll-out kernel's per-lane episode body (csrc/dql_rollout.hpp) run on the CPU and held bit for bit to the oracle's STEPWISE loop (CPU only, no GPU).

tests/host_emu/rollout_emu.cpp compiles the real device headers as host C++ (the stand-in runtime header of step_emu.cpp) and flies every env's first
greedy episode lane by lane, exactly as k_rollout does.  The yardstick is the unchanged oracle driven one period at a time — `Oracle.eval_steps(1)`
repeated, the first FL_DONE of every env captured from `get_fields()` (tests/rollout_checks.py) —, which knows nothing of the roll-out: code, step count
and every record field must agree in every bit.  Built twice: plain, and with ASan + UBSan (any report fails); the builds, the child process and the
result reader are tests/host_emu_harness.py's.

Every case asserts on the ORACLE's result, before comparing, that it is not vacuous (several terminal codes, nothing unfinished — or, for the cut-off
case, a real share of unfinished envs): a change of defaults cannot quietly turn these into one-code tests."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F64
from oracle.oracle import Oracle

import host_emu_harness as heh
import rollout_checks as rc

X_TWO, X_ONLY = 0, 1  # dql_device.hpp
N_REC, N_TRACE = len(rc.RECORD_FIELDS), len(rc.TRACE_FIELDS)
N_ENVS, SEED, MAX_STEPS = 512, 123, 600

emu = heh.emu_fixture("rollout_emu")


def run_emu(exe, cfg, tables, n, seed, max_steps, tmp, trace_envs=0, sanitized=False):
    """the roll-out of `tables` (one (qa, qb) pair or a list) as ops.rollout returns it: arrays [n_tables, n], "trace" or None"""
    sets = [tables] if isinstance(tables, tuple) else list(tables)
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = struct.pack("<8i", len(c), cfg.dtype, X_TWO if cfg.two_axis else X_ONLY, K, max_steps, trace_envs, 0, 0) + struct.pack("<2q", n, seed)
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + qa.tobytes() + qb.tobytes(), tmp, "rollout", sanitized))
    code, steps, rec = r.take(np.int32, (K, n)), r.take(np.int32, (K, n)), r.take(np.float64, (N_REC, K, n))
    trace = r.take(np.float64, (max_steps + 1, N_TRACE, trace_envs)) if trace_envs else None
    r.done()
    out = {"code": code, "steps": steps, "trace": trace}
    out.update({f: rec[k] for k, f in enumerate(rc.RECORD_FIELDS)})
    return out


def oracle_yardstick(cfg, tables, n=N_ENVS, seed=SEED, max_steps=MAX_STEPS, trace_envs=0):
    return rc.stepwise_first_episodes(Oracle(cfg, n, seed=seed), tables, max_steps, trace_envs)


def assert_not_vacuous(case_id, want):
    """the properties of the ORACLE's result that make the case worth comparing"""
    h = rc.histogram(want["code"])
    assert h["unfinished"] == 0, f"{case_id}: {h}"
    codes = {k for k, v in h.items() if v and k != "unfinished"}
    if case_id.startswith("simulation"):
        assert len(codes) >= 3 and {"TERMINAL_CONTACT", "TERMINAL_FLYZONE_X", "TERMINAL_MINIMUM_ALTITUDE"} <= codes, f"{case_id}: {h}"
        if "two-axis" in case_id:
            assert "TERMINAL_FLYZONE_Y" in codes, f"{case_id}: {h}"
    else:
        assert len(codes) >= 2, f"{case_id}: {h}"
    assert want["steps"].max() < MAX_STEPS and want["steps"].min() >= 1


@pytest.mark.parametrize("case_id", [c[0] for c in rc.CASES])
def test_rollout_bit_exact_vs_the_oracle_s_stepwise_loop(emu, case_id, tmp_path):
    """code, step count and every record field of 512 first episodes on the reference's stage-4 tables, against the oracle driven one period at a time"""
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    want = oracle_yardstick(cfg, tables)
    assert_not_vacuous(case_id, want)
    got = run_emu(emu["plain"], cfg, tables, N_ENVS, SEED, MAX_STEPS, tmp_path)
    assert got["code"].shape == (1, N_ENVS)
    rc.assert_rows_equal(got, want, case_id, row=0)


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-f64"])
def test_cut_off_at_200_steps_leaves_unfinished_rows_with_the_last_state(emu, case_id, tmp_path):
    """max_steps = 200: first episodes of the simulation flavour end around step 197 - 217, so a real share of the envs is still flying; their rows are
    code -1 with the fields of the state after period 200"""
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    want = oracle_yardstick(cfg, tables, max_steps=200)
    unfinished = int((want["code"] < 0).sum())
    assert 0.10 * N_ENVS <= unfinished <= 0.90 * N_ENVS, f"{unfinished} of {N_ENVS} unfinished: the cut would test almost nothing"
    assert (want["steps"][want["code"] < 0] == 200).all()
    got = run_emu(emu["plain"], cfg, tables, N_ENVS, SEED, 200, tmp_path)
    rc.assert_rows_equal(got, want, f"{case_id} cut at 200", row=0)


def test_three_table_sets_fly_paired_episodes_and_equal_single_runs(emu, tmp_path):
    """K = 3 (the reference's tables, zeros, Q_table_b negated): every row equals the single-set run, which equals the oracle"""
    cfg = rc.case_config("simulation-f32")
    sets = rc.three_table_sets()
    got = run_emu(emu["plain"], cfg, sets, N_ENVS, SEED, MAX_STEPS, tmp_path)
    assert got["code"].shape == (3, N_ENVS)
    hists = []
    for k, t in enumerate(sets):
        want = oracle_yardstick(cfg, t)
        rc.assert_rows_equal(got, want, f"table set {k} of 3", row=k)
        single = run_emu(emu["plain"], cfg, t, N_ENVS, SEED, MAX_STEPS, tmp_path)
        rc.assert_rows_equal(got, {f: single[f][0] for f in ("code", "steps") + rc.RECORD_FIELDS}, f"table set {k} of 3 vs its single run", row=k)
        hists.append(rc.histogram(want["code"]))
    assert hists[0] != hists[1], f"the table sets must fly differently: {hists}"


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-two-axis-f32"])
def test_rollout_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """the same episodes at 128 envs through the ASan + UBSan build, with a trace: no report, and still the oracle's bits"""
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    want = oracle_yardstick(cfg, tables, n=128, trace_envs=8)
    assert len(set(want["code"].tolist())) >= 2
    got = run_emu(emu["san"], cfg, tables, 128, SEED, MAX_STEPS, tmp_path, trace_envs=8, sanitized=True)
    rc.assert_rows_equal(got, want, f"sanitized {case_id}", row=0)
    rc.assert_trace_equal(got["trace"], want["trace"], f"sanitized {case_id}")


@pytest.mark.parametrize("case_id", ["simulation-f32", "simulation-two-axis-f32", "training4-f64"])
def test_trace_of_the_first_envs_matches_get_fields_after_every_period(emu, case_id, tmp_path):
    """M = 8: the trace rows are get_fields() after every period the env flies, NaN after its end"""
    cfg = rc.case_config(case_id)
    tables = rc.stage4_tables()
    want = oracle_yardstick(cfg, tables, n=64, trace_envs=8)
    got = run_emu(emu["plain"], cfg, tables, 64, SEED, MAX_STEPS, tmp_path, trace_envs=8)
    t = want["trace"]
    assert t.shape == (MAX_STEPS + 1, N_TRACE, 8)
    last = want["steps"][:8]
    assert np.isnan(t[-1]).all() and not np.isnan(t[0]).any()  # every env of the case ends well before max_steps
    for i in range(8):  # an env's rows stop with the period its episode ended in
        assert not np.isnan(t[: last[i] + 1, :, i]).any() and np.isnan(t[last[i] + 1:, :, i]).all()
    rc.assert_trace_equal(got["trace"], t, case_id)
    rc.assert_rows_equal(got, want, case_id, row=0)
    if cfg.dtype == F64:
        assert cfg.two_axis == 0
