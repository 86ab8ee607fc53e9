"""The scenario-grid scoring kernel's device code (csrc/dql_score_grid.hpp: grid_coords, touch_bin, score_grid_episodes) run on the CPU and held to the oracle's
STEPWISE loop with == (CPU only, no GPU).

tests/host_emu/grid_emu.cpp compiles the real device headers as host C++ and walks every block of the launch: grid_coords picks the block's scenario, table set
and envs, every lane flies its episodes under that scenario's record of constants, and each lane's tally is added to row (scenario, set).  The yardstick is
tests/grid_checks.py: one fresh, unchanged Oracle per (scenario, set), driven one period at a time, the touch bins formed in numpy.  Built twice: plain, and with
ASan + UBSan (any report fails); the builds, the child process and the result reader are tests/host_emu_harness.py's.

Every case asserts on the ORACLE's result, before comparing, that the events it is there for occurred."""
import struct

import numpy as np
import pytest

from oracle.oracle import Oracle

import grid_checks as gc
import host_emu_harness as heh

X_TWO, X_ONLY = 0, 1  # dql_device.hpp

emu = heh.emu_fixture("grid_emu")


def run_emu(exe, cfgs, sets, n, seed, max_steps, episodes, tmp, log=True, touch=True, sanitized=False):
    """the grid score of the table sets `sets` under `cfgs` as ops.score_grid returns it"""
    S, K = len(cfgs), len(sets)
    c = [bytes(cfg.to_c()) for cfg in cfgs]
    hdr = struct.pack("<8i", len(c[0]), cfgs[0].dtype, X_TWO if cfgs[0].two_axis else X_ONLY, K, max_steps, episodes, (1 if log else 0) | (2 if touch else 0), S)
    hdr += struct.pack("<2q", n, seed)
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + b"".join(c) + qa.tobytes() + qb.tobytes(), tmp, "grid", sanitized))
    out = {"by_code": r.take(np.int64, (S, K, gc.N_COLS)), "steps_sum": r.take(np.int64, (S, K)), "touch_hist": r.take(np.int64, (S, K, gc.N_BINS)) if touch else None}
    out["ep_code"], out["ep_steps"] = (r.take(np.uint8, (S, episodes, K * n)), r.take(np.uint16, (S, episodes, K * n))) if log else (None, None)
    r.done()
    return out


_YARDSTICKS = {}


def oracle_yardstick(case_id):
    """the stepwise grid of a case group, computed once and left unchanged"""
    if case_id not in _YARDSTICKS:
        cfgs, n, episodes = gc.case(case_id)
        _YARDSTICKS[case_id] = gc.stepwise_grid(lambda cfg, n_, seed: Oracle(cfg, n_, seed=seed), cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes)
    return _YARDSTICKS[case_id]


@pytest.mark.parametrize("case_id", gc.CASE_IDS)
def test_every_output_of_the_grid_equals_the_oracle_s_stepwise_loop(emu, case_id, tmp_path):
    cfgs, n, episodes = gc.case(case_id)
    want = oracle_yardstick(case_id)
    print(case_id, "by_code set 0:", want["by_code"][:, 0].tolist(), "touch set 0:", want["touch_hist"][:, 0].tolist())
    gc.assert_not_vacuous(case_id, want)
    got = run_emu(emu["plain"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path)
    gc.assert_grid_equal(got, want, case_id)
    nolog = run_emu(emu["plain"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path, log=False)
    assert nolog["ep_code"] is None and nolog["ep_steps"] is None
    gc.assert_grid_equal(nolog, want, f"{case_id} without the log", ("by_code", "steps_sum", "touch_hist"))
    notouch = run_emu(emu["plain"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path, touch=False)
    assert notouch["touch_hist"] is None
    gc.assert_grid_equal(notouch, want, f"{case_id} without touch_hist", ("by_code", "steps_sum", "ep_code", "ep_steps"))
    neither = run_emu(emu["plain"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path, log=False, touch=False)
    gc.assert_grid_equal(neither, want, f"{case_id} without the log and touch_hist", ("by_code", "steps_sum"))


@pytest.mark.parametrize("case_id", gc.CASE_IDS)
def test_grid_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """the same launches through the ASan + UBSan build: no report, and still the oracle's result"""
    cfgs, n, episodes = gc.case(case_id)
    want = oracle_yardstick(case_id)
    got = run_emu(emu["san"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path, sanitized=True)
    gc.assert_grid_equal(got, want, f"sanitized {case_id}")
    bare = run_emu(emu["san"], cfgs, gc.table_sets(), n, gc.SEED, gc.MAX_STEPS, episodes, tmp_path, log=False, touch=False, sanitized=True)
    gc.assert_grid_equal(bare, want, f"sanitized {case_id} without the log and touch_hist", ("by_code", "steps_sum"))
