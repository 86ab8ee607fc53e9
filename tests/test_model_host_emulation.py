"""The transition-model kernel's per-lane body (csrc/dql_model.hpp) run on the CPU and held to the oracle's stepwise loop with == (CPU only, no GPU).

tests/host_emu/model_emu.cpp compiles the real device headers as host C++ and flies every env lane by lane exactly as k_model does: model_episodes with the
one exploration threshold, the sink adding to the table set's three tables, the tally added to the set's rows.  The yardstick is the unchanged oracle stepped
with external actions (tests/model_checks.py), which knows nothing of the kernel: pairs, reward_fx, terminal, by_code, steps_sum and visits must be equal.
Built twice: plain, and with ASan + UBSan as a stand-alone program (any report fails).

Every case asserts on the ORACLE's result, before comparing, that the events it is there for occurred (model_checks.yardstick).  A host wave is one lane: that
64 lanes add to the same pair in one period shows on the GPU only (tests/test_gpu_model.py)."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import N_CELLS

import host_emu_harness as heh
import model_checks as mc

emu = heh.emu_fixture("model_emu")


def run_emu(exe, cfg, sets, n, seed, eps, max_steps, episodes, tmp, sanitized=False):
    """the model of the table sets `sets` as ops.transition_model returns it"""
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = struct.pack("<6i", len(c), cfg.dtype, K, max_steps, episodes, 0) + struct.pack("<2q", n, seed) + struct.pack("<d", eps)
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + qa.tobytes() + qb.tobytes(), tmp, "model", sanitized))
    pairs, reward_fx, terminal = r.take(np.uint32, (K, N_CELLS, mc.N_STATES)), r.take(np.int64, (K, N_CELLS)), r.take(np.int64, (K, N_CELLS, mc.N_CODES))
    by_code, steps_sum, faults = r.take(np.int64, (K, mc.N_COLS)), r.take(np.int64, (K,)), r.take(np.int64, (1,))
    r.done()
    assert faults[0] == 0, "a range check counted a fault: the guard dropped a contribution"
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "by_code": by_code, "steps_sum": steps_sum,
            "visits": pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1)}


def fly_case(exe, case_id, tmp, sanitized=False):
    cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
    want = mc.yardstick(case_id)
    got = run_emu(exe, cfg, [tables], n, mc.SEED, eps, max_steps, episodes, tmp, sanitized)
    mc.assert_model_set_equal(got, 0, want, f"case {case_id}{' (sanitized)' if sanitized else ''}")
    return got, want


@pytest.mark.parametrize("case_id", list(mc.CASES))
def test_the_model_of_a_case_equals_the_oracle_s_stepwise_model(emu, case_id, tmp_path):
    got, want = fly_case(emu["plain"], case_id, tmp_path)
    # conservation: every decision is a pair or a terminal, and the terminals are the finished episodes
    assert int(got["visits"].sum()) == want["events"]["decisions"]
    assert np.array_equal(got["terminal"][0].sum(axis=0), got["by_code"][0][:mc.N_CODES])


@pytest.mark.parametrize("case_id", list(mc.CASES))
def test_model_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """every case through the ASan + UBSan build: no report, and still the oracle's result"""
    fly_case(emu["san"], case_id, tmp_path, sanitized=True)


def test_two_table_sets_in_one_launch_keep_their_tables_apart(emu, tmp_path):
    """case D's set and the all-zero set in one launch: each equals its own single launch, so nothing of a set lands in its neighbour's tables"""
    cfg, tables, eps, n, max_steps, episodes = mc.case_args("D")
    zeros = (np.zeros(N_CELLS), np.zeros(N_CELLS))
    both = run_emu(emu["plain"], cfg, [tables, zeros], n, mc.SEED, eps, max_steps, episodes, tmp_path)
    mc.assert_model_set_equal(both, 0, mc.yardstick("D"), "set 0 of two")
    alone = run_emu(emu["plain"], cfg, [zeros], n, mc.SEED, eps, max_steps, episodes, tmp_path)
    assert alone["pairs"][0].tolist() != both["pairs"][0].tolist(), "the two sets fly differently"
    for f in mc.FIELDS:
        assert np.array_equal(both[f][1], alone[f][0]), f
