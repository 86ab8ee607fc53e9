"""The split transition-model kernel's per-lane body (csrc/dql_model_split.hpp) run on the CPU and held to the oracle's stepwise loop with == (CPU only, no GPU).

tests/host_emu/split_model_emu.cpp compiles the real device headers as host C++ and flies every env lane by lane exactly as k_model_split does:
model_split_episodes with the one exploration threshold, the feature and the cut, the sink adding to the table set's four tables.  The yardstick is the unchanged
oracle stepped with external actions, every feature's field read BEFORE each step (tests/split_model_checks.py): it knows nothing of the kernel.  Built twice:
plain, and with ASan + UBSan as a stand-alone program (any report fails).

Every case asserts on the ORACLE's recorded decisions, before comparing, that the events it is there for occurred (split_model_checks.flight).  A host wave is
one lane: that two lanes of a wave hold the same (cell, s') in different halves shows on the GPU only (tests/test_gpu_split_model.py)."""
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import N_CELLS

import host_emu_harness as heh
import model_checks as mc
import split_model_checks as sc

emu = heh.emu_fixture("split_model_emu")


def run_emu(exe, cfg, sets, n, seed, eps, max_steps, episodes, feature, cut, tmp, sanitized=False, stem="split"):
    """the split model of the table sets `sets` as ops.split_model returns it"""
    K = len(sets)
    c = bytes(cfg.to_c())
    hdr = struct.pack("<8i", len(c), cfg.dtype, K, max_steps, episodes, feature, 0, 0) + struct.pack("<2q", n, seed) + struct.pack("<d", eps)
    cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cut, np.float64), (sc.N_STATES,)))
    qa = np.stack([np.ascontiguousarray(s[0], np.float64).ravel() for s in sets]); qb = np.stack([np.ascontiguousarray(s[1], np.float64).ravel() for s in sets])
    r = heh.Reader(heh.run(exe, hdr + c + cut.tobytes() + qa.tobytes() + qb.tobytes(), tmp, stem, sanitized))
    pairs, reward_fx = r.take(np.uint32, (K, 2, N_CELLS, sc.N_STATES)), r.take(np.int64, (K, 2, N_CELLS))
    terminal, feat = r.take(np.int64, (K, 2, N_CELLS, sc.N_CODES)), r.take(np.int64, (K, sc.N_STATES))
    by_code, steps_sum, faults = r.take(np.int64, (K, sc.N_COLS)), r.take(np.int64, (K,)), r.take(np.int64, (1,))
    r.done()
    assert faults[0] == 0, "a range check counted a fault: the guard dropped a contribution"
    visits = pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1)
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "feat_sum_fx": feat, "by_code": by_code, "steps_sum": steps_sum, "visits": visits,
            "state_visits": visits.sum(axis=1).reshape(K, sc.N_STATES, 3).sum(axis=-1)}


def fly(exe, case_id, feature, cut, tmp, sanitized=False):
    cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
    return run_emu(exe, cfg, [tables], n, sc.SEED, eps, max_steps, episodes, feature, cut, tmp, sanitized, stem=f"split_{case_id}_{feature}")


def fly_every_feature(exe, case_id, tmp, sanitized=False):
    """all eleven features of a case at the yardstick's cuts, flown side by side: {feature: result}"""
    d = sc.flight(case_id)
    with ThreadPoolExecutor(len(sc.FEATURES)) as ex:
        return dict(zip(range(len(sc.FEATURES)), ex.map(lambda f: fly(exe, case_id, f, sc.cut_of(d, f), tmp, sanitized), range(len(sc.FEATURES)))))


@pytest.mark.parametrize("case_id", sc.CASE_IDS)
def test_every_feature_of_a_case_equals_the_oracle_s_stepwise_split(emu, case_id, tmp_path):
    d = sc.flight(case_id)
    for f, got in fly_every_feature(emu["plain"], case_id, tmp_path).items():
        what = f"case {case_id}, {sc.FEATURES[f]}"
        sc.assert_split_set_equal(got, 0, sc.expected(d, f, sc.cut_of(d, f)), what)
        # the split changes no flight: the halves sum to the model's yardstick, whatever the feature and the cut
        sc.assert_halves_sum_to_the_model(case_id, got, 0, what)
        # the feature sums are consistent with the recorded values
        assert int(got["feat_sum_fx"].sum()) == int(np.rint(d["value"][f] * float(1 << sc.FRAC_BITS)).astype(np.int64).sum()), what
        assert int(got["state_visits"].sum()) == d["env"].size


@pytest.mark.parametrize("case_id", sc.CASE_IDS)
def test_split_model_clean_under_asan_and_ubsan(emu, case_id, tmp_path):
    """every case and feature through the ASan + UBSan build: no report, and still the oracle's result"""
    d = sc.flight(case_id)
    for f, got in fly_every_feature(emu["san"], case_id, tmp_path, sanitized=True).items():
        sc.assert_split_set_equal(got, 0, sc.expected(d, f, sc.cut_of(d, f)), f"case {case_id}, {sc.FEATURES[f]} (sanitized)")


@pytest.mark.parametrize("case_id", ["A", "B64"])
def test_infinite_cuts_send_everything_to_one_half(emu, case_id, tmp_path):
    d = sc.flight(case_id)
    f = sc.FEATURES.index("pitch_sp")
    for cut, empty in ((np.inf, 1), (-np.inf, 0)):
        got = fly(emu["plain"], case_id, f, cut, tmp_path)
        sc.assert_split_set_equal(got, 0, sc.expected(d, f, cut), f"case {case_id}, cut {cut}")
        assert not got["pairs"][0, empty].any() and not got["terminal"][0, empty].any() and not got["reward_fx"][0, empty].any(), cut
        assert got["visits"][0, 1 - empty].sum() == d["env"].size
        sc.assert_halves_sum_to_the_model(case_id, got, 0, f"cut {cut}")


@pytest.mark.parametrize("case_id", ["A", "B64"])
def test_a_value_equal_to_its_cut_is_in_half_one(emu, case_id, tmp_path):
    """one case per dtype: the crafted cut holds a recorded decision's exact value; the result is the `>=` yardstick and not the `>` one"""
    d = sc.flight(case_id)
    f, cut = sc.EQUAL_TO_CUT_FEATURE, sc.equal_to_cut(sc.flight(case_id))
    got = fly(emu["plain"], case_id, f, cut, tmp_path)
    sc.assert_split_set_equal(got, 0, sc.expected(d, f, cut), f"case {case_id}, crafted cut")
    wrong = sc.expected(d, f, cut, strict=True)
    assert not np.array_equal(got["visits"][0], wrong["visits"]), "`>` would have given the same result: the crafted cut shows nothing"


def test_two_table_sets_in_one_launch_keep_their_tables_apart(emu, tmp_path):
    """case D's set and the all-zero set in one launch: each equals its own single launch, so nothing of a set lands in its neighbour's tables"""
    cfg, tables, eps, n, max_steps, episodes = mc.case_args("D")
    d = sc.flight("D")
    f = sc.FEATURES.index("obs_v_x")
    cut = sc.cut_of(d, f)
    zeros = (np.zeros(N_CELLS), np.zeros(N_CELLS))
    both = run_emu(emu["plain"], cfg, [tables, zeros], n, sc.SEED, eps, max_steps, episodes, f, cut, tmp_path)
    sc.assert_split_set_equal(both, 0, sc.expected(d, f, cut), "set 0 of two")
    alone = run_emu(emu["plain"], cfg, [zeros], n, sc.SEED, eps, max_steps, episodes, f, cut, tmp_path)
    assert alone["pairs"][0].tolist() != both["pairs"][0].tolist(), "the two sets fly differently"
    for name in sc.FIELDS:
        assert np.array_equal(both[name][1], alone[name][0]), name
